"""The memory contract of include/krotov_hip.h ("Memory contract"), enforced on guarded, minimally aligned buffers.

Every other GPU parity test hands the library freshly allocated torch tensors: 512-byte aligned, padded by the caching
allocator, surrounded by finite numbers nobody looks at.  Here every tensor an engine sees -- operators, CSR arrays,
inputs, outputs, the co-state store, the second-order pair, the engine's own persistent buffers -- is carved from ONE
arena (tests/guarded.py): at the element type's own alignment and no more, between guard bands of at least one
trailing-two-dimensions plane that hold a NaN pattern (zero words next to index arrays).  After every sweep the arena is
compared bytewise on the device: every guard must hold its pattern (no write outside an extent), every tensor the call
may not write must hold what it held before (no input is written: operators, CSR arrays, the co-state store, the previous
trajectory, an inactive replica's slices), and the results must still be the oracle's at the project's tolerances
(1e-12 Hilbert, 1e-11 Liouville) -- a read outside an extent that reaches a result meets a NaN.

What runs: every case of ``test_engine_reuse.CASES`` through the unchanged ``run_sequence`` (steps 1-7: single launch,
per interval, second order, reduced grid, row split), its three captured-graph cases, its Lindblad and replica engines
(with the mask, first and second order); six parametrized sweeps of ``test_parametrization.SWEEPS`` against that file's
restatement; ``tau`` / ``chi_boundary`` / ``expect`` against NumPy; and what the Python layer refuses before a launch.

NOT seen: a read outside an extent whose value is discarded (a prefetch one interval ahead that is dropped) leaves no
trace in a canary; it stays inside the arena here.  No page protection, no sanitizer.

``tau`` and ``chi_boundary`` take host arrays and tensors of any dtype, device and stride and stage them (``dev()``):
for these two only a wrong SHAPE is an error; a view that is not contiguous must be staged, never handed to a kernel."""
import types

import numpy as np
import pytest

import guarded
import parametrization_cases as pc
import test_engine_reuse as ter
import test_parametrization as tp
from guarded import GuardedArena, GuardedDevice, GuardedEngine, GuardViolation
from krotov_amd import configs
from krotov_amd.engine import HipKrotovEngine
from oracle import krotov_oracle as ko
from test_absent_controls import TOL_HILBERT, TOL_LIOUVILLE, _check, _engine_ops

PAR_SWEEPS = ('tile_n5_L1', 'tile_n64_L4_so', 'tile256_k257', 'gen_n70_tile128_so', 'gen_csr_n20', 'gen_stepwise')
SMALL = ((1, 1), (7, 33), (5, 64))  # (K, N) of the tau / chi_boundary runs


# ---------------------------------------------------------------------------
# host only: the checker itself
# ---------------------------------------------------------------------------
def _cpu_arena():
    import torch

    arena = GuardedArena('cpu', 1 << 20)
    t = dict(c=arena.carve('c', (3, 5, 7), torch.complex128), f=arena.carve('f', (4,), torch.float64),
             i=arena.carve('i', (9,), torch.int32), plane=arena.carve('plane', (2, 40, 16), torch.complex128, 'output'),
             own=arena.carve('own', (6,), torch.float64, 'scratch'))
    return arena, t


def test_checker_layout_on_cpu_tensors():
    """Alignment residues are exactly 16 / 8 / 4, the guards are at least max(4096 B, one plane), those of an int32 array
    hold zeros, all others the NaN pattern."""
    import torch

    arena, t = _cpu_arena()
    assert arena.check_layout()
    assert t['c'].data_ptr() % 32 == 16 and t['plane'].data_ptr() % 32 == 16
    assert t['f'].data_ptr() % 16 == 8 and t['own'].data_ptr() % 16 == 8
    assert t['i'].data_ptr() % 8 == 4
    for name, x in t.items():
        e = arena.entries[name]
        assert x.is_contiguous() and not x.any() and tuple(x.shape) == e['shape']
        need = max(4096, int(np.prod(e['shape'][-2:])) * x.element_size())
        assert e['lo'] - e['before'] >= need and e['after'] - e['hi'] >= need
    assert guarded.guard_bytes((2, 40, 16), 16) == 40 * 16 * 16 > 4096
    e = arena.entries['i']
    assert not arena.buf[e['before']:e['lo']].any() and not arena.buf[e['hi']:e['after']].any()
    for name in ('c', 'f', 'plane', 'own'):
        e = arena.entries[name]
        for lo, hi in ((e['before'], e['lo']), (e['hi'], e['after'])):
            words = arena.buf[lo:hi].view(torch.float64)
            assert torch.isnan(words).all() and bytes(arena.buf[lo:lo + 8].tolist()) == guarded.GUARD_BYTES
    # a NaN as a double whichever 32-bit half comes first
    assert np.isnan(np.frombuffer(guarded.GUARD_BYTES[4:] + guarded.GUARD_BYTES[:4], dtype='<f8'))[0]


def test_checker_names_tensor_side_offset_and_step():
    arena, t = _cpu_arena()
    assert arena.verify('clean') is None
    # a write before and behind a tensor
    e = arena.entries['plane']
    arena.buf[e['lo'] - 16] ^= 1
    with pytest.raises(GuardViolation) as err:
        arena.verify('step 3')
    assert 'step 3' in str(err.value) and 'the guard before plane' in str(err.value)
    assert 'byte offset %d ' % (e['lo'] - 16 - e['before']) in str(err.value)
    arena.buf[e['lo'] - 16] ^= 1
    assert arena.verify('restored') is None
    arena.buf[e['hi'] + 40] = 0
    with pytest.raises(GuardViolation) as err:
        arena.verify('step 4', outputs=['plane'])
    assert 'step 4' in str(err.value) and 'the guard after plane' in str(err.value) and 'byte offset 40 ' in str(err.value)
    arena.buf[e['hi'] + 40] = guarded.GUARD_BYTES[0]
    # one row past a [K][nt][N] store lands in the guard, whatever the row
    assert e['after'] - e['hi'] >= 40 * 16 * 16
    # the zero guard of an index array
    arena.buf[arena.entries['i']['hi'] + 4] = 1
    with pytest.raises(GuardViolation) as err:
        arena.verify('step 5')
    assert 'the guard after i' in str(err.value) and 'byte offset 4 ' in str(err.value)
    arena.buf[arena.entries['i']['hi'] + 4] = 0
    # one element of an input; an output and the engine's own buffer may change
    t['plane'][1, 2, 3] = 1.5
    t['own'][2] = 4.0
    assert arena.verify('an output', outputs=['plane']) is None
    t['plane'][1, 39, 15] = 2.5
    assert arena.verify('a slice of an output', outputs=[t['plane'][1:2]]) is None
    t['plane'][0, 0, 1] = 1.0 / 3.0  # (every byte of it non-zero)
    with pytest.raises(GuardViolation) as err:
        arena.verify('step 6', outputs=[t['plane'][1:2]])
    assert 'plane, which is no output of this call' in str(err.value) and 'byte offset 16 ' in str(err.value)
    arena.snapshot()
    assert arena.verify('after a snapshot') is None
    t['f'][3] = -1.0 / 3.0
    with pytest.raises(GuardViolation) as err:
        arena.verify('step 7', outputs=['plane'])
    assert 'step 7' in str(err.value) and 'f, which is no output' in str(err.value) and 'byte offset 24 ' in str(err.value)
    # a snapshot never takes a damaged guard for the pattern
    t['f'][3] = 0.0
    arena.buf[arena.entries['c']['hi']] = 0
    arena.snapshot()
    with pytest.raises(GuardViolation):
        arena.verify('step 8')


def _engines_of_the_tables():
    """(name, K, N, L, nt, replicas, operator lists) of every engine the GPU tests below create."""
    import test_replicas as tr

    for name, c in list(ter.CASES.items()) + list(ter.GRAPH_CASES.items()):
        p = ter.inputs(c.prob)[0]
        fmt = ter.PROBLEMS[c.prob].fmt
        spec = p.spec
        yield name, spec.K, max(getattr(spec, 'dims', None) or [spec.N]), spec.L, len(spec.tlist), 0, _engine_ops(spec, fmt), None
    case_ = ter.lindblad_inputs()[0]
    yield 'lindblad_form', case_.K, case_.d ** 2, case_.L, len(case_.dt) + 1, 0, case_.H, case_.C
    reps = list(tr.batch(ter.REPLICAS)[:3])
    arrays = tr._inputs(reps)
    yield 'replicas', len(arrays['ops']), reps[0].N, reps[0].L, len(reps[0].tlist), len(reps), arrays['ops'], None
    for name in PAR_SWEEPS:
        spec = tp.SWEEPS[name]['build']()
        yield name, spec.K, spec.N, spec.L, len(spec.tlist), 0, _engine_ops(spec, tp.SWEEPS[name]['fmt']), None


def test_guards_meet_the_condition_for_every_tensor_of_every_case():
    """The layout of every engine of the tables, built on the host: every tensor minimally aligned, between guards of at
    least max(4096 B, its trailing-two-dimensions plane) -- and all of it inside the arena a ``GuardedEngine`` allocates,
    with the headroom left."""
    import torch

    largest = 0
    for name, K, N, L, nt, B, ops, c_ops in _engines_of_the_tables():
        uploads, own = guarded.upload_shapes(list(ops) + list(c_ops or [])), guarded.own_shapes(K, N, L, nt)
        nbytes = guarded.engine_arena_bytes(ops, np.zeros(nt - 1), c_ops, B)
        stub = types.SimpleNamespace(K=K, N=N, L=L, nt=nt, device=torch.device('cpu'), arena=GuardedArena('cpu', nbytes))
        for i, (shape, dtype) in enumerate(uploads + own):
            stub.arena.carve('engine%d' % i, shape, dtype, 'input' if i < len(uploads) else 'scratch')
        extra = {x: ((L, nt - 1), torch.float64) for x in ('u_guess', 'dfdu', 'u_opt')}
        dev = GuardedDevice(stub, B=B, extra=extra)
        assert dev.arena.check_layout() and len(dev.arena.entries) == len(uploads) + len(own) + 15 + 3, name
        assert dev.arena.verify(name) is None
        assert dev.arena.cursor + guarded.HEADROOM <= nbytes, (name, dev.arena.cursor, nbytes)
        largest = max(largest, nbytes)
    print('largest arena: %.1f MiB' % (largest / 2.0 ** 20))


def test_dev_hands_a_carved_view_to_the_kernels_unchanged():
    """``HipKrotovEngine.dev`` (every ``_c`` / ``_f``) returns a carved view itself: the kernels see the arena's
    addresses; what is not contiguous, of another dtype or a host array is staged."""
    import torch

    arena, t = _cpu_arena()
    eng = types.SimpleNamespace(device=torch.device('cpu'))
    assert HipKrotovEngine.dev(eng, t['c'], torch.complex128) is t['c']
    assert HipKrotovEngine.dev(eng, t['f'], torch.float64) is t['f']
    eng.dev = lambda x, dtype: HipKrotovEngine.dev(eng, x, dtype)
    assert HipKrotovEngine._c(eng, t['plane'], (2, 40, 16)) is t['plane']
    assert HipKrotovEngine._f(eng, t['own'], (6,)) is t['own']
    assert HipKrotovEngine._out(eng, t['plane'], (2, 40, 16), torch.complex128) is t['plane']
    strided = t['plane'][:, :, ::2]
    staged = HipKrotovEngine.dev(eng, strided, torch.complex128)
    assert staged is not strided and staged.is_contiguous() and torch.equal(staged, strided)
    with pytest.raises(ValueError):
        HipKrotovEngine._c(eng, t['plane'], (2, 16, 40))
    with pytest.raises(ValueError):
        HipKrotovEngine._out(eng, strided, (2, 40, 8), torch.complex128)


# ---------------------------------------------------------------------------
# GPU: the harness of tests/test_engine_reuse.py on the arena
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(ter.CASES))
def test_sweeps_on_guarded_buffers(name, monkeypatch):
    ter.run_sequence(name, ter.CASES[name], monkeypatch, device_cls=GuardedDevice, engine_cls=GuardedEngine)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(ter.GRAPH_CASES))
def test_captured_graph_on_guarded_buffers(name, monkeypatch):
    ter.test_captured_graph_reused_with_changed_inputs(name, monkeypatch, device_cls=GuardedDevice, engine_cls=GuardedEngine)


@pytest.mark.gpu
def test_lindblad_engine_on_guarded_buffers():
    """(the refusals of the per-interval form, second order and a reduced grid are verified like every sweep: the arena
    is untouched after them)"""
    ter.test_lindblad_engine_reused_with_changed_inputs(device_cls=GuardedDevice, engine_cls=GuardedEngine)


@pytest.mark.gpu
def test_replica_engine_on_guarded_buffers():
    """First and second order, with the mask: an inactive replica's slices of every output are no outputs."""
    ter.test_replica_engine_reused_with_changed_inputs_and_mask(device_cls=GuardedDevice, engine_cls=GuardedEngine)


# ---------------------------------------------------------------------------
# GPU: parametrized sweeps (tests/test_parametrization.py: SWEEPS, against its restatement)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', PAR_SWEEPS)
def test_parametrized_sweep_on_guarded_buffers(name, monkeypatch):
    """``u_guess``, ``dfdu`` and ``u_opt`` carved too; the inputs of ``test_parametrization._run_sweep``."""
    import torch

    from krotov_amd import _lib

    case = tp.SWEEPS[name]
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    spec = case['build']()
    prob, gp, S, lam = pc.oracle_side(spec)
    rng = np.random.default_rng(17)
    nt, L, kinds = len(prob.tlist), len(gp), case['kinds']
    tol = TOL_LIOUVILLE if prob.is_super else TOL_HILBERT
    eng = GuardedEngine(_engine_ops(spec, case['fmt']), np.diff(spec.tlist), is_super=spec.is_super)
    try:
        if case['kernel'] is not None:
            assert eng.kernel == case['kernel'], eng.kernel
        dev = GuardedDevice(eng, extra={x: ((L, nt - 1), torch.float64) for x in ('u_guess', 'dfdu', 'u_opt')})
        t = dev.t
        chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
        norms = (0.2 + rng.random(prob.K)) * min(1.0, 8.0 / prob.K)
        dev.put(types.SimpleNamespace(prob=types.SimpleNamespace(init=spec.init), gp=np.array(gp), S=np.array(S), lam=np.array(lam),
                                      norms=norms, chi_T=chi_T))
        ref_chi = ko.backward_sweep(prob, chi_T, gp)
        errs = dict(chi=np.abs(dev.backward() - ref_chi).max())
        kind, a, b, u_guess, dfdu = tp._device_arrays(kinds, gp)
        dev.put_extra(u_guess=u_guess, dfdu=dfdu)
        kw = {}
        if case['so']:
            older = [p * (1.0 + 0.1 * rng.standard_normal(p.shape)) for p in gp]
            _, prev = ko.forward_propagation(prob, older, store=True)
            sigma_vals = -(1.0 + rng.random(nt - 1)) * min(1.0, 8.0 / prob.K)
            kw = dict(sigma_vals=sigma_vals, fw_prev=prev, store=True)
            dev.put_second_order(prev, sigma_vals)
            eng.set_second_order(t['prev'], t['store'], t['sigma'])
            dev.second_order = True
        eng.set_parametrization(kind, a, b, t['u_guess'], t['dfdu'], t['u_opt'])
        assert eng._par[0] is t['u_guess'] and eng._par[1] is t['dfdu'] and eng._par[2] is t['u_opt']
        dev.update_outputs = ('u_opt',)
        dev.nan('u_opt')
        _lib.forget_launched_kernels()
        if case['mode'] == 'stepwise':
            got = dev.sharded(0) + ((dev.host('store')[0],) if case['so'] else ())
        else:
            got = dev.update()
        launched = _lib.kernel_instantiations(launched_only=True)
        ref = pc.update_sweep(prob, ref_chi, norms, list(u_guess), kinds, S, lam, **kw)
        rel = lambda x, y: np.abs(x - np.array(y)).max() / max(1.0, np.abs(np.array(y)).max())  # noqa: E731
        errs.update(opt=rel(got[0], ref[0]), u=rel(dev.host('u_opt')[0], ref[1]), psi_T=np.abs(got[1] - ref[2]).max(),
                    g_a=rel(got[2], ref[3]))
        if case['so']:
            errs['fw_store'] = np.abs(got[3] - ref[4]).max()
        _check(errs, tol, name, 'parametrized sweep')
        for want in case['expect']:
            assert want in launched, (want, launched)
        # off again: the plain sweep writes no u_opt any more
        eng.set_parametrization()
        dev.update_outputs = ()
        if case['so']:
            eng.set_second_order()
            dev.second_order = False
        dev.update()
        assert dev.unchanged()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# GPU: the small kernels
# ---------------------------------------------------------------------------
def _small_engine(K, N):
    rng = np.random.default_rng(100 * K + N)
    H = [configs.herm(rng, N, 1.0) for _ in range(K)]
    Hc = configs.herm(rng, N, 0.5)
    return GuardedEngine([[H[k], Hc] for k in range(K)], np.full(4, 0.1)), rng


def _rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.gpu
@pytest.mark.parametrize('K,N', SMALL)
def test_tau_and_chi_boundary_on_guarded_buffers(K, N):
    """``kh_tau`` against ``numpy.vdot``, ``kh_chi_boundary`` against (c target + d psi) / ||.|| (the host form of
    tests/test_hip_parity.py), inputs and results in the arena; a strided view is staged."""
    import torch

    eng, rng = _small_engine(K, N)
    try:
        arena = eng.arena
        c128 = torch.complex128
        t = dict(targets=arena.carve('targets', (K, N), c128), psi_T=arena.carve('psi_T', (K, N), c128),
                 c=arena.carve('c', (K,), c128), d=arena.carve('d', (K,), c128), wide=arena.carve('wide', (K, 2 * N), c128))
        host = dict(targets=_rand(rng, K, N), psi_T=_rand(rng, K, N), c=_rand(rng, K), d=_rand(rng, K))
        for name, x in host.items():
            t[name].copy_(torch.from_numpy(x))
        t['wide'][:, ::2] = t['psi_T']
        arena.check_layout()
        arena.snapshot()
        tau = eng.tau(t['targets'], t['psi_T'])
        chi, norms = eng.chi_boundary(t['targets'], t['psi_T'], t['c'], t['d'])
        tau_strided = eng.tau(t['targets'], t['wide'][:, ::2])
        torch.cuda.synchronize()
        arena.verify('tau, chi_boundary')
        for x in (tau, chi, norms):  # (the results are the engine's: in the arena, between guards)
            assert arena._where(x.data_ptr() - arena.base)[1] == 'inside'
        want_tau = np.array([np.vdot(host['targets'][k], host['psi_T'][k]) for k in range(K)])
        v = host['c'][:, None] * host['targets'] + host['d'][:, None] * host['psi_T']
        want_norms = np.linalg.norm(v, axis=1)
        scale = max(1.0, np.abs(want_tau).max())
        _check(dict(tau=np.abs(tau.cpu().numpy() - want_tau).max() / scale,
                    tau_strided=np.abs(tau_strided.cpu().numpy() - want_tau).max() / scale,
                    chi=np.abs(chi.cpu().numpy() - v / want_norms[:, None]).max(),
                    norms=np.abs(norms.cpu().numpy() - want_norms).max() / max(1.0, want_norms.max())),
               TOL_HILBERT, 'K%d_N%d' % (K, N), 'tau, chi_boundary')
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('liouville', [False, True])
def test_expect_on_guarded_buffers(liouville):
    """``kh_expect`` on the Hilbert (N = 17) and the Liouville (d = 4) store of ``test_propagate_batch.test_guarded_store``
    (here nt = 9), against its NumPy form and bound; states, operators and ``out`` in the arena."""
    import torch

    import test_propagate_batch as tpb
    from helpers import oracle_controls

    K, nt, n_e = 3, 9, 3
    if liouville:
        spec = configs.config_sparse_lindblad(d=4, nt=nt, K=1)
        eng = GuardedEngine([[spec.H0[0], spec.Hc[0][0]]] * K, np.diff(spec.tlist), is_super=True)
        side, tol = 4, TOL_LIOUVILLE
    else:
        spec = configs.config_c5(K=K, N=17, nt=nt, distinct=True)
        eng = GuardedEngine([[spec.H0[k]] + list(spec.Hc[k]) for k in range(K)], np.diff(spec.tlist))
        side, tol = 17, TOL_HILBERT
    try:
        rng = np.random.default_rng(side)
        dev = GuardedDevice(eng)
        init = tpb._rand(rng, K, eng.N)
        init /= np.linalg.norm(init, axis=1)[:, None] * (side if liouville else 1.0)
        dev.put(types.SimpleNamespace(prob=types.SimpleNamespace(init=init), gp=np.array(oracle_controls(spec)[0]),
                                      S=np.ones((eng.L, nt - 1)), lam=np.ones(eng.L), norms=np.ones(K), chi_T=init))
        _, host = dev.forward()
        out = eng.arena.carve('expect_out', (n_e, K, nt), torch.complex128, 'output')
        out.fill_(complex(float('nan'), float('nan')))
        eng.arena.snapshot()
        ops = tpb._operators(rng, side, n_e)
        assert eng.expect(dev.t['states'], ops, out=out) is out
        torch.cuda.synchronize()
        eng.arena.verify('expect', outputs=[out])
        got = out.cpu().numpy()
        for e, op in enumerate(ops):
            err, bound = np.abs(got[e] - tpb._want(op, host, liouville)).max(), tpb._bound(op, host, tol)
            print('expect side %d op %d: err %.3e (bound %.3e)' % (side, e, err, bound))
            assert err <= bound
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# GPU: what the Python layer refuses before anything is launched
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.no_oracle
def test_python_boundary_refuses_before_a_launch():
    """``backward(out=)`` and ``set_second_order(fw_store=)`` -- buffers the kernels write in place -- raise ``ValueError``
    for a wrong shape, dtype or device and for a view that is not contiguous; ``tau`` and ``chi_boundary`` for a wrong
    shape (every other input of theirs is staged).  Nothing is launched and the arena is untouched."""
    import torch

    from krotov_amd import _lib

    K, N = 3, 9
    eng, rng = _small_engine(K, N)
    try:
        dev = GuardedDevice(eng)
        t, nt = dev.t, eng.nt
        c128 = torch.complex128
        wide = eng.arena.carve('wide', (K, nt, 2 * N), c128, 'output')
        eng.arena.snapshot()
        torch.cuda.synchronize()
        _lib.forget_launched_kernels()
        bad = dict(shape=torch.zeros((K, nt + 1, N), dtype=c128, device=eng.device),
                   transposed=torch.zeros((nt, K, N), dtype=c128, device=eng.device),
                   dtype=torch.zeros((K, nt, N), dtype=torch.complex64, device=eng.device),
                   real=torch.zeros((K, nt, N), dtype=torch.float64, device=eng.device),
                   device=torch.zeros((K, nt, N), dtype=c128), strided=wide[:, :, ::2], numpy=np.zeros((K, nt, N), dtype=complex))
        assert tuple(bad['strided'].shape) == (K, nt, N) and not bad['strided'].is_contiguous()
        for why, x in bad.items():
            with pytest.raises(ValueError):
                eng.backward(t['chi_T'], t['gp'], out=x)
            with pytest.raises(ValueError):
                eng.set_second_order(t['prev'], x, t['sigma'])
            assert getattr(eng, '_so', None) is None, why
        for shape in ((K, N + 1), (K + 1, N), (N, K), (K * N,)):
            x = torch.zeros(shape, dtype=c128, device=eng.device)
            with pytest.raises(ValueError):
                eng.tau(x, t['psi_T'])
            with pytest.raises(ValueError):
                eng.tau(t['chi_T'], x)
            with pytest.raises(ValueError):
                eng.chi_boundary(x, t['psi_T'], t['norms'], t['norms'])
            with pytest.raises(ValueError):
                eng.chi_boundary(t['chi_T'], x, t['norms'], t['norms'])
        for n in (K - 1, K + 1):
            with pytest.raises(ValueError):
                eng.chi_boundary(t['chi_T'], t['psi_T'], np.zeros(n), np.zeros(K))
            with pytest.raises(ValueError):
                eng.chi_boundary(t['chi_T'], t['psi_T'], np.zeros(K), np.zeros(n))
        torch.cuda.synchronize()
        assert list(_lib.kernel_instantiations(launched_only=True)) == []
        eng.arena.verify('after the refusals')
        assert not np.isnan(wide.cpu().numpy()).any()
    finally:
        eng.close()
