"""Batched propagation of objective lists (``krotov_amd.propagate_objectives``) and the device-side expectation values
behind it (``kh_expect`` / ``HipKrotovEngine.expect``, krotov_amd/csrc/kh_expect.h).

Every GPU comparison is against NumPy on host data: the kernel against ``einsum`` on the very store it read, the public
function against the per-objective host loop with the NumPy propagator of ``helpers.numpy_plugins()``.  Tolerances are
the project's: 1e-12 in Hilbert space, 1e-11 in Liouville space, relative to max(1, ||O||_F) max ||state||^2.
"""
import ctypes

import numpy as np
import pytest

from helpers import numpy_plugins, oracle_controls
from qobj_double import QobjDouble

import krotov_amd
from krotov_amd import _lib, configs

# the kernels' own sizes (krotov_amd/csrc/kh_expect.h), restated: time points per workgroup of the two forms, operators
# per pass
H_POINTS, L_POINTS, MAX_OPS = 256, 16, 8
NT_SET = (2, 17, 67, H_POINTS + 1)  # (17 = L_POINTS + 1)


def _rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _hermitian(rng, n):
    G = _rand(rng, n, n)
    return (G + G.conj().T) / 2


def _bound(op, states, tol):
    return tol * max(1.0, np.linalg.norm(op)) * float((np.abs(states) ** 2).sum(axis=-1).max())


# ---------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------


def test_kh_expect_validates_before_touching_the_device():
    lib = _lib.load()
    table = (ctypes.c_void_p * 1)()
    assert lib.kh_expect(None, None, table, 1, None, None) == -1
    assert lib.kh_last_error() != b''
    assert lib.kh_expect(None, None, None, 0, None, None) == -1


def _host_system(K=3, N=4, nt=9, seed=2):
    rng = np.random.default_rng(seed)
    H1 = _hermitian(rng, N) / 4
    eps = lambda t, args: 0.6 * np.cos(2 * t) + args.get('offset', 0.0)  # noqa: E731
    objectives = []
    for k in range(K):
        psi0 = _rand(rng, N)
        psi0 /= np.linalg.norm(psi0)
        objectives.append(krotov_amd.Objective(initial_state=psi0, target=psi0, H=[_hermitian(rng, N) / 2, [H1, eps]]))
    ops = [_hermitian(rng, N), _rand(rng, N, N)]
    return objectives, ops, np.linspace(0, 2, nt), rng


def _same_result(a, b):
    assert a.solver == b.solver and a.num_expect == b.num_expect and a.num_collapse == b.num_collapse
    assert np.array_equal(a.times, b.times)
    assert len(a.states) == len(b.states) and all(np.array_equal(x, y) for x, y in zip(a.states, b.states))
    assert len(a.expect) == len(b.expect)
    for x, y in zip(a.expect, b.expect):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def test_host_propagator_equals_the_per_objective_loop():
    prop, _, _ = numpy_plugins()
    objectives, ops, tlist, rng = _host_system()
    args = {'offset': 0.1}
    for e_ops in (None, ops):
        got = krotov_amd.propagate_objectives(objectives, tlist, propagator=prop, e_ops=e_ops, args=args)
        assert len(got) == len(objectives)
        for obj, res in zip(objectives, got):
            want = obj.propagate(tlist, propagator=prop, e_ops=e_ops, args=args)
            assert isinstance(res, krotov_amd.objectives.PropagationResult)
            _same_result(res, want)
    assert got[0].solver == 'propagator' and got[0].num_expect == 2 and len(got[0].states) == 0
    assert got[0].expect[0].dtype == np.float64 and got[0].expect[1].dtype == np.complex128
    # a single grid point (possible for an objective without controls): the initial state, no step
    drift_only = [krotov_amd.Objective(initial_state=obj.initial_state, target=None, H=[obj.H[0]]) for obj in objectives]
    for p in (prop, krotov_amd.propagators.expm):  # (the device propagator too: the per-objective loop, no engine)
        one = krotov_amd.propagate_objectives(drift_only, tlist[:1], propagator=p)
        assert [len(r.states) for r in one] == [1] * len(objectives) and one[1].states[0] is objectives[1].initial_state


def test_per_objective_e_ops_and_initial_states_are_honoured():
    prop, _, _ = numpy_plugins()
    objectives, ops, tlist, rng = _host_system()
    rows = [[ops[0]], [ops[1], ops[0]], []]
    starts = [_rand(rng, 4), None, _rand(rng, 4)]
    got = krotov_amd.propagate_objectives(objectives, tlist, propagator=prop, e_ops=rows, initial_states=starts)
    for k, obj in enumerate(objectives):
        _same_result(got[k], obj.propagate(tlist, propagator=prop, e_ops=rows[k], rho0=starts[k]))
    assert [r.num_expect for r in got] == [1, 2, 0] and len(got[2].states) == len(tlist)
    assert np.array_equal(got[2].states[0], starts[2]) and np.array_equal(got[1].states, [])
    with pytest.raises(ValueError):
        krotov_amd.propagate_objectives(objectives, tlist, propagator=prop, e_ops=rows[:2])
    with pytest.raises(ValueError):
        krotov_amd.propagate_objectives(objectives, tlist, propagator=prop, initial_states=starts[:2])


def test_custom_expect_callable_is_called():
    prop, _, _ = numpy_plugins()
    objectives, ops, tlist, _ = _host_system()
    calls = []

    def first_amplitude(oper, state):
        calls.append(oper)
        return complex(np.asarray(state).reshape(-1)[0])

    got = krotov_amd.propagate_objectives(objectives, tlist, propagator=prop, e_ops=ops[:1], expect=first_amplitude)
    assert len(calls) == len(objectives) * len(tlist) and all(c is ops[0] for c in calls)
    for obj, res in zip(objectives, got):
        want = obj.propagate(tlist, propagator=prop)
        assert np.array_equal(res.expect[0], np.array([s[0] for s in want.states]))


# ---------------------------------------------------------------------------
# GPU 1-3: the kernels against NumPy on the same stored states
# ---------------------------------------------------------------------------


def _hilbert_store(N, nt, K=3):
    """Engine and stored trajectory of a ``config_c5`` problem with per-objective drifts (the real store)."""
    import torch
    from krotov_amd.engine import HipKrotovEngine

    spec = configs.config_c5(K=K, N=N, nt=nt, distinct=True)
    eng = HipKrotovEngine([[spec.H0[k]] + list(spec.Hc[k]) for k in range(K)], np.diff(spec.tlist))
    rng = np.random.default_rng(N * 1000 + nt)
    init = _rand(rng, K, N)
    init /= np.linalg.norm(init, axis=1)[:, None]
    _, states = eng.forward(np.array(oracle_controls(spec)[0]), init, store=True)
    torch.cuda.synchronize()
    return eng, states, rng


def _liouville_store(d, nt, K=3):
    """The same for ``config_sparse_lindblad`` Liouvillians (dense) on random NON-Hermitian rho."""
    import torch
    from krotov_amd.engine import HipKrotovEngine

    spec = configs.config_sparse_lindblad(d=d, nt=nt, K=1)
    eng = HipKrotovEngine([[spec.H0[0], spec.Hc[0][0]]] * K, np.diff(spec.tlist), is_super=True)
    rng = np.random.default_rng(d * 1000 + nt)
    init = _rand(rng, K, d * d) / d
    _, states = eng.forward(np.array(oracle_controls(spec)[0]), init, store=True)
    torch.cuda.synchronize()
    return eng, states, rng


def _operators(rng, n, count):
    """Hermitian, non-Hermitian complex, identity, then more random ones."""
    ops = [_hermitian(rng, n), _rand(rng, n, n), np.eye(n, dtype=complex)]
    return (ops + [_rand(rng, n, n) for _ in range(max(0, count - 3))])[:count]


def _want(op, host, liouville):
    if liouville:  # tr(O rho) with rho[j, i] = vec[j + d i]
        d = op.shape[0]
        rho = host.reshape(host.shape[:-1] + (d, d)).swapaxes(-1, -2)  # [..., row, column]
        return np.einsum('ij,...ji->...', op, rho)
    return np.einsum('...i,ij,...j->...', host.conj(), op, host)


def _check_expect(eng, states, rng, side, liouville, tol):
    host = states.cpu().numpy()
    K = host.shape[0]
    for n_e in (1, 3, MAX_OPS + 1):
        ops = _operators(rng, side, n_e)
        got = eng.expect(states, ops).cpu().numpy()
        assert got.shape == (n_e, K, host.shape[1]) and got.dtype == np.complex128
        for e, op in enumerate(ops):
            want = _want(op, host, liouville)
            err = np.abs(got[e] - want).max()
            print("side %d nt %d n_e %d op %d: err %.3e (bound %.3e)" % (side, host.shape[1], n_e, e, err, _bound(op, host, tol)))
            assert np.abs(got[e].real - want.real).max() <= _bound(op, host, tol)
            assert np.abs(got[e].imag - want.imag).max() <= _bound(op, host, tol)
    # the identity gives ||psi||^2 (Hilbert space) / the trace (Liouville space); a Hermitian operator a real value
    if not liouville:
        assert np.abs(eng.expect(states, [np.eye(side)]).cpu().numpy()[0].real
                      - (np.abs(host) ** 2).sum(axis=-1)).max() <= _bound(np.eye(side), host, tol)
        assert np.abs(eng.expect(states, [ops[0]]).cpu().numpy().imag).max() <= _bound(ops[0], host, tol)
    # per-objective tables: one shared pointer, one distinct per objective, one NULL entry
    shared, own = _rand(rng, side, side), [_rand(rng, side, side) for _ in range(K)]
    table = [[shared, own[k], None if k == 1 else own[0]] for k in range(K)]
    got = eng.expect(states, table).cpu().numpy()
    for k in range(K):
        for e, op in enumerate(table[k]):
            if op is None:
                assert np.all(got[e, k] == 0) and not np.signbit(got[e, k].real).any()
            else:
                assert np.abs(got[e, k] - _want(op, host[k], liouville)).max() <= _bound(op, host, tol)
    assert len(eng._expect_keep[1]) == 1 + K  # every distinct object uploaded once


@pytest.mark.gpu
@pytest.mark.parametrize('N', [5, 16, 17, 64, 81])
def test_hilbert_kernel_against_numpy(N):
    for nt in NT_SET:
        eng, states, rng = _hilbert_store(N, nt)
        _check_expect(eng, states, rng, N, False, 1e-12)
        eng.close()
    assert 'kh_expect_hilbert' in _lib.kernel_instantiations(launched_only=True)


@pytest.mark.gpu
@pytest.mark.parametrize('d', [2, 5, 9])
def test_liouville_kernel_against_numpy(d):
    for nt in NT_SET:
        eng, states, rng = _liouville_store(d, nt)
        _check_expect(eng, states, rng, d, True, 1e-11)
        eng.close()
    assert 'kh_expect_liouville' in _lib.kernel_instantiations(launched_only=True)


@pytest.mark.gpu
def test_wrong_shapes_and_mixed_engines_are_refused():
    import torch
    from krotov_amd.engine import HipKrotovEngine

    eng, states, rng = _hilbert_store(5, 17)
    for bad in ([np.eye(4)], [[np.eye(5)], [np.eye(5)]], [], [[np.eye(5)], [np.eye(5)], [np.eye(5), np.eye(5)]]):
        with pytest.raises(ValueError):
            eng.expect(states, bad)
    with pytest.raises(ValueError):
        eng.expect(states[:, :5], [np.eye(5)])
    eng.close()
    eng, states, rng = _liouville_store(2, 17)
    with pytest.raises(ValueError):
        eng.expect(states, [np.eye(4)])  # (d x d operators, not N x N)
    eng.close()
    spec = configs.config_mixed('dims', nt=11)
    eng = HipKrotovEngine([[spec.H0[k]] + list(spec.Hc[k]) for k in range(spec.K)], np.diff(spec.tlist), is_super=spec.kinds)
    assert eng.mixed
    states = torch.zeros((eng.K, eng.nt, eng.N), dtype=torch.complex128, device=eng.device)
    with pytest.raises(_lib.KrotovHipError) as err:
        eng.expect(states, [np.eye(eng.N)])
    assert err.value.code == _lib.KH_ERR_UNSUPPORTED
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('liouville', [False, True])
def test_guarded_store(liouville):
    """States as a contiguous slice in the middle of a NaN-filled tensor, ``out`` inside a tensor of sentinels: nothing
    outside the store is read into a result, nothing outside ``out`` is written.  N = 17 (d = 17 would be N = 289: the
    Liouville case takes d = 4, N = 16, next to the ragged Hilbert one), nt = 67."""
    import torch

    nt, n_e, K = 67, 3, 3
    eng, states, rng = _liouville_store(4, nt) if liouville else _hilbert_store(17, nt)
    side, tol = (4, 1e-11) if liouville else (17, 1e-12)
    big = torch.full((K + 2, nt, eng.N), float('nan'), dtype=torch.complex128, device=eng.device)
    big[1:K + 1] = states
    guarded = big[1:K + 1]
    assert guarded.is_contiguous() and guarded.data_ptr() != big.data_ptr()
    sentinel = complex(-7.25, 3.5)
    frame = torch.full((n_e + 2, K, nt), sentinel, dtype=torch.complex128, device=eng.device)
    out = frame[1:n_e + 1]
    ops = _operators(rng, side, n_e)
    assert eng.expect(guarded, ops, out=out).data_ptr() == out.data_ptr()
    got, host = frame.cpu().numpy(), states.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.all(got[0] == sentinel) and np.all(got[-1] == sentinel)
    for e, op in enumerate(ops):
        assert np.abs(got[1 + e] - _want(op, host, liouville)).max() <= _bound(op, host, tol)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('liouville', [False, True])
def test_bitwise_repeatability(liouville):
    eng, states, rng = _liouville_store(5, 67) if liouville else _hilbert_store(17, 67)
    ops = _operators(rng, 5 if liouville else 17, 3)
    a = eng.expect(states, ops).cpu().numpy()
    b = eng.expect(states, ops).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    eng.close()


# ---------------------------------------------------------------------------
# GPU 4: propagate_objectives end to end
# ---------------------------------------------------------------------------


def _five_objectives(seed=5, N=6, K=5):
    """The system of test_objective_propagate_on_device as a list: own drifts, one shared control."""
    rng = np.random.default_rng(seed)
    H1 = _hermitian(rng, N) / 4
    eps = lambda t, args: 0.7 * np.sin(3 * t) + 0.2  # noqa: E731
    drifts = [_hermitian(rng, N) / 2 for _ in range(K)]
    psi0 = np.zeros(N, dtype=complex)
    psi0[0] = 1.0
    P0 = np.zeros((N, N), dtype=complex)
    P0[0, 0] = 1.0
    A = _rand(rng, N, N)  # non-Hermitian
    return drifts, H1, eps, psi0, [P0, drifts[0], A], np.linspace(0, 4, 201)


def _launched_between(call):
    _lib.forget_launched_kernels()
    out = call()
    return out, _lib.kernel_instantiations(launched_only=True)


def _check_kinds(results, e_ops):
    for res in results:
        assert len(res.states) == 0 and len(res.expect) == len(e_ops)
        for vals, op in zip(res.expect, e_ops):
            herm = np.array_equal(np.asarray(op), np.asarray(op).conj().T)
            assert vals.dtype == (np.float64 if herm else np.complex128)


@pytest.mark.gpu
def test_end_to_end_hilbert_and_liouville():
    prop, _, _ = numpy_plugins()
    drifts, H1, eps, psi0, e_ops, tlist = _five_objectives()
    objectives = [krotov_amd.Objective(initial_state=psi0, target=psi0, H=[H0, [H1, eps]]) for H0 in drifts]
    host = [obj.propagate(tlist, propagator=prop, e_ops=e_ops) for obj in objectives]
    dev, launched = _launched_between(lambda: krotov_amd.propagate_objectives(
        objectives, tlist, propagator=krotov_amd.propagators.expm, e_ops=e_ops))
    assert 'kh_expect_hilbert' in launched and 'kh_expect_liouville' not in launched
    from krotov_amd.engine import LAST_ENGINE
    assert LAST_ENGINE().K == len(objectives)  # one engine for the list
    _check_kinds(dev, e_ops)
    for d, h in zip(dev, host):
        assert d.solver == 'expm' and d.num_expect == 3 and np.array_equal(d.times, tlist)
        for i, op in enumerate(e_ops):
            assert np.abs(d.expect[i] - h.expect[i]).max() < 1e-12 * max(1.0, np.linalg.norm(op))
    # no e_ops: the trajectories
    dev_s = krotov_amd.propagate_objectives(objectives, tlist, propagator=krotov_amd.propagators.expm)
    host_s = objectives[3].propagate(tlist, propagator=prop)
    assert len(dev_s[3].states) == len(tlist) and len(dev_s[3].expect) == 0
    assert max(np.abs(a - b).max() for a, b in zip(dev_s[3].states, host_s.states)) < 1e-12
    # the same systems as Liouvillians on density matrices
    L1 = krotov_amd.objectives.liouvillian(H1, [])
    rho0 = np.outer(psi0, psi0.conj())
    objectives_l = [krotov_amd.Objective(initial_state=rho0, target=rho0, H=[krotov_amd.objectives.liouvillian(H0, []), [L1, eps]])
                    for H0 in drifts]
    dev_l, launched = _launched_between(lambda: krotov_amd.propagate_objectives(
        objectives_l, tlist, propagator=krotov_amd.propagators.HipExpm(liouville=True), e_ops=e_ops))
    assert 'kh_expect_liouville' in launched and 'kh_expect_hilbert' not in launched
    _check_kinds(dev_l, e_ops)
    for d, h in zip(dev_l, host):
        for i, op in enumerate(e_ops):
            assert np.abs(d.expect[i] - h.expect[i]).max() < 1e-11 * max(1.0, np.linalg.norm(op))


@pytest.mark.gpu
def test_end_to_end_sparse_list():
    spec = configs.config_sparse_lindblad(d=6, nt=41, K=3)
    d = 6
    ops = configs.sparse_ops(spec)
    objectives = [krotov_amd.Objective(initial_state=spec.init[k].reshape(d, d, order='F'), target=None,
                                       H=[ops[k][0], [ops[k][1], spec.controls[0]]]) for k in range(spec.K)]
    rng = np.random.default_rng(8)
    e_ops = [np.diag(np.arange(d)).astype(complex), _rand(rng, d, d)]
    dev, launched = _launched_between(lambda: krotov_amd.propagate_objectives(
        objectives, spec.tlist, propagator=krotov_amd.propagators.DensityMatrixODEPropagator(), e_ops=e_ops))
    from krotov_amd.engine import LAST_ENGINE
    assert LAST_ENGINE().kernel.endswith('/csr') and 'kh_expect_liouville' in launched
    _check_kinds(dev, e_ops)
    prop, _, _ = numpy_plugins(is_super=True)
    for k in range(spec.K):
        dense = krotov_amd.Objective(initial_state=spec.init[k], target=None, H=[spec.H0[k], [spec.Hc[k][0], spec.controls[0]]])
        states = dense.propagate(spec.tlist, propagator=prop).states  # vec(rho), column-stacked
        for i, op in enumerate(e_ops):
            want = np.array([np.trace(op @ s.reshape(d, d, order='F')) for s in states])
            assert np.abs(dev[k].expect[i] - (want.real if i == 0 else want)).max() < 1e-11 * max(1.0, np.linalg.norm(op))


@pytest.mark.gpu
def test_end_to_end_lindblad_form():
    rng = np.random.default_rng(12)
    d = 7
    H0, H1 = configs.herm(rng, d, 2.0), configs.herm(rng, d, 1.0)
    C = 0.3 * _rand(rng, d, d) / np.sqrt(d)
    eps = lambda t, args: 0.5 * np.sin(2 * t) + 0.1  # noqa: E731
    tlist = np.linspace(0, 2, 67)
    rhos = []
    for _ in range(3):
        G = _rand(rng, d, d)
        rho = G @ G.conj().T
        rhos.append(rho / np.trace(rho).real)
    e_ops = [np.diag(np.arange(d)).astype(complex), _rand(rng, d, d)]
    lind = [krotov_amd.Objective(initial_state=rho, target=None, H=[H0, [H1, eps]], c_ops=[C]) for rho in rhos]
    dev, launched = _launched_between(lambda: krotov_amd.propagate_objectives(
        lind, tlist, propagator=krotov_amd.propagators.LindbladExpm(), e_ops=e_ops))
    from krotov_amd.engine import LAST_ENGINE
    assert LAST_ENGINE().kernel == 'lindblad/matrix' and 'kh_expect_liouville' in launched
    assert dev[0].num_collapse == 1
    _check_kinds(dev, e_ops)
    liou = [krotov_amd.Objective(initial_state=rho, target=None, H=krotov_amd.objectives.liouvillian([H0, [H1, eps]], [C]))
            for rho in rhos]
    ref = krotov_amd.propagate_objectives(liou, tlist, propagator=krotov_amd.propagators.HipExpm(liouville=True), e_ops=e_ops)
    # ... and the Liouvillian form against NumPy on the host
    prop, _, _ = numpy_plugins(is_super=True)
    for k in range(3):
        vec = krotov_amd.Objective(initial_state=rhos[k].ravel(order='F'), target=None, H=liou[k].H)
        states = vec.propagate(tlist, propagator=prop).states
        for i, op in enumerate(e_ops):
            want = np.array([np.trace(op @ s.reshape(d, d, order='F')) for s in states])
            bound = 1e-11 * max(1.0, np.linalg.norm(op))
            assert np.abs(ref[k].expect[i] - (want.real if i == 0 else want)).max() < bound
            assert np.abs(dev[k].expect[i] - ref[k].expect[i]).max() < bound


@pytest.mark.gpu
def test_end_to_end_mixed_list_is_evaluated_on_the_host():
    spec = configs.config_mixed('dims', nt=41)
    objectives, _ = configs.mixed_to_objectives(spec, krotov_amd)
    rng = np.random.default_rng(4)
    rows = []
    for k, obj in enumerate(objectives):
        n = np.asarray(obj.initial_state).shape[0]
        rows.append([_hermitian(rng, n), _rand(rng, n, n)])
    got, launched = _launched_between(lambda: krotov_amd.propagate_objectives(
        objectives, spec.tlist, propagator=krotov_amd.propagators.expm, e_ops=rows))
    from krotov_amd.engine import LAST_ENGINE
    assert LAST_ENGINE().kernel == 'generic/mixed' and not any(n.startswith('kh_expect') for n in launched)
    for k, obj in enumerate(objectives):
        prop, _, _ = numpy_plugins(is_super=spec.kinds[k])
        init = np.asarray(obj.initial_state)
        vec = krotov_amd.Objective(initial_state=init.ravel(order='F') if spec.kinds[k] else init, target=None, H=obj.H)
        states = vec.propagate(spec.tlist, propagator=prop).states
        n = init.shape[0]
        assert len(got[k].states) == 0 and got[k].expect[0].dtype == np.float64
        for i, op in enumerate(rows[k]):
            if spec.kinds[k]:
                want = np.array([np.trace(op @ s.reshape(n, n, order='F')) for s in states])
            else:
                want = np.array([np.vdot(s.reshape(-1), op @ s.reshape(-1)) for s in states])
            tol = 1e-11 if spec.kinds[k] else 1e-12
            assert np.abs(got[k].expect[i] - (want.real if i == 0 else want)).max() < tol * max(1.0, np.linalg.norm(op))


# ---------------------------------------------------------------------------
# GPU 5: Qobj-like inputs
# ---------------------------------------------------------------------------


@pytest.mark.gpu
def test_qobj_like_inputs():
    drifts, H1, eps, psi0, e_ops, tlist = _five_objectives(K=3)
    tlist = tlist[:41]
    arrays = [krotov_amd.Objective(initial_state=psi0.reshape(-1, 1), target=None, H=[H0, [H1, eps]]) for H0 in drifts]
    qH1 = QobjDouble(H1)
    qobjs = [krotov_amd.Objective(initial_state=QobjDouble(psi0.reshape(-1, 1)), target=None, H=[QobjDouble(H0), [qH1, eps]])
             for H0 in drifts]
    q_ops = [QobjDouble(op) for op in e_ops]
    a = krotov_amd.propagate_objectives(arrays, tlist, propagator=krotov_amd.propagators.expm, e_ops=e_ops)
    q = krotov_amd.propagate_objectives(qobjs, tlist, propagator=krotov_amd.propagators.expm, e_ops=q_ops)
    for ra, rq in zip(a, q):
        for x, y in zip(ra.expect, rq.expect):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    states = krotov_amd.propagate_objectives(qobjs, tlist, propagator=krotov_amd.propagators.expm)[1].states
    plain = krotov_amd.propagate_objectives(arrays, tlist, propagator=krotov_amd.propagators.expm)[1].states
    assert len(states) == len(tlist) and all(type(s) is QobjDouble and s.type == 'ket' for s in states)
    assert all(np.array_equal(s.full(), p) for s, p in zip(states, plain))
