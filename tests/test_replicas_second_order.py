"""The second-order update of replica engines (``kh_set_second_order_replicas``, ``kh_rep_forward_update_so<L>``,
krotov_amd/csrc/kh_replica.h) and ``optimize_pulses_batch(..., sigma=[...])`` on the GPU.

Tolerances are the project's own (tests/test_replicas.py): 1e-12 against the oracle in Hilbert space, 1e-11 in Liouville
space; pulses and g_a relative to max(1, max|.|).  The protocol-free properties (a replica's result depends neither on
B, nor on its place in the batch, nor on the other replicas' sigma rows; repeatability; the active mask; the way back to
first order) are bitwise.  Reference: optimize.py:434-443, 451-452, 468-469, 492-500 (the sigma term), :566-577
(``sigma.refresh``)."""
import copy
import functools

import numpy as np
import pytest

import helpers
from helpers import SigmaA, product_sigma, spec_to_oracle  # noqa: F401  (SigmaA: the oracle-side form of product_sigma)
from krotov_amd import configs
from oracle import krotov_oracle as ko
from test_replicas import TOL_HILBERT, TOL_LIOUVILLE, _c5, _close, _inputs, _problems, _replica, _tls, batch

B = 3


@functools.lru_cache(maxsize=None)
def so_batch(name):
    """Three replicas of a batch of tests/test_replicas.py.  Between them: N = 2 and K_r = 1 (`tls`), N not a multiple
    of 4 (5, 7), N = 16 (`L1_full`, `L4`), K_r = 8 (`L1_full`), Liouville space, per-replica non-uniform dt (`regimes`),
    a control absent from one objective (`L4`), L = 1 ... 4."""
    if name == 'L3':  # (two replicas there)
        return list(batch('L3')) + [_replica(_c5(2, 3, 4, 9, L=3, seed0=30), 2)]
    if name == 'tls':
        # the two-level problems of `many` on seven grid points: on five, the update shape of the third is non-zero on
        # one interval only, and the sigma term -- zero on the first interval that is updated -- never shows
        return [_replica(_tls(j, nt=7), j) for j in range(B)]
    if name == 'regimes':  # (not the replica scaled by 1e-7, whose sigma term is below 1e-6)
        return list(batch(name)[1:1 + B])
    return list(batch(name)[:B])


SO_CASES = {'L1_small': 1, 'L1_full': 1, 'L2': 2, 'L3': 3, 'L4': 4, 'liouville': 1, 'tls': 1, 'regimes': 2}


def sigma_rows(reps, seed=17):
    """One row per replica, all different; the conditioning of tests/test_instantiations.py."""
    rng = np.random.default_rng(seed)
    return -(1.0 + rng.random((len(reps), len(reps[0].tlist) - 1))) * min(1.0, 8.0 / reps[0].K)


@functools.lru_cache(maxsize=None)
def oracle_so(name, b):
    """(first-order opt, (opt, psi_T, g_a, fw_store)) of replica b through the oracle, fw_prev being the trajectory
    under the guess (computed once)."""
    reps = so_batch(name)
    r, sig = reps[b], sigma_rows(reps)[b]
    prob = spec_to_oracle(r)
    chi_T = r.target / np.linalg.norm(r.target, axis=1)[:, None]
    with helpers.MemoExpm():
        _, prev = ko.forward_propagation(prob, r.pulses, store=True)
        chi = ko.backward_sweep(prob, chi_T, r.pulses)
        first = ko.forward_update_sweep(prob, chi, r.chi_norms, r.pulses, r.shapes, r.lambdas)[0]
        so = ko.forward_update_sweep(prob, chi, r.chi_norms, r.pulses, r.shapes, r.lambdas, sigma_vals=sig, fw_prev=prev,
                                     store=True)
    return first, so


def _nans(shape, dtype):
    import torch

    fill = complex(float('nan'), float('nan')) if dtype == torch.complex128 else float('nan')
    return torch.full(shape, fill, dtype=dtype, device='cuda')


def run_so(reps, sigma, mask=None, nan_outputs=False, first_order_too=False, then_first_order=False, tol=0.0):
    """Forward sweep with storage (fw_prev), backward sweep and second-order update sweep of a replica engine over
    `reps`.  Host arrays: dict(opt, psi_T, g_a, fw_store, init[, first: (opt, psi_T, g_a) of the first-order sweep run
    before][, back: the same of a first-order sweep run after three NULLs])."""
    import torch

    from krotov_amd.engine import HipKrotovEngine

    a = _inputs(reps)
    nB, Kr, N, L, nt = len(reps), reps[0].K, reps[0].N, reps[0].L, len(reps[0].tlist)
    eng = HipKrotovEngine(a['ops'], a['dt'], is_super=reps[0].is_super, replicas=nB, tol=tol)
    try:
        assert eng.kernel == 'replica16/wave'
        if mask is not None:
            eng.set_active_replicas(mask)
        new = _nans if nan_outputs else (lambda shape, dtype: torch.zeros(shape, dtype=dtype, device='cuda'))
        c128, f64 = torch.complex128, torch.float64
        psi0, prev = eng.forward(a['pulses'], a['init'], store=True, out=(new((nB * Kr, N), c128), new((nB * Kr, nt, N), c128)))
        chi = eng.backward(a['chi_T'], a['pulses'], out=new((nB * Kr, nt, N), c128))
        args = (chi, a['chi_norms'], a['init'], a['pulses'], a['shapes'], a['lambdas'])
        got = dict(init=a['init'])
        if first_order_too:
            got['first'] = tuple(x.cpu().numpy() for x in eng.forward_update(*args))
        store = new((nB * Kr, nt, N), c128)
        eng.set_second_order_replicas(prev, store, sigma)
        assert eng.replica_occupancy() >= 1
        opt, psi_T, g_a = eng.forward_update(*args, out=(new((nB, L, nt - 1), f64), new((nB * Kr, N), c128), new((nB, L), f64)))
        eng.check()
        got.update(opt=opt.cpu().numpy(), psi_T=psi_T.cpu().numpy(), g_a=g_a.cpu().numpy(), fw_store=store.cpu().numpy(),
                   stats=eng.stats())
        if then_first_order:
            eng.set_second_order_replicas()
            got['back'] = tuple(x.cpu().numpy() for x in eng.forward_update(*args))
            eng.check()
        return got
    finally:
        eng.close()


def _of_replica(got, b, Kr):
    rows = slice(b * Kr, (b + 1) * Kr)
    return got['opt'][b], got['psi_T'][rows], got['g_a'][b], got['fw_store'][rows]


def _bitwise(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


# ---------------------------------------------------------------------------
# 1. every second-order instantiation against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SO_CASES))
def test_second_order_replica_sweep_vs_oracle(name):
    from krotov_amd import _lib

    reps = so_batch(name)
    L, Kr, nt = SO_CASES[name], reps[0].K, len(reps[0].tlist)
    assert len(reps) == B and reps[0].L == L and 5 <= nt <= 12
    sig = sigma_rows(reps)
    assert not np.array_equal(sig[0], sig[1]) and not np.array_equal(sig[1], sig[2])
    _lib.load()
    _lib.forget_launched_kernels()
    got = run_so(reps, sig, first_order_too=True)
    launched = _lib.kernel_instantiations(launched_only=True)
    for want in ('kh_rep_sweep_store<%d>' % L, 'kh_rep_forward_update<%d>' % L, 'kh_rep_forward_update_so<%d>' % L):
        assert want in launched, (want, launched)
    tol = TOL_LIOUVILLE if reps[0].is_super else TOL_HILBERT
    for b in range(B):
        first, (ref_opt, ref_psi, ref_ga, ref_store) = oracle_so(name, b)
        opt, psi_T, g_a, store = _of_replica(got, b, Kr)
        scale = max(1.0, np.abs(np.array(ref_opt)).max())
        errs = dict(
            opt=np.abs(opt - np.array(ref_opt)).max() / scale,
            psi_T=np.abs(psi_T - ref_psi).max(),
            g_a=np.abs(g_a - ref_ga).max() / max(1.0, np.abs(ref_ga).max()),
            fw_store=np.abs(store - ref_store).max(),
        )
        off = np.abs(got['opt'][b] - got['first'][0][b]).max()
        print("%s replica %d: %s; second vs first order %.2e (oracle %.2e)" % (
            name, b, ", ".join("%s %.2e" % kv for kv in errs.items()), off, np.abs(np.array(ref_opt) - np.array(first)).max()))
        for what, err in errs.items():
            assert err < tol, (name, b, what, err)
        rows = slice(b * Kr, (b + 1) * Kr)
        assert np.array_equal(store[:, 0], got['init'][rows])  # bitwise
        assert np.array_equal(store[:, nt - 1], psi_T)
        assert off > 1e-6  # the sigma term is really on
    assert got['stats']['matvecs'] > 0 and got['stats']['workgroups'] == B


# ---------------------------------------------------------------------------
# 2. a zero sigma row
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.no_oracle
@pytest.mark.parametrize('name', ['L1_small', 'L2'])
def test_zero_sigma_row_gives_the_first_order_sweep(name):
    """bra = fma(0, phi - phi_prev, chi) = chi: the replica whose row is zero gets the first-order kernel's numbers
    (asserted to 1e-14 relative; printed whether bitwise)."""
    reps = so_batch(name)
    Kr = reps[0].K
    sig = sigma_rows(reps)
    sig[1] = 0.0
    got = run_so(reps, sig, first_order_too=True)
    rows = slice(Kr, 2 * Kr)
    pairs = ((got['opt'][1], got['first'][0][1]), (got['psi_T'][rows], got['first'][1][rows]), (got['g_a'][1], got['first'][2][1]))
    print("%s: zero sigma row bitwise equal to first order: %s" % (name, all(np.array_equal(x, y) for x, y in pairs)))
    for x, y in pairs:
        assert np.abs(x - y).max() <= 1e-14 * max(1.0, np.abs(y).max())
    assert np.abs(got['opt'][0] - got['first'][0][0]).max() > 1e-6  # (the other rows are on)


# ---------------------------------------------------------------------------
# 3. independence, 4. the active mask (bitwise; no oracle involved)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.no_oracle
@pytest.mark.parametrize('name', ['L1_small', 'L4'])
def test_second_order_replica_is_independent_of_its_batch(name):
    reps = so_batch(name)
    Kr = reps[0].K
    sig = sigma_rows(reps)
    whole, again = run_so(reps, sig), run_so(reps, sig)
    for key in ('opt', 'psi_T', 'g_a', 'fw_store'):
        assert np.array_equal(whole[key], again[key]), key
    alone = run_so([reps[1]], sig[1:2])
    assert _bitwise(_of_replica(alone, 0, Kr), _of_replica(whole, 1, Kr))
    other = sigma_rows(reps, seed=99)
    other[1] = sig[1]
    changed = run_so(reps, other)
    assert _bitwise(_of_replica(changed, 1, Kr), _of_replica(whole, 1, Kr))
    assert not np.array_equal(changed['opt'][0], whole['opt'][0])


@pytest.mark.gpu
@pytest.mark.no_oracle
@pytest.mark.parametrize('name', ['L1_small', 'L2'])
def test_inactive_second_order_replica_is_left_untouched(name):
    reps = so_batch(name)
    Kr = reps[0].K
    sig = sigma_rows(reps)
    full = run_so(reps, sig)
    masked = run_so(reps, sig, mask=[1, 0, 1], nan_outputs=True)
    for x in _of_replica(masked, 1, Kr):
        assert np.all(np.isnan(x.real)) and (not np.iscomplexobj(x) or np.all(np.isnan(x.imag)))
    for b in (0, 2):
        assert _bitwise(_of_replica(masked, b, Kr), _of_replica(full, b, Kr))


# ---------------------------------------------------------------------------
# 5. refusals and the way back to first order
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.no_oracle
def test_set_second_order_replicas_refusals_and_switching_back():
    import torch

    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    reps = so_batch('L2')
    a = _inputs(reps)
    K, nt, N = len(a['ops']), a['dt'].shape[1] + 1, reps[0].N
    store = torch.zeros((K, nt, N), dtype=torch.complex128, device='cuda')
    plain = HipKrotovEngine(a['ops'][:2], a['dt'][0])
    plain_store = torch.zeros((2, nt, N), dtype=torch.complex128, device='cuda')
    for call in (lambda: plain.set_second_order_replicas(plain_store, plain_store.clone(), np.zeros((1, nt - 1))),
                 lambda: plain.set_second_order_replicas()):
        with pytest.raises(_lib.KrotovHipError) as err:
            call()
        assert err.value.code == _lib.KH_ERR_UNSUPPORTED
    plain.close()
    eng = HipKrotovEngine(a['ops'], a['dt'], replicas=B)
    with pytest.raises(ValueError):
        eng.set_second_order_replicas(store, store.clone(), np.zeros(nt - 1))  # one row cannot describe B replicas
    with pytest.raises(ValueError):
        eng.set_second_order_replicas(store, None, np.zeros((B, nt - 1)))
    with pytest.raises(_lib.KrotovHipError) as err:
        eng.set_second_order_replicas(store, store, np.zeros((B, nt - 1)))  # fw_store aliases fw_prev
    assert err.value.code == _lib.KH_ERR_INVALID
    lib = _lib.load()
    assert lib.kh_set_second_order_replicas(eng._handle, store.data_ptr(), None, None) == _lib.KH_ERR_INVALID  # mixed
    with pytest.raises(_lib.KrotovHipError) as err:  # the single-row entry point keeps refusing a replica engine
        eng.set_second_order(store, store.clone(), np.zeros(nt - 1))
    assert err.value.code == _lib.KH_ERR_UNSUPPORTED
    eng.close()
    got = run_so(reps, sigma_rows(reps), first_order_too=True, then_first_order=True)
    assert _bitwise(got['back'], got['first'])
    assert not np.array_equal(got['opt'], got['first'][0])


# ---------------------------------------------------------------------------
# 6., 7. optimize_pulses_batch(sigma=)
# ---------------------------------------------------------------------------
def _c3_specs(nt):
    specs = [configs.config_c3(nt=nt) for _ in range(B)]
    for spec, lam in zip(specs, (10.0, 20.0, 40.0)):
        spec.lambda_a = lam
    return specs


def _sm_kw():
    import krotov_amd

    return dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_sm)


@pytest.mark.gpu
def test_second_order_batch_three_iterations_vs_loop_and_reference():
    """B = 3 problems of the config-3 system (notebook 07's Hamiltonian) under lambda_a = 10, 20, 40: every replica equals
    its own ``optimize_pulses(sigma=)`` run, the lambda_a = 20 one reproduces the reference's second-order loop
    (tests/golden/ref_so_c3.npz; the bounds of tests/test_hip_parity.py), and the hooks see the trajectories."""
    import krotov_amd
    from krotov_amd.engine import LAST_ENGINE

    g = helpers.golden('ref_so_c3')
    iters = int(g['iter_stop'])
    assert iters == 3
    specs = _c3_specs(201)
    problems = _problems(specs)
    own = {id(p['objectives']): b for b, p in enumerate(problems)}
    probe = {}

    def hook(**kw):
        if kw['iteration'] == 2:
            b = own[id(kw['objectives'])]
            probe[b] = dict(fw=np.array(kw['forward_states'][1][57]), fw0=np.array(kw['forward_states0'][1][57]),
                            len=(len(kw['forward_states']), len(kw['forward_states'][0])), sigma=kw['sigma'])

    sig_b = [product_sigma(0.0, 2.0) for _ in range(B)]
    results = krotov_amd.optimize_pulses_batch(problems, sigma=sig_b, iter_stop=iters, store_all_pulses=True, info_hook=hook,
                                               **_sm_kw())
    assert LAST_ENGINE().kernel == 'replica16/wave'
    sig_s = [product_sigma(0.0, 2.0) for _ in range(B)]
    loop = [krotov_amd.optimize_pulses(p['objectives'], p['pulse_options'], p['tlist'], sigma=s, iter_stop=iters,
                                       store_all_pulses=True, **_sm_kw()) for p, s in zip(problems, sig_s)]
    for b, (spec, res, seq, sb, ss) in enumerate(zip(specs, results, loop, sig_b, sig_s)):
        d_pulse = np.abs(np.array(res.all_pulses) - np.array(seq.all_pulses)).max() / max(1.0, np.abs(np.array(seq.all_pulses)).max())
        d_tau = np.abs(np.array(res.tau_vals) - np.array(seq.tau_vals)).max()
        d_A = np.abs(np.array(sb.history) - np.array(ss.history)).max() / max(1.0, np.abs(np.array(ss.history)).max())
        print("replica %d: pulses %.2e tau %.2e A %.2e (A = %s)" % (b, d_pulse, d_tau, d_A, sb.history))
        assert res.iters == seq.iters == [0, 1, 2, 3] and res.message == seq.message
        assert _close(res.all_pulses, seq.all_pulses, TOL_HILBERT) and _close(res.tau_vals, seq.tau_vals, TOL_HILBERT)
        assert _close(sb.history, ss.history, TOL_HILBERT)
        assert sb.calls == [(spec.K, len(spec.tlist), True)] * 2  # two refreshes with full trajectories
        assert probe[b]['sigma'] is sb and probe[b]['len'] == (spec.K, len(spec.tlist))
        # the trajectories handed to the hooks are those of iterations 2 and 1
        prob = spec_to_oracle(spec)
        got = np.array([np.array(p) for p in res.all_pulses])
        with helpers.MemoExpm():
            for key, pulses in (('fw', got[2]), ('fw0', got[1])):
                want = ko.forward_propagation(prob, [pulses[0]], store=True)[1][1, 57]
                assert np.abs(probe[b][key].reshape(-1) - want).max() < 1e-12
    got = np.array([np.array(p) for p in results[1].all_pulses])  # lambda_a = 20: the reference's own run
    assert np.abs(got - g['all_pulses']).max() < 1e-9
    assert np.abs(np.array(results[1].tau_vals) - g['tau_vals']).max() < 1e-9
    assert np.abs(np.array(sig_b[1].history) - g['A_history']).max() < 1e-8
    assert len({tuple(s.history) for s in sig_b}) == B  # every replica under its own sigma


@pytest.mark.gpu
def test_second_order_replica_stops_early_and_the_others_go_on():
    """Replica 1 of three stops after iteration 1; the others run to iteration 3 through two buffer swaps and still equal
    their solo runs; the stopped replica's Result is not touched again and holds nothing of the device."""
    import krotov_amd

    specs = _c3_specs(41)
    problems = _problems(specs)
    own = {id(p['objectives']): b for b, p in enumerate(problems)}

    def snapshot(res):
        return copy.deepcopy(dict(iters=res.iters, all_pulses=res.all_pulses, tau_vals=res.tau_vals, message=res.message,
                                  optimized_controls=res.optimized_controls, states=res.states))

    def checker(held):
        def check(result):
            b = own[id(result.objectives)]
            if b == 1 and result.iters[-1] >= 1:
                held['result'] = result
                return 'enough'
            if b == 2 and result.iters[-1] == 2 and 'result' in held:  # (a pass after replica 1 was finished)
                held['then'] = snapshot(held['result'])
            return None

        return check

    held = {}
    kw = dict(iter_stop=3, store_all_pulses=True, **_sm_kw())
    sig_b = [product_sigma(0.0, 2.0) for _ in range(B)]
    results = krotov_amd.optimize_pulses_batch(problems, sigma=sig_b, check_convergence=checker(held), **kw)
    sig_s = [product_sigma(0.0, 2.0) for _ in range(B)]
    loop = [krotov_amd.optimize_pulses(p['objectives'], p['pulse_options'], p['tlist'], sigma=s,
                                       check_convergence=checker({}), **kw) for p, s in zip(problems, sig_s)]
    assert [r.iters for r in results] == [[0, 1, 2, 3], [0, 1], [0, 1, 2, 3]]
    for res, seq, sb, ss in zip(results, loop, sig_b, sig_s):
        assert res.iters == seq.iters and res.message == seq.message
        assert _close(res.all_pulses, seq.all_pulses, TOL_HILBERT) and _close(res.tau_vals, seq.tau_vals, TOL_HILBERT)
        assert _close(res.optimized_controls, seq.optimized_controls, TOL_HILBERT)
        assert len(sb.history) == len(ss.history) == len(res.iters) - 2  # (no refresh behind a replica's last iteration)
        assert not sb.history or _close(sb.history, ss.history, TOL_HILBERT)
    stopped = results[1]
    assert held['result'] is stopped and 'Reached convergence' in stopped.message
    def same(x, y):
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        return np.array_equal(np.asarray(x), np.asarray(y))

    now = snapshot(stopped)
    for key, then in held['then'].items():
        assert same(then, now[key]), key
    assert type(stopped.states) is list
    for value in list(vars(stopped).values()) + list(stopped.states):
        assert not type(value).__module__.startswith('torch'), type(value)
