"""Replica engines (``kh_engine_create_replicas``, kernel family ``"replica16/wave"``, krotov_amd/csrc/kh_replica.h) and
``krotov_amd.optimize_pulses_batch``: B independent small problems in one launch per sweep.

Tolerances are the project's own (tests/test_instantiations.py): 1e-12 against the oracle in Hilbert space, 1e-11 in
Liouville space; pulses and g_a relative to max(1, max|.|).  The protocol-free properties (a replica's result depends
neither on B nor on its place in the batch; repeatability; the active mask) are bitwise.  Reference: optimize.py:444-508
(update sweep), :849-886 (backward sweep), :392-581 (the driver's loop).
"""
import copy
import ctypes
import functools
import logging

import numpy as np
import pytest

import helpers
from helpers import spec_to_oracle
from krotov_amd import configs
from oracle import krotov_oracle as ko

TOL_HILBERT, TOL_LIOUVILLE = 1e-12, 1e-11


# ---------------------------------------------------------------------------
# batches: lists of replica problems (ProblemSpec with explicit pulses / shapes / lambdas and chi norms)
# ---------------------------------------------------------------------------
def _replica(spec, seed):
    r = helpers.explicit(spec, 'dense')
    r.chi_norms = 0.2 + np.random.default_rng(1000 + seed).random(r.K)
    return r


def _c5(b, K, N, nt, L=1, seed0=0):
    T = (nt - 1) / 4000.0 * (1.0 + 0.25 * b)  # (every replica its own grid and step width)
    return configs.config_c5(K=K, N=N, nt=nt, L=L, distinct=True, seed=seed0 + b, T=T, lambda_a=50.0 * (1.0 + 0.5 * b))


def _tls(j, nt=5):
    """Three different two-level problems (config 1's Hamiltonian at another frequency, duration and lambda_a)."""
    spec = configs.config_c1(nt=nt)
    omega, T, lam = ((1.0, 5.0, 5.0), (1.7, 3.0, 2.0), (0.4, 8.0, 11.0))[j]
    spec.H0 = [omega * spec.H0[0]]
    spec.tlist = np.linspace(0, T, nt)
    spec.lambda_a = lam
    return spec


@functools.lru_cache(maxsize=None)
def batch(name):
    if name == 'L1_small':
        return [_replica(_c5(b, 3, 5, 9), b) for b in range(5)]
    if name == 'L1_absent':  # (tests/test_absent_controls.py) objective 0 of replica 1 lacks the only control
        reps = [_replica(_c5(b, 3, 5, 9), b) for b in range(3)]
        reps[1].Hc = [list(row) for row in reps[1].Hc]
        reps[1].Hc[0][0] = None
        return reps
    if name == 'L1_full':
        return [_replica(_c5(b, 8, 16, 7, seed0=10), b) for b in range(3)]
    if name == 'L2':
        return [_replica(_c5(b, 2, 7, 9, L=2, seed0=20), b) for b in range(4)]
    if name == 'L3':
        return [_replica(_c5(b, 3, 4, 9, L=3, seed0=30), b) for b in range(2)]
    if name == 'L4':
        reps = [_replica(_c5(b, 3, 16, 7, L=4, seed0=40), b) for b in range(3)]
        reps[1].Hc = [list(row) for row in reps[1].Hc]
        reps[1].Hc[2][1] = None  # objective 2 of replica 1 lacks control 1
        return reps
    if name == 'liouville':
        reps = []
        for b, s in enumerate((1.0, 0.7, 1.3)):
            spec = configs.config_c2_liouville(nt=9)
            L1 = s * spec.Hc[0][0]
            spec.Hc = [[L1]] * 3
            reps.append(_replica(spec, b))
        return reps
    if name == 'many':
        base = [_replica(_tls(j), j) for j in range(3)]
        return [base[b % 3] for b in range(300)]
    if name == 'regimes':
        reps = []
        grid = np.array([0.5, 1.0, 1.5, 0.25, 1.25, 0.75, 1.0, 0.6])
        for b, factor in enumerate((1e-7, 1.0, 3.0, 6.0, 12.0)):
            r = _replica(configs.config_c5(K=2, N=7, nt=9, L=2, distinct=True, seed=50), 50)
            dt = np.diff(r.tlist) * grid  # non-uniform
            r.tlist = np.concatenate([[0.0], np.cumsum(dt)])
            helpers._scale_operators(r, factor)
            r.lambdas = [lam * factor for lam in r.lambdas]
            r.pulses = [np.array(p) for p in r.pulses]
            if b == 2:  # exactly 0.0 on the first and the last interval
                for p in r.pulses:
                    p[0] = p[-1] = 0.0
            reps.append(r)
        return reps
    raise KeyError(name)


COMPARED = {'many': (0, 255, 256, 299)}  # replicas compared with the oracle (default: all)


def _inputs(reps):
    """The arrays a replica engine takes for `reps`."""
    return dict(
        ops=[[r.H0[k]] + [r.Hc[k][l] for l in range(r.L)] for r in reps for k in range(r.K)],
        dt=np.array([np.diff(r.tlist) for r in reps]),
        init=np.concatenate([r.init for r in reps]),
        chi_T=np.concatenate([r.target / np.linalg.norm(r.target, axis=1)[:, None] for r in reps]),
        chi_norms=np.concatenate([r.chi_norms for r in reps]),
        pulses=np.array([np.array(r.pulses) for r in reps]),
        shapes=np.array([np.array(r.shapes) for r in reps]),
        lambdas=np.array([np.array(r.lambdas, dtype=np.float64) for r in reps]),
    )


@functools.lru_cache(maxsize=None)
def oracle_sweeps(name, b):
    """(forward final states, chi store, (opt, psi_T, g_a)) of replica b of a batch through the oracle (computed once)."""
    r = batch(name)[b]
    prob = spec_to_oracle(r)
    chi_T = r.target / np.linalg.norm(r.target, axis=1)[:, None]
    with helpers.MemoExpm():
        fw = ko.forward_propagation(prob, r.pulses)
        chi = ko.backward_sweep(prob, chi_T, r.pulses)
        upd = ko.forward_update_sweep(prob, chi, r.chi_norms, r.pulses, r.shapes, r.lambdas)
    return fw, chi, upd


def run_engine(reps, mask=None, out=None, theta_max=0.0, tol=0.0, op_norms=None):
    """Forward, backward and update sweep of a replica engine over `reps`; host arrays (psi0, chi, opt, psi_T, g_a)."""
    from krotov_amd.engine import HipKrotovEngine

    a = _inputs(reps)
    eng = HipKrotovEngine(a['ops'], a['dt'], is_super=reps[0].is_super, replicas=len(reps), theta_max=theta_max, tol=tol,
                          op_norms=op_norms)
    try:
        assert eng.kernel == 'replica16/wave'
        if mask is not None:
            eng.set_active_replicas(mask)
        out = out or {}
        psi0 = eng.forward(a['pulses'], a['init'], out=out.get('psi0'))
        chi = eng.backward(a['chi_T'], a['pulses'], out=out.get('chi'))
        opt, psi_T, g_a = eng.forward_update(chi, a['chi_norms'], a['init'], a['pulses'], a['shapes'], a['lambdas'],
                                             out=out.get('update'))
        eng.check()
        stats = eng.stats()
        return tuple(x.cpu().numpy() for x in (psi0, chi, opt, psi_T, g_a)) + (stats,)
    finally:
        eng.close()


def compare_with_oracle(name, got, which=None):
    reps = batch(name)
    psi0, chi, opt, psi_T, g_a = got[:5]
    Kr = reps[0].K
    tol = TOL_LIOUVILLE if reps[0].is_super else TOL_HILBERT
    for b in (which if which is not None else COMPARED.get(name, range(len(reps)))):
        fw, ref_chi, (ref_opt, ref_psi, ref_ga) = oracle_sweeps(name, b)
        rows = slice(b * Kr, (b + 1) * Kr)
        errs = dict(
            forward=np.abs(psi0[rows] - fw).max(),
            chi=np.abs(chi[rows] - ref_chi).max(),
            opt=np.abs(opt[b] - np.array(ref_opt)).max() / max(1.0, np.abs(np.array(ref_opt)).max()),
            psi_T=np.abs(psi_T[rows] - ref_psi).max(),
            g_a=np.abs(g_a[b] - ref_ga).max() / max(1.0, np.abs(ref_ga).max()),
        )
        print("%s replica %d: %s" % (name, b, ", ".join("%s %.2e" % kv for kv in errs.items())))
        for what, err in errs.items():
            assert err < tol, (name, b, what, err)


# ---------------------------------------------------------------------------
# GPU, engine level: every instantiation against the oracle
# ---------------------------------------------------------------------------
ENGINE_CASES = {'L1_small': 1, 'L1_full': 1, 'L2': 2, 'L3': 3, 'L4': 4, 'liouville': 1, 'many': 1}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(ENGINE_CASES))
def test_replica_sweeps_vs_oracle(name):
    from krotov_amd import _lib

    reps = batch(name)
    _lib.load()
    _lib.forget_launched_kernels()
    got = run_engine(reps)
    launched = _lib.kernel_instantiations(launched_only=True)
    L = ENGINE_CASES[name]
    assert reps[0].L == L
    for want in ('kh_rep_sweep_store<%d>' % L, 'kh_rep_forward_update<%d>' % L):
        assert want in launched, (want, launched)
    compare_with_oracle(name, got)
    assert got[5]['matvecs'] > 0 and got[5]['workgroups'] == len(reps)
    if name == 'many':  # replicas with equal inputs: bitwise equal results, wherever they sit
        Kr = reps[0].K
        for arr, per in ((got[0], Kr), (got[1], Kr), (got[2], 1), (got[3], Kr), (got[4], 1)):
            arr = arr.reshape((len(reps), per) + arr.shape[1:])
            for b in range(3, len(reps)):
                assert np.array_equal(arr[b], arr[b % 3]), b


def _regime_plans():
    """Per replica of the `regimes` batch: (sub-steps, degrees) of its largest-theta objective under its own pulses and
    grid, from the library's own tables (host only; every operator here is Hermitian: the real-spectrum table)."""
    tab = helpers.series_degree_tables()['real']
    plans = []
    for r in batch('regimes'):
        theta = helpers.theta_sequence(r)
        k = int(np.argmax(theta.max(axis=1)))
        plans.append(helpers.series_plan(theta[k], 1.0, tab))
    return plans


def test_regime_batch_spans_degrees_and_substeps():
    """Host only: the replicas of the `regimes` batch really differ in degree and in sub-step count."""
    plans = _regime_plans()
    nsub = [int(p[0].max()) for p in plans]
    deg = [int(p[1].max()) for p in plans]
    print("regimes: sub-steps", nsub, "degrees", deg)
    assert len(set(nsub)) >= 3 and max(nsub) >= 2 and min(nsub) == 1
    assert min(deg) <= 4 and len({d for p in plans for d in p[1].tolist()}) >= 3
    keys = [(tuple(p[0].tolist()), tuple(p[1].tolist())) for p in plans]
    assert len(set(keys)) == len(keys)  # no two replicas run the same plan
    for p in plans[2:]:
        assert len(set(p[0].tolist())) >= 2  # (the non-uniform grid: the sub-step count changes along the sweep)
    r = batch('regimes')[2]
    assert all(p[0] == 0.0 and p[-1] == 0.0 for p in r.pulses)


@pytest.mark.gpu
def test_replica_regimes_vs_oracle():
    test_regime_batch_spans_degrees_and_substeps()
    compare_with_oracle('regimes', run_engine(batch('regimes')))


# ---------------------------------------------------------------------------
# GPU, protocol-free properties (bitwise; no oracle involved)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.no_oracle
def test_replica_alone_equals_its_place_in_a_batch():
    reps = batch('many')
    whole, alone = run_engine(reps), run_engine([reps[217]])
    Kr = reps[0].K
    rows = slice(217 * Kr, 218 * Kr)
    assert np.array_equal(alone[0], whole[0][rows]) and np.array_equal(alone[1], whole[1][rows])
    assert np.array_equal(alone[2][0], whole[2][217]) and np.array_equal(alone[3], whole[3][rows])
    assert np.array_equal(alone[4][0], whole[4][217])


@pytest.mark.gpu
@pytest.mark.no_oracle
@pytest.mark.parametrize('name', ['L1_small', 'L4'])
def test_two_runs_of_a_batch_are_equal(name):
    one, two = run_engine(batch(name)), run_engine(batch(name))
    for x, y in zip(one[:5], two[:5]):
        assert np.array_equal(x, y)


@pytest.mark.gpu
@pytest.mark.no_oracle
@pytest.mark.parametrize('name', ['L1_small', 'L2'])
def test_inactive_replica_is_left_untouched(name):
    import torch

    reps = batch(name)[:3]
    B, Kr, N, L, nt = 3, reps[0].K, reps[0].N, reps[0].L, len(reps[0].tlist)
    full = run_engine(reps)

    def nans(shape, dtype):
        fill = complex(float('nan'), float('nan')) if dtype == torch.complex128 else float('nan')
        return torch.full(shape, fill, dtype=dtype, device='cuda')

    out = dict(psi0=nans((B * Kr, N), torch.complex128), chi=nans((B * Kr, nt, N), torch.complex128),
               update=(nans((B, L, nt - 1), torch.float64), nans((B * Kr, N), torch.complex128), nans((B, L), torch.float64)))
    masked = run_engine(reps, mask=[1, 0, 1], out=out)
    for x, y, per in zip(masked[:5], full[:5], (Kr, Kr, 1, Kr, 1)):
        x = x.reshape((B, per) + x.shape[1:])
        y = y.reshape((B, per) + y.shape[1:])
        assert np.all(np.isnan(x[1].real)) and (not np.iscomplexobj(x) or np.all(np.isnan(x[1].imag)))
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2])


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_replica_engine_refuses_what_it_does_not_run():
    import torch

    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    reps = batch('L2')
    a = _inputs(reps)
    eng = HipKrotovEngine(a['ops'], a['dt'], replicas=len(reps))
    K, nt, N = len(a['ops']), a['dt'].shape[1] + 1, reps[0].N
    store = torch.zeros((K, nt, N), dtype=torch.complex128, device='cuda')
    for call in (lambda: eng.set_second_order(store, store.clone(), np.zeros(nt - 1)),
                 lambda: eng.set_update_workgroups(1), lambda: eng.set_row_split(2)):
        with pytest.raises(_lib.KrotovHipError) as err:
            call()
        assert err.value.code == _lib.KH_ERR_UNSUPPORTED
    assert eng.replica_occupancy() >= 1
    eng.close()
    plain = HipKrotovEngine(a['ops'][:2], a['dt'][0])
    with pytest.raises(_lib.KrotovHipError) as err:
        plain.set_active_replicas([1])
    assert err.value.code == _lib.KH_ERR_UNSUPPORTED
    plain.close()


# ---------------------------------------------------------------------------
# optimize_pulses_batch
# ---------------------------------------------------------------------------
def _problems(specs):
    import krotov_amd

    out = []
    for spec in specs:
        objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
        out.append(dict(objectives=objectives, pulse_options=pulse_options, tlist=spec.tlist))
    return out


def _opt_specs(kind, B=3):
    if kind == 'L1_small':
        return [_c5(b, 3, 5, 9) for b in range(B)]
    return [_c5(b, 2, 7, 9, L=2, seed0=20) for b in range(B)]


def _shared_kw():
    import krotov_amd

    return dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_re)


def _loop(problems, **kw):
    import krotov_amd

    prev = kw.pop('continue_from', None) or [None] * len(problems)
    return [krotov_amd.optimize_pulses(p['objectives'], p['pulse_options'], p['tlist'], continue_from=c, **kw)
            for p, c in zip(problems, prev)]


def _J_T(**kw):
    import krotov_amd

    return krotov_amd.functionals.J_T_re(kw['fw_states_T'], kw['objectives'], tau_vals=kw['tau_vals'])


def _close(a, b, tol):
    a, b = np.array(a, dtype=complex), np.array(b, dtype=complex)
    return a.shape == b.shape and np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['L1_small', 'L2'])
def test_batch_three_iterations_vs_oracle_and_loop(kind):
    import krotov_amd
    from krotov_amd.engine import LAST_ENGINE

    specs = _opt_specs(kind)
    problems = _problems(specs)
    results = krotov_amd.optimize_pulses_batch(problems, iter_stop=3, store_all_pulses=True, **_shared_kw())
    assert LAST_ENGINE().kernel == 'replica16/wave'
    loop = _loop(problems, iter_stop=3, store_all_pulses=True, **_shared_kw())
    for b, (spec, res, seq) in enumerate(zip(specs, results, loop)):
        ref = helpers.oracle_optimize(spec, 3)
        d_pulse = np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() / max(1.0, np.abs(ref['all_pulses']).max())
        d_tau = np.abs(np.array(res.tau_vals) - ref['tau_vals']).max()
        print("%s replica %d: pulses %.2e tau %.2e" % (kind, b, d_pulse, d_tau))
        assert d_pulse < TOL_HILBERT and d_tau < TOL_HILBERT
        assert res.iters == seq.iters == [0, 1, 2, 3] and res.message == seq.message
        assert _close(res.all_pulses, seq.all_pulses, TOL_HILBERT) and _close(res.tau_vals, seq.tau_vals, TOL_HILBERT)
        assert _close(res.optimized_controls, seq.optimized_controls, TOL_HILBERT)
        assert _close([np.asarray(s).ravel() for s in res.states], [np.asarray(s).ravel() for s in seq.states], TOL_HILBERT)


def _stopping_specs():
    """One problem under three step widths: the smaller lambda_a, the faster J_T falls."""
    return [configs.config_c5(K=3, N=5, nt=9, distinct=True, seed=3, lambda_a=lam) for lam in (15.0, 50.0, 400.0)]


def _stopping_limit(specs, iters=4):
    """The mid-point between J_T after iterations 1 and 2 of the middle replica, from the oracle's own sequence; and the
    iteration at which every replica's oracle sequence first falls below it (None: never)."""
    J = [[1.0 - float(np.mean(t).real) for t in helpers.oracle_optimize(s, iters)['tau_vals']] for s in specs]
    limit = 0.5 * (J[1][1] + J[1][2])
    first = [next((i for i in range(1, iters + 1) if seq[i] < limit), None) for seq in J]
    return limit, first


def _check_stopping(results, loop, first, iters=4):
    stops = []
    for res, seq, at in zip(results, loop, first):
        assert res.iters == seq.iters and res.message == seq.message and len(res.tau_vals) == len(seq.tau_vals)
        assert res.iters[-1] == (at if at is not None else iters)
        stops.append(res.iters[-1])
    assert len(set(stops)) >= 2, stops  # the replicas really stopped after different iterations
    return stops


@pytest.mark.gpu
def test_batch_replicas_stop_on_their_own():
    import krotov_amd

    specs = _stopping_specs()
    limit, first = _stopping_limit(specs)
    kw = dict(iter_stop=4, info_hook=_J_T, store_all_pulses=True,
              check_convergence=krotov_amd.convergence.value_below(limit, name='J_T'), **_shared_kw())
    problems = _problems(specs)
    results = krotov_amd.optimize_pulses_batch(problems, **kw)
    loop = _loop(problems, **kw)
    stops = _check_stopping(results, loop, first)
    early = int(np.argmin(stops))
    assert _close(results[early].all_pulses, loop[early].all_pulses, TOL_HILBERT)
    assert _close(results[early].optimized_controls, loop[early].optimized_controls, TOL_HILBERT)
    for res, seq in zip(results, loop):
        assert _close(res.info_vals, seq.info_vals, TOL_HILBERT)


def _doubling_hook(which):
    """modify_params_after_iter: doubles lambda_a of the replica whose lambda_a is `which`, after iteration 1."""
    seen = []

    def hook(**kw):
        seen.append((kw['iteration'], float(kw['lambda_vals'][0]), len(kw['objectives'])))
        if kw['iteration'] == 1 and kw['lambda_vals'][0] == which:
            kw['lambda_vals'][0] *= 2.0

    hook.seen = seen
    return hook


@pytest.mark.gpu
def test_batch_hook_changes_one_replicas_step_width():
    import krotov_amd

    specs = _stopping_specs()
    problems = _problems(specs)
    plain = krotov_amd.optimize_pulses_batch(problems, iter_stop=3, store_all_pulses=True, **_shared_kw())
    hook_b, hook_s = _doubling_hook(50.0), _doubling_hook(50.0)
    results = krotov_amd.optimize_pulses_batch(problems, iter_stop=3, store_all_pulses=True, modify_params_after_iter=hook_b,
                                               **_shared_kw())
    loop = _loop(problems, iter_stop=3, store_all_pulses=True, modify_params_after_iter=hook_s, **_shared_kw())
    assert sorted(hook_b.seen) == sorted(hook_s.seen)
    for b, (res, seq, before) in enumerate(zip(results, loop, plain)):
        assert _close(res.all_pulses, seq.all_pulses, TOL_HILBERT)
        changed = not np.array_equal(np.array(res.all_pulses[2]), np.array(before.all_pulses[2]))
        assert changed == (b == 1)  # iteration 2 of replica 1 alone ran under the doubled lambda_a
        assert np.array_equal(np.array(res.all_pulses[1]), np.array(before.all_pulses[1]))


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['N17', 'unequal_nt'])
def test_batch_falls_back_to_the_loop(case, caplog):
    import krotov_amd
    from krotov_amd.engine import LAST_ENGINE

    if case == 'N17':
        specs = [configs.config_c5(K=2, N=17, nt=7, distinct=True, seed=b) for b in range(2)]
    else:
        specs = [configs.config_c5(K=2, N=5, nt=7 + 2 * b, distinct=True, seed=b) for b in range(2)]
    problems = _problems(specs)
    with caplog.at_level(logging.INFO, logger='krotov'):
        results = krotov_amd.optimize_pulses_batch(problems, iter_stop=2, store_all_pulses=True, **_shared_kw())
    assert sum('optimize_pulses_batch: sequential' in rec.getMessage() for rec in caplog.records) == 1
    assert LAST_ENGINE().kernel != 'replica16/wave'
    loop = _loop(problems, iter_stop=2, store_all_pulses=True, **_shared_kw())
    for spec, res, seq in zip(specs, results, loop):
        assert np.array_equal(np.array(res.all_pulses), np.array(seq.all_pulses))
        ref = helpers.oracle_optimize(spec, 2)
        assert np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() < TOL_HILBERT * max(1.0, np.abs(ref['all_pulses']).max())


# ---------------------------------------------------------------------------
# without a GPU: the driver on an oracle-backed engine double; the C ABI's argument checks
# ---------------------------------------------------------------------------
@pytest.fixture
def replica_double(monkeypatch):
    import krotov_amd.engine as engine_mod
    from replica_double import ReplicaEngineDouble

    monkeypatch.setattr(engine_mod, 'HipKrotovEngine', ReplicaEngineDouble)
    ReplicaEngineDouble.created = []
    return ReplicaEngineDouble


def _same_result(res, seq):
    """Bit for bit, the wall-clock fields aside."""
    assert res.iters == seq.iters and res.message == seq.message
    for name in ('tau_vals', 'all_pulses', 'optimized_controls', 'guess_controls', 'info_vals'):
        a, b = getattr(res, name), getattr(seq, name)
        assert len(a) == len(b), name
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)), name
    assert res.controls_mapping == seq.controls_mapping
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(res.states, seq.states))
    assert type(res.states) is type(seq.states) is list


def _recording_hook():
    calls = []

    def hook(**kw):
        calls.append(dict(
            iteration=kw['iteration'], keys=sorted(kw), K=len(kw['objectives']), tlist=np.array(kw['tlist']),
            lambda_vals=np.array(kw['lambda_vals']), shape_arrays=np.array(kw['shape_arrays']),
            guess=np.array(kw['guess_pulses']), opt=np.array(kw['optimized_pulses']), g_a=np.array(kw['g_a_integrals']),
            tau=np.array(kw['tau_vals']), psi=np.array([np.asarray(s).ravel() for s in kw['fw_states_T']]),
            chi0=None if kw['backward_states'] is None else np.array(kw['backward_states'][0][0]).ravel().copy(),
            iter_stop=kw['iter_stop'], info_vals=len(kw['info_vals'])))
        return _J_T(**kw)

    hook.calls = calls
    return hook


@pytest.mark.parametrize('kind', ['L1_small', 'L2'])
def test_batch_on_the_double_equals_separate_runs(kind, replica_double):
    import krotov_amd

    problems = _problems(_opt_specs(kind, B=4))
    hook_b, hook_s = _recording_hook(), _recording_hook()
    results = krotov_amd.optimize_pulses_batch(problems, iter_stop=3, store_all_pulses=True, info_hook=hook_b, **_shared_kw())
    batch_engines = list(replica_double.created)
    assert [e.replicas for e in batch_engines] == [4] and batch_engines[0].kernel == 'replica16/wave'
    # one forward sweep, then one backward and one update sweep per iteration of the whole batch
    assert [s[0] for s in batch_engines[0].sweeps] == ['forward'] + ['backward', 'update'] * 3
    loop = _loop(problems, iter_stop=3, store_all_pulses=True, info_hook=hook_s, **_shared_kw())
    for res, seq in zip(results, loop):
        _same_result(res, seq)
    # every call of the hook got that replica's own keyword arguments (the batch calls replica by replica per iteration)
    key = lambda c: (c['lambda_vals'][0], c['iteration'])  # noqa: E731  (lambda_a differs per replica)
    assert len(hook_b.calls) == len(hook_s.calls) == 4 * 4
    for cb, cs in zip(sorted(hook_b.calls, key=key), sorted(hook_s.calls, key=key)):
        assert cb['keys'] == cs['keys'] and cb['iteration'] == cs['iteration'] and cb['K'] == cs['K']
        assert cb['iter_stop'] == cs['iter_stop'] and cb['info_vals'] == cs['info_vals']
        for name in ('tlist', 'lambda_vals', 'shape_arrays', 'guess', 'opt', 'g_a', 'tau', 'psi'):
            assert np.array_equal(cb[name], cs[name]), name
        assert (cb['chi0'] is None) == (cs['chi0'] is None) and (cb['chi0'] is None or np.array_equal(cb['chi0'], cs['chi0']))


def test_batch_on_the_double_stops_per_replica(replica_double):
    import krotov_amd

    specs = _stopping_specs()
    limit, first = _stopping_limit(specs)
    kw = dict(iter_stop=4, info_hook=_J_T, store_all_pulses=True,
              check_convergence=krotov_amd.convergence.value_below(limit, name='J_T'), **_shared_kw())
    problems = _problems(specs)
    results = krotov_amd.optimize_pulses_batch(problems, **kw)
    eng = replica_double.created[0]
    loop = _loop(problems, **kw)
    stops = _check_stopping(results, loop, first)
    for res, seq in zip(results, loop):
        _same_result(res, seq)
    # a finished replica is frozen through the active mask: no sweep touches it after its last iteration
    for b, stop in enumerate(stops):
        masks = [m for name, m in eng.sweeps if name == 'update']
        assert [m[b] for m in masks] == [1] * stop + [0] * (len(masks) - stop)
    assert len([1 for name, _ in eng.sweeps if name == 'update']) == max(stops)


def test_batch_on_the_double_hooks_and_continuation(replica_double):
    import krotov_amd

    problems = _problems(_stopping_specs())

    def run(fn, **kw):
        hook = _doubling_hook(50.0)
        return fn(problems, iter_stop=3, store_all_pulses=True, modify_params_after_iter=hook, info_hook=_J_T, **kw,
                  **_shared_kw()), hook

    (results, hook_b), (loop, hook_s) = run(krotov_amd.optimize_pulses_batch), run(_loop)
    assert sorted(hook_b.seen) == sorted(hook_s.seen) and (2, 100.0, 3) in hook_b.seen
    for res, seq in zip(results, loop):
        _same_result(res, seq)
    # continuation: two more iterations from the batch's own results
    more_b = krotov_amd.optimize_pulses_batch(problems, iter_stop=5, store_all_pulses=True, info_hook=_J_T,
                                              continue_from=results, **_shared_kw())
    more_s = _loop(problems, iter_stop=5, store_all_pulses=True, info_hook=_J_T, continue_from=copy.deepcopy(loop),
                   **_shared_kw())
    for res, seq in zip(more_b, more_s):
        assert res.iters == [0, 1, 2, 3, 4, 5]
        _same_result(res, seq)


def test_batch_on_the_double_falls_back(replica_double, caplog):
    import krotov_amd

    specs = [configs.config_c5(K=2, N=5, nt=7 + 2 * b, distinct=True, seed=b) for b in range(2)]
    problems = _problems(specs)
    with caplog.at_level(logging.INFO, logger='krotov'):
        results = krotov_amd.optimize_pulses_batch(problems, iter_stop=2, store_all_pulses=True, **_shared_kw())
    assert sum('optimize_pulses_batch: sequential' in rec.getMessage() for rec in caplog.records) == 1
    assert all(not e.replicas for e in replica_double.created)
    for res, seq in zip(results, _loop(problems, iter_stop=2, store_all_pulses=True, **_shared_kw())):
        _same_result(res, seq)
    assert krotov_amd.optimize_pulses_batch([], **_shared_kw()) == []
    assert 'optimize_pulses_batch' in krotov_amd.__all__


def test_batch_splits_when_the_costate_store_does_not_fit(replica_double, monkeypatch, caplog):
    import krotov_amd
    import krotov_amd.batch as batch_mod

    problems = _problems(_opt_specs('L1_small', B=4))
    per_replica = 3 * 9 * 5 * 16
    monkeypatch.setattr(batch_mod, '_free_device_bytes', lambda: 4 * (2 * per_replica + 1))  # a quarter holds two replicas
    with caplog.at_level(logging.INFO, logger='krotov'):
        results = krotov_amd.optimize_pulses_batch(problems, iter_stop=2, store_all_pulses=True, **_shared_kw())
    assert [e.replicas for e in replica_double.created] == [2, 2]
    assert any('sub-batches' in rec.getMessage() for rec in caplog.records)
    for res, seq in zip(results, _loop(problems, iter_stop=2, store_all_pulses=True, **_shared_kw())):
        _same_result(res, seq)


def _abi_problem(K, N, L, nt):
    """A kh_problem whose host-side fields are all valid (nothing behind `ops` is read before the first HIP call)."""
    from krotov_amd import _lib

    keep = dict(dt=np.full(nt - 1, 0.1), blob=np.zeros(4, dtype=np.complex128), ptrs=(ctypes.c_void_p * (K * (1 + L)))())
    for i in range(K * (1 + L)):
        keep['ptrs'][i] = keep['blob'].ctypes.data
    pr = _lib.kh_problem()
    pr.K, pr.N, pr.L, pr.nt = K, N, L, nt
    pr.dt = keep['dt'].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    pr.ops = ctypes.cast(keep['ptrs'], ctypes.POINTER(ctypes.c_void_p))
    pr._keep = keep
    return pr


def test_create_replicas_checks_its_arguments_without_a_device():
    from krotov_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, 'kh_engine_create_replicas') and hasattr(lib, 'kh_set_active_replicas')
    assert 'replica16/wave' in lib.kh_version().decode()
    handle = ctypes.c_void_p()
    assert lib.kh_engine_create_replicas(None, 2, None, ctypes.byref(handle)) == _lib.KH_ERR_INVALID
    pr = _abi_problem(6, 4, 1, 5)
    assert lib.kh_engine_create_replicas(ctypes.byref(pr), 2, None, None) == _lib.KH_ERR_INVALID
    assert lib.kh_engine_create_replicas(ctypes.byref(pr), 4, None, ctypes.byref(handle)) == _lib.KH_ERR_INVALID
    assert lib.kh_engine_create_replicas(ctypes.byref(pr), 0, None, ctypes.byref(handle)) == _lib.KH_ERR_INVALID
    bad_dt = np.full((2, 4), 0.1)
    bad_dt[1, 2] = 0.0
    assert lib.kh_engine_create_replicas(ctypes.byref(pr), 2, bad_dt.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                         ctypes.byref(handle)) == _lib.KH_ERR_INVALID
    for K, N, L in ((4, 17, 1), (18, 4, 1), (4, 4, 5), (4, 4, 0)):  # N = 17, K_r = 9, L = 5, L = 0
        pr = _abi_problem(K, N, L, 5)
        assert lib.kh_engine_create_replicas(ctypes.byref(pr), 2, None, ctypes.byref(handle)) == _lib.KH_ERR_UNSUPPORTED, (K, N, L)
        assert not handle.value
    assert lib.kh_set_active_replicas(None, None) == _lib.KH_ERR_INVALID
    names = _lib.kernel_instantiations()
    for L in (1, 2, 3, 4):
        assert 'kh_rep_sweep_store<%d>' % L in names and 'kh_rep_forward_update<%d>' % L in names
