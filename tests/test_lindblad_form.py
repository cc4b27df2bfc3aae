"""Objectives in Lindblad form (``Objective.H`` a d x d Hamiltonian, ``Objective.c_ops`` the Lindblad operators) on the
device, in matrix form: ``kh_engine_create_lindblad`` / kernel family ``"lindblad/matrix"`` (krotov_amd/csrc/kh_lind.h),
``krotov_amd.propagators.LindbladExpm``.

The defined behaviour is: identical, to rounding, to the same objective with ``H = liouvillian(H, c_ops)``,
``c_ops = []`` -- so every GPU test compares with the oracle (or the reference's own loop, tests/golden) run on
``liouvillian_dense`` of the very same operators.  Tolerances: 1e-11 against the oracle (what DESIGN.md section 5 uses
for Liouville problems), the existing fixtures' own bounds against the reference's loop, 1e-12 per single step.
"""
import logging

import numpy as np
import pytest

import krotov_amd
from helpers import golden, product_sigma, SigmaA
from krotov_amd import configs, mixed
from krotov_amd.configs import liouvillian_dense
from oracle import krotov_oracle as ko

TOL = 1e-11


# ---------------------------------------------------------------------------
# cases: per objective [H0, H_1 .. H_L] (d x d; None: control absent) and its Lindblad operators
# ---------------------------------------------------------------------------
class Case:
    def __init__(self, H, C, init, target, dt):
        self.H, self.C, self.init, self.target = H, C, np.array(init), np.array(target)
        self.dt = np.asarray(dt, dtype=np.float64)
        self.tlist = np.concatenate([[0.0], np.cumsum(self.dt)])
        self.K, self.L, self.d = len(H), len(H[0]) - 1, H[0][0].shape[0]

    def vec(self, rhos):
        return np.array([np.asarray(r).ravel(order='F') for r in rhos])

    def oracle(self):
        """The same problem in Liouvillian form (one dense super-operator per distinct operator list)."""
        made = {}

        def sup(op, cs=()):
            key = (id(op),) + tuple(id(c) for c in cs)
            if key not in made:
                made[key] = liouvillian_dense(op, cs)
            return made[key]

        ops = [[sup(row[0], self.C[k])] + [None if h is None else sup(h) for h in row[1:]] for k, row in enumerate(self.H)]
        return ko.OracleProblem(ops, self.vec(self.init), self.vec(self.target), self.tlist, True)


def _rho(rng, d):
    G = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    r = G @ G.conj().T
    return r / np.trace(r).real


def _random(d, K, L, n_c, nt, seed, nonherm=False, per_objective=False, missing=None, no_cops=None, dt=None):
    rng = np.random.default_rng(seed)
    dt = np.full(nt - 1, 0.05) if dt is None else np.asarray(dt)

    def make_row():
        H0 = configs.herm(rng, d, 6.0)
        if nonherm:
            H0 = H0 - 0.3j * configs.herm(rng, d, 1.0) @ configs.herm(rng, d, 1.0)
        return [H0] + [configs.herm(rng, d, 2.0) for _ in range(L)]

    def make_cs():
        return [0.4 * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) / np.sqrt(d) for _ in range(n_c)]

    row, cs = make_row(), make_cs()
    H, C = [], []
    for k in range(K):
        r, c = (make_row(), make_cs()) if per_objective else (list(row), list(cs))
        if missing is not None and k == missing[0]:
            r[1 + missing[1]] = None
        if no_cops is not None and k == no_cops:
            c = []
        H.append(r)
        C.append(c)
    return Case(H, C, [_rho(rng, d) for _ in range(K)], [_rho(rng, d) for _ in range(K)], dt)


def _from_spec(ls, n_intervals):
    H = [[ls.H0, ls.H1]] * ls.K
    return Case(H, [list(ls.c_ops)] * ls.K, ls.init, ls.target, np.diff(ls.tlist)[:n_intervals])


CASES = {
    'c4_d5': lambda: _from_spec(configs.config_c4_lindblad(d=5, nt=201, n_logical=2), 12),
    'c4_d20': lambda: _from_spec(configs.config_c4_lindblad(), 6),
    'ladder_d12': lambda: _from_spec(configs.config_sparse_lindblad_form(), 60),
    'd7': lambda: _random(7, 3, 1, 1, 9, 1),
    'd32_two_cops_two_controls': lambda: _random(32, 2, 2, 2, 3, 2),
    'nonhermitian_H0': lambda: _random(6, 2, 1, 1, 8, 3, nonherm=True),
    'one_objective_without_cops': lambda: _random(5, 3, 1, 2, 8, 4, no_cops=1),
    'per_objective_H0': lambda: _random(8, 4, 2, 1, 7, 5, per_objective=True),
    'control_missing_in_one_objective': lambda: _random(6, 3, 2, 1, 7, 6, per_objective=True, missing=(1, 0)),
    'K300': lambda: _random(4, 300, 1, 1, 4, 7, per_objective=True),
    'unequal_dt': lambda: _random(9, 2, 1, 3, 8, 8, dt=[0.05, 0.01, 0.08, 0.02, 0.05, 0.11, 0.03]),
    'four_cops_d32': lambda: _random(32, 1, 1, 4, 2, 9),
}


def _pulses(case, seed=11):
    rng = np.random.default_rng(seed)
    return [0.8 * rng.standard_normal(len(case.dt)) for _ in range(case.L)]


def _engine(case, **kw):
    from krotov_amd.engine import HipKrotovEngine

    return HipKrotovEngine(case.H, case.dt, c_ops=case.C, **kw)


# ---------------------------------------------------------------------------
# host
# ---------------------------------------------------------------------------
def test_config_helpers_reproduce_the_liouvillians_bit_for_bit():
    for lind, spec in ((configs.config_c4_lindblad(d=5, nt=201, n_logical=2), configs.config_c4(d=5, nt=201, n_logical=2)),
                       (configs.config_sparse_lindblad_form(), configs.config_sparse_lindblad())):
        assert np.array_equal(liouvillian_dense(lind.H0, lind.c_ops), spec.H0[0])
        assert np.array_equal(liouvillian_dense(lind.H1), spec.Hc[0][0])
        assert np.array_equal(np.array([r.ravel(order='F') for r in lind.init]), spec.init)
        assert np.array_equal(np.array([r.ravel(order='F') for r in lind.target]), spec.target)
        assert np.array_equal(lind.tlist, spec.tlist) and lind.K == spec.K


def _objectives(d, n_c=1, K=2, ket=False):
    rng = np.random.default_rng(d)
    H = [configs.herm(rng, d, 1.0), [configs.herm(rng, d, 1.0), lambda t, args: 0.1]]
    cs = [0.1 * configs.herm(rng, d, 1.0) for _ in range(n_c)]
    objs = [krotov_amd.Objective(initial_state=_rho(rng, d), target=_rho(rng, d), H=H, c_ops=cs) for _ in range(K)]
    if ket:
        e = np.zeros(d, dtype=complex)
        e[0] = 1
        objs.append(krotov_amd.Objective(initial_state=e, target=e, H=H))
    return objs


def test_layout_helper_decides_matrix_form_or_liouvillian_fallback():
    lay = mixed.lindblad_layout_of(configs.config_c4_lindblad(d=5, nt=201, n_logical=2).objectives(krotov_amd)[0])
    assert lay.decision == 'matrix' and lay.d == 5 and lay.n_c == 1
    lay = mixed.lindblad_layout_of(configs.config_sparse_lindblad_form().objectives(krotov_amd)[0])
    assert lay.decision == 'matrix' and lay.d == 12
    assert mixed.lindblad_layout_of(_objectives(32, n_c=4), n_controls=4).decision == 'matrix'
    # Liouvillian fallback
    for objs, kw in ((_objectives(4) + _objectives(5), {}), (_objectives(4, ket=True), {}), (_objectives(33), {}),
                     (_objectives(4, n_c=5), {}), (_objectives(4), dict(n_controls=5)), (_objectives(4), dict(second_order=True))):
        lay = mixed.lindblad_layout_of(objs, **kw)
        assert lay.decision == 'liouvillian' and lay.reason
        conv = lay.liouvillian_objectives(objs)
        assert all(len(o.c_ops) == 0 for o in conv) and len(conv) == len(objs)
    conv = mixed.LindbladLayout.liouvillian_objectives(_objectives(4))
    assert np.asarray(conv[0].H[0]).shape == (16, 16) and callable(conv[0].H[1][1])
    # a control inside c_ops
    objs = _objectives(4)
    objs[1] = krotov_amd.Objective(initial_state=objs[1].initial_state, target=objs[1].target, H=objs[1].H,
                                   c_ops=[[np.eye(4, dtype=complex), lambda t, args: 1.0]])
    with pytest.raises(NotImplementedError, match="Time-dependent collapse operators not implemented"):
        mixed.lindblad_layout_of(objs)


def test_control_inside_c_ops_raises_before_any_gpu_work():
    objs = _objectives(4)
    ctl = lambda t, args: 1.0  # noqa: E731
    objs[0] = krotov_amd.Objective(initial_state=objs[0].initial_state, target=objs[0].target, H=objs[0].H,
                                   c_ops=[[np.eye(4, dtype=complex), ctl]])
    opts = {objs[0].H[1][1]: dict(lambda_a=1.0, update_shape=1), ctl: dict(lambda_a=1.0, update_shape=1)}
    with pytest.raises(NotImplementedError, match="Time-dependent collapse operators not implemented"):
        krotov_amd.optimize_pulses(objs, opts, np.linspace(0, 1, 5), propagator=krotov_amd.propagators.LindbladExpm(),
                                   chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1)


def test_only_lindblad_expm_opts_in():
    from krotov_amd.optimize import _use_device_path
    from krotov_amd.propagators import DensityMatrixODEPropagator, HipExpm, LindbladExpm, expm

    objs = _objectives(4)
    assert _use_device_path(LindbladExpm(), None, None, None, 'array', objs)
    assert _use_device_path([LindbladExpm(), LindbladExpm()], None, None, None, 'array', objs)
    for prop in (expm, HipExpm(), DensityMatrixODEPropagator(), [LindbladExpm(), HipExpm()]):
        assert not _use_device_path(prop, None, None, None, 'array', objs)
    # the reference's behaviour stays: c_ops are refused before anything touches a GPU
    H = [objs[0].H[0], [objs[0].H[1][0], 0.1]]
    for prop in (expm, HipExpm(), DensityMatrixODEPropagator()):
        with pytest.raises(NotImplementedError, match="Liouville exponentiation not implemented"):
            prop(H, objs[0].initial_state, 0.1, c_ops=objs[0].c_ops)
    with pytest.raises(NotImplementedError, match="Time-dependent collapse operators not implemented"):
        LindbladExpm()(H, objs[0].initial_state, 0.1, c_ops=[[np.eye(4), 0.3]])


def test_c_abi_and_instantiations():
    import os

    from krotov_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'krotov_hip.h')).read()
    assert 'int kh_engine_create_lindblad(const kh_problem_lindblad *problem, kh_engine **out);' in header
    assert hasattr(_lib.load(), 'kh_engine_create_lindblad')
    names = _lib.kernel_instantiations()
    for rb in (1, 2, 4):
        assert 'kh_lind_sweep_store<%d>' % rb in names and 'kh_lind_forward_update<%d>' % rb in names
    assert b'lindblad/matrix' in _lib.load().kh_version()


# ---------------------------------------------------------------------------
# GPU: the sweeps against the oracle on liouvillian_dense of the same operators
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_sweeps_vs_oracle(name):
    case = CASES[name]()
    prob = case.oracle()
    pulses = _pulses(case)
    eng = _engine(case)
    assert eng.kernel == 'lindblad/matrix' and eng.N == case.d ** 2
    # forward with storage
    ref_T, ref_states = ko.forward_propagation(prob, pulses, store=True)
    psi_T, states = eng.forward(np.array(pulses), prob.init, store=True)
    d_fw = np.abs(states.cpu().numpy() - ref_states).max()
    d_T = np.abs(psi_T.cpu().numpy() - ref_T).max()
    stats = eng.stats()
    assert stats['matvecs'] > 0 and stats['intervals'] == len(case.dt)
    # backward
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    ref_chi = ko.backward_sweep(prob, chi_T, pulses)
    chi = eng.backward(chi_T, np.array(pulses))
    d_bw = np.abs(chi.cpu().numpy() - ref_chi).max()
    # one update sweep
    rng = np.random.default_rng(5)
    norms = 0.5 * (1.0 + rng.random(case.K)) / case.K
    S = [np.linspace(0.2, 1.0, len(case.dt)) for _ in range(case.L)]
    lam = [0.7 + 0.3 * l for l in range(case.L)]
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, pulses, S, lam)
    opt, psi, g_a = eng.forward_update(chi, norms, prob.init, np.array(pulses), np.array(S), np.array(lam))
    eng.check()
    d_opt = np.abs(opt.cpu().numpy() - np.array(ref_opt)).max()
    d_psi = np.abs(psi.cpu().numpy() - ref_psi).max()
    d_ga = np.abs(g_a.cpu().numpy() - np.array(ref_ga)).max()
    moved = np.abs(np.array(ref_opt) - np.array(pulses)).max()
    # tau and the boundary co-states run on N = d^2 unchanged
    tau = eng.tau(prob.target, psi).cpu().numpy()
    d_tau = np.abs(tau - np.array([np.vdot(prob.target[k], ref_psi[k]) for k in range(case.K)])).max()
    print("lindblad_form %s: forward %.2e final %.2e backward %.2e pulses %.2e psi_T %.2e g_a %.2e tau %.2e (update moved "
          "the pulses by %.2e)" % (name, d_fw, d_T, d_bw, d_opt, d_psi, d_ga, d_tau, moved))
    eng.close()
    assert moved > 1e-6  # the update is not a no-op here
    assert max(d_fw, d_T, d_bw, d_opt, d_psi, d_ga, d_tau) <= TOL


@pytest.mark.gpu
def test_two_runs_bitwise_identical_and_entry_points_outside_the_scope():
    from krotov_amd import _lib
    from krotov_amd._lib import KH_ERR_UNSUPPORTED, KrotovHipError

    case = CASES['per_objective_H0']()
    prob = case.oracle()
    pulses = np.array(_pulses(case))
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    norms = np.full(case.K, 0.4)
    S, lam = np.ones((case.L, len(case.dt))), np.ones(case.L)
    runs = []
    for _ in range(2):
        eng = _engine(case)
        chi = eng.backward(chi_T, pulses)
        opt, psi, g_a = eng.forward_update(chi, norms, prob.init, pulses, S, lam)
        eng.check()
        runs.append([x.cpu().numpy().copy() for x in (chi, opt, psi, g_a)])
        if len(runs) == 2:
            import torch

            buf = torch.empty((case.K, len(case.dt) + 1, eng.N), dtype=torch.complex128, device=eng.device)
            with pytest.raises(KrotovHipError) as err:
                eng.set_second_order(buf, buf.clone(), np.ones(len(case.dt)))
            assert err.value.code == KH_ERR_UNSUPPORTED
            with pytest.raises(KrotovHipError) as err:
                eng.set_update_workgroups(1)
            assert err.value.code == KH_ERR_UNSUPPORTED
            handle = (__import__('ctypes').c_ubyte * 64)()
            assert eng._lib.kh_p2p_create_window(eng._handle, 1, 0, handle) == KH_ERR_UNSUPPORTED
            with pytest.raises(KrotovHipError) as err:
                eng.forward_update_sharded(chi, norms, prob.init, pulses, S, lam, lambda t: None, graph_chunk=0)
            assert err.value.code == KH_ERR_UNSUPPORTED
        eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    # outside the limits the C ABI refuses
    big = _random(33, 1, 1, 1, 2, 1)
    with pytest.raises(KrotovHipError) as err:
        _engine(big)
    assert err.value.code == KH_ERR_UNSUPPORTED
    assert _lib.load().kh_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['c4_d20', 'd32_two_cops_two_controls', 'd7'])
def test_sweeps_right_behind_a_kernel_that_left_nans_in_lds(name):
    """As test_kernels_do_not_read_uninitialised_lds (tests/test_hip_parity.py): ``kh_debug_occupy`` leaves all-ones (NaN)
    in the LDS of every CU; the sweeps launched right behind it must still be the oracle's."""
    import torch

    from krotov_amd import _lib

    case = CASES[name]()
    prob = case.oracle()
    pulses = _pulses(case)
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    norms = np.full(case.K, 0.5 / case.K)
    S, lam = [np.ones(len(case.dt))] * case.L, [1.0] * case.L
    ref_chi = ko.backward_sweep(prob, chi_T, pulses)
    ref = ko.forward_update_sweep(prob, ref_chi, norms, pulses, S, lam)
    eng = _engine(case)
    num_cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count

    def poison():
        _lib.check(eng._lib.kh_debug_occupy(eng._handle, 2 * num_cus, 0.05, eng._stream()))

    poison()
    chi = eng.backward(chi_T, np.array(pulses))
    poison()
    opt, psi_T, g_a = eng.forward_update(chi, norms, prob.init, np.array(pulses), np.array(S), np.array(lam))
    eng.check()
    assert np.abs(chi.cpu().numpy() - ref_chi).max() <= TOL
    assert np.abs(opt.cpu().numpy() - np.array(ref[0])).max() <= TOL
    assert np.abs(psi_T.cpu().numpy() - ref[1]).max() <= TOL
    eng.close()


# ---------------------------------------------------------------------------
# GPU: optimize_pulses(propagator=LindbladExpm()) against the reference's own loop (existing fixtures, produced by the
# reference on the Liouvillian of the very same operators)
# ---------------------------------------------------------------------------
def _optimize(ls, iters, chi=None, **kw):
    objectives, pulse_options = ls.objectives(krotov_amd)
    return krotov_amd.optimize_pulses(
        objectives, pulse_options, ls.tlist, propagator=krotov_amd.propagators.LindbladExpm(),
        chi_constructor=getattr(krotov_amd.functionals, 'chis_' + (chi or ls.chi)), iter_stop=iters,
        store_all_pulses=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('name,chi,tol', [('ref_c4_small', 're', 2e-11), ('ref_c4_small_hs', 'hs', 1e-10), ('ref_c4_full5', 're', 1e-9)])
def test_optimize_pulses_vs_reference_loop_goldens(name, chi, tol, caplog):
    from krotov_amd.engine import LAST_ENGINE

    g = golden(name)
    iters = int(g['iter_stop'])
    ls = configs.config_c4_lindblad() if name == 'ref_c4_full5' else configs.config_c4_lindblad(d=5, nt=201, n_logical=2)
    caplog.set_level(logging.INFO, logger='krotov')
    res = _optimize(ls, iters, chi=chi)
    assert LAST_ENGINE().kernel == 'lindblad/matrix'
    assert 'matrix-form engine' in caplog.text
    got = np.array([np.array(p) for p in res.all_pulses])
    assert got.shape == g['all_pulses'].shape
    scale = max(1.0, np.abs(g['all_pulses']).max())
    fw_T = np.array([np.asarray(s).ravel(order='F') for s in res.states])
    d_p = [np.abs(got[i] - g['all_pulses'][i]).max() for i in range(iters + 1)]
    d_t = [np.abs(np.array(res.tau_vals[i]) - g['tau_vals'][i]).max() for i in range(iters + 1)]
    d_s = np.abs(fw_T - g['fw_T']).max()
    print("lindblad_form %s: pulses %.2e tau %.2e final states %.2e" % (name, max(d_p), max(d_t), d_s))
    for i in range(iters + 1):
        assert d_p[i] < tol * scale, 'pulses after iteration %d' % i
        assert d_t[i] < tol, 'tau after iteration %d' % i
    assert d_s < tol
    assert np.asarray(res.states[0]).shape == (ls.d, ls.d)
    assert len(res.objectives[0].c_ops) == 1  # the caller's objectives, not a rewritten list


@pytest.mark.gpu
def test_ensemble_objectives_and_per_objective_operators_through_optimize_pulses():
    """``ensemble_objectives`` on a Lindblad-form objective: per-objective Hamiltonians, shared c_ops -- vs the oracle."""
    from krotov_amd.engine import LAST_ENGINE

    ls = configs.config_c4_lindblad(d=5, nt=41, n_logical=2)
    ls.tlist = np.linspace(0, 0.4, 41)
    objs, opts = ls.objectives(krotov_amd)
    ctl = objs[0].H[1][1]
    Hs = [[ls.H0 * f, [ls.H1, ctl]] for f in (0.98, 1.03)]
    ens = krotov_amd.objectives.ensemble_objectives(objs[:2], Hs)
    res = krotov_amd.optimize_pulses(ens, opts, ls.tlist, propagator=krotov_amd.propagators.LindbladExpm(),
                                     chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2, store_all_pulses=True)
    assert LAST_ENGINE().kernel == 'lindblad/matrix' and LAST_ENGINE().K == len(ens) == 6
    ops = [[liouvillian_dense(np.asarray(o.H[0]), o.c_ops), liouvillian_dense(ls.H1)] for o in ens]
    prob = ko.OracleProblem(ops, np.array([np.asarray(o.initial_state).ravel(order='F') for o in ens]),
                            np.array([np.asarray(o.target).ravel(order='F') for o in ens]), ls.tlist, True)
    _, gp, S = ko.initialize_controls(ls.controls, [ls.update_shape], ls.tlist)
    ref = ko.optimize(prob, gp, S, [ls.lambda_a], ko.chis_re, 2, norm=lambda p, c: float(np.linalg.norm(c)))
    assert np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() <= TOL
    assert np.abs(np.array(res.tau_vals) - ref['tau_vals']).max() <= TOL


# ---------------------------------------------------------------------------
# GPU: single steps and Objective.propagate
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('d,n_c', [(5, 1), (20, 2), (33, 1)])
def test_single_step_vs_dense_exponential(d, n_c):
    rng = np.random.default_rng(d)
    H0, H1 = configs.herm(rng, d, 3.0), configs.herm(rng, d, 1.0)
    cs = [0.3 * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) / np.sqrt(d) for _ in range(n_c)]
    rho, dt = _rho(rng, d), 0.1
    prop = krotov_amd.propagators.LindbladExpm()
    Lv = liouvillian_dense(H0 + 0.7 * H1, cs)
    out = prop([H0, [H1, 0.7]], rho, dt, c_ops=cs)
    want = (ko.expm_dense(Lv * dt) @ rho.ravel(order='F')).reshape(d, d, order='F')
    assert np.asarray(out).shape == (d, d) and np.abs(np.asarray(out) - want).max() <= 1e-12
    # backwards: the adjoint objective's operators, the adjoint generator
    out = prop([H0.conj().T, [H1.conj().T, 0.7]], rho, dt, c_ops=[c.conj().T for c in cs], backwards=True)
    want = (ko.expm_dense(Lv.conj().T * dt) @ rho.ravel(order='F')).reshape(d, d, order='F')
    assert np.abs(np.asarray(out) - want).max() <= 1e-12
    # no c_ops: HipExpm
    H0s, H1s = liouvillian_dense(H0), liouvillian_dense(H1)
    out = prop([H0s, [H1s, 0.7]], rho, dt)
    want = (ko.expm_dense((H0s + 0.7 * H1s) * dt) @ rho.ravel(order='F')).reshape(d, d, order='F')
    assert np.abs(np.asarray(out) - want).max() <= 1e-12


@pytest.mark.gpu
def test_objective_propagate_with_c_ops():
    from krotov_amd.engine import LAST_ENGINE

    ls = configs.config_sparse_lindblad_form(nt=21)
    obj = ls.objectives(krotov_amd)[0][0]
    res = obj.propagate(ls.tlist, propagator=krotov_amd.propagators.LindbladExpm())
    assert LAST_ENGINE().kernel == 'lindblad/matrix' and LAST_ENGINE().K == 1
    assert len(res.states) == len(ls.tlist) and res.num_collapse == 1
    _, gp, _ = ko.initialize_controls(ls.controls, [ls.update_shape], ls.tlist)
    # (Objective.propagate samples the controls at the interval mid-points' neighbours as the reference does: take the
    # pulses from its own conversion)
    from krotov_amd.conversions import control_onto_interval, discretize

    pulse = control_onto_interval(discretize(ls.controls[0], ls.tlist, args=({},)))
    state = ls.init[0].ravel(order='F')
    for n in range(len(ls.tlist) - 1):
        Lv = liouvillian_dense(ls.H0 + pulse[n] * ls.H1, ls.c_ops)
        state = ko.expm_dense(Lv * (ls.tlist[n + 1] - ls.tlist[n])) @ state
        assert np.abs(np.asarray(res.states[n + 1]).ravel(order='F') - state).max() <= 1e-12 * (n + 1)


# ---------------------------------------------------------------------------
# GPU: fallbacks
# ---------------------------------------------------------------------------
EXISTING_FAMILIES = ('generic', 'coop16/mfma', 'tile64q2/512', 'tile64/512', 'mini16/wave', 'mini4/wave', 'tile128/512',
                     'generic/mixed', 'tile64/256')


def _small_problem(d, K, nt, seed):
    rng = np.random.default_rng(seed)
    T = 0.05 * (nt - 1)
    ls = configs.LindbladSpec(
        name='small', H0=configs.herm(rng, d, 4.0), H1=configs.herm(rng, d, 2.0),
        c_ops=[0.3 * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) / np.sqrt(d)],
        init=np.array([_rho(rng, d) for _ in range(K)]), target=np.array([_rho(rng, d) for _ in range(K)]),
        tlist=np.linspace(0, T, nt), controls=[lambda t, args: 0.5 * np.sin(np.pi * t / T)],
        update_shape=lambda t: np.sin(np.pi * t / T) ** 2, lambda_a=0.5, chi='re')
    return ls


def _oracle_of(ls):
    ops = [[liouvillian_dense(ls.H0, ls.c_ops), liouvillian_dense(ls.H1)]] * ls.K
    prob = ko.OracleProblem(ops, np.array([r.ravel(order='F') for r in ls.init]),
                            np.array([r.ravel(order='F') for r in ls.target]), ls.tlist, True)
    _, gp, S = ko.initialize_controls(ls.controls, [ls.update_shape], ls.tlist)
    return prob, gp, S


@pytest.mark.gpu
def test_fallback_d33_runs_the_liouvillian(caplog):
    from krotov_amd.engine import LAST_ENGINE

    ls = _small_problem(33, 1, 3, 1)
    caplog.set_level(logging.INFO, logger='krotov')
    res = _optimize(ls, 1)
    assert 'Liouvillian fallback' in caplog.text
    assert LAST_ENGINE().kernel in EXISTING_FAMILIES and LAST_ENGINE().N == 33 * 33
    prob, gp, S = _oracle_of(ls)
    ref = ko.optimize(prob, gp, S, [ls.lambda_a], ko.chis_re, 1, norm=lambda p, c: float(np.linalg.norm(c)))
    assert np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() <= TOL
    assert np.abs(np.array(res.tau_vals) - ref['tau_vals']).max() <= TOL


@pytest.mark.gpu
def test_fallback_second_order_runs_the_liouvillian(caplog):
    from krotov_amd.engine import LAST_ENGINE

    ls = _small_problem(4, 3, 21, 2)
    caplog.set_level(logging.INFO, logger='krotov')
    res = _optimize(ls, 2, chi='sm', sigma=product_sigma(0.0, 2.0))
    assert 'Liouvillian fallback' in caplog.text
    assert LAST_ENGINE().kernel in EXISTING_FAMILIES
    prob, gp, S = _oracle_of(ls)
    ref = ko.optimize(prob, gp, S, [ls.lambda_a], ko.chis_sm, 2, norm=lambda p, c: float(np.linalg.norm(c)),
                      sigma=SigmaA(0.0, 2.0))
    assert np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() <= TOL
    assert np.abs(np.array(res.tau_vals) - ref['tau_vals']).max() <= TOL


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_kets_and_lindblad_form_objectives_mixed_run_the_mixed_engine(caplog):
    from krotov_amd.engine import LAST_ENGINE

    ls = _small_problem(4, 2, 11, 3)
    objs, opts = ls.objectives(krotov_amd)
    e0, e1 = np.eye(4, dtype=complex)[0], np.eye(4, dtype=complex)[1]
    objs.append(krotov_amd.Objective(initial_state=e0, target=e1, H=objs[0].H))
    caplog.set_level(logging.INFO, logger='krotov')
    res = krotov_amd.optimize_pulses(objs, opts, ls.tlist, propagator=krotov_amd.propagators.LindbladExpm(),
                                     chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1, store_all_pulses=True)
    assert 'Liouvillian fallback' in caplog.text and LAST_ENGINE().kernel == 'generic/mixed'
    assert np.asarray(res.states[0]).shape == (4, 4) and np.asarray(res.states[2]).shape == (4,)
    assert np.all(np.isfinite(np.array(res.all_pulses[1])))


@pytest.mark.gpu
def test_process_group_raises_for_the_matrix_engine():
    ls = _small_problem(4, 2, 5, 4)
    with pytest.raises(ValueError, match="process_group"):
        _optimize(ls, 1, process_group=object())
