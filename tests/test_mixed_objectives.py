"""Objectives of different dimension or kind on one engine (kh_engine_create_mixed, kernel family "generic/mixed").

The reference propagates every objective on its own (optimize.py:254-261, 806-911), so its objective lists may mix
dimensions and kinds; tests/golden/ref_mixed.npz holds what its own loop computes on such lists
(tests/golden/make_mixed_goldens.py).  The sweeps are also compared with an independent restatement: every objective
zero-padded to the stride S, and every Liouvillian L written as the Hilbert-space operator i L (f = -i then gives
-i (i L) = L forward and +i (i L)^+ = L^+ backward, and the Hilbert mu factor 1 gives mu = i L), so the oracle's
uniform Hilbert-space sweeps apply unchanged.
"""
import types

import numpy as np
import pytest

from helpers import golden
from oracle import krotov_oracle as ko
from qobj_double import QobjDouble

import krotov_amd
from krotov_amd import configs
from krotov_amd.mixed import Layout, layout_of

RUNS = {'re': ('re', False), 'sm': ('sm', False), 'so': ('re', True)}


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------


def _pad_op(op, S):
    out = np.zeros((S, S), dtype=np.complex128)
    n = op.shape[0]
    out[:n, :n] = op
    return out


def _pad_vec(v, S):
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    out = np.zeros(S, dtype=np.complex128)
    out[:v.size] = v
    return out


def _vec(state):
    arr = np.asarray(state, dtype=np.complex128)
    return arr.ravel(order='F') if arr.ndim == 2 and arr.shape[0] == arr.shape[1] and arr.shape[0] > 1 else arr.ravel()


def oracle_adapter(spec):
    """The oracle problem of a config_mixed spec: zero-padded to S, Liouvillians L as i L (Hilbert form)."""
    S = spec.N
    ops = []
    for k in range(spec.K):
        scale = 1j if spec.kinds[k] else 1.0
        ops.append([_pad_op(scale * spec.H0[k], S)] + [_pad_op(scale * spec.Hc[k][l], S) for l in range(spec.L)])
    init = np.array([_pad_vec(_vec(s), S) for s in spec.init])
    target = np.array([_pad_vec(_vec(s), S) for s in spec.target])
    return ko.OracleProblem(ops, init, target, spec.tlist, is_super=False)


def spec_controls(spec):
    _, gp, shapes = ko.initialize_controls(spec.controls, [spec.update_shape] * spec.L, spec.tlist)
    return gp, shapes, [spec.lambda_a] * spec.L


class ConstSigma(krotov_amd.second_order.Sigma):
    def __init__(self, value):
        self.value = value

    def __call__(self, t):
        return self.value

    def refresh(self, **kwargs):
        pass


# ---------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------


def test_layout_pads_and_unpads_kets_density_matrices_and_qobjs():
    layout = Layout([3, 9, 4, 4], [False, True, False, True])
    assert layout.mixed and layout.stride == 9
    rng = np.random.default_rng(1)
    ket = rng.standard_normal((3, 1)) + 1j * rng.standard_normal((3, 1))
    rho = rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))
    qket = QobjDouble(rng.standard_normal((4, 1)) + 0j)
    qrho = QobjDouble(rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2)))
    for k, st in enumerate([ket, rho, qket, qrho]):
        row = layout.vector(st, k)
        n = layout.dims[k]
        assert row.shape == (9,)
        assert np.all(row[n:] == 0)
        full = st.full() if hasattr(st, 'full') else st
        assert np.array_equal(row[:n], full.ravel(order='F') if layout.kinds[k] else full.ravel())
        # anything behind N_k is cut off on the way back; the state keeps its class and shape
        back = layout.state(np.concatenate([row[:n], np.full(9 - n, 7.0 + 7j)]), k, st)
        assert type(back) is type(st)
        back_arr = back.full() if hasattr(back, 'full') else back
        assert back_arr.shape == full.shape and np.array_equal(back_arr, full)
    assert layout.vector('PE', 0) is None
    assert layout.vector(rho, 0) is None  # a density matrix is no state of a Hilbert-space objective
    assert not Layout([4, 4], [True, True]).mixed


def test_layout_kind_precedence():
    spec = configs.config_mixed('same_n')
    objectives, _ = configs.mixed_to_objectives(spec, krotov_amd)
    expm, HipExpm = krotov_amd.propagators.expm, krotov_amd.propagators.HipExpm
    # 3. the initial state's shape: a 4-level ket next to a (2, 2) density matrix
    assert layout_of(objectives, expm).kinds == [False, True]
    # 1. the objective's own HipExpm(liouville=...) in a propagator list
    assert layout_of(objectives, [HipExpm(liouville=True), expm]).kinds == [True, True]
    assert layout_of(objectives, [expm, HipExpm(liouville=False)]).kinds == [False, False]
    # 2. .type of the first drift operator (ahead of the state's shape)
    class Typed:
        def __init__(self, arr, type_):
            self.shape, self.type = arr.shape, type_

    typed = [types.SimpleNamespace(H=[Typed(spec.H0[0], 'super')] + objectives[0].H[1:],
                                   initial_state=objectives[0].initial_state),
             types.SimpleNamespace(H=[Typed(spec.H0[1], 'oper')] + objectives[1].H[1:],
                                   initial_state=objectives[1].initial_state)]
    assert layout_of(typed, expm).kinds == [True, False]
    assert layout_of(typed, [expm, HipExpm(liouville=True)]).kinds == [True, True]


def test_mixed_lists_refuse_sharding_before_any_collective():
    spec = configs.config_mixed('dims', nt=11)
    objectives, opts = configs.mixed_to_objectives(spec, krotov_amd)
    with pytest.raises(ValueError, match="different dimension or kind"):
        # (the group is never touched: the error comes first, the same on every rank)
        krotov_amd.optimize_pulses(objectives, opts, spec.tlist, propagator=krotov_amd.propagators.expm,
                                   chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1,
                                   process_group=object())


@pytest.mark.parametrize('case', ['dims', 'same_n'])
def test_adapter_reproduces_the_reference_loop(case):
    """The restatement (padding + i L) run through the oracle gives the reference's pulses and tau."""
    ref = golden('ref_mixed')
    spec = configs.config_mixed(case, nt=int(ref['nt']))
    prob = oracle_adapter(spec)
    gp, shapes, lam = spec_controls(spec)
    pulses = [np.array(p) for p in gp]
    fw_T = ko.forward_propagation(prob, pulses, use_scipy=True)
    tau = ko.tau_vals(prob, fw_T)
    nrm = lambda p, c: float(np.linalg.norm(c))  # noqa: E731
    all_pulses = ref['%s_re_all_pulses' % case]
    taus = ref['%s_re_tau_vals' % case]
    np.testing.assert_allclose(tau, taus[0], rtol=0, atol=1e-11)
    for it in range(1, int(ref['iter_stop']) + 1):
        pulses, fw_T, tau, _ = ko.krotov_iteration(prob, pulses, shapes, lam, fw_T, tau, ko.chis_re, use_scipy=True,
                                                   norm=nrm)
        np.testing.assert_allclose(np.array(pulses), all_pulses[it], rtol=0, atol=1e-11)
        np.testing.assert_allclose(tau, taus[it], rtol=0, atol=1e-11)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize('run', list(RUNS))
@pytest.mark.parametrize('case', ['dims', 'same_n'])
def test_optimize_pulses_matches_the_reference(case, run):
    """optimize_pulses with the device propagator on a list that mixes dimensions (N = 3, 5, 9) or kinds (a 4-level
    ket next to a damped qubit density matrix): pulses and tau after every iteration as the reference's own loop.
    Before mixed engines, the first raised and the second propagated one objective with the other's factors."""
    from krotov_amd.engine import LAST_ENGINE

    ref = golden('ref_mixed')
    chi, so = RUNS[run]
    spec = configs.config_mixed(case, nt=int(ref['nt']), chi=chi)
    objectives, opts = configs.mixed_to_objectives(spec, krotov_amd)
    res = krotov_amd.optimize_pulses(
        objectives, opts, spec.tlist, propagator=krotov_amd.propagators.expm,
        chi_constructor=getattr(krotov_amd.functionals, 'chis_' + chi), iter_stop=int(ref['iter_stop']),
        store_all_pulses=True, sigma=ConstSigma(float(ref['so_sigma'])) if so else None)
    assert LAST_ENGINE().kernel == 'generic/mixed'
    assert LAST_ENGINE().dims == spec.dims
    want_pulses = ref['%s_%s_all_pulses' % (case, run)]
    got = np.array([np.array(p) for p in res.all_pulses])
    assert got.shape == want_pulses.shape
    np.testing.assert_allclose(got, want_pulses, rtol=0, atol=1e-11)
    np.testing.assert_allclose(np.array(res.tau_vals), ref['%s_%s_tau_vals' % (case, run)], rtol=0, atol=1e-11)
    # final states in each objective's own shape, as the reference's
    want_T = ref['%s_%s_fw_T' % (case, run)]
    for k, st in enumerate(res.states):
        assert np.shape(st) == np.shape(spec.init[k])
        np.testing.assert_allclose(_vec(st), want_T[k, :spec.dims[k]], rtol=0, atol=1e-11)


def _padded_garbage(rows, S, rng):
    """rows zero-padded to S, then random values behind N_k (the engine must not read them)."""
    out = np.array([_pad_vec(r, S) for r in rows])
    for k, r in enumerate(rows):
        n = np.asarray(r).size
        out[k, n:] = rng.standard_normal(S - n) + 1j * rng.standard_normal(S - n)
    return out


def _engine_ops(spec):
    return [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]


def _assert_padding_zero(arr, dims):
    for k, n in enumerate(dims):
        assert np.all(arr[k, ..., n:] == 0), "objective %d: non-zero padding" % k


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['dims', 'same_n'])
def test_sweeps_match_the_restatement(case):
    """Stored forward and backward trajectories, update-sweep pulses, g_a and psi(T), first and second order, against
    the padded Hilbert-form oracle; every padding entry written by the engine is exactly zero, whatever the inputs
    held there."""
    from krotov_amd.engine import HipKrotovEngine

    spec = configs.config_mixed(case, nt=61)
    prob = oracle_adapter(spec)
    S, dims = spec.N, spec.dims
    rng = np.random.default_rng(5)
    gp, shapes, lam = spec_controls(spec)
    pulses = np.array(gp)
    eng = HipKrotovEngine(_engine_ops(spec), np.diff(spec.tlist), is_super=spec.kinds)
    assert eng.kernel == 'generic/mixed' and eng.mixed and eng.dims == dims and eng.N == S
    init = _padded_garbage([_vec(s) for s in spec.init], S, rng)
    psi_T, states = eng.forward(pulses, init, store=True)
    psi_T, states = psi_T.cpu().numpy(), states.cpu().numpy()
    fw_T, fw_states = ko.forward_propagation(prob, list(pulses), store=True)
    np.testing.assert_allclose(states, fw_states, rtol=0, atol=1e-12)
    np.testing.assert_allclose(psi_T, fw_T, rtol=0, atol=1e-12)
    _assert_padding_zero(states, dims)
    _assert_padding_zero(psi_T, dims)

    chi_T = np.array([_pad_vec(0.5 * _vec(t), S) for t in spec.target])
    chi_norms = np.linalg.norm(chi_T, axis=1)
    chi_T /= chi_norms[:, None]
    chi_in = chi_T.copy()
    for k, n in enumerate(dims):
        chi_in[k, n:] = rng.standard_normal(S - n)
    chi_store = eng.backward(chi_in, pulses).cpu().numpy()
    want_chi = ko.backward_sweep(prob, chi_T, list(pulses))
    np.testing.assert_allclose(chi_store, want_chi, rtol=0, atol=1e-12)
    _assert_padding_zero(chi_store, dims)

    opt, psi_T, g_a = (x.cpu().numpy() for x in eng.forward_update(chi_store, chi_norms, init, pulses, shapes, lam))
    w_opt, w_T, w_ga = ko.forward_update_sweep(prob, want_chi, chi_norms, list(pulses), shapes, lam)
    np.testing.assert_allclose(opt, np.array(w_opt), rtol=0, atol=1e-12)
    np.testing.assert_allclose(g_a, w_ga, rtol=0, atol=1e-12)
    np.testing.assert_allclose(psi_T, w_T, rtol=0, atol=1e-12)
    _assert_padding_zero(psi_T, dims)

    # second order: sigma term and the stored forward states under the optimized pulses
    import torch

    sig = np.full(len(spec.tlist) - 1, -1.5)
    fw_prev = eng.dev(states, torch.complex128)
    fw_store = torch.empty_like(fw_prev)
    eng.set_second_order(fw_prev, fw_store, sig)
    opt2, psi2, ga2 = (x.cpu().numpy() for x in eng.forward_update(chi_store, chi_norms, init, pulses, shapes, lam))
    eng.set_second_order()
    w_opt2, w_T2, w_ga2, w_store = ko.forward_update_sweep(prob, want_chi, chi_norms, list(pulses), shapes, lam,
                                                           sigma_vals=sig, fw_prev=fw_states, store=True)
    np.testing.assert_allclose(opt2, np.array(w_opt2), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ga2, w_ga2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(psi2, w_T2, rtol=0, atol=1e-12)
    store = fw_store.cpu().numpy()
    np.testing.assert_allclose(store, w_store, rtol=0, atol=1e-12)
    _assert_padding_zero(store, dims)


def _many_objectives(K=300, nt=41, seed=11):
    """K objectives alternating N = 4 and N = 6 (kets), one control: more objectives than workgroups."""
    rng = np.random.default_rng(seed)
    spec = configs.config_mixed('dims', nt=nt)
    H0, Hc, init, target, kinds = [], [], [], [], []
    for k in range(K):
        d = 4 if k % 2 == 0 else 6
        H0.append(configs.herm(rng, d, 1.0))
        Hc.append([configs.herm(rng, d, 0.4)])
        v = rng.standard_normal((d, 1)) + 1j * rng.standard_normal((d, 1))
        init.append(v / np.linalg.norm(v))
        target.append(np.eye(d, 1, dtype=np.complex128))
        kinds.append(False)
    spec.__dict__.update(H0=H0, Hc=Hc, init=init, target=target, kinds=kinds, dims=[h.shape[0] for h in H0],
                         is_super=kinds, K=K, N=6)
    return spec


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['dims', 'many', 'wide'])
def test_single_launch_and_per_interval_updates_agree(which):
    """The single-launch update sweep and the per-interval form (graph_chunk=0 and the default HIP-graph chunks) agree;
    with more objectives than workgroups (300 of N = 4 and 6) and with N_k > 96 (the scratch generator).  The
    per-interval form is checked against the restatement too."""
    from krotov_amd.engine import HipKrotovEngine

    spec = {'dims': lambda: configs.config_mixed('dims', nt=201), 'many': lambda: _many_objectives(nt=41),
            'wide': lambda: configs.config_mixed('wide', nt=41)}[which]()
    S = spec.N
    gp, shapes, lam = spec_controls(spec)
    pulses = np.array(gp)
    eng = HipKrotovEngine(_engine_ops(spec), np.diff(spec.tlist), is_super=spec.kinds)
    assert eng.kernel == 'generic/mixed'
    init = np.array([_pad_vec(_vec(s), S) for s in spec.init])
    chi_T = np.array([_pad_vec(_vec(t), S) for t in spec.target])
    chi_norms = np.linalg.norm(chi_T, axis=1)
    chi_store = eng.backward(chi_T / chi_norms[:, None], pulses)
    one = [x.cpu().numpy() for x in eng.forward_update(chi_store, chi_norms, init, pulses, shapes, lam)]
    eng.check()
    for chunk in (0, None):
        per = [x.cpu().numpy() for x in eng.forward_update_sharded(chi_store, chi_norms, init, pulses, shapes, lam,
                                                                    all_reduce=lambda x: None, graph_chunk=chunk)]
        for a, b in zip(one, per):
            np.testing.assert_allclose(b, a, rtol=0, atol=1e-13)
    _assert_padding_zero(one[1], spec.dims)
    prob = oracle_adapter(spec)
    w_opt, w_T, w_ga = ko.forward_update_sweep(prob, chi_store.cpu().numpy(), chi_norms, list(pulses), shapes, lam)
    np.testing.assert_allclose(one[0], np.array(w_opt), rtol=0, atol=1e-12)
    np.testing.assert_allclose(one[1], w_T, rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_hilbert_only_mix_equals_padding_on_the_uniform_engine(monkeypatch):
    """Kets of N = 40 and 100 (scratch generator) and a 3- and 5-level pair: the mixed engine and today's uniform
    engine on the zero-padded problem (generic kernels, Taylor series, forward-side sums) agree."""
    from krotov_amd.engine import HipKrotovEngine

    for case in ('wide', 'dims_kets'):
        spec = configs.config_mixed('wide' if case == 'wide' else 'dims', nt=41)
        if case == 'dims_kets':  # the two ket objectives of the 'dims' case
            for name in ('H0', 'Hc', 'init', 'target', 'kinds', 'dims'):
                setattr(spec, name, getattr(spec, name)[:2])
            spec.K, spec.N = 2, 5
        S = spec.N
        gp, shapes, lam = spec_controls(spec)
        pulses = np.array(gp)
        init = np.array([_pad_vec(_vec(s), S) for s in spec.init])
        chi_T = np.array([_pad_vec(_vec(t), S) for t in spec.target])
        chi_norms = np.linalg.norm(chi_T, axis=1)
        chi_T /= chi_norms[:, None]
        mixed = HipKrotovEngine(_engine_ops(spec), np.diff(spec.tlist), is_super=False)
        assert mixed.kernel == 'generic/mixed'
        with monkeypatch.context() as m:
            for name, val in (('KH_KERNEL', 'generic'), ('KH_TAYLOR', '1'), ('KH_GEN_ADJ', '0')):
                m.setenv(name, val)
            padded = HipKrotovEngine([[_pad_op(op, S) for op in row] for row in _engine_ops(spec)], np.diff(spec.tlist),
                                     is_super=False)
        assert padded.kernel == 'generic' and not padded.mixed
        out = []
        for eng in (mixed, padded):
            psi_T, states = eng.forward(pulses, init, store=True)
            chi_store = eng.backward(chi_T, pulses)
            opt, psi_u, g_a = eng.forward_update(chi_store, chi_norms, init, pulses, shapes, lam)
            out.append([x.cpu().numpy() for x in (psi_T, states, chi_store, opt, psi_u, g_a)])
        for a, b in zip(*out):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_uniform_problems_never_run_the_mixed_kernels():
    from krotov_amd.engine import LAST_ENGINE, HipKrotovEngine

    spec = configs.config_c1(nt=41)
    objectives, opts = configs.spec_to_objectives(spec, krotov_amd)
    krotov_amd.optimize_pulses(objectives, opts, spec.tlist, propagator=krotov_amd.propagators.expm,
                               chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1)
    assert LAST_ENGINE().kernel != 'generic/mixed' and not LAST_ENGINE().mixed
    # the same dimension and kind, given per objective: the uniform engine
    rng = np.random.default_rng(2)
    ops = [[configs.herm(rng, 6, 1.0), configs.herm(rng, 6, 0.3)] for _ in range(3)]
    eng = HipKrotovEngine(ops, np.full(10, 0.1), is_super=[False, False, False])
    assert eng.kernel != 'generic/mixed' and not eng.mixed and eng.is_super is False
    # the mixed engine's limits
    mixed = HipKrotovEngine([ops[0], [configs.herm(rng, 4, 1.0), None]], np.full(10, 0.1))
    assert mixed.kernel == 'generic/mixed' and mixed.dims == [6, 4] and mixed.N == 6
    with pytest.raises(krotov_amd._lib.KrotovHipError):
        mixed.set_update_workgroups(8)
    import scipy.sparse as sp

    with pytest.raises(ValueError, match="dense operators"):
        HipKrotovEngine([[sp.csr_matrix(ops[0][0])], [sp.csr_matrix(np.eye(4))]], np.full(10, 0.1))
