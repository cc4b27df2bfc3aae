"""The two-terms-per-phase kernels at odd series degrees (kh_tile64q2.h), against the oracle.

Engines whose series is the exactly-Hermitian Chebyshev form hand ``kh_q2_sweep_store`` and ``kh_q2_forward_update`` a
threshold table with odd degrees; an odd degree m = 2P - 1 ends with the A product on s alone (P products instead of the
P + 1 of degree m + 1).  Every other kernel such an engine launches keeps the even-only table.

Cases (the smallest shapes at which this can go wrong): K = 3 objectives with control operators of different norm,
N = 64 and N = 37 (padded rows and columns), nine intervals, one control, Hermitian operators with ||H0|| = 1, so that
theta_kn = dt (1 + |eps_n| ||H1_k||) and the guess pulse -- a linear ramp -- walks theta across ONE threshold of the
table inside the sweep, at a different interval for every objective:

* ``odd_even``: across theta[m], degree m -> m + 1, for m = 1, 3, 5, 11, 13;
* ``even_odd``: across theta[m - 1], degree m - 1 -> m (m = 1: there is no degree 0; theta falls across theta[1],
  degree 2 -> 1);
* ``substeps``: theta = 2.2 ... 2.4 with theta_max = 1: three sub-steps of degree 13 each;
* ``refresh``: 70 intervals across theta[11] (the resident tiles restart after KH_Q2_REFRESH = 64 intervals).

Each case runs the forward sweep with storage, the backward sweep and the update sweep in its three forms
(``<false, true, *>``, ``<false, false, *>`` under KH_NO_ADJ=1, second order ``<true, false, *>``), and the
per-interval form of the update sweep (``kh_tile_forward_update``: a kernel that must NOT see an odd degree).  The
products counted by the engine must equal what the exported table predicts interval by interval, and exceed it under
KH_ODD_DEGREES=0 by exactly the skipped products.

Tolerances are the project's (tests/test_series_regimes.py): 1e-12 in Hilbert space, 1e-11 where
theta > 1 (sub-steps).
"""
import collections
import ctypes

import numpy as np
import pytest

from krotov_amd import _lib
from oracle import krotov_oracle as ko

Q2_STORE = 'kh_q2_sweep_store'
Q2_ADJ, Q2_FWD, Q2_SO = ('kh_q2_forward_update<false, true, true>', 'kh_q2_forward_update<false, false, true>',
                         'kh_q2_forward_update<true, false, true>')
SCALES = (0.15, 0.12, 0.10)  # ||H1_k||: every objective crosses the threshold, each on another interval

Case = collections.namedtuple('Case', 'id N M lo hi falling degrees nsub tol')


@pytest.fixture(scope='module')
def tabs():
    """(odd-capable thresholds, even-only thresholds) from the library's host code."""
    lib = _lib.load()
    th_o, c0, rows = (ctypes.c_double * 65)(), (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 32 * 2))()
    assert lib.kh_series_tables_odd(0.0, th_o, c0, rows) == 0
    th_e, ra = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
    assert lib.kh_series_tables(1, 0.0, th_e, ra) == 0
    return np.array(th_o), np.array(th_e)


def _cases():
    out = []
    for N in (64, 37):
        for m in (1, 3, 5, 11, 13):
            # theta of objective 0 runs over [0.93, 1.07] x the threshold, of objective 2 over [0.93, 1.023] x
            out.append(Case('n%d-m%d-odd_even' % (N, m), N, 9, ('tab', m), None, False, (m, m + 1), 1, 1e-12))
            if m == 1:
                out.append(Case('n%d-m1-even_odd' % N, N, 9, ('tab', 1), None, True, (2, 1), 1, 1e-12))
            else:
                out.append(Case('n%d-m%d-even_odd' % (N, m), N, 9, ('tab', m - 1), None, False, (m - 1, m), 1, 1e-12))
    out.append(Case('n64-substeps', 64, 9, ('theta', 2.2), None, False, (13,), 3, 1e-11))
    out.append(Case('n37-substeps', 37, 9, ('theta', 2.2), None, False, (13,), 3, 1e-11))
    out.append(Case('n64-refresh', 64, 70, ('tab', 11), None, False, (11, 12), 1, 1e-12))
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


def _hermitian(rng, N, norm):
    G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    H = (G + G.conj().T) / 2
    return H * (norm / np.linalg.norm(H, 2))


Problem = collections.namedtuple('Problem', 'ops dt pulses shapes lambdas init chi_T norms prob')


def _problem(N, M, K, dt, falling, scales, seed=11):
    rng = np.random.default_rng(seed)
    ops = [[_hermitian(rng, N, 1.0), _hermitian(rng, N, scales[k % len(scales)])] for k in range(K)]
    ramp = np.linspace(0.0, 1.0, M)
    pulses = [ramp[::-1].copy() if falling else ramp]
    unit = lambda a: a / np.linalg.norm(a, axis=1)[:, None]  # noqa: E731
    init = unit(rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N)))
    target = unit(rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N)))
    chi_T = unit(target + 0.5 * (rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))) / np.sqrt(N))
    tlist = np.concatenate([[0.0], np.cumsum(np.full(M, dt))])
    prob = ko.OracleProblem(ops, init, target, tlist)
    norms = np.full(K, 0.3 * min(1.0, 8.0 / K))  # (tests/test_series_regimes.py: chi_norms)
    return Problem(ops, np.diff(tlist), pulses, [np.linspace(0.2, 1.0, M)], [1.0], init, chi_T, norms, prob)


_refs = {}


def _reference(case, tabs):
    """The case's problem and the oracle's sweeps (once per case)."""
    if case.id in _refs:
        return _refs[case.id]
    kind, val = case.lo
    dt = 0.93 * tabs[0][val] if kind == 'tab' else val  # (||H0|| = 1)
    scales = SCALES if kind == 'tab' else (0.09, 0.07, 0.05)  # sub-steps: theta 2.2 ... 2.4, no threshold crossed
    p = _problem(case.N, case.M, 3, dt, case.falling, scales)
    ref = {'p': p}
    ref['psi_T'], ref['states'] = ko.forward_propagation(p.prob, p.pulses, store=True)
    ref['chi'] = ko.backward_sweep(p.prob, p.chi_T, p.pulses)
    out = ko.forward_update_sweep(p.prob, ref['chi'], p.norms, p.pulses, p.shapes, p.lambdas)
    ref['opt'], ref['upd_T'], ref['g_a'] = np.array(out[0]), out[1], np.array(out[2])
    rng = np.random.default_rng(5)
    older = [q * (1.0 + 0.2 * rng.standard_normal(q.shape)) for q in p.pulses]
    ref['prev'] = ko.forward_propagation(p.prob, older, store=True)[1]
    ref['sigma'] = -(1.0 + rng.random(case.M))
    out = ko.forward_update_sweep(p.prob, ref['chi'], p.norms, p.pulses, p.shapes, p.lambdas, sigma_vals=ref['sigma'],
                                  fw_prev=ref['prev'], store=True)
    ref['so_opt'], ref['so_T'], ref['so_g_a'], ref['so_store'] = np.array(out[0]), out[1], np.array(out[2]), out[3]
    _refs[case.id] = ref
    return ref


def _plan(theta, tab, theta_max=1.0):
    """(sub-steps, degree) per entry of theta: kh_degree_cached restated."""
    theta = np.asarray(theta, dtype=np.float64)
    nsub = np.where(theta > theta_max, np.ceil(theta * (1.0 / theta_max)), 1.0)
    th = theta / nsub
    deg = np.array([next((m for m in range(1, 64) if t <= tab[m]), 64) for t in th.ravel()]).reshape(th.shape)
    return nsub.astype(int), deg


def _products(op_norms, dt, pulse, tab, odd):
    """Matrix-vector products of one sweep's series under ``pulse`` (nt - 1 values), summed over the objectives: P + 1
    per sub-step of degree 2P or, without the odd form, 2P - 1; P at degree 2P - 1 in the odd form."""
    theta = dt[None, :] * (op_norms[:, :1] + op_norms[:, 1:2] * np.abs(np.asarray(pulse))[None, :])
    nsub, deg = _plan(theta, tab)
    margin = np.abs(theta / nsub - tab[deg]) / tab[deg]
    assert margin.min() > 1e-9, "a theta sits on a threshold: the prediction is not robust"
    per = (deg + 1) // 2 + np.where((deg % 2 == 1) & odd, 0, 1)
    return int((nsub * per).sum()), deg, nsub


def _engine(p, **kw):
    from krotov_amd.engine import HipKrotovEngine

    return HipKrotovEngine(p.ops, p.dt, **kw)


def _update_devs(got, ref_opt, ref_T, ref_ga, tag):
    opt, upd_T, g_a = got
    scale = max(1.0, np.abs(ref_opt).max())
    return {tag + 'opt': np.abs(opt.cpu().numpy() - ref_opt).max() / scale,
            tag + 'upd_T': np.abs(upd_T.cpu().numpy() - ref_T).max(),
            tag + 'g_a': np.abs(g_a.cpu().numpy() - ref_ga).max() / max(1.0, np.abs(ref_ga).max())}


@pytest.mark.gpu
@pytest.mark.parametrize('cid', CASE_IDS)
def test_q2_odd_degree_sweeps(cid, tabs, monkeypatch):
    import torch

    case = CASES[CASE_IDS.index(cid)]
    tab_o, tab_e = tabs
    ref = _reference(case, tabs)
    p = ref['p']
    pulses, S, lam = np.array(p.pulses), np.array(p.shapes), np.array(p.lambdas)
    K, M = 3, case.M
    dev = {}
    _lib.forget_launched_kernels()
    eng = _engine(p)
    assert eng.kernel == 'tile64q2/512'
    # the witness: under the guess pulse objective 0 runs exactly the degrees the case is about, odd ones among them
    want, deg, nsub = _products(eng.op_norms, p.dt, pulses[0], tab_o, True)
    want_even, deg_e, _ = _products(eng.op_norms, p.dt, pulses[0], tab_e, False)
    for k in range(K):
        seq = [int(d) for i, d in enumerate(deg[k]) if i == 0 or d != deg[k][i - 1]]
        assert tuple(seq) == case.degrees, (k, deg[k])
    assert nsub.min() == nsub.max() == case.nsub
    n_odd = int(np.sum(nsub * (deg % 2 == 1)))
    assert n_odd > 0 and want_even == want + n_odd and np.all(deg_e % 2 == 0)
    # ---- plain sweeps ----
    psi_T, states = eng.forward(pulses, p.init, store=True)
    assert eng.stats()['matvecs'] == want and eng.stats()['intervals'] == M
    dev['states'] = np.abs(states.cpu().numpy() - ref['states']).max()
    dev['psi_T'] = np.abs(psi_T.cpu().numpy() - ref['psi_T']).max()
    chi = eng.backward(p.chi_T, pulses)
    assert eng.stats()['matvecs'] == want
    dev['chi'] = np.abs(chi.cpu().numpy() - ref['chi']).max()
    # ---- update sweep, sums on the adjoint side: kh_q2_forward_update<false, true, *> ----
    got = eng.forward_update(chi, p.norms, p.init, pulses, S, lam)
    eng.check()
    dev.update(_update_devs(got, ref['opt'], ref['upd_T'], ref['g_a'], 'adj/'))
    # (the series under the UPDATED pulse, and one product per interval and objective for the update sums)
    want_upd, deg_u, _ = _products(eng.op_norms, p.dt, got[0].cpu().numpy()[0], tab_o, True)
    assert np.any(deg_u % 2 == 1)
    assert eng.stats()['matvecs'] == want_upd + K * M
    # ---- the per-interval form: kh_tile_forward_update reads the even-only table ----
    got2 = eng.forward_update_sharded(chi, p.norms, p.init, pulses, S, lam, lambda x: x, graph_chunk=0)
    eng.check()
    dev.update(_update_devs(got2, ref['opt'], ref['upd_T'], ref['g_a'], 'step/'))
    # ---- second order: kh_q2_forward_update<true, false, *> ----
    store = torch.full((K, M + 1, case.N), float('nan'), dtype=torch.complex128, device=eng.device)
    eng.set_second_order(ref['prev'], store, ref['sigma'])
    got = eng.forward_update(chi, p.norms, p.init, pulses, S, lam)
    eng.check()
    dev.update(_update_devs(got, ref['so_opt'], ref['so_T'], ref['so_g_a'], 'so/'))
    dev['so/store'] = np.abs(store.cpu().numpy() - ref['so_store']).max()
    want_so, deg_s, _ = _products(eng.op_norms, p.dt, got[0].cpu().numpy()[0], tab_o, True)
    assert np.any(deg_s % 2 == 1)
    assert eng.stats()['matvecs'] == want_so + K * M
    eng.close()
    # ---- sums on the forward side: kh_q2_forward_update<false, false, *> ----
    monkeypatch.setenv('KH_NO_ADJ', '1')
    eng = _engine(p)
    got = eng.forward_update(chi, p.norms, p.init, pulses, S, lam)
    eng.check()
    dev.update(_update_devs(got, ref['opt'], ref['upd_T'], ref['g_a'], 'fwd/'))
    assert eng.stats()['matvecs'] == _products(eng.op_norms, p.dt, got[0].cpu().numpy()[0], tab_o, True)[0] + K * M
    eng.close()
    monkeypatch.delenv('KH_NO_ADJ')
    launched = _lib.kernel_instantiations(launched_only=True)
    for name in (Q2_STORE, Q2_ADJ, Q2_FWD, Q2_SO):
        assert name in launched, launched
    assert any(n.startswith('kh_tile_forward_update<') for n in launched), launched
    # ---- KH_ODD_DEGREES=0: the even-only table for these kernels too -- more products, the same results ----
    monkeypatch.setenv('KH_ODD_DEGREES', '0')
    eng = _engine(p)
    assert eng.kernel == 'tile64q2/512'
    psi_T, states = eng.forward(pulses, p.init, store=True)
    assert eng.stats()['matvecs'] == want_even > want
    dev['off/states'] = np.abs(states.cpu().numpy() - ref['states']).max()
    chi0 = eng.backward(p.chi_T, pulses)
    assert eng.stats()['matvecs'] == want_even
    dev['off/chi'] = np.abs(chi0.cpu().numpy() - ref['chi']).max()
    got = eng.forward_update(chi, p.norms, p.init, pulses, S, lam)
    eng.check()
    dev.update(_update_devs(got, ref['opt'], ref['upd_T'], ref['g_a'], 'off/'))
    off_upd = _products(eng.op_norms, p.dt, got[0].cpu().numpy()[0], tab_e, False)[0]
    assert eng.stats()['matvecs'] == off_upd + K * M > want_upd + K * M
    eng.close()
    print('q2_odd_degrees %s: degrees %s x %d sub-steps, products %d (even-only %d); %s' % (
        case.id, case.degrees, case.nsub, want, want_even, ' '.join('%s %.1e' % kv for kv in dev.items())))
    assert max(dev.values()) < case.tol, dev


@pytest.mark.gpu
def test_more_objectives_than_workgroups_take_turns(tabs, monkeypatch):
    """K = 260: the plain sweeps run kh_q2_sweep_store in turns -- at odd degrees --, the update sweep the
    one-term-per-phase kernel with two workgroups per CU, which keeps the even-only table.  All against the oracle."""
    tab_o, tab_e = tabs
    K, N, M = 260, 12, 9
    p = _problem(N, M, K, 0.93 * tab_o[11], False, SCALES, seed=23)
    pulses, S, lam = np.array(p.pulses), np.array(p.shapes), np.array(p.lambdas)
    norms = p.norms
    _lib.forget_launched_kernels()
    eng = _engine(p)
    assert eng.kernel == 'tile64/256'
    want, deg, _ = _products(eng.op_norms, p.dt, pulses[0], tab_o, True)
    want_even = _products(eng.op_norms, p.dt, pulses[0], tab_e, False)[0]
    assert set(np.unique(deg)) == {11, 12}
    dev = {}
    psi_T, states = eng.forward(pulses, p.init, store=True)
    assert eng.stats()['matvecs'] == want < want_even
    ref_T, ref_states = ko.forward_propagation(p.prob, p.pulses, store=True)
    dev['states'] = np.abs(states.cpu().numpy() - ref_states).max()
    dev['psi_T'] = np.abs(psi_T.cpu().numpy() - ref_T).max()
    chi = eng.backward(p.chi_T, pulses)
    assert eng.stats()['matvecs'] == want
    ref_chi = ko.backward_sweep(p.prob, p.chi_T, p.pulses)
    dev['chi'] = np.abs(chi.cpu().numpy() - ref_chi).max()
    got = eng.forward_update(chi, norms, p.init, pulses, S, lam)
    eng.check()
    out = ko.forward_update_sweep(p.prob, ref_chi, norms, p.pulses, p.shapes, p.lambdas)
    dev.update(_update_devs(got, np.array(out[0]), out[1], np.array(out[2]), 'upd/'))
    eng.close()
    launched = _lib.kernel_instantiations(launched_only=True)
    assert Q2_STORE in launched and 'kh_tile_forward_update<2, 1, false, true>' in launched, launched
    assert not any(n.startswith('kh_q2_forward_update<') for n in launched), launched
    print('q2_odd_degrees K = 260: products %d (even-only %d); %s' % (want, want_even, ' '.join('%s %.1e' % kv for kv in dev.items())))
    assert max(dev.values()) < 1e-12, dev
