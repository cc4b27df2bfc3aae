"""Every kernel family under a caller-set series tolerance and under caller-set (or absent) norm bounds.

Every engine constructor of the C ABI takes ``tol`` (the truncation tolerance per sub-step), ``theta_max`` and ``op_norms``
(the caller's norm bounds, or NULL: the engine computes Frobenius norms).  ``tests/test_series_regimes.py`` covers
``theta_max``; this module covers the other two, on that module's family x base-case table (its smallest base case per
family, ``ramp`` regime: non-uniform grid, degrees rise and fall, sub-steps).

At the default tolerance every fixture runs at degree 12 ... 16.  At ``tol = 1e-4`` the degrees are 1 ... 6, change from
interval to interval and sub-steps occur at low degree, so the kernels' edge branches -- a single phase, m = 1, odd
degrees rounded up, coefficient-row loops that run zero times, the degree-bracket cache walking down from its hint of 12
-- are the main path.

Three references:

* the exact oracle (``oracle/krotov_oracle.py``); a tolerance run must stay within ``series_oracle.tolerance_bound`` of
  it -- a bound derived from the tolerance, the plan and the problem (its docstring), plus the project's rounding
  tolerance -- and, at ``tol = 1e-4``, be more than 100 times farther from it than the default run (an engine that
  ignores ``tol`` fails that);
* the series oracle (``tests/series_oracle.py``): the same sweeps with every step replaced by ``nsub`` sub-steps of the
  polynomial the library exports for the planned degree.  An engine that uses that table agrees with it to the project's
  rounding tolerance (1e-12 in Hilbert space, 1e-11 in Liouville space and in the ``ramp`` regime) at ANY ``tol``;
* the host plan's product count (``eng.stats()['matvecs']``), which proves which table ran.

Exact-polynomial check (the row names its tables; one product per term unless noted):
generic, generic/csr, generic/mixed (Taylor), tile64/512, tile64x/512, tile128/512, lindblad/matrix (Taylor),
ell / ellstream / ellglobal / ellsplit (Chebyshev form, cap 6), replica16/wave with two controls, the update sweeps of
tile64/256 and tile64/stream, and tile64q2/512 -- whose kernels also run the plain sweeps of tile64/256 and
tile64/stream -- with the table with odd degrees (P products at degree 2P - 1, P + 1 at 2P), the even-only table
(KH_ODD_DEGREES=0) and Taylor's (KH_TAYLOR=1: an odd degree m is evaluated as m + 1).

Bound only (bound, ordering of the product counts, repeatability): mini16/wave and mini4/wave (A^2-chain forms; in
mini4/wave every objective also takes the sub-steps and the degree of the largest theta of its wave, which the bound's
plan restates), ens64/mfma and coop16/mfma (A^2-chain forms that round up; which table the cooperative kernels get
depends on a Hermitian defect measured on the device that the library does not export).

The replica batch (tests/test_replicas.py's `regimes`, two controls) has the exact-polynomial check, the bound and the
counts; its second-order twin (tests/test_replicas_second_order.py's harness) takes the engine's own forward sweep as
the older trajectory, so its reference is the series oracle alone.

The update sweeps here use boundary co-states and ||chi_k|| of this module's own (``reference``): with the random
co-states of tests/test_series_regimes.py the update sums add up like sqrt(K) while any worst-case bound adds up like K,
and the feedback of the pulse error into the states makes the bound blow up -- it would be empty.

Measured error / tol of the exported polynomials at theta = theta[m] (``test_tables``, which prints them; the largest
over the degrees with theta[m] below the form's cap -- Taylor: below 8 --, 801 grid points per branch, extended
precision), tol = 1e-4 / 1e-8 / 1e-12:
    taylor 1.00 / 1.00 / 1.00     real, caps 2, 4 and 6 alike: 0.98 / 1.00 / 1.00     odd 1.00 / 1.00 / 1.00
    defect 0.01: 0.34 / 0.39 / 0.41     defect 0.05: 0.36 / 0.41 / 0.41  (the bound carries Crouzeix's constant 1 + sqrt 2)
No lower limit is asserted.  The one excess over ``tol`` is rounding, not truncation: degree 1 of the odd table at 1e-12
(c_0 = 1 - 1e-12 as a double) is 2e-5 tol beyond it.
"""
import collections
import re
import os

import numpy as np
import pytest

import helpers as hp
import series_oracle as so
import test_series_regimes as tsr
from oracle import krotov_oracle as ko

TOLS = (1e-4, 1e-8)

# what a row adds to tests/test_series_regimes.py's Row: the table of the update sweep and of the plain sweeps (None:
# bound only), which of the two run the two-terms-per-phase kernels, a row split (ellsplit)
Spec = collections.namedtuple('Spec', 'row table store_table q2_update q2_store row_split')

SPECS = {}


def _absent_L2():
    """tests/test_absent_controls.py's tile64/512 case with two controls (control 0 absent from objective 0, control 1 from
    objective 1) on a grid long enough for a ramp."""
    import test_absent_controls as tac
    from krotov_amd import configs

    return tac._drop(configs.config_c5(K=4, N=17, nt=12, L=2, distinct=True), [(0, 0), (1, 1)])


tsr.BASES.setdefault('absent_L2', (_absent_L2, 'dense'))


def spec(family, base, theta_max=1.0, env=None, tag='', so=False, table=None, store_table=None, q2=(False, False),
         regime='ramp', row_split=None, into=SPECS):
    rid = '%s-%s%s-%s' % (family, base, tag, regime)
    row = tsr.Row(rid, family, base, tsr.BASES[base][1], regime, theta_max, theta_max, dict(env or {}), so)
    assert rid not in into
    into[rid] = Spec(row, table, store_table if store_table is not None else table, q2[0], q2[1], row_split)


REAL, ODD, TAYLOR = ('real', 2.0), ('odd', 2.0), ('taylor', 2.0)
REAL6 = ('real', 6.0)
spec('tile64/256', 'c5_k300', table=REAL, store_table=ODD, q2=(False, True))
spec('tile64/stream', 'c5_k600_distinct', table=REAL, store_table=ODD, q2=(False, True))
spec('tile64x/512', 'L6_n20', table=REAL)
spec('tile128/512', 'c5_n80', table=REAL)
spec('tile64q2/512', 'c5_n33', table=ODD, q2=(True, True))
spec('tile64q2/512', 'c5_n33', table=ODD, q2=(True, True), env={'KH_NO_ADJ': '1'}, tag='_noadj')
spec('tile64q2/512', 'c5_n33', table=REAL, q2=(True, True), env={'KH_ODD_DEGREES': '0'}, tag='_even')
spec('tile64q2/512', 'c5_n33', table=TAYLOR, q2=(True, True), env={'KH_TAYLOR': '1'}, tag='_taylor')
spec('tile64q2/512', 'c5_n33', table=ODD, q2=(True, True), tag='_so', so=True)
spec('tile64q2/512', 'c5_n33', table=ODD, q2=(True, True), regime='pulse_ramp')
spec('tile64/512', 'c5_n24_L4', table=REAL)  # (c5_n12_L3: 80 intervals; its derived bound at 1e-4 is beyond 1e-2)
spec('tile64/512', 'c5_n24_L4', table=REAL, regime='pulse_ramp')
spec('ell/csr', 'c5_n16_csr', theta_max=4.0, table=REAL6)
spec('ellstream/csr', 'c5_n16_csr', theta_max=4.0, table=REAL6, env={'KH_KERNEL': 'ellstream'}, tag='_forced')
spec('ellglobal/csr', 'c5_n16_csr', theta_max=4.0, table=REAL6, env={'KH_KERNEL': 'ellglobal'}, tag='_forced')
spec('ellsplit/csr', 'c5_n16_csr', theta_max=4.0, table=REAL6, env={'KH_KERNEL': 'ellglobal'}, tag='_split2', row_split=2)
spec('generic/csr', 'c5_n33_csr', table=REAL)
spec('generic/csr', 'c5_n16_csr', table=REAL, env={'KH_KERNEL': 'generic'}, tag='_forced')
for _adj in ('1', '0'):
    spec('generic', 'L2_n160', table=REAL, env={'KH_KERNEL': 'generic', 'KH_GEN_ADJ': _adj}, tag='_adj' + _adj)
spec('generic', 'L2_n160', table=REAL, env={'KH_KERNEL': 'generic'}, tag='_so', so=True)
spec('generic/mixed', 'mixed_dims', table=TAYLOR)
spec('lindblad/matrix', 'd7', table=TAYLOR)
spec('mini16/wave', 'c5_n16_norms')
spec('mini4/wave', 'c3_norms')
spec('ens64/mfma', 'k40_n64', env={'KH_ENS': '1', 'KH_ENS_NCG': '1'}, tag='_cg1')
spec('ens64/mfma', 'k100_n16', env={'KH_ENS': '1', 'KH_ENS_NCG': '8'}, tag='_cg8')
spec('ens64/mfma', 'k520_n8', tag='_ens2')
spec('ens64/mfma', 'k520_n8', env={'KH_ENS2': '0'}, tag='_ens2off')
for _cols in ('2', '16'):
    spec('coop16/mfma', 'shared_n96_L2', theta_max=4.0, env={'KH_COOP_COLS': _cols}, tag='_cols' + _cols)
for _nosq in ('0', '1'):
    spec('coop16/mfma', 'shared_n300', theta_max=4.0, env={'KH_COOP_COLS': '4', 'KH_COOP_NOSQ': _nosq}, tag='_nosq' + _nosq)
spec('coop16/mfma', 'shared_n300', theta_max=4.0, tag='_so', so=True)

CASES = [(rid, tol) for rid in SPECS for tol in TOLS]
CASE_IDS = ['%s-tol%g' % c for c in CASES]

# the cheap rows, one per create function, that also run tol = -1 and tol = NaN (bitwise the tol = 0 run)
DOMAIN_ROWS = ('tile64q2/512-c5_n33-ramp', 'ell/csr-c5_n16_csr-ramp', 'generic/mixed-mixed_dims-ramp', 'lindblad/matrix-d7-ramp')


def project_tol(row):
    obj = tsr.problem(row)
    liouville = obj.fmt == 'lindblad' or bool(np.any(obj.is_super))
    return 1e-11 if liouville or row.regime == 'ramp' else 1e-12


def candidate_tables(sp, tol):
    """(update-sweep table, plain-sweep table) of a row that names them; else every form an engine may have chosen."""
    cap = tsr.SERIES_CAP.get(sp.row.family, 2.0)
    if sp.table is None:
        return [so.table('taylor', tol), so.table('real', tol, cap), so.table('defect', tol, cap, 3e-3)]
    return [so.table(name, tol, c, round_up=q2 and name == 'taylor')
            for (name, c), q2 in ((sp.table, sp.q2_update), (sp.store_table, sp.q2_store))]


_series = {}


def series_reference(sp, tol):
    """The series oracle's sweeps of a row at ``tol`` (cached): plain sweeps under the plain sweeps' table, the update
    sweep -- on the series oracle's own co-states -- under the update sweep's."""
    row = sp.row
    tabs = candidate_tables(sp, tol)
    t_upd, t_store = (tabs[0], tabs[1]) if sp.table is not None else (tabs[0], tabs[0])
    key = (row.base, row.regime, row.theta_max, row.so, tol, t_upd.name, t_store.name, t_upd.round_up, t_store.round_up,
           t_upd.theta[64], t_store.theta[64])
    if key in _series:
        return _series[key]
    obj, ref = tsr.problem(row), reference(sp)
    prob, bounds = ref['prob'], hp.series_bounds(obj)
    out = {}
    with so.SeriesOracle(prob, bounds, t_store, row.theta_max):
        out['psi_T'], out['states'] = ko.forward_propagation(prob, obj.pulses, store=True)
        out['chi'] = ko.backward_sweep(prob, ref['chi_T'], obj.pulses)
    kw = dict(sigma_vals=ref['sigma'], fw_prev=ref['prev'], store=True) if row.so else {}
    with so.SeriesOracle(prob, bounds, t_upd, row.theta_max):
        res = ko.forward_update_sweep(prob, out['chi'], ref['norms'], obj.pulses, obj.shapes, obj.lambdas, **kw)
    out['opt'], out['upd_T'], out['g_a'] = np.array(res[0]), res[1], np.array(res[2])
    if row.so:
        out['store'] = res[3]
    _series[key] = out
    return out


def nsub_plans(sp, tol):
    """What ``tolerance_bound`` takes: the sub-steps under the guess and the updated pulses and, for the rows that name
    their tables, the refined step errors (``series_oracle.step_errors``: the larger of the two tables')."""
    obj, ref = tsr.problem(sp.row), reference(sp)
    tabs = candidate_tables(sp, tol)
    theta_max = sp.row.theta_max
    theta, nsub_opt, _ = so.plan(obj, ref['opt'], theta_max, tabs[0])
    plans = dict(guess=so.plan(obj, obj.pulses, theta_max, tabs[0])[1], opt=nsub_opt)
    if sp.row.family == 'mini4/wave':
        # kh_quad_*: the objectives share one wave and every one of them takes the sub-steps (and the degree) of the wave's
        # largest theta -- more sub-steps than its own plan, each within tol
        plans = {name: np.broadcast_to(nsub.max(axis=0), nsub.shape) for name, nsub in plans.items()}
    if sp.table is not None:
        plans['tol_guess'] = so.step_errors(obj, ref['prob'], obj.pulses, theta_max, tabs[1], tol)
        plans['tol_opt'] = so.step_errors(obj, ref['prob'], ref['opt'], theta_max, tabs[0], tol, so.WIDEN)
        plans['theta_opt'] = theta
    return plans


# ||chi_k|| of the update sweeps here: tests/test_series_regimes.py's rule, shrunk by that rule's factor until the feedback
# of the pulse error into the states leaves the derived bound at tol = 1e-4 non-empty (decided on the host, from the
# bound alone)
CHI_SHRINK = (1.0, 0.02, 4e-4)
_references = {}


def bound_is_not_empty(bound, change):
    worst = max(bound['states'].max(), bound['chi'].max(), bound['upd'].max())
    return bool(np.isfinite(worst) and worst < 1e-2 and bound['opt'].max() < 0.1 * change)


def reference(sp):
    """tests/test_series_regimes.py's reference of the row (forward states, the older trajectory and sigma of a
    second-order row) with boundary co-states and an update sweep of this module's own:

    * chi_k(T) = that reference's plus 2 (-i mu_k phi_k(T)) / ||mu_k phi_k(T)||, normalised (mu_k: the first control's
      dH/d eps).  <chi_k | mu_k phi_k> then has the imaginary part ||mu_k phi_k|| for every objective, so the update sums
      add up over the objectives the way the bound's worst case does.  With random co-states they add up like sqrt(K)
      and no worst-case bound stays below a tenth of the pulse change.
    * ||chi_k|| -- and sigma, whose term feeds back the same way -- shrunk by CHI_SHRINK (above)."""
    row = sp.row
    key = (row.base, row.regime, row.theta_max, row.so, sp.table, sp.store_table, sp.q2_update, sp.q2_store)
    if key in _references:
        return _references[key]
    obj, base = tsr.problem(row), tsr.reference(row, states=True)
    prob = base['prob']
    chi_T = np.array(base['chi_T'])
    for k in range(prob.K):
        m = ko._mu_apply(prob, k, 0, base['psi_T'][k])
        if np.linalg.norm(m) > 0.0:
            chi_T[k] = chi_T[k] + 2.0 * (-1j) * m / np.linalg.norm(m)
    chi_T = chi_T / np.linalg.norm(chi_T, axis=1)[:, None]
    with hp.MemoExpm():
        chi = ko.backward_sweep(prob, chi_T, obj.pulses)
    for shrink in CHI_SHRINK:
        ref = dict(base, chi_T=chi_T, chi=chi, norms=base['norms'] * shrink)
        kw = {}
        if row.so:
            ref['sigma'] = base['sigma'] * shrink
            kw = dict(sigma_vals=ref['sigma'], fw_prev=ref['prev'], store=True)
        with hp.MemoExpm():
            out = ko.forward_update_sweep(prob, chi, ref['norms'], obj.pulses, obj.shapes, obj.lambdas, **kw)
        ref['opt'], ref['upd_T'], ref['g_a'] = np.array(out[0]), out[1], np.array(out[2])
        if row.so:
            ref['store'] = out[3]
        _references[key] = ref  # (nsub_plans reads it)
        bound = so.tolerance_bound(obj, TOLS[0], nsub_plans(sp, TOLS[0]), ref, row.so)
        if bound_is_not_empty(bound, np.abs(ref['opt'] - np.array(obj.pulses)).max()):
            break
    return ref


def deviations(got, ref, so_row):
    """Largest entry of the difference per quantity, as the rest of the suite measures it (pulses and g_a relative to
    max(1, max |.|))."""
    names = ('states', 'chi', 'upd_T', 'opt', 'g_a') + (('store',) if so_row else ())
    dev = {name: float(np.abs(got[name] - ref[name]).max()) for name in names}
    for name in ('opt', 'g_a'):
        dev[name] /= max(1.0, np.abs(ref[name]).max())
    return dev


def within_bound(got, ref, bound, so_row, slack):
    """Entry by entry: every deviation from the exact oracle is at most its bound (+ ``slack`` for rounding)."""
    checks = {
        'states': (np.linalg.norm(got['states'] - ref['states'], axis=2), bound['states']),
        'chi': (np.linalg.norm(got['chi'] - ref['chi'], axis=2), bound['chi']),
        'upd_T': (np.linalg.norm(got['upd_T'] - ref['upd_T'], axis=1), bound['upd'][:, -1]),
        'opt': (np.abs(got['opt'] - ref['opt']), bound['opt']),
        'g_a': (np.abs(got['g_a'] - ref['g_a']), bound['g_a']),
    }
    if so_row:
        checks['store'] = (np.linalg.norm(got['store'] - ref['store'], axis=2), bound['upd'])
    return {name: float((d - b).max()) for name, (d, b) in checks.items() if (d - b).max() > slack}


# ---------------------------------------------------------------------------
# host: the tables at a caller's tolerance
# ---------------------------------------------------------------------------
TABLE_FORMS = [('taylor', 2.0, 0.0), ('real', 2.0, 0.0), ('real', 4.0, 0.0), ('real', 6.0, 0.0), ('defect', 2.0, 0.01),
               ('defect', 2.0, 0.05), ('odd', 2.0, 0.0)]
TABLE_RATIOS = {}


@pytest.mark.parametrize('form', TABLE_FORMS, ids=lambda f: '%s-cap%g-d%g' % f)
def test_tables(form):
    """Thresholds rise with the degree and with the tolerance, the table with odd degrees keeps the even-only entries bit
    for bit, and every exported polynomial is within ``tol`` of exp(z) on the scalar spectrum it is built for, at the
    largest theta it serves."""
    name, cap, defect = form
    x = np.linspace(-1.0, 1.0, 801)
    tabs = {tol: so.table(name, tol, cap, defect) for tol in (0.0, 1e-12, 1e-8, 1e-4)}
    for tol in (1e-4, 1e-8, 1e-12):
        tab = tabs[tol]
        assert np.all(np.diff(tab.theta) >= 0.0)
        tighter = tabs[{1e-4: 1e-8, 1e-8: 1e-12, 1e-12: 0.0}[tol]]
        assert np.all(tab.theta >= tighter.theta)
        assert np.any(tab.theta[1:40] > tighter.theta[1:40])
        if name == 'odd':
            assert np.array_equal(tab.theta[0::2], so.table('real', tol, 2.0).theta[0::2])
            even = so.table('real', tol, 2.0)
            for m in range(2, 65, 2):
                # (rebuilt from the rows {r1_p, r2_p} here, from the ratios c_j / c_{j-1} there: equal up to those roundings)
                assert np.allclose(tab.coeff[m, :m + 1], even.coeff[m, :m + 1], rtol=1e-13, atol=0.0), m
        worst = 0.0
        for m in range(1, 65):
            theta = tab.theta[m]
            if not theta > 0.0 or (m > 1 and theta == tab.theta[m - 1]) or theta > 8.0:
                # (a degree the smallest-degree search never lands on; beyond 8 -- the largest theta_cap the library
                # accepts, no family sub-steps beyond 6 -- the double rounding of the coefficients themselves, ~ 1e-16
                # e^theta, is what an evaluation measures, not the truncation)
                continue
            c = so.polynomial(tab, m)
            z = [1j * theta * x]
            if defect > 0.0:
                d = defect / theta
                if d >= 1.0:
                    continue
                a = theta * np.sqrt(1.0 - d * d)
                z.append(np.array([1j * a + defect, 1j * a - defect, -1j * a + defect, -1j * a - defect]))
            # (extended precision: the rounding of this evaluation itself, ~ eps e^theta, stays far below tol)
            err = float(max(np.abs(hp.series_polynomial(c, zz, np.clongdouble) - np.exp(zz.astype(np.clongdouble))).max()
                            for zz in z))
            # (the exported coefficients are doubles, each a product of up to m rounded ratios: 8 x 2^-53 e^theta for that --
            # 2e-5 tol at degree 1 of the odd table at 1e-12, where c_0 = 1 - 1e-12 is rounded)
            assert err <= tol + 8 * 2.0 ** -53 * np.exp(theta), (name, tol, m, theta, err)
            if theta < cap or name == 'taylor':
                worst = max(worst, err / tol)
        TABLE_RATIOS[form + (tol,)] = worst
        print('series table %s cap %g defect %g tol %g: largest error / tol %.2f' % (name, cap, defect, tol, worst))


def test_tol_domain_is_documented():
    """``include/krotov_hip.h`` states the domain the code implements: tol <= 0 or NaN gives the tables of 2^-53; a CSR
    problem's norm bounds are required."""
    header = open(os.path.join(os.path.dirname(hp.GOLDEN), os.pardir, 'include', 'krotov_hip.h')).read()
    text = re.sub(r'[\s*]+', ' ', header)
    assert 'tol <= 0 or NaN -> 2^-53' in text
    assert 'required: NULL is KH_ERR_INVALID' in text
    default = so.table('taylor', 2.0 ** -53).theta
    for tol in (0.0, -1.0, float('nan'), -float('inf')):
        assert np.array_equal(hp.series_taylor_coefficients(tol)[0], default)
        assert np.array_equal(hp.series_tables_odd(tol)[0], hp.series_tables_odd(2.0 ** -53)[0])
        assert np.array_equal(hp.series_coefficients(4.0, tol, 0.01)[0], hp.series_coefficients(4.0, 2.0 ** -53, 0.01)[0])


def test_sparse_frobenius_is_refused_before_the_gpu():
    """``op_norms='frobenius'`` with sparse operators: ValueError, raised before the engine looks for a device."""
    import scipy.sparse as sp

    from krotov_amd.engine import HipKrotovEngine

    ops = [[sp.identity(4, dtype=np.complex128, format='csr'), np.eye(4, dtype=np.complex128)]]
    with pytest.raises(ValueError, match='sparse'):
        HipKrotovEngine(ops, np.full(3, 0.1), op_norms='frobenius')
    with pytest.raises(ValueError, match='frobenius'):
        HipKrotovEngine(ops, np.full(3, 0.1), op_norms='spectral')


def test_csr_constructor_rejects_missing_norms():
    """``kh_engine_create_csr`` with ``op_norms == NULL``: KH_ERR_INVALID, answered before any device call (no GPU here)."""
    import ctypes

    from krotov_amd import _lib

    lib = _lib.load()
    slots, dt = (_lib.kh_csr * 2)(), (ctypes.c_double * 3)(0.1, 0.1, 0.1)
    pr = _lib.kh_problem_csr()
    pr.K, pr.N, pr.L, pr.nt, pr.is_super = 1, 4, 1, 4, 0
    pr.dt, pr.ops, pr.ops_adj, pr.op_norms = dt, slots, slots, None
    handle = ctypes.c_void_p()
    assert lib.kh_engine_create_csr(ctypes.byref(pr), ctypes.byref(handle)) == _lib.KH_ERR_INVALID
    assert not handle.value and b'op_norms are required' in lib.kh_last_error()


def test_every_family_is_listed():
    assert {sp.row.family for sp in SPECS.values()} | {'replica16/wave'} == {r.family for r in tsr.ROWS} | {
        'ellglobal/csr', 'ellsplit/csr', 'replica16/wave'}


@pytest.mark.parametrize('cid', CASE_IDS)
def test_witness(cid):
    """Host only, per (row, tol): the plan is in the regime this module is about, no theta sits near a threshold, and the
    series oracle stays within the derived bound of the exact oracle -- a bound that is not empty."""
    rid, tol = CASES[CASE_IDS.index(cid)]
    sp = SPECS[rid]
    row, obj = sp.row, tsr.problem(sp.row)
    ref = reference(sp)
    ptol = project_tol(row)
    for tab in candidate_tables(sp, tol):
        default = so.at_tolerance(tab, 0.0)
        for pulses in (obj.pulses, ref['opt']):
            theta, nsub, deg = so.plan(obj, pulses, row.theta_max, tab)
            assert so.threshold_distance(theta, nsub, row.theta_max, tab) > 1e-9
            k = int(np.argmax(theta.max(axis=1)))
            if tol == 1e-4:
                assert len(set(deg[k].tolist())) >= 3, deg[k]
                assert deg[k].min() <= 2 and deg[k].max() >= 5, deg[k]
                assert np.any(nsub[k] > 1)
            else:
                deg0 = so.plan(obj, pulses, row.theta_max, default)[2]
                assert np.all(deg[k] != deg0[k]), (deg[k], deg0[k])
    plans = nsub_plans(sp, tol)
    bound = so.tolerance_bound(obj, tol, plans, ref, row.so)
    ser = series_reference(sp, tol)
    dev = deviations(ser, ref, row.so)
    change = np.abs(ref['opt'] - np.array(obj.pulses)).max()
    print('series_tolerance witness %s: deviation of the series oracle %s; bound states %.1e chi %.1e upd %.1e opt %.1e '
          '(largest pulse change %.1e) g_a %.1e' % (cid, ' '.join('%s %.1e' % kv for kv in dev.items()), bound['states'].max(),
                                                    bound['chi'].max(), bound['upd'].max(), bound['opt'].max(), change,
                                                    bound['g_a'].max()))
    assert not within_bound(ser, ref, bound, row.so, ptol)
    if tol == 1e-4:
        assert min(dev['states'], dev['chi'], dev['upd_T']) > 100.0 * ptol, dev
        assert max(bound['states'].max(), bound['chi'].max(), bound['upd'].max()) < 1e-2
        assert bound['opt'].max() < 0.1 * change
        assert change > 1e-6  # the update sweep still moves the pulses


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def run_sweeps(eng, obj, ref, row, chi_T=None):
    """The sweeps of a row on ``eng``: host arrays, the products of each sweep."""
    import torch

    prob = ref['prob']
    pulses, S, lam = np.array(obj.pulses), np.array(obj.shapes), np.array(obj.lambdas)
    M = pulses.shape[1]
    out, count = {}, {}
    psi_T, states = eng.forward(pulses, prob.init, store=True)
    count['forward'] = eng.stats()['matvecs']
    assert eng.stats()['intervals'] == M
    out['psi_T'], out['states'] = psi_T.cpu().numpy(), states.cpu().numpy()
    chi = eng.backward(ref['chi_T'], pulses)
    count['backward'] = eng.stats()['matvecs']
    out['chi'] = chi.cpu().numpy()
    if row.so:
        store = torch.full((obj.K, M + 1, prob.N), float('nan'), dtype=torch.complex128, device=eng.device)
        eng.set_second_order(ref['prev'], store, ref['sigma'])
    opt, upd_T, g_a = eng.forward_update(chi, ref['norms'], prob.init, pulses, S, lam)
    eng.check()
    count['update'] = eng.stats()['matvecs']
    out['opt'], out['upd_T'], out['g_a'] = opt.cpu().numpy(), upd_T.cpu().numpy(), g_a.cpu().numpy()
    if row.so:
        out['store'] = store.cpu().numpy()
    return out, count


def engine_of(sp, tol=0.0, op_norms=None):
    eng = hp.regime_engine(tsr.problem(sp.row), sp.row.theta_arg, tol=tol, op_norms=op_norms)
    if sp.row_split:
        assert eng.set_row_split(sp.row_split) == sp.row_split
    return eng


_default_runs = {}


def default_run(sp, monkeypatch):
    """The row at the default tolerance (once per row): results, products, kernel family and launched instantiations."""
    from krotov_amd import _lib

    if sp.row.id not in _default_runs:
        obj, ref = tsr.problem(sp.row), reference(sp)
        _lib.forget_launched_kernels()
        eng = engine_of(sp)
        got, count = run_sweeps(eng, obj, ref, sp.row)
        _default_runs[sp.row.id] = dict(got=got, count=count, kernel=eng.kernel, op_norms=np.array(eng.op_norms),
                                        launched=sorted(_lib.kernel_instantiations(launched_only=True)))
        eng.close()
    return _default_runs[sp.row.id]


def planned_products(sp, tol, obj, pulses, sweep, bounds=None):
    """The series' products of one sweep under ``pulses`` from the host plan (rows that name their tables)."""
    tabs = candidate_tables(sp, tol)
    tab, two = (tabs[0], sp.q2_update) if sweep == 'update' else (tabs[1], sp.q2_store)
    theta, nsub, deg = so.plan(obj, pulses, sp.row.theta_max, tab, bounds)
    assert so.threshold_distance(theta, nsub, sp.row.theta_max, tab) > 1e-9
    return so.products(tab, nsub, deg, two)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', CASE_IDS)
def test_tolerance(cid, monkeypatch):
    from krotov_amd import _lib

    rid, tol = CASES[CASE_IDS.index(cid)]
    sp = SPECS[rid]
    row, obj = sp.row, tsr.problem(sp.row)
    ref = reference(sp)
    ptol = project_tol(row)
    for name, value in row.env.items():
        monkeypatch.setenv(name, value)
    base = default_run(sp, monkeypatch)
    assert base['kernel'] == row.family
    _lib.forget_launched_kernels()
    eng = engine_of(sp, tol)
    got, count = run_sweeps(eng, obj, ref, row)
    again, count2 = run_sweeps(eng, obj, ref, row)
    kernel, launched = eng.kernel, sorted(_lib.kernel_instantiations(launched_only=True))
    domain = {}
    eng.close()
    if tol == TOLS[0] and rid in DOMAIN_ROWS:
        for odd_tol in (-1.0, float('nan')):
            e2 = engine_of(sp, odd_tol)
            domain[odd_tol] = run_sweeps(e2, obj, ref, row)
            e2.close()
    dev = deviations(got, ref, row.so)
    dev0 = deviations(base['got'], ref, row.so)
    plans = nsub_plans(sp, tol)
    bound = so.tolerance_bound(obj, tol, plans, ref, row.so)
    print('series_tolerance %s [%s]: products %s (default %s); from the exact oracle: %s (default: %s); bound states %.1e '
          'chi %.1e upd %.1e opt %.1e g_a %.1e' % (
              cid, kernel, count, base['count'], ' '.join('%s %.1e' % kv for kv in dev.items()),
              ' '.join('%s %.1e' % kv for kv in dev0.items()), bound['states'].max(), bound['chi'].max(), bound['upd'].max(),
              bound['opt'].max(), bound['g_a'].max()))
    failures = []
    # ---- the same kernel
    if kernel != base['kernel'] or launched != base['launched']:
        failures.append(('kernels', kernel, launched, base['launched']))
    # ---- products
    for sweep in ('forward', 'backward', 'update'):
        if not count[sweep] < base['count'][sweep]:
            failures.append(('no fewer products than at the default tolerance', sweep, count[sweep], base['count'][sweep]))
    if tol == TOLS[1]:
        eng4 = engine_of(sp, TOLS[0])
        eng4.forward(np.array(obj.pulses), ref['prob'].init, store=False)
        if not eng4.stats()['matvecs'] < count['forward']:
            failures.append(('no fewer products at 1e-4 than at 1e-8', eng4.stats()['matvecs'], count['forward']))
        eng4.close()
    if sp.table is not None:
        for sweep in ('forward', 'backward'):
            want = planned_products(sp, tol, obj, obj.pulses, sweep)
            print('    %s: planned products %d, counted %d' % (sweep, want, count[sweep]))
            if count[sweep] != want:
                failures.append(('products', sweep, count[sweep], want))
        # the update sweep: the series under the device's own updated pulses, plus the products of the update sums, which
        # do not depend on the tolerance (two-terms-per-phase kernels: one per objective and interval)
        extra = count['update'] - planned_products(sp, tol, obj, got['opt'], 'update')
        extra0 = base['count']['update'] - planned_products(sp, 0.0, obj, base['got']['opt'], 'update')
        print('    update: products beyond the planned series %d (default tolerance: %d)' % (extra, extra0))
        if extra != extra0 or extra < 0 or (sp.q2_update and extra != obj.K * len(obj.pulses[0])):
            failures.append(('products', 'update', extra, extra0))
    # ---- the exact polynomial
    if sp.table is not None:
        ser = series_reference(sp, tol)
        sdev = deviations(got, ser, row.so)
        print('    from the series oracle: %s' % ' '.join('%s %.1e' % kv for kv in sdev.items()))
        for name, value in sdev.items():
            if not value < ptol:
                failures.append(('series oracle', name, value))
    # ---- the bound against the exact oracle, and a tolerance that is not ignored
    over = within_bound(got, ref, bound, row.so, ptol)
    if over:
        failures.append(('beyond the bound', over))
    if tol == 1e-4:
        for name in ('states', 'chi', 'upd_T'):
            if not dev[name] > 100.0 * dev0[name]:
                failures.append(('not 100 x the default deviation', name, dev[name], dev0[name]))
    # ---- repeatability
    for name in got:
        if not np.array_equal(got[name], again[name]):
            failures.append(('second run differs', name))
    if count2 != count:
        failures.append(('second run counts', count2, count))
    for odd_tol, (res, cnt) in domain.items():
        for name in res:
            if not np.array_equal(res[name], base['got'][name]):
                failures.append(('tol = %r is not the default run' % odd_tol, name))
        if cnt != base['count']:
            failures.append(('tol = %r counts' % odd_tol, cnt, base['count']))
    assert not failures, failures


# ---------------------------------------------------------------------------
# GPU: replica batch (tests/test_replicas.py's harness)
# ---------------------------------------------------------------------------
def _replica_refs(reps):
    """Per replica of a batch: the exact oracle's sweeps in the form ``tolerance_bound`` and ``deviations`` take."""
    refs = []
    for r in reps:
        prob = hp.spec_to_oracle(r)
        chi_T = r.target / np.linalg.norm(r.target, axis=1)[:, None]
        with hp.MemoExpm():
            psi_T, states = ko.forward_propagation(prob, r.pulses, store=True)
            chi = ko.backward_sweep(prob, chi_T, r.pulses)
            opt, upd_T, g_a = ko.forward_update_sweep(prob, chi, r.chi_norms, r.pulses, r.shapes, r.lambdas)
        refs.append(dict(prob=prob, chi_T=chi_T, norms=r.chi_norms, psi_T=psi_T, states=states, chi=chi, opt=np.array(opt),
                         upd_T=upd_T, g_a=np.array(g_a)))
    return refs


def _replica_series(r, ref, tab):
    prob = ref['prob']
    with so.SeriesOracle(prob, hp.series_bounds(r), tab, 1.0):
        psi_T = ko.forward_propagation(prob, r.pulses)
        chi = ko.backward_sweep(prob, ref['chi_T'], r.pulses)
        opt, upd_T, g_a = ko.forward_update_sweep(prob, chi, r.chi_norms, r.pulses, r.shapes, r.lambdas)
    return dict(psi_T=psi_T, chi=chi, opt=np.array(opt), upd_T=upd_T, g_a=np.array(g_a))


def test_replica_witness():
    """Host only: the `regimes` batch of tests/test_replicas.py at both tolerances (two controls: term by term, the
    real-spectrum table; every operator of it is Hermitian)."""
    import test_replicas as tr

    reps = tr.batch('regimes')
    for tol in TOLS:
        tab, degs = so.table('real', tol), set()
        for r in reps:
            theta, nsub, deg = so.plan(r, r.pulses, 1.0, tab)
            assert so.threshold_distance(theta, nsub, 1.0, tab) > 1e-9
            degs |= set(deg.ravel().tolist())
            if tol == 1e-8 and r is not reps[0]:  # (replica 0: every operator x 1e-7, degree 2 at any tolerance)
                assert np.all(deg != so.plan(r, r.pulses, 1.0, so.table('real', 0.0))[2])
        if tol == 1e-4:
            assert len(degs) >= 3 and min(degs) <= 2 and max(degs) >= 5, degs


@pytest.mark.gpu
@pytest.mark.parametrize('tol', TOLS)
def test_replica_tolerance(tol):
    import test_replicas as tr

    reps = tr.batch('regimes')
    refs = _replica_refs(reps)
    Kr = reps[0].K
    base, got, again = tr.run_engine(reps), tr.run_engine(reps, tol=tol), tr.run_engine(reps, tol=tol)
    for x, y in zip(got[:5], again[:5]):
        assert np.array_equal(x, y)
    for odd_tol in ((-1.0, float('nan')) if tol == TOLS[0] else ()):
        for x, y in zip(tr.run_engine(reps, tol=odd_tol)[:5], base[:5]):
            assert np.array_equal(x, y)
    assert got[5]['matvecs'] < base[5]['matvecs']
    tab = so.table('real', tol)
    planned = planned0 = 0
    failures = []
    for b, (r, ref) in enumerate(zip(reps, refs)):
        rows = slice(b * Kr, (b + 1) * Kr)
        mine = dict(psi_T=got[0][rows], chi=got[1][rows], opt=got[2][b], upd_T=got[3][rows], g_a=got[4][b])
        mine0 = dict(psi_T=base[0][rows], chi=base[1][rows], opt=base[2][b], upd_T=base[3][rows], g_a=base[4][b])
        planned += so.products(tab, *so.plan(r, mine['opt'], 1.0, tab)[1:])
        planned0 += so.products(so.table('real', 0.0), *so.plan(r, mine0['opt'], 1.0, so.table('real', 0.0))[1:])
        plans = dict(guess=so.plan(r, r.pulses, 1.0, tab)[1], opt=so.plan(r, ref['opt'], 1.0, tab)[1])
        bound = so.tolerance_bound(r, tol, plans, ref)
        ser = _replica_series(r, ref, tab)
        dist = lambda a, c: {'psi_T': np.linalg.norm(a['psi_T'] - c['psi_T'], axis=1).max(),  # noqa: E731
                             'chi': np.linalg.norm(a['chi'] - c['chi'], axis=2).max(),
                             'upd_T': np.linalg.norm(a['upd_T'] - c['upd_T'], axis=1).max(),
                             'opt': np.abs(a['opt'] - c['opt']).max(), 'g_a': np.abs(a['g_a'] - c['g_a']).max()}
        dev, dev0, sdev = dist(mine, ref), dist(mine0, ref), dist(mine, ser)
        print('series_tolerance replica %d tol %g: exact %s; default %s; series oracle %s' % (
            b, tol, ' '.join('%s %.1e' % kv for kv in dev.items()), ' '.join('%s %.1e' % kv for kv in dev0.items()),
            ' '.join('%s %.1e' % kv for kv in sdev.items())))
        limit = {'psi_T': bound['states'][:, -1].max(), 'chi': bound['chi'].max(), 'upd_T': bound['upd'][:, -1].max(),
                 'opt': bound['opt'].max(), 'g_a': bound['g_a'].max()}
        for name in dev:
            if dev[name] > limit[name] + 1e-12:
                failures.append((b, 'beyond the bound', name, dev[name], limit[name]))
            if not sdev[name] / (max(1.0, np.abs(ser[name]).max()) if name in ('opt', 'g_a') else 1.0) < 1e-12:
                failures.append((b, 'series oracle', name, sdev[name]))
        if tol == 1e-4 and b > 0:  # (replica 0: every operator x 1e-7, degree 1 or 2 at either tolerance)
            for name in ('psi_T', 'chi', 'upd_T'):
                if not dev[name] > 100.0 * dev0[name]:
                    failures.append((b, 'not 100 x the default deviation', name, dev[name], dev0[name]))
    # (the update sweep is the last one counted: its series under the updated pulses plus the update sums' products)
    extra, extra0 = got[5]['matvecs'] - planned, base[5]['matvecs'] - planned0
    print('series_tolerance replicas tol %g: products beyond the planned series %d (default tolerance: %d)' % (tol, extra, extra0))
    assert extra == extra0 >= 0
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize('tol', TOLS)
def test_replica_second_order_tolerance(tol):
    """tests/test_replicas_second_order.py's harness on its `regimes` batch (two controls: term by term).  The older
    trajectory is the engine's own forward sweep at the same tolerance, so the reference is the series oracle throughout
    (exact polynomial; the derived bound assumes an exact older trajectory and is not used here); the tolerance must
    show against the exact oracle and in the products."""
    import test_replicas_second_order as trs

    reps = trs.so_batch('regimes')
    sigma = trs.sigma_rows(reps)
    base, got, again = trs.run_so(reps, sigma), trs.run_so(reps, sigma, tol=tol), trs.run_so(reps, sigma, tol=tol)
    for name in ('opt', 'psi_T', 'g_a', 'fw_store'):
        assert np.array_equal(got[name], again[name]), name
    assert got['stats']['matvecs'] < base['stats']['matvecs']
    tab, Kr = so.table('real', tol), reps[0].K
    failures = []
    for b, r in enumerate(reps):
        prob = hp.spec_to_oracle(r)
        chi_T = r.target / np.linalg.norm(r.target, axis=1)[:, None]
        theta, nsub, deg = so.plan(r, r.pulses, 1.0, tab)
        assert so.threshold_distance(theta, nsub, 1.0, tab) > 1e-9
        with so.SeriesOracle(prob, hp.series_bounds(r), tab, 1.0):
            prev = ko.forward_propagation(prob, r.pulses, store=True)[1]
            chi = ko.backward_sweep(prob, chi_T, r.pulses)
            ser = ko.forward_update_sweep(prob, chi, r.chi_norms, r.pulses, r.shapes, r.lambdas, sigma_vals=sigma[b],
                                          fw_prev=prev, store=True)
        theta, nsub, deg = so.plan(r, ser[0], 1.0, tab)
        assert so.threshold_distance(theta, nsub, 1.0, tab) > 1e-9
        exact = trs.oracle_so('regimes', b)[1]
        dev = {}
        for name, mine, mine0, s, e in zip(('opt', 'psi_T', 'g_a', 'fw_store'), trs._of_replica(got, b, Kr),
                                           trs._of_replica(base, b, Kr), ser, exact):
            scale = max(1.0, np.abs(np.array(s)).max()) if name in ('opt', 'g_a') else 1.0
            dev[name] = (np.abs(mine - np.array(s)).max() / scale, np.abs(mine - np.array(e)).max() / scale,
                         np.abs(mine0 - np.array(e)).max() / scale)
        print('series_tolerance second-order replica %d tol %g: (series oracle, exact, default run from exact) %s' % (
            b, tol, ' '.join('%s %.1e %.1e %.1e' % ((k,) + v) for k, v in dev.items())))
        for name, (from_series, from_exact, default) in dev.items():
            if not from_series < 1e-12:
                failures.append((b, 'series oracle', name, from_series))
            if tol == 1e-4 and name in ('psi_T', 'fw_store') and not from_exact > 100.0 * default:
                failures.append((b, 'not 100 x the default deviation', name, from_exact, default))
    assert not failures, failures


# ---------------------------------------------------------------------------
# GPU: the caller's norm bounds, or none
# ---------------------------------------------------------------------------
NORM_ROWS = ['tile64q2/512-c5_n33-ramp', 'tile128/512-c5_n80-ramp', 'coop16/mfma-shared_n96_L2_cols2-ramp',
             'ens64/mfma-k100_n16_cg8-ramp', 'mini16/wave-c5_n16_norms-ramp', 'generic-L2_n160_adj1-ramp',
             'generic/mixed-mixed_dims-ramp', 'lindblad/matrix-d7-ramp']
NORM_SPECS = {rid: SPECS[rid] for rid in NORM_ROWS}
spec('tile64/512', 'c5_n64_L2', table=REAL, into=NORM_SPECS)
spec('tile64/512', 'absent_L2', table=REAL, into=NORM_SPECS)
NORM_ROWS = list(NORM_SPECS)
NORM_CASES = [(rid, mode) for rid in NORM_ROWS for mode in ('frobenius', 'loose')]
NORM_IDS = ['%s-%s' % c for c in NORM_CASES]


def _norm_bounds(obj, mode):
    return hp.series_bounds(obj, norm='frobenius') if mode == 'frobenius' else hp.series_bounds(obj, factor=3.0)


@pytest.mark.parametrize('cid', NORM_IDS)
def test_norms_witness(cid):
    """Host only: under the Frobenius norms and under three times the default bounds no theta sits near a threshold (the
    device sums a Frobenius norm in another order), and both plans cost at least the default one."""
    rid, mode = NORM_CASES[NORM_IDS.index(cid)]
    sp = NORM_SPECS[rid]
    obj, ref = tsr.problem(sp.row), reference(sp)
    bounds = _norm_bounds(obj, mode)
    assert np.all(bounds >= hp.series_bounds(obj) * (1.0 - 1e-12))  # (true upper bounds)
    for tab in candidate_tables(sp, 0.0):
        for pulses in (obj.pulses, ref['opt']):
            theta, nsub, deg = so.plan(obj, pulses, sp.row.theta_max, tab, bounds)
            assert so.threshold_distance(theta, nsub, sp.row.theta_max, tab) > 1e-9
            assert so.products(tab, nsub, deg) >= so.products(tab, *so.plan(obj, pulses, sp.row.theta_max, tab)[1:])
    if rid.startswith('tile64/512-absent'):
        assert any(op is None for row in obj.Hc for op in row)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', NORM_IDS)
def test_norms(cid, monkeypatch):
    """``op_norms='frobenius'`` (a NULL pointer: the library computes the norms) and a true but loose bound, 3 x the
    default: every sweep matches the exact oracle to the project's tolerance, costs at least the default run's products
    and -- where the count per degree is documented -- exactly the plan of the norms handed in."""
    rid, mode = NORM_CASES[NORM_IDS.index(cid)]
    sp = NORM_SPECS[rid]
    row, obj = sp.row, tsr.problem(sp.row)
    ref = reference(sp)
    ptol = project_tol(row)
    for name, value in row.env.items():
        monkeypatch.setenv(name, value)
    base = default_run(sp, monkeypatch)
    eng = engine_of(sp, op_norms='frobenius' if mode == 'frobenius' else 3.0 * base['op_norms'])
    kernel, handed = eng.kernel, np.array(eng.op_norms)
    got, count = run_sweeps(eng, obj, ref, row)
    eng.close()
    dev = deviations(got, ref, row.so)
    print('series_tolerance norms %s [%s]: products %s (default %s); from the exact oracle: %s' % (
        cid, kernel, count, base['count'], ' '.join('%s %.1e' % kv for kv in dev.items())))
    assert kernel == base['kernel'] == row.family
    if mode == 'frobenius':  # self.op_norms: the host's Frobenius norms, 0 for an absent operator
        if obj.fmt == 'lindblad':
            want = [[np.linalg.norm(op, 'fro') if op is not None else 0.0 for op in list(obj.H[k]) + list(obj.C[k])]
                    for k in range(obj.K)]
            want = [w + [0.0] * (handed.shape[1] - len(w)) for w in want]
        else:
            want = [[np.linalg.norm(op, 'fro') if op is not None else 0.0 for op in [obj.H0[k]] + list(obj.Hc[k])]
                    for k in range(obj.K)]
        assert np.array_equal(handed, np.array(want))
    else:
        assert np.array_equal(handed, 3.0 * base['op_norms'])
    bounds = _norm_bounds(obj, mode)
    for sweep in ('forward', 'backward', 'update'):
        assert count[sweep] >= base['count'][sweep], sweep
    if sp.table is not None:
        for sweep in ('forward', 'backward'):
            assert count[sweep] == planned_products(sp, 0.0, obj, obj.pulses, sweep, bounds), sweep
        extra = count['update'] - planned_products(sp, 0.0, obj, got['opt'], 'update', bounds)
        extra0 = base['count']['update'] - planned_products(sp, 0.0, obj, base['got']['opt'], 'update')
        assert extra == extra0, (extra, extra0)
    for name, value in dev.items():
        assert value < ptol, (name, value)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['frobenius', 'loose'])
def test_replica_norms(mode):
    import test_replicas as tr

    reps = tr.batch('regimes')
    base = tr.run_engine(reps)
    spectral = np.concatenate([hp.series_bounds(r) for r in reps])
    got = tr.run_engine(reps, op_norms='frobenius' if mode == 'frobenius' else 3.0 * spectral)
    tr.compare_with_oracle('regimes', got)
    assert got[5]['matvecs'] >= base[5]['matvecs']
    tab = so.table('real', 0.0)
    planned = planned0 = 0
    Kr = reps[0].K
    for b, r in enumerate(reps):
        bounds = _norm_bounds(r, mode)
        theta, nsub, deg = so.plan(r, got[2][b], 1.0, tab, bounds)
        assert so.threshold_distance(theta, nsub, 1.0, tab) > 1e-9
        planned += so.products(tab, nsub, deg)
        planned0 += so.products(tab, *so.plan(r, base[2][b], 1.0, tab)[1:])
    assert got[5]['matvecs'] - planned == base[5]['matvecs'] - planned0
