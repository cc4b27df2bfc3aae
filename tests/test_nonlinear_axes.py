"""The non-linear update sweeps on every engine and along every axis the rest of the suite covers for the other kernel
families.

``kh_tile_forward_update_nl<RPT, J, SO>`` / ``kh_gen_forward_update_nl<MIXED>`` (terms eps_c^p H_j of one
control) are separate compilations that take the plan of whatever engine they are set on (``theta_max``, the degree table,
the coefficient rows, the Hermitian classification, the update grid).  tests/test_nonlinear_controls.py runs them at
|eps| <= 0.3 with powers up to 3, tables whose controls are ascending and contiguous, Hermitian operators, on tile,
``tile128`` and one CSR engine.  This module runs them

1. under term tables chosen by the number of slots J of the base case (``nonlinear_cases.AXES_TABLES``: every power 1..4
   under both kernel forms, slot 0 not control 0, one control's terms apart, controls interleaved, six slots),
2. on every base of tests/test_bounded_constrained_axes.py's ``BASES`` that ``refuse_form`` lets through (the refusals
   with their codes),
3. along the series' regimes ENTERED UNDER THE COEFFICIENT PULSES c_j = eps_c(j)^p_j (``helpers.theta_sequence`` with a
   term table, the non-linear ``regime_pulse_ramp``) and the ``amplitude`` regime (``helpers.regime_amplitude``: the guesses
   straddle |eps| = 1, where |eps|^p and |eps| part ways), the ends of the interval pipeline, absent terms, term operators
   that are not self-adjoint, a caller-set series tolerance and loose norm bounds (the series oracle of the same plan to
   rounding, the exact restatement within the derived bound ``nl_bound``), one engine whose table and inputs change (every
   step bit for bit a fresh engine's), and the per-interval form,
4. on a fixed-seed slice of ``tests/fuzz_parity.py --nonlinear``.

Yardstick: ``nonlinear_cases.update_sweep`` on the oracle's exact step, with ``ko.backward_sweep`` on the coefficient
pulses.  lambda_a: ``nonlinear_cases.lambdas_in_eps``; in the ``amplitude`` regime halved until the update moves max |eps|
by at least 1 %.

Every GPU case has a host-only witness over the very table it runs (``test_witness``): the regime is entered under the
guess and under the restatement's updated pulses, the update moves the pulse on at least 90 % of the intervals (an exact
zero of a control without a power-1 term stays 0.0 -- bit for bit on the device, too), the restatement with every weight
replaced by 1 moves every compared quantity by more than 1e3 tolerances, and -- variants -- filling an absent entry or
taking H_j for H_j^dagger moves every compared quantity by more than 1e-6.  ``test_theta_from_eps_would_underplan`` shows
that a kernel forming theta from |eps| instead of |eps^p| would plan another series on the ``amplitude`` rows and be off
by more than 1e3 tolerances (evaluated with the pulses held at the exact restatement's: a propagation, not the whole
update sweep, so that a series gone wrong does not feed back into the pulses and theta).

Tolerances are the project's: 1e-12 against the restatement in Hilbert space, 1e-11 in Liouville
space and in the ``ramp`` / ``amplitude`` regimes (non-uniform grid, theta > 1); pulses and g_a relative to max(1, largest
reference magnitude); bit for bit where a docstring says so.
"""
import collections
import copy
import functools

import numpy as np
import pytest

import helpers as hp
import nonlinear_cases as nc
import test_absent_controls as tac
import test_bounded_constrained_axes as bca
import test_series_regimes as tsr
from oracle import krotov_oracle as ko
from test_bounded_constrained_axes import BASES, generic_grid, make_engine

TOL_HILBERT, TOL_LIOUVILLE, TOL_RAMP = 1e-12, 1e-11, 1e-11
GEN_NL, GEN_NL_MIXED = 'kh_gen_forward_update_nl<false>', 'kh_gen_forward_update_nl<true>'
REGIME_INTERVALS, LONG_INTERVALS, ENGINE_INTERVALS = 33, 140, 5
BITES = 1e3  # "every case bites": the restatement with weight 1 is this many tolerances away


def TILE_NL(rpt, J, so):
    return 'kh_tile_forward_update_nl<%d, %d, %s>' % (rpt, J, 'true' if so else 'false')


# ---------------------------------------------------------------------------
# the bases by kernel form, their slots and their term tables
# ---------------------------------------------------------------------------
TILE_FORM = ('quad', 'mini16', 'q2', 'tile_L2', 'tile_L3', 'tile_L4', 'tile256')
GEN_FORM = ('tile128', 'coop', 'coop_L2', 'coop_c4_d9', 'ens', 'stream', 'tilex', 'ell', 'ellstream', 'gencsr', 'ellglobal',
            'mixed')
SLOTS = {b: BASES[b].build(2).L for b in TILE_FORM + GEN_FORM}  # (the operator slots J of the built base case)


def terms_of(base):
    """``nc.AXES_TABLES`` by the base's slots; the two single-slot tables alternate over the single-slot bases of a form."""
    J = SLOTS[base]
    if J > 1:
        return list(nc.AXES_TABLES[J])
    singles = [b for b in (TILE_FORM if base in TILE_FORM else GEN_FORM) if SLOTS[b] == 1]
    return list(nc.AXES_TABLES[1][singles.index(base) % 2])


def nl_kernel(base, so, mode='whole'):
    if base == 'mixed':
        return GEN_NL_MIXED
    if base in TILE_FORM and mode == 'whole':
        return TILE_NL(BASES[base].par[0], SLOTS[base], so)
    return GEN_NL  # (the per-interval form is one launch per interval: the generic kernels', on every engine)


# ---------------------------------------------------------------------------
# variants of a base case
# ---------------------------------------------------------------------------
def _variant_spec(base, variant, nt):
    import test_nonselfadjoint_controls as tnc

    if variant == 'liouv':  # (the d = 5 Lindbladian, dense: N = 25 on the q2 engine, one slot)
        return tnc._liouv(bca._lindblad5(nt))
    spec = BASES[base].build(nt)
    if variant is None:
        return spec
    if variant == 'absent':  # the last term is absent from the first and the last objective
        return tac._drop(spec, [(0, spec.L - 1), (spec.K - 1, spec.L - 1)])
    if variant == 'only':  # additionally the ONLY term of a control (J = 3: slot 1 is all of control 0) from objective 1
        assert [c for c, _ in terms_of(base)].count(terms_of(base)[1][0]) == 1
        return tac._drop(spec, [(0, spec.L - 1), (spec.K - 1, spec.L - 1), (1, 1)])
    if variant in ('lower', 'ladder'):  # every term operator
        for l in range(spec.L):
            tnc._nsa(spec, variant, l=l, seed=5 + l)
        return spec
    raise KeyError(variant)


def variant_terms(base, variant):
    return [(0, 3)] if variant == 'liouv' else terms_of(base)


# ---------------------------------------------------------------------------
# problems: a base case (or its variant) with its term table under an axis
#   how = ('ends', I)            helpers.grid_ends on I intervals at the engine's own theta_max
#         (regime, theta_max)    helpers.REGIMES[regime] on REGIME_INTERVALS intervals (long: LONG_INTERVALS)
# ---------------------------------------------------------------------------
def engine_theta(base, how):
    return BASES[base].theta_max if how[0] == 'ends' else how[1]


def intervals(how):
    return how[1] if how[0] == 'ends' else LONG_INTERVALS if how[0] == 'long' else REGIME_INTERVALS


@functools.lru_cache(maxsize=None)
def problem(base, how, variant=None):
    b = BASES[base]
    obj = nc.with_terms(hp.explicit(_variant_spec(base, variant, intervals(how) + 1), b.fmt), variant_terms(base, variant))
    obj = hp.grid_ends(obj, b.theta_max) if how[0] == 'ends' else hp.REGIMES[how[0]](obj, how[1])
    obj.lambdas = nc.lambdas_in_eps(obj)
    return obj


def _oracle(obj):
    return bca._oracle(nc.coefficient_view(obj))


def tolerance(obj, how):
    if bca.liouville(obj):
        return TOL_LIOUVILLE
    return TOL_RAMP if how[0] in ('ramp', 'amplitude') else TOL_HILBERT


def restate(obj, prob, chi, norms, so_inputs=None, lambdas=None, linear_weights=False, pulses=None, shapes=None):
    """``nc.update_sweep`` as a dict."""
    kw = {} if so_inputs is None else dict(sigma_vals=so_inputs[1], fw_prev=so_inputs[0], store=True)
    out = nc.update_sweep(prob, chi, norms, obj.pulses if pulses is None else pulses, obj.terms,
                          obj.shapes if shapes is None else shapes, obj.lambdas if lambdas is None else lambdas,
                          linear_weights=linear_weights, **kw)
    ref = dict(opt=np.array(out[0]), psi_T=out[1], g_a=np.array(out[2]))
    if so_inputs is not None:
        ref['store'] = out[3]
    return ref


AMPLITUDE_MOVE = 0.01  # the ``amplitude`` rows: the update moves max |eps| by at least this fraction


def build_reference(obj, so, regime=None, liouv=False, norms_factor=1.0, seed=5):
    """The restated non-linear update sweep of a problem and its inputs."""
    view = nc.coefficient_view(obj)
    prob = bca._oracle(view)
    norms = tsr.chi_norms(view) * norms_factor
    if liouv:  # (tests/test_bounded_constrained_axes.py: ||chi|| = 1.2 lets a wrong adjoint move g_a by > 1e-6)
        norms = np.full(obj.K, 1.2)
    chi_T = bca.boundary_costates(view, prob)
    lambdas = list(obj.lambdas)
    with hp.MemoExpm():
        chi = ko.backward_sweep(prob, chi_T, view.pulses)
        so_inputs = bca.second_order_inputs(view, prob, seed) if so else None
        ref = restate(obj, prob, chi, norms, so_inputs, lambdas)
        if regime == 'amplitude':
            top = np.abs(np.array(obj.pulses)).max()
            for _ in range(24):
                if np.abs(ref['opt'] - np.array(obj.pulses)).max() >= AMPLITUDE_MOVE * top:
                    break
                assert np.abs(ref['opt']).max() < 2.0 * top
                lambdas = [0.5 * lam for lam in lambdas]
                ref = restate(obj, prob, chi, norms, so_inputs, lambdas)
        wrong = None
        if regime == 'tiny':
            # every operator x 1e-7: psi(T) hardly depends on the pulses and g_a is of the order lambda_a (x 1e-7, too), so
            # that under the ||chi_k|| of tests/test_series_regimes.py (chosen to keep the feedback of a base case small; here
            # there is none) a device that forgot the weights would be told by its pulses alone.  ||chi_k|| x 4 until
            # it would be told by every compared quantity; the witness asserts that the row still is in its regime
            tol = TOL_LIOUVILLE if bca.liouville(obj) else TOL_HILBERT
            for _ in range(12):
                wrong = restate(obj, prob, chi, norms, so_inputs, lambdas, linear_weights=True)
                if all(bca._distance(wrong[w], ref[w]) / scale(ref, w) > BITES * tol for w in wrong):
                    break
                if max(np.abs(ref['opt']).max(), np.abs(wrong['opt']).max()) > 4.0 * max(1.0, np.abs(np.array(obj.pulses)).max()):
                    break  # (no further: the pulses would leave the regime; the witness then says which quantity does not bite)
                norms = 4.0 * norms
                ref = restate(obj, prob, chi, norms, so_inputs, lambdas)
        ref['wrong'] = wrong
    assert np.all(np.isfinite(ref['opt'])) and np.all(np.isfinite(ref['psi_T']))
    ref.update(obj=obj, prob=prob, norms=norms, chi_T=chi_T, chi=chi, so_inputs=so_inputs, lambdas=np.array(lambdas),
               coef=np.array(view.pulses), dcde=nc.weights(obj.terms, obj.pulses))
    return ref


@functools.lru_cache(maxsize=None)
def reference(base, how, so=False, variant=None):
    """The restatement of a row (computed once and shared; nobody writes to it)."""
    return build_reference(problem(base, how, variant), so, how[0], variant == 'liouv')


@functools.lru_cache(maxsize=None)
def wrong_weights(base, how, so=False, variant=None):
    """The same sweep with every weight replaced by its power-1 value."""
    ref = reference(base, how, so, variant)
    if ref['wrong'] is not None:
        return ref['wrong']
    with hp.MemoExpm():
        return restate(ref['obj'], ref['prob'], ref['chi'], ref['norms'], ref['so_inputs'], ref['lambdas'], linear_weights=True)


def scale(ref, what):
    return max(1.0, float(np.abs(ref[what]).max())) if what in ('opt', 'g_a') else 1.0


def distances(got, ref):
    return {w: bca._distance(got[w], ref[w]) / scale(ref, w) for w in got if w in ref and w in ('opt', 'psi_T', 'g_a', 'store')}


# ---------------------------------------------------------------------------
# the table of cases
# ---------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'id group base how so variant mode')
CASES = collections.OrderedDict()


def add(group, base, how, so=False, variant=None, mode='whole'):
    cid = '%s-%s-%s%s%s%s%s' % (group, base, how[0], ('%g' % how[1]).replace('.', 'p'), '-so' if so else '',
                                '-' + variant if variant else '', '-stepwise' if mode != 'whole' else '')
    assert cid not in CASES, cid
    CASES[cid] = Case(cid, group, base, how, so, variant, mode)


ENGINE = ('ends', ENGINE_INTERVALS)
# 1. engine rows: every base, first and second order
for _b in TILE_FORM + GEN_FORM:
    for _so in (False, True):
        add('engine', _b, ENGINE, so=_so)

# 2. regimes: one tile-form base per J and six generic-form bases at the engine's own theta_max; second order under the two
# non-uniform regimes (the tile forms: the <.., true> instantiations); the tile256 form (two rows per thread) under the ramps
REGIME_TILE, REGIME_GEN = ('q2', 'tile_L2', 'tile_L3', 'tile_L4'), ('tile128', 'coop', 'ell', 'gencsr', 'tilex', 'mixed')
FOUR = ('ramp', 'pulse_ramp', 'tiny', 'amplitude')
for _b in REGIME_TILE + REGIME_GEN:
    for _r in FOUR:
        add('regime', _b, (_r, BASES[_b].theta_max))
    for _r in ('ramp', 'amplitude') if _b in REGIME_TILE else ('ramp',):
        add('regime', _b, (_r, BASES[_b].theta_max), so=True)
for _so in (False, True):
    add('regime', 'tile256', ('ramp', 1.0), so=_so)
    add('regime', 'tile256', ('amplitude', 1.0), so=_so)
LONG = ('tile_L2', 'tile128')
for _b in LONG:
    add('regime', _b, ('long', 1.0))

# 3. the ends of the pipeline: 1, 2, 3 intervals, 63, 64, 65 and 257 time points
ENDS = ('tile_L3', 'tile128')
for _b in ENDS:
    for _I in (1, 2, 3, 62, 63, 64, 256):
        add('ends', _b, ('ends', _I))
    for _I in (1, 2, 3):
        add('ends', _b, ('ends', _I), so=True)

# 4. absent terms (J = 3: control 0 has one term only), term operators that are not self-adjoint
for _b in ('tile_L3', 'ellglobal'):
    for _v in ('absent', 'only'):
        add('absent', _b, ENGINE, variant=_v)
add('absent', 'tile_L4', ENGINE, variant='absent')
add('absent', 'tilex', ENGINE, variant='absent')
for _b, _v in (('tile_L2', 'lower'), ('tile_L4', 'ladder'), ('tile128', 'ladder'), ('tilex', 'lower'), ('q2', 'liouv')):
    add('nsa', _b, ENGINE, variant=_v)
    add('nsa', _b, ENGINE, variant=_v, so=True)

# 5. the per-interval form
for _b in ('tile_L3', 'tile128'):
    for _so in (False, True):
        add('stepwise', _b, ENGINE, so=_so, mode='0')

CASE_IDS = list(CASES)


def case_reference(c):
    return reference(c.base, c.how, c.so, c.variant)


def expected_kernel(c):
    if c.variant == 'liouv':  # (N = 25, one slot)
        return TILE_NL(1, 1, c.so)
    return nl_kernel(c.base, c.so, 'whole' if c.mode == 'whole' else 'stepwise')


def case_terms(c):
    return variant_terms(c.base, c.variant)


# ---------------------------------------------------------------------------
# host
# ---------------------------------------------------------------------------
def test_tables_are_what_the_docstring_says():
    from krotov_amd import _lib

    names = {n for n in _lib.kernel_instantiations() if '_nl<' in n}
    assert {expected_kernel(c) for c in CASES.values()} == names  # ten tile forms and two generic ones
    assert {expected_kernel(c) for c in CASES.values() if c.group == 'regime'} == names
    tile = lambda c: expected_kernel(c).startswith('kh_tile')  # noqa: E731
    for form in (True, False):
        tables = [case_terms(c) for c in CASES.values() if tile(c) == form]
        assert {p for t in tables for _, p in t} == {1, 2, 3, 4}, 'every power under both forms'
        assert any(t[0][0] != 0 for t in tables), 'slot 0 of a control other than 0'
        apart = lambda t: any(t[j][0] == t[i][0] and t[j - 1][0] != t[i][0] for i in range(len(t)) for j in range(i + 2, len(t)))  # noqa: E731
        assert any(apart(t) for t in tables), "one control's terms apart"
    assert len(nc.AXES_TABLES[6]) > 4  # (beyond KH_MAX_L slots: the generic form)
    assert set(TILE_FORM + GEN_FORM) == set(BASES) - {'tile256_noq2'}
    for c in CASES.values():
        obj = problem(c.base, c.how, c.variant)
        assert obj.L == len(case_terms(c)) and (c.variant == 'liouv' or obj.L == SLOTS[c.base])
        assert len(obj.pulses) == nc.n_controls(obj.terms) == len(obj.shapes) == len(obj.lambdas)
        if c.how[0] != 'ends':
            assert c.how[1] == BASES[c.base].theta_max
        assert obj.N <= (144 if c.base == 'ell' else 100)
    families = {BASES[c.base].family for c in CASES.values() if expected_kernel(c) == GEN_NL and c.mode == 'whole'}
    assert families >= {'tile128/512', 'coop16/mfma', 'ens64/mfma', 'tile64/stream', 'tile64x/512', 'ell/csr', 'ellstream/csr',
                        'generic/csr', 'ellglobal/csr'}


def _series_tables(obj, theta_max, regime):
    return bca._tables(obj, theta_max, regime)


def in_regime(obj, regime, theta_max, pulses, tables):
    """The conditions of a regime under ``pulses`` (C rows), for the objective with the largest theta and the thresholds
    of every table an engine family may use: ramps reach one, two and three sub-steps and at least four distinct degrees;
    ``tiny`` stays at one sub-step of degree <= 4."""
    theta_all = hp.theta_sequence(obj, pulses)
    theta = theta_all[int(np.argmax(theta_all.max(axis=1)))]
    for name, tab in tables.items():
        nsub, deg = hp.series_plan(theta, theta_max, tab)
        if regime == 'tiny':
            assert nsub.max() == 1 and deg.max() <= 4, (name, deg.max())
        else:
            assert set(nsub.tolist()) >= {1, 2, 3}, (name, sorted(set(nsub.tolist())))
            assert len(set(deg.tolist())) >= 4, (name, sorted(set(deg.tolist())))
    return theta


def no_linear_term(terms):
    """The controls without a power-1 term: their weight at eps = 0 is exactly 0."""
    return [c for c in range(nc.n_controls(terms)) if not any(cj == c and p == 1 for cj, p in terms)]


@pytest.mark.parametrize('cid', CASE_IDS)
def test_witness(cid):
    """Host only, over the very table the GPU test runs: module docstring."""
    c = CASES[cid]
    obj = problem(c.base, c.how, c.variant)
    ref = case_reference(c)
    I, guess = intervals(c.how), np.array(obj.pulses)
    tol = tolerance(obj, c.how)
    assert len(hp.regime_dt(obj)) == I and len(obj.tlist) == I + 1 and guess.shape == (nc.n_controls(obj.terms), I)
    regime, theta_max = c.how[0], engine_theta(c.base, c.how)
    if regime == 'ends':
        hp.grid_ends_witness(obj, theta_max)
    else:
        tables = _series_tables(obj, theta_max, regime)
        if regime != 'amplitude':  # (the suite's own conditions of the regime, under the guess)
            hp.regime_witness(obj, regime, theta_max, guess, tables)
        for pulses in (guess, ref['opt']):
            in_regime(obj, regime, theta_max, pulses, tables)
    if regime == 'amplitude':
        mags = np.abs(guess)
        assert np.all(mags.max(axis=1) >= 1.5) and all(m[m > 0].min() <= 0.5 for m in mags)
        assert any(p.min() < 0.0 < p.max() for p in guess)
        assert np.abs(ref['opt'] - guess).max() >= AMPLITUDE_MOVE * mags.max()
        assert np.ptp(hp.regime_dt(obj)) > 0
    moved = np.count_nonzero(ref['opt'] != guess, axis=1)
    assert np.all(moved >= 0.9 * I), moved
    if regime in ('pulse_ramp', 'long'):
        assert np.all(np.count_nonzero(guess == 0.0, axis=1) >= 3)
        for cc in no_linear_term(obj.terms):
            assert np.all(ref['opt'][cc][guess[cc] == 0.0] == 0.0)
    wrong = distances(wrong_weights(c.base, c.how, c.so, c.variant), ref)
    print('witness %s: weight 1 moves %s (x tolerance %.0e); pulse change %.1e; lambdas %s' % (
        cid, ' '.join('%s %.1e' % (w, d / tol) for w, d in sorted(wrong.items())), tol, np.abs(ref['opt'] - guess).max(),
        ref['lambdas']))
    assert all(d > BITES * tol for d in wrong.values()), wrong
    if c.variant is not None:
        for tag, d in _wrong_results(c, obj, ref).items():
            for what, x in d.items():
                print('witness %s (%s): %s moves by %.2e' % (cid, tag, what, x))
                assert x > 1e-6, (cid, tag, what, x)


def _wrong_results(c, obj, ref):
    """{mistake: {quantity: distance from the right result}} of a variant row: an absent entry filled, the backward
    generator built from H_j for H_j^dagger, the update sums with H_j chi for H_j^dagger chi."""
    import test_nonselfadjoint_controls as tnc

    out = {}
    if c.variant in ('absent', 'only'):
        filled = tac._filled(obj)
        filled.terms, filled.pulses = obj.terms, obj.pulses
        wrong_probs = {'filled': _oracle(filled)}
    else:
        wrong_probs = {'H_j for its adjoint': tnc._with_adjoints(ref['prob'], lambda o: o)}
    with hp.MemoExpm():
        for tag, prob in wrong_probs.items():
            chi = ko.backward_sweep(prob, ref['chi_T'], list(ref['coef']))
            fw = prob if c.variant in ('absent', 'only') else ref['prob']
            got = restate(obj, fw, chi, ref['norms'], ref['so_inputs'], ref['lambdas'])
            out[tag] = {w: bca._distance(got[w], ref[w]) for w in ('opt', 'psi_T', 'g_a')}
            out[tag]['chi'] = bca._distance(chi, ref['chi'])
        if c.variant not in ('absent', 'only'):
            with tnc._Mu(lambda o: o.conj().T):
                got = restate(obj, ref['prob'], ref['chi'], ref['norms'], ref['so_inputs'], ref['lambdas'])
            out['mu: H_j chi'] = {w: bca._distance(got[w], ref[w]) for w in ('opt', 'psi_T', 'g_a')}
    return out


def series_table(obj, theta_max):
    """The table of the one-term-per-phase kernels on an engine of ``obj``: the Chebyshev form (cap max(2, theta_max)) on
    Hermitian operators, Taylor's otherwise (tests/test_series_tolerance.py names them so)."""
    import series_oracle as so

    ops = [op for k in range(obj.K) for op in [obj.H0[k]] + list(obj.Hc[k]) if op is not None]
    if obj.fmt == 'mixed' or bca.liouville(obj) or not all(np.array_equal(op, np.asarray(op).conj().T) for op in ops):
        return so.table('taylor', 0.0, 2.0)
    return so.table('real', 0.0, max(2.0, theta_max))


UNDERPLAN = [(c.base, c.how) for c in CASES.values() if c.how[0] == 'amplitude' and not c.so]


@pytest.mark.parametrize('base,how', UNDERPLAN, ids=['%s-%g' % (b, h[1]) for b, h in UNDERPLAN])
def test_theta_from_eps_would_underplan(base, how):
    """A kernel that formed theta from |eps| instead of |eps^p| (``kh_tile64_update.inc``, ``kh_gen_update.inc``: the
    coefficient's magnitude): on the ``amplitude`` rows the plan from sum_j |eps_c(j)| n_j, the powers ignored, differs from
    the right one in sub-steps or degree on at least half of the intervals, and the restatement evaluated through the series
    oracle with that plan is more than 1e3 tolerances away from the exact one in the final states (with the right plan it
    is within the tolerance: the distance is the plan's).  ``helpers.regime_amplitude`` scales every control to the same
    largest coefficient |eps^p| = 256 for this: with |eps| <= 4 on every table the row with powers 2 and 1 was
    under-planned by a factor 2 only, which the series' margin absorbed (4.3e-13)."""
    import series_oracle as so

    ref = reference(base, how)
    obj, prob = ref['obj'], ref['prob']
    theta_max, tab = how[1], series_table(ref['obj'], how[1])
    ignored = [(c, 1) for c, _ in obj.terms]
    differs = 0
    for k in range(obj.K):
        right = hp.series_plan(hp.theta_sequence(obj, ref['opt'])[k], theta_max, tab.theta)
        wrong = hp.series_plan(hp.theta_sequence(obj, ref['opt'], terms=ignored)[k], theta_max, tab.theta)
        differs = max(differs, int(np.count_nonzero((right[0] != wrong[0]) | (right[1] != wrong[1]))))
    I = intervals(how)
    inv = np.array([1.0 / p for _, p in obj.terms])

    def theta_from_eps(norms, coef, dt):  # (the step sees the coefficients eps^p: |eps| is their p-th root)
        return dt * (norms[0] + float(np.dot(np.abs(coef) ** inv, norms[1:])))

    view = nc.coefficient_view(obj)
    dist = {}
    for tag, theta_of in (('right plan', None), ('plan from |eps|', theta_from_eps)):
        with so.SeriesOracle(prob, hp.series_bounds(view), tab, theta_max, theta_of=theta_of):
            # (the sweep's final states are the propagation under its updated pulses; those are held at the exact
            # restatement's, so that a series that went wrong does not feed back into the pulses and theta)
            got = ko.forward_propagation(prob, nc.coefficients(obj.terms, ref['opt']))
        dist[tag] = bca._distance(got, ref['psi_T'])
    tol = tolerance(obj, how)
    print('%s %s: the plan from |eps| differs on %d of %d intervals; final states off by %.1e (right plan: %.1e)' % (
        base, how, differs, I, dist['plan from |eps|'], dist['right plan']))
    assert differs >= 0.5 * I
    assert dist['right plan'] < tol and dist['plan from |eps|'] > BITES * tol


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def table_arrays(terms):
    return np.array([c for c, _ in terms], dtype=np.int32), np.array([p for _, p in terms], dtype=np.int32)


def run_nl(eng, ref, so, mode='whole', chi=None, lambdas=None, set_table=True, dcde=None, guess=None):
    """One non-linear update sweep of ``ref`` on ``eng`` into NaN-filled outputs; returns (outputs on the host, deviations
    from the restatement, launched instantiations).  ``set_table=False``: the table in force stays as it is; ``dcde`` /
    ``guess``: device tensors to use for the weights / the guess pulses (default: fresh uploads of the reference's)."""
    import torch

    from krotov_amd import _lib

    obj, prob = ref['obj'], ref['prob']
    c128, f64, dv = torch.complex128, torch.float64, eng.device
    pulses, S = np.array(obj.pulses), np.array(obj.shapes)
    lam = ref['lambdas'] if lambdas is None else lambdas
    C, I = pulses.shape
    dev = {}
    if chi is None:
        chi = eng.backward(ref['chi_T'], ref['coef'], out=bca._nans((obj.K, I + 1, prob.N), c128, dv))
        dev['chi'] = bca._distance(chi.cpu().numpy(), ref['chi'])
    store = None
    if so:
        store = bca._nans((obj.K, I + 1, prob.N), c128, dv)
        eng.set_second_order(ref['so_inputs'][0], store, ref['so_inputs'][1])
    if set_table:
        tc, tp = table_arrays(obj.terms)
        eng.set_nonlinear(tc, tp, ref['dcde'] if dcde is None else dcde)
    _lib.forget_launched_kernels()
    if mode == 'whole':
        opt, psi_T, g_a = eng.forward_update(chi, ref['norms'], prob.init, pulses if guess is None else guess, S, lam,
                                             out=(bca._nans((C, I), f64, dv), bca._nans((obj.K, prob.N), c128, dv),
                                                  bca._nans((C,), f64, dv)))
    else:
        if getattr(eng, '_sh', None) is not None:
            for name in ('opt', 'psi_T', 'g_a'):
                eng._sh[name].fill_(float('nan'))
        opt, psi_T, g_a = eng.forward_update_sharded(chi, ref['norms'], prob.init, pulses, S, lam, lambda x: None,
                                                     graph_chunk=int(mode))
        assert eng._sh['graph'] is None, 'no capture while a table is set'
    eng.check()
    launched = sorted(_lib.kernel_instantiations(launched_only=True))
    assert eng.stats()['intervals'] == I
    out = dict(opt=opt.cpu().numpy(), psi_T=psi_T.cpu().numpy(), g_a=g_a.cpu().numpy())
    assert out['opt'].shape == (C, I) and out['g_a'].shape == (C,)
    if so:
        out['store'] = store.cpu().numpy()
        assert np.array_equal(out['store'][:, 0], np.asarray(prob.init, dtype=np.complex128)), 'slice 0 is the initial states'
    dev.update(distances(out, ref))
    for cc in no_linear_term(obj.terms):  # an exact zero of a control without a power-1 term stays 0.0
        assert np.all(out['opt'][cc][pulses[cc] == 0.0] == 0.0)
    return out, dev, launched


DEVIATIONS = {}  # row group / regime: the largest deviation (printed for DESIGN.md)


def _record(c, worst):
    group = c.group if c.group != 'regime' else 'regime/' + c.how[0]
    DEVIATIONS[group] = max(DEVIATIONS.get(group, 0.0), worst) if np.isfinite(worst) else float('nan')
    return group, DEVIATIONS[group]


@pytest.mark.gpu
@pytest.mark.parametrize('cid', CASE_IDS)
def test_matrix(cid, monkeypatch):
    """One non-linear update sweep (opt, psi(T), g_a with C rows; second order: the stored trajectory, slice 0 bit for bit
    the initial states) against ``nc.update_sweep``; every output NaN-filled before the sweep, the kernel family and the
    launched instantiation asserted, ``stats()['intervals']`` the grid's, exact zeros of a control without a power-1 term
    bit for bit 0.0, and -- on the generic form -- the grid that ran against the clamp rule of ``update_generic``."""
    c = CASES[cid]
    for name, value in BASES[c.base].env.items():
        monkeypatch.setenv(name, value)
    ref = case_reference(c)
    obj = ref['obj']
    tol = tolerance(obj, c.how)
    want = expected_kernel(c)
    eng = make_engine(c.base, obj, engine_theta(c.base, c.how), family=c.variant in (None, 'absent', 'only'))
    try:
        _, dev, launched = run_nl(eng, ref, c.so, c.mode)
        update = [n for n in launched if 'update' in n]
        assert want in launched and [n for n in launched if '_nl<' in n] == [want], (cid, want, launched)
        if want in (GEN_NL, GEN_NL_MIXED) and c.mode == 'whole':
            assert eng.stats()['workgroups'] == generic_grid(eng), (eng.stats(), generic_grid(eng))
        kernel = eng.kernel
    finally:
        eng.close()
    worst = max(dev.values())
    group, so_far = _record(c, worst)
    print('nonlinear_axes %s [%s]: %s; %s so far %.1e; launched: %s' % (
        cid, kernel, ' '.join('%s %.1e' % kv for kv in sorted(dev.items())), group, so_far, ', '.join(update)))
    assert np.isfinite(worst) and worst < tol, dev


# ---------------------------------------------------------------------------
# GPU: refusals, with the error code and no sweep launched
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.no_oracle
def test_refusals(monkeypatch):
    """``set_nonlinear`` on a Lindblad-form, a replica, a row-split and a sharded-window engine and on one whose vectors do
    not fit the generic kernels' LDS: ``refuse_form``'s code (KH_ERR_UNSUPPORTED) and words, the table not in force
    afterwards, and no sweep kernel launched.  Every call returns before any launch."""
    import ctypes

    import torch

    from krotov_amd import _lib, configs
    from krotov_amd.engine import HipKrotovEngine

    def refused(eng, words):
        L, I = eng.L, eng.nt - 1
        w = torch.ones((L, I), dtype=torch.float64, device=eng.device)
        with pytest.raises(_lib.KrotovHipError, match=words) as err:
            eng.set_nonlinear(np.zeros(L, dtype=np.int32), np.full(L, 2, dtype=np.int32), w)
        assert err.value.code == _lib.KH_ERR_UNSUPPORTED
        assert eng._nl is None and eng._update_rows() == L
        return w

    _lib.forget_launched_kernels()
    rng = np.random.default_rng(2)
    nt = 6
    rho_ops = [[configs.herm(rng, 3, 1.0), configs.herm(rng, 3, 0.5)]]
    lind = HipKrotovEngine(rho_ops, np.full(nt - 1, 0.1), c_ops=[[0.1 * configs.herm(rng, 3, 1.0)]])
    refused(lind, 'Lindblad-form engines')
    lind.close()
    ops = [[configs.herm(rng, 4, 1.0), configs.herm(rng, 4, 0.5), configs.herm(rng, 4, 0.5)] for _ in range(2)]
    rep = HipKrotovEngine(ops, np.full((1, nt - 1), 0.1), replicas=1)
    refused(rep, 'replica engines')
    rep.close()
    sharded = HipKrotovEngine(ops, np.full(nt - 1, 0.1))
    handle = (ctypes.c_ubyte * 64)()
    assert sharded._lib.kh_p2p_create_window(sharded._handle, 1, 0, handle) == 0  # (the window alone: no peer, no self-test)
    refused(sharded, 'sharded engines')
    sharded.close()
    monkeypatch.setenv('KH_KERNEL', 'ellsplit')
    monkeypatch.setenv('KH_ELL_SPLIT', '2')
    spec = tsr._banded(600, 21, nt=4, K=2)
    split = HipKrotovEngine(configs.sparse_ops(spec), np.diff(spec.tlist))
    assert split.kernel == 'ellsplit/csr' and split.row_split == 2
    refused(split, 'split engine')
    assert split.set_row_split(1) == 1 and split.kernel == 'ellglobal/csr'
    w = torch.ones((1, 3), dtype=torch.float64, device=split.device)
    split.set_nonlinear([0], [2], w)  # (row split 1: accepted)
    assert split._update_rows() == 1
    split.close()
    monkeypatch.delenv('KH_KERNEL')
    monkeypatch.delenv('KH_ELL_SPLIT')
    spec = configs.config_sparse_lindblad(d=65, nt=4, K=2)
    big = HipKrotovEngine(configs.sparse_ops(spec), np.diff(spec.tlist), is_super=True)
    assert big.kernel == 'ellglobal/csr' and big.N == 4225
    refused(big, 'do not fit LDS')
    big.check()
    big.close()
    assert _lib.kernel_instantiations(launched_only=True) == []


# ---------------------------------------------------------------------------
# one engine, changed tables and inputs: every step bit for bit a fresh engine's
# ---------------------------------------------------------------------------
REUSE = ('tile_L3', 'tile128', 'ellglobal')  # a tile-form, a generic-form and a CSR base
# table B of a base with J slots: the same J, another C and other powers (``opt`` and ``g_a`` change their row count)
TABLE_B = {2: [(1, 3), (0, 2)], 3: [(2, 2), (0, 3), (1, 1)]}


@functools.lru_cache(maxsize=None)
def reuse_inputs(base):
    """(A, A second order, B, A2, parametrized) on ONE grid, A's: B has table B with pulses of its own; A2 is A with other
    pulses (0.8 x, reversed in time), other norms and another sigma seed -- for the in-place changes; the parametrized
    reference (tests/test_bounded_constrained_axes.py) takes A's coefficient pulses as its J guess pulses."""
    b = BASES[base]
    A, A_so = reference(base, ENGINE), reference(base, ENGINE, True)
    obj = A['obj']
    I = len(obj.pulses[0])
    plain = hp.explicit(b.build(I + 1), b.fmt)  # (lambda_a and shapes of the base case)

    def other(terms, pulses):
        new = copy.copy(obj)
        new.terms = list(terms)
        C = nc.n_controls(terms)
        new.pulses = pulses(new)
        new.shapes = [np.array(obj.shapes[0]) for _ in range(C)]
        new.lambdas = list(plain.lambdas[:C])
        new.lambdas = nc.lambdas_in_eps(new)
        return new

    B = build_reference(other(TABLE_B[obj.L], lambda new: hp.grid_ends_pulses(new, I)), False, norms_factor=0.7)
    A2 = build_reference(other(obj.terms, lambda new: [0.8 * np.asarray(p)[::-1].copy() for p in obj.pulses]), False,
                         norms_factor=0.6)
    lin = nc.coefficient_view(obj)
    lin.shapes = [np.array(obj.shapes[0]) for _ in range(obj.L)]
    lin.lambdas = list(plain.lambdas[:obj.L])
    par = bca.build_par_reference(lin, False)
    return A, A_so, B, A2, par


@pytest.mark.parametrize('base', REUSE)
def test_reuse_inputs_differ(base):
    """Host only: the tables differ in C and in every power, every input of the sets differs and so does every result -- a
    stale table, weight tensor or pulse would be told."""
    A, A_so, B, A2, par = reuse_inputs(base)
    ta, tb = A['obj'].terms, B['obj'].terms
    assert len(ta) == len(tb) and nc.n_controls(ta) != nc.n_controls(tb) and all(x[1] != y[1] for x, y in zip(ta, tb))
    assert A['opt'].shape != B['opt'].shape
    for X in (B, A2):
        for what in ('coef', 'dcde', 'chi', 'norms', 'psi_T'):
            assert bca._distance(A[what], X[what]) > 1e-6, what
    for what in ('opt', 'g_a', 'psi_T'):
        assert bca._distance(A[what], A2[what]) > 1e-6 and bca._distance(A[what], A_so[what]) > 1e-9, what
    assert np.abs(par['opt'] - np.array(par['obj'].pulses)).max() > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('base', REUSE)
def test_one_engine_changed_tables_and_inputs(base, monkeypatch):
    """One engine through: table A; table B (the same J, another C, other powers); A again with ``dcde`` in a new tensor;
    second order on, then off; ``set_parametrization`` while the table is set (KH_ERR_INVALID, the table stays in force,
    the next sweep -- without setting it again -- equals the first); ``set_nonlinear()`` off and a parametrized sweep (a
    fresh engine's, on the same kernel); back to A; a reduced update grid set while the table is on (where the family has
    one), then the table off: the linear sweep runs the kernels, on the grid, of an engine on which nothing was ever set;
    pulses, ``dcde`` and chi changed in place between sweeps.  Every step bit for bit a fresh engine's given the same inputs,
    and within the tolerance of its restatement."""
    import torch

    from krotov_amd import _lib

    for name, value in BASES[base].env.items():
        monkeypatch.setenv(name, value)
    A, A_so, B, A2, par = reuse_inputs(base)
    obj, prob = A['obj'], A['prob']
    theta_max, tol = BASES[base].theta_max, tolerance(obj, ENGINE)
    worst = {}

    def same(tag, got, want):
        for what in want:
            assert np.array_equal(got[what], want[what]), '%s: %s' % (tag, what)

    def fresh(run):
        eng = make_engine(base, obj, theta_max)
        try:
            return run(eng)
        finally:
            eng.close()

    def nl(ref, so=False, **kw):
        def run(eng):
            out, dev, launched = run_nl(eng, ref, so, **kw)
            return out, dev, [n for n in launched if 'update' in n]
        return run

    def linear(eng):
        """The linear sweep of the J coefficient pulses (what an engine without a table computes)."""
        J, I = A['coef'].shape
        chi = eng.backward(A['chi_T'], A['coef'])
        _lib.forget_launched_kernels()
        res = eng.forward_update(chi, A['norms'], prob.init, A['coef'], np.array(par['obj'].shapes), np.array(par['obj'].lambdas))
        eng.check()
        out = dict(zip(('opt', 'psi_T', 'g_a'), (x.cpu().numpy() for x in res)))
        return out, eng.stats()['workgroups'], sorted(n for n in _lib.kernel_instantiations(launched_only=True) if 'update' in n)

    def parametrized(eng):
        out, dev, launched = bca.run_par(eng, par, False)
        return out, dev, [n for n in launched if 'update' in n]

    want = {tag: fresh(nl(ref, so)) for tag, ref, so in (('A', A, False), ('B', B, False), ('A so', A_so, True), ('A2', A2, False))}
    want_par, want_linear = fresh(parametrized), fresh(linear)
    assert not any('_nl<' in n or '_par<' in n for n in want_linear[2]), want_linear[2]
    eng = make_engine(base, obj, theta_max)
    try:
        def step(tag, key, ref, so=False, **kw):
            out, dev, launched = nl(ref, so, **kw)(eng)
            same(tag, out, want[key][0])
            assert launched == want[key][2], (tag, launched, want[key][2])
            worst[tag] = max(dev.values())
            return out

        step('A', 'A', A)
        step('B', 'B', B)
        assert eng._update_rows() == nc.n_controls(B['obj'].terms)
        step('A, dcde in a new tensor', 'A', A, dcde=eng.dev(A['dcde'], torch.float64).clone())
        step('second order on', 'A so', A_so, so=True)
        eng.set_second_order()
        step('second order off', 'A', A)
        # a parametrization next to the table: refused, and the table stays in force
        kind, a, b = bca.device_kinds(par['kinds'], par['obj'].pulses)
        u_opt = bca._nans(par['u_guess'].shape, torch.float64, eng.device)
        with pytest.raises(_lib.KrotovHipError) as err:
            eng.set_parametrization(kind, a, b, par['u_guess'], par['dfdu'], u_opt)
        assert err.value.code == _lib.KH_ERR_INVALID
        assert eng._update_rows() == nc.n_controls(obj.terms)
        step('after the refused parametrization', 'A', A, set_table=False)
        # table off, a parametrized sweep: a fresh engine's, on the same kernel
        eng.set_nonlinear()
        out, dev, launched = parametrized(eng)
        same('parametrized', out, want_par[0])
        assert launched == want_par[2] and any('_par<' in n for n in launched), (launched, want_par[2])
        worst['parametrized'] = max(dev.values())
        eng.set_parametrization(None)
        step('back to A', 'A', A)
        # a reduced grid set while the table is on; the table off drops it
        K = obj.K
        try:
            reduced = eng.set_update_workgroups(max(1, K - 2))
        except _lib.KrotovHipError as exc:
            assert exc.code == _lib.KH_ERR_UNSUPPORTED and base != 'tile_L3', exc
            reduced = None
        if reduced is not None:
            out, dev, launched = nl(A, set_table=False)(eng)
            assert eng.stats()['workgroups'] <= reduced
            worst['reduced grid'] = max(dev.values())
        eng.set_nonlinear()
        out, grid, launched = linear(eng)
        same('linear after the table', out, want_linear[0])
        assert (grid, launched) == want_linear[1:], (grid, launched, want_linear[1:])
        # inputs changed in place between sweeps
        f64, c128 = torch.float64, torch.complex128
        t_guess, t_dcde = eng.dev(np.array(obj.pulses), f64).clone(), eng.dev(A['dcde'], f64).clone()
        t_chi = bca._nans(A['chi'].shape, c128, eng.device)
        eng.backward(A['chi_T'], A['coef'], out=t_chi)
        step('A on kept tensors', 'A', A, chi=t_chi, dcde=t_dcde, guess=t_guess)
        t_guess.copy_(torch.from_numpy(np.array(A2['obj'].pulses)))
        t_dcde.copy_(torch.from_numpy(np.ascontiguousarray(A2['dcde'])))
        eng.backward(A2['chi_T'], A2['coef'], out=t_chi)
        step('A2 in place', 'A2', A2, chi=t_chi, guess=t_guess, set_table=False)
        kernel = eng.kernel
    finally:
        eng.close()
    print('nonlinear_axes reuse %s [%s]: %s; update kernels %s / %s / %s' % (
        base, kernel, ' '.join('%s %.1e' % kv for kv in worst.items()), want['A'][2], want_par[2], want_linear[2]))
    assert max(worst.values()) < tol, worst


# ---------------------------------------------------------------------------
# tests/fuzz_parity.py --nonlinear
# ---------------------------------------------------------------------------
FUZZ_SEED, FUZZ_CASES = 3, 12


def test_fuzz_generator_is_its_own():
    """Host only: ``--nonlinear`` decides with a generator of its own -- the default stream draws the same problems with
    and without it -- and over the fixed-seed slice every table meets ``kh_set_nonlinear``'s rules (J in 1..6, every control
    0..C-1 with a term, powers 1..4), every power and both signs occur, more than one base and regime are drawn, and the
    update moves the pulses."""
    import fuzz_parity

    plain, other = np.random.default_rng(FUZZ_SEED), np.random.default_rng(FUZZ_SEED)
    rng_nl = np.random.default_rng([FUZZ_SEED, 0x4e11])
    powers, signs, tags, slots = set(), set(), set(), set()
    for _ in range(FUZZ_CASES):
        a, tag_a, fmt_a = fuzz_parity.draw(plain)
        b, tag_b, fmt_b = fuzz_parity.draw(other)
        assert (a.name, a.K, a.N, a.L, len(a.tlist), fmt_a, tag_a) == (b.name, b.K, b.N, b.L, len(b.tlist), fmt_b, tag_b)
        obj, tag, theta_max = fuzz_parity.draw_nonlinear(rng_nl)
        J, C = len(obj.terms), nc.n_controls(obj.terms)
        assert 1 <= J <= 6 and J == obj.L and {c for c, _ in obj.terms} == set(range(C)) and len(obj.pulses) == C
        assert all(1 <= p <= 4 for _, p in obj.terms) and max(p for _, p in obj.terms) > 1
        powers |= {p for _, p in obj.terms}
        signs |= {float(np.sign(p[np.nonzero(p)[0][0]])) for p in obj.pulses if np.any(p)}
        slots.add(J)
        tags.add(tuple(tag.split()[:2]))
        r = fuzz_parity.nonlinear_inputs(obj)
        assert np.all(np.isfinite(r['opt'])) and np.abs(r['opt'] - np.array(obj.pulses)).max() > 1e-9
    assert powers == {1, 2, 3, 4} and signs == {-1.0, 1.0} and len(slots) >= 3 and len({t[0] for t in tags}) >= 3 and len({t[1] for t in tags}) >= 3
    assert plain.random() == other.random()


@pytest.mark.gpu
def test_fuzz_parity_nonlinear_fixed_seed():
    """A fixed-seed slice of ``tests/fuzz_parity.py --nonlinear``."""
    import fuzz_parity

    done, failures = fuzz_parity.fuzz(FUZZ_SEED, cases=FUZZ_CASES, verbose=True, nonlinear=True)
    assert done == FUZZ_CASES and not failures, failures


# ---------------------------------------------------------------------------
# a caller-set series tolerance and caller-set norm bounds (the three references of tests/test_series_tolerance.py)
# ---------------------------------------------------------------------------
# One tile-form and one generic-form row under the ramp at theta_max 1 (Hermitian operators: the one-term-per-phase kernels
# evaluate the Chebyshev-form table with cap 2, as tests/test_bounded_constrained_axes.py's rows).  The co-state store of
# the update sweep is the exact one, uploaded, so that the update sweep's own series is what is measured.
TOLS, TOL_HOW, TOL_BASES, NORM_FACTOR = (1e-6, 1e-9), ('ramp', 1.0), ('tile_L3', 'tile128'), 3.0
TOL_CASES = [(b, t) for b in TOL_BASES for t in TOLS]
TOL_IDS = ['%s-tol%g' % c for c in TOL_CASES]
EPS_MARGIN = 1.01  # sup |d eps^p / d eps| is taken up to this multiple of the largest |eps| of the guess and the exact update


def coefficient_sup(ref):
    """p_j (EPS_MARGIN max |eps_c(j)|)^(p_j - 1) per slot: |eps'^p - eps^p| <= that x |eps' - eps| while both stay below
    EPS_MARGIN x the largest magnitude of the guess and the exact updated pulse (the bound on the pulse error, asserted
    by the witness to be below that margin for every control, keeps the device's pulse inside)."""
    obj = ref['obj']
    top = np.maximum(np.abs(np.array(obj.pulses)).max(axis=1), np.abs(ref['opt']).max(axis=1)) * EPS_MARGIN
    return np.array([p * top[c] ** (p - 1) for c, p in obj.terms])


def nl_bound(ref, tol):
    """``series_oracle.tolerance_bound`` for the update in eps of a term table, derived from the tolerance, the plan and
    the problem alone.  With delta_i[n] the bound's error of the update sum of slot i, the pulse of control c is off by at
    most  e_c = S_c / lambda_c sum_{i in c} |w_i| delta_i  (w_i = p_i eps_guess^(p_i - 1), the weights of the update), the
    coefficient of slot j in c by at most sup_j e_c (``coefficient_sup``: sup |f'| of the parametrized bound replaced by
    p_j max|eps|^(p_j - 1)), and the generator of objective k by
        dt sum_j h_kj sup_j e_c(j)  =  dt sum_i delta_i S_c(i) / lambda_c(i) |w_i| sum_{j in c(i)} h_kj sup_j
                                    <= dt sum_i h_ki [S_c(i) |w_i| r_i / lambda_c(i)] delta_i,
    r_i = max_k (sum_{j in c(i)} h_kj sup_j) / h_ki: the bound's own recursion on the J-slot problem of the coefficient
    pulses with the shape S_c(i) |w_i| r_i in the place of S_i.  Its 'opt' (per slot: d_i) gives the pulse bound
    e_c = sum_{i in c} d_i / r_i, returned as 'opt' (C rows); the slots' as 'slots'."""
    import series_oracle as so

    obj, prob = ref['obj'], ref['prob']
    view = nc.coefficient_view(obj)
    tab = bca._table(tol, view)
    h = hp.series_bounds(view)
    sup, w = coefficient_sup(ref), np.abs(ref['dcde'])
    own = [[j for j, (cj, _) in enumerate(obj.terms) if cj == c] for c, _ in obj.terms]
    r = np.array([max(sum(h[k, 1 + j] * sup[j] for j in own[i]) / h[k, 1 + i] for k in range(obj.K)) for i in range(obj.L)])
    scaled = copy.copy(view)
    scaled.shapes = [np.asarray(obj.shapes[c]) * w[i] * r[i] for i, (c, _) in enumerate(obj.terms)]
    scaled.lambdas = [ref['lambdas'][c] for c, _ in obj.terms]
    opt_coef = nc.coefficients(obj.terms, ref['opt'])
    theta, nsub_opt, _ = so.plan(view, opt_coef, TOL_HOW[1], tab)
    plans = dict(guess=so.plan(view, view.pulses, TOL_HOW[1], tab)[1], opt=nsub_opt,
                 tol_guess=so.step_errors(view, prob, view.pulses, TOL_HOW[1], tab, tol),
                 tol_opt=so.step_errors(view, prob, opt_coef, TOL_HOW[1], tab, tol, so.WIDEN), theta_opt=theta)
    as_linear = dict(ref, opt=np.array(opt_coef))
    out = so.tolerance_bound(scaled, tol, plans, as_linear, False)
    out['slots'] = out['opt']
    out['opt'] = np.array([sum(out['slots'][i] / r[i] for i, (ci, _) in enumerate(obj.terms) if ci == c)
                           for c in range(nc.n_controls(obj.terms))])
    return out


@functools.lru_cache(maxsize=None)
def tol_reference(base):
    """The exact restatement of a tolerance row with its forward states; ||chi_k|| shrunk by tests/test_series_tolerance.py's
    ``CHI_SHRINK`` until the bound at the larger tolerance is not empty (that module's condition)."""
    import test_series_tolerance as tst

    obj = problem(base, TOL_HOW)
    view = nc.coefficient_view(obj)
    prob = bca._oracle(view)
    with hp.MemoExpm():
        states = ko.forward_propagation(prob, view.pulses, store=True)[1]
        chi_T = bca.boundary_costates(view, prob)
        chi = ko.backward_sweep(prob, chi_T, view.pulses)
        for shrink in tst.CHI_SHRINK:
            norms = tsr.chi_norms(view) * shrink
            ref = restate(obj, prob, chi, norms)
            ref.update(obj=obj, prob=prob, norms=norms, chi_T=chi_T, chi=chi, so_inputs=None, lambdas=np.array(obj.lambdas),
                       coef=np.array(view.pulses), dcde=nc.weights(obj.terms, obj.pulses), states=states, wrong=None)
            if tst.bound_is_not_empty(nl_bound(ref, TOLS[0]), np.abs(ref['opt'] - np.array(obj.pulses)).max()):
                break
    return ref


@functools.lru_cache(maxsize=None)
def tol_series(base, tol, factor=1.0):
    """The series oracle's sweep of a tolerance row (``nc.update_sweep`` inside the ``SeriesOracle`` context: it steps
    through ``ko._step``) at ``tol`` under ``factor`` x the default norm bounds."""
    import series_oracle as so

    ref = tol_reference(base)
    view = nc.coefficient_view(ref['obj'])
    with so.SeriesOracle(ref['prob'], hp.series_bounds(view, factor=factor), bca._table(tol, view), TOL_HOW[1]):
        return restate(ref['obj'], ref['prob'], ref['chi'], ref['norms'], None, ref['lambdas'])


def _beyond(got, ref, tol, slack):
    """The quantities beyond their derived bound (+ ``slack`` for rounding)."""
    bound = nl_bound(ref, tol)
    checks = {'opt': (np.abs(got['opt'] - ref['opt']), bound['opt']),
              'psi_T': (np.linalg.norm(got['psi_T'] - ref['psi_T'], axis=1), bound['upd'][:, -1])}
    return {w: float((d - b).max()) for w, (d, b) in checks.items() if (d - b).max() > slack}


@pytest.mark.parametrize('tid', TOL_IDS)
def test_tolerance_witness(tid):
    """Host only, per (row, tol): no theta sits near a threshold, the two tolerances (and the default) plan different
    series -- other degrees on at least half of the intervals of the objective with the largest theta --, the bound at 1e-6 is not empty
    (tests/test_series_tolerance.py's condition) and keeps the pulse error of every control inside the margin ``EPS_MARGIN`` allows,
    the series oracle stays within the bound of the exact restatement while being more than 100 x the project's rounding
    tolerance away at 1e-6, and three times the norm bounds plan another series at the default tolerance."""
    import series_oracle as so
    import test_series_tolerance as tst

    base, tol = TOL_CASES[TOL_IDS.index(tid)]
    ref = tol_reference(base)
    obj = ref['obj']
    view = nc.coefficient_view(obj)
    tab = bca._table(tol, view)
    for pulses in (view.pulses, nc.coefficients(obj.terms, ref['opt'])):
        theta, nsub, deg = so.plan(view, pulses, TOL_HOW[1], tab)
        assert so.threshold_distance(theta, nsub, TOL_HOW[1], tab) > 1e-9
        k = int(np.argmax(theta.max(axis=1)))
        for other in [t for t in TOLS + (0.0,) if t != tol]:
            theirs = so.plan(view, pulses, TOL_HOW[1], so.at_tolerance(tab, other))[2][k]
            # (where the ramp is at theta <= 1e-3 the smallest degree serves every tolerance: half of the intervals)
            assert np.count_nonzero(deg[k] != theirs) >= 0.5 * len(theirs), (other, deg[k], theirs)
    loose = so.plan(view, view.pulses, TOL_HOW[1], so.at_tolerance(tab, 0.0), hp.series_bounds(view, factor=NORM_FACTOR))
    tight = so.plan(view, view.pulses, TOL_HOW[1], so.at_tolerance(tab, 0.0))
    assert so.threshold_distance(loose[0], loose[1], TOL_HOW[1], so.at_tolerance(tab, 0.0)) > 1e-9
    assert np.any(loose[1] != tight[1]) and so.products(tab, loose[1], loose[2]) > so.products(tab, tight[1], tight[2])
    ser, bound = tol_series(base, tol), nl_bound(ref, tol)
    dev = distances(ser, ref)
    change = np.abs(ref['opt'] - np.array(obj.pulses)).max()
    print('tolerance witness %s: series oracle off by %s; bound upd %.1e pulse %.1e (pulse change %.1e)' % (
        tid, ' '.join('%s %.1e' % kv for kv in dev.items()), bound['upd'].max(), bound['opt'].max(), change))
    if tol == TOLS[0]:
        assert tst.bound_is_not_empty(bound, change) and change > 1e-6
        assert dev['psi_T'] > 100.0 * TOL_RAMP
    assert np.all(bound['opt'].max(axis=1) < (EPS_MARGIN - 1.0) * np.abs(np.array(obj.pulses)).max(axis=1))
    assert not _beyond(ser, ref, tol, 1e-11)


def _tol_run(base, tol=0.0, factor=None):
    import torch

    ref = tol_reference(base)
    view = nc.coefficient_view(ref['obj'])
    op_norms = None if factor is None else hp.series_bounds(view, factor=factor)
    eng = make_engine(base, ref['obj'], TOL_HOW[1], tol=tol, op_norms=op_norms)
    try:
        if factor is not None:
            assert np.allclose(np.array(eng.op_norms).reshape(op_norms.shape), op_norms, rtol=1e-14, atol=0.0)
        got, _, launched = run_nl(eng, ref, False, chi=eng.dev(ref['chi'], torch.complex128))
        return got, eng.stats()['matvecs'], [n for n in launched if '_nl<' in n], eng.kernel
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('tid', TOL_IDS)
def test_tolerance(tid):
    """``tol`` = 1e-6 and 1e-9: the device agrees with the series oracle's restatement of the same plan to rounding (1e-11:
    the ramp's), with the exact restatement within the derived bound (``nl_bound``), runs the same instantiation as at the
    default tolerance and fewer products."""
    base, tol = TOL_CASES[TOL_IDS.index(tid)]
    ref, ser = tol_reference(base), tol_series(base, tol)
    got0, count0, launched0, kernel0 = _tol_run(base)
    got, count, launched, kernel = _tol_run(base, tol)
    sdev, dev, dev0 = distances(got, ser), distances(got, ref), distances(got0, ref)
    print('nonlinear_axes tolerance %s [%s]: products %d (default tolerance %d); from the series oracle %s; from the exact '
          'restatement %s (default: %s); launched: %s' % (tid, kernel, count, count0, ' '.join('%s %.1e' % kv for kv in sdev.items()),
                                                          ' '.join('%s %.1e' % kv for kv in dev.items()),
                                                          ' '.join('%s %.1e' % kv for kv in dev0.items()), ', '.join(launched)))
    assert launched == launched0 == [nl_kernel(base, False)] and kernel == kernel0 == BASES[base].family
    assert count < count0
    assert max(sdev.values()) < TOL_RAMP, sdev
    assert max(dev0.values()) < TOL_RAMP, dev0
    assert not _beyond(got, ref, tol, TOL_RAMP)


@pytest.mark.gpu
@pytest.mark.parametrize('base', TOL_BASES)
def test_loose_norm_bounds(base):
    """Caller-set norm bounds, three times the default ones (``series_bounds(factor=3)``; the engine reports them back): the
    device agrees with the series oracle's restatement of THAT plan and with the exact restatement to 1e-11, on the same
    instantiation, at more products than under the default bounds."""
    ref, ser = tol_reference(base), tol_series(base, 0.0, NORM_FACTOR)
    got0, count0, launched0, kernel0 = _tol_run(base)
    got, count, launched, kernel = _tol_run(base, factor=NORM_FACTOR)
    sdev, dev = distances(got, ser), distances(got, ref)
    print('nonlinear_axes norm bounds %s [%s]: products %d (default bounds %d); from the series oracle %s; from the exact '
          'restatement %s' % (base, kernel, count, count0, ' '.join('%s %.1e' % kv for kv in sdev.items()),
                              ' '.join('%s %.1e' % kv for kv in dev.items())))
    assert launched == launched0 == [nl_kernel(base, False)] and kernel == kernel0
    assert count > count0
    assert max(sdev.values()) < TOL_RAMP and max(dev.values()) < TOL_RAMP, (sdev, dev)
