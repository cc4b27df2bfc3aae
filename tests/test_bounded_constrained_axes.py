"""The parametrized update sweeps and the backward sweeps with a source term on every engine and along every axis the
rest of the suite covers for the other kernel families.

``kh_tile_forward_update_par<RPT, L, SO>`` / ``kh_gen_forward_update_par<MIXED>`` and
``kh_tile_sweep_store_src<1, L>`` / ``kh_gen_sweep_store_src<false>`` are separate compilations that take the
plan of whatever engine they are set on (``theta_max``, the degree table, the coefficient rows, the Hermitian
classification, the update grid).  tests/test_parametrization.py and tests/test_state_constraint.py run them at
theta ~ 0.4 on a uniform grid, on tile, ``tile128`` and one CSR engine.  This module runs them

1. on every other engine family that accepts the features (``ENGINE_PAR``, ``ENGINE_SRC``; the refusals with their codes),
2. along the axes of the cross-cutting modules: the series' regimes (``helpers.REGIMES``: sub-steps, degree changes, the
   reload of the coefficient rows), the ends of the interval pipeline (``helpers.grid_ends``: 1, 2, 3 intervals, the
   64-point edges, 257 time points), a caller-set series tolerance (the three references of
   tests/test_series_tolerance.py), an absent control, controls that are not self-adjoint, one engine whose inputs
   change in place, and the graph replay of the per-interval form,
3. on a fixed-seed slice of ``tests/fuzz_parity.py --bounded-constrained``.

Yardsticks: ``parametrization_cases.update_sweep`` (the oracle's update sweep restated with the update in u) and
``constraint_cases.backward_sweep`` (the oracle's backward sweep with the trapezoid source), both on the oracle's own exact
step.  The kinds are chosen AFTER the regime transform, from the transformed guess (``choose_kinds``): ``TANH`` with bounds
+-1.25 max|guess| on a control that changes sign, ``TANHSQ`` with eps_max = 1.25 max on one that is >= 0 everywhere, and the
last of two or more controls stays ``LINEAR`` or unparametrized.

Every (row, axis) pair has a host-only witness over the very table the GPU test runs (the regime is entered under the
guess and under f(u_new), the inverse is finite, f' != 0 on 90 % of the intervals, the update moves the pulses; filling an
absent entry or taking H_l for H_l^dagger moves every compared quantity by more than 1e-6), and
``test_theta_from_u_would_plan_another_series`` shows that a kernel forming theta from u_new instead of f(u_new) would
plan another series.

Tolerances are the project's: 1e-12 against the restatements in Hilbert space, 1e-11 in Liouville
space; pulses, u and g_a relative to max(1, largest reference magnitude); bit for bit where a docstring says so.
"""
import collections
import copy
import warnings

import numpy as np
import pytest

import constraint_cases as cc
import helpers as hp
import parametrization_cases as pc
import test_absent_controls as tac
import test_series_regimes as tsr
from krotov_amd import configs
from oracle import krotov_oracle as ko

TOL_HILBERT, TOL_LIOUVILLE = 1e-12, 1e-11
LAMBDA_B = -1.5
GEN_PAR, GEN_PAR_MIXED = 'kh_gen_forward_update_par<false>', 'kh_gen_forward_update_par<true>'
GEN_SRC = 'kh_gen_sweep_store_src<false>'
REGIME_INTERVALS = 33  # three exact zeros of a pulse ramp are < 10 % of the intervals
ENGINE_INTERVALS = 5   # the engine rows: helpers.grid_ends on five intervals (non-uniform grid, one sub-step)


def TILE_PAR(rpt, L, so):
    return 'kh_tile_forward_update_par<%d, %d, %s>' % (rpt, L, 'true' if so else 'false')


def TILE_SRC(L):
    return 'kh_tile_sweep_store_src<1, %d>' % L


# ---------------------------------------------------------------------------
# base cases: the smallest one of each engine family in the tables of tests/test_series_regimes.py, tests/test_grid_ends.py
# and tests/test_state_constraint.py; build(nt)
# ---------------------------------------------------------------------------
Base = collections.namedtuple('Base', 'build fmt family theta_max env par src')


def _c5(**kw):
    return lambda nt: configs.config_c5(nt=nt, **kw)


_ENS = {'KH_ENS': '1', 'KH_ENS_NCG': '1'}
BASES = {
    # register-tile engines: the parametrized tile form <rows per thread, L, second order>, the source tile form <1, L>
    'quad': Base(_c5(K=2, N=4), 'dense', 'mini4/wave', 1.0, {}, (1, 1), TILE_SRC(1)),
    'mini16': Base(_c5(K=6, N=16), 'dense', 'mini16/wave', 1.0, {}, (1, 1), TILE_SRC(1)),
    'q2': Base(_c5(K=5, N=33), 'dense', 'tile64q2/512', 1.0, {}, (1, 1), TILE_SRC(1)),
    'tile_L2': Base(_c5(K=4, N=64, L=2, distinct=True), 'dense', 'tile64/512', 1.0, {}, (1, 2), TILE_SRC(2)),
    'tile_L3': Base(_c5(K=5, N=12, L=3, distinct=True), 'dense', 'tile64/512', 1.0, {}, (1, 3), TILE_SRC(3)),
    'tile_L4': Base(_c5(K=4, N=24, L=4, distinct=True), 'dense', 'tile64/512', 1.0, {}, (1, 4), TILE_SRC(4)),
    'tile256': Base(_c5(K=300, N=16, distinct=True), 'dense', 'tile64/256', 1.0, {}, (2, 1), TILE_SRC(1)),
    'tile256_noq2': Base(_c5(K=300, N=16, distinct=True), 'dense', 'tile64/256', 1.0, {'KH_Q2_STORE': '0'}, (2, 1), GEN_SRC),
    # every other engine: the generic forms
    'tile128': Base(_c5(K=3, N=80, L=2), 'dense', 'tile128/512', 1.0, {}, GEN_PAR, GEN_SRC),
    'coop': Base(lambda nt: configs.config_shared(K=8, N=96, nt=nt, L=1), 'dense', 'coop16/mfma', 4.0, {}, GEN_PAR, GEN_SRC),
    'coop_L2': Base(lambda nt: configs.config_shared(K=8, N=96, nt=nt, L=2), 'dense', 'coop16/mfma', 4.0, {}, GEN_PAR, GEN_SRC),
    'coop_c4_d9': Base(lambda nt: configs.config_c4(d=9, nt=nt, n_logical=2), 'dense', 'coop16/mfma', 4.0, {}, GEN_PAR, GEN_SRC),
    # (the plain sweeps of the ens and stream engines are the q2 kernel's -- ``kind_store`` -- so their source sweep is the
    # register-tile form, as on the tile256 engine: DESIGN 3.11)
    'ens': Base(_c5(K=40, N=64), 'dense', 'ens64/mfma', 1.0, _ENS, GEN_PAR, TILE_SRC(1)),
    'stream': Base(_c5(K=600, N=8, distinct=True), 'dense', 'tile64/stream', 1.0, {}, GEN_PAR, TILE_SRC(1)),
    'tilex': Base(_c5(K=5, N=20, L=6, distinct=True), 'dense', 'tile64x/512', 1.0, {}, GEN_PAR, GEN_SRC),
    'ell': Base(lambda nt: tsr._coherent(configs.config_sparse_lindblad(d=12, nt=nt), 12), 'csr', 'ell/csr', 4.0, {}, GEN_PAR,
                GEN_SRC),
    'ellstream': Base(_c5(K=6, N=16), 'csr', 'ellstream/csr', 4.0, {'KH_KERNEL': 'ellstream'}, GEN_PAR, GEN_SRC),
    'gencsr': Base(_c5(K=5, N=33), 'csr', 'generic/csr', 1.0, {}, GEN_PAR, GEN_SRC),
    # (forced at small N, as tests/test_sparse_large.py does: the generic kernels' vectors fit, so it takes both features)
    'ellglobal': Base(_c5(K=5, N=12, L=3, distinct=True), 'csr', 'ellglobal/csr', 4.0, {'KH_KERNEL': 'ellglobal'}, GEN_PAR, GEN_SRC),
    'mixed': Base(lambda nt: configs.config_mixed('dims', nt=nt), 'mixed', 'generic/mixed', 1.0, {}, GEN_PAR_MIXED, None),
}


def par_kernel(base, so):
    want = BASES[base].par
    return TILE_PAR(want[0], want[1], so) if isinstance(want, tuple) else want


# ---------------------------------------------------------------------------
# variants of a base case: an absent control, a control that is not self-adjoint
# ---------------------------------------------------------------------------
def _absent(spec):
    """Objective 0 and the last objective lack the last control."""
    return tac._drop(spec, [(0, spec.L - 1), (spec.K - 1, spec.L - 1)])


def _lindblad5(nt):
    return configs.config_sparse_lindblad(d=5, nt=nt, K=3)


def _variant_spec(base, variant, nt):
    import test_nonselfadjoint_controls as tnc

    if variant == 'liouv':  # (the d = 5 Lindbladian, dense: N = 25 on the q2 engine)
        return tnc._liouv(_lindblad5(nt))
    spec = BASES[base].build(nt)
    if variant is None:
        return spec
    if variant == 'absent':
        return _absent(spec)
    if variant in ('lower', 'anti'):
        return tnc._nsa(spec, variant)
    raise KeyError(variant)


# ---------------------------------------------------------------------------
# problems: a base case (or its variant) under an axis
#   how = ('ends', I)            helpers.grid_ends on I intervals at the engine's own theta_max
#         (regime, theta_max)    helpers.REGIMES[regime] on REGIME_INTERVALS intervals
# ---------------------------------------------------------------------------
_problems = {}


def engine_theta(base, how):
    return BASES[base].theta_max if how[0] == 'ends' else how[1]


def problem(base, how, variant=None):
    key = (base.replace('_noq2', ''), how, variant)
    if key not in _problems:
        b = BASES[base]
        if how[0] == 'ends':
            obj = hp.grid_ends(hp.explicit(_variant_spec(base, variant, how[1] + 1), b.fmt), b.theta_max)
        else:
            obj = hp.REGIMES[how[0]](hp.explicit(_variant_spec(base, variant, REGIME_INTERVALS + 1), b.fmt), how[1])
        _problems[key] = obj
    return _problems[key]


def _oracle(obj):
    if obj.fmt == 'mixed' and any(op is None for row in obj.Hc for op in row):
        zero = copy.copy(obj)  # (the restatement pads arrays: the absent control goes in as the zero operator)
        zero.Hc = [[np.zeros_like(obj.H0[k]) if op is None else op for op in row] for k, row in enumerate(obj.Hc)]
        return hp.regime_oracle(zero)
    return hp.regime_oracle(obj)


def liouville(obj):
    return bool(np.any(obj.is_super))


def tolerance(obj):
    return TOL_LIOUVILLE if liouville(obj) else TOL_HILBERT


def choose_kinds(pulses, b_shift=0.0):
    """The kinds of a (transformed) guess: module docstring.  ``b_shift``: the TANH bounds moved by that fraction of
    max|guess| (b != 0: the row of the theta witness)."""
    L, out = len(pulses), []
    for l, p in enumerate(pulses):
        p = np.asarray(p, dtype=np.float64)
        m = float(np.abs(p).max())
        if L >= 2 and l == L - 1:
            out.append(None if L % 2 else ('linear', 0.7, 0.3 * m))
        elif p.min() >= 0.0 and b_shift == 0.0:
            out.append(('tanhsq', 1.25 * m))
        else:
            out.append(('tanh', (b_shift - 1.25) * m, (b_shift + 1.25) * m))
    return out


def boundary_costates(obj, prob):
    """chi_k(T) of tests/test_series_regimes.py (``oracle_sweeps``): the targets plus a random complex part, normalised."""
    rng = np.random.default_rng(17)
    chi_T = prob.target + 0.5 * (
        rng.standard_normal(prob.target.shape) + 1j * rng.standard_normal(prob.target.shape)) / np.sqrt(prob.N)
    if obj.fmt == 'mixed':
        for k, n in enumerate(obj.dims):
            chi_T[k, n:] = 0.0
    return chi_T / np.linalg.norm(chi_T, axis=1)[:, None]


def second_order_inputs(obj, prob, seed=5):
    rng = np.random.default_rng(seed)
    older = [p * (1.0 + 0.2 * rng.standard_normal(p.shape)) for p in obj.pulses]
    prev = ko.forward_propagation(prob, older, store=True)[1]
    # (many objectives add up: as tests/test_absent_controls.py scales it)
    sigma = -(1.0 + rng.random(len(obj.pulses[0]))) * min(1.0, 8.0 / obj.K) * (1e-3 if getattr(obj, 'name', '').startswith('shared') else 1.0)
    return prev, sigma


def lambdas_in_u(lambdas, dfdu):
    """lambda_a of the update in u.  The update moves the pulse by about f'(u)^2 S / lambda Im D (``LINEAR``: exactly, the
    unparametrized update with lambda / a^2), and the transformed guesses span |eps| up to 1e3 with f' of that size: with
    the base case's lambda_a the first interval would throw every bounded pulse onto its bound, where f' = 0 and theta no
    longer follows the regime.  lambda_l max(1, max_n f'_l(u_guess[n])^2) keeps the pulse change what the regime helpers
    arranged for the unparametrized update."""
    return [lam * max(1.0, float(np.abs(c).max()) ** 2) for lam, c in zip(lambdas, dfdu)]


def restate_par(obj, prob, chi, norms, kinds, so_inputs=None, u_guess=None, shapes=None, lambdas=None):
    """``pc.update_sweep`` as a dict (``lambdas``: default ``lambdas_in_u`` of the problem's)."""
    u_guess = [pc.inverse(k, p) for k, p in zip(kinds, obj.pulses)] if u_guess is None else u_guess
    dfdu = [pc.dfdu(k, u) for k, u in zip(kinds, u_guess)]
    lambdas = lambdas_in_u(obj.lambdas, dfdu) if lambdas is None else lambdas
    kw = {} if so_inputs is None else dict(sigma_vals=so_inputs[1], fw_prev=so_inputs[0], store=True)
    out = pc.update_sweep(prob, chi, norms, u_guess, kinds, obj.shapes if shapes is None else shapes, lambdas, **kw)
    ref = dict(opt=np.array(out[0]), u=np.array(out[1]), psi_T=out[2], g_a=np.array(out[3]), u_guess=np.array(u_guess),
               dfdu=np.array(dfdu), lambdas=np.array(lambdas))
    if so_inputs is not None:
        ref['store'] = out[4]
    return ref


_par_refs = {}


def par_reference(base, how, so, variant=None, b_shift=0.0):
    """The restated parametrized update sweep of a problem (computed once and shared; nobody writes to it)."""
    key = (base.replace('_noq2', ''), how, so, variant, b_shift)
    if key not in _par_refs:
        _par_refs[key] = build_par_reference(problem(base, how, variant), so, variant == 'liouv', b_shift)
    return _par_refs[key]


def build_par_reference(obj, so, liouv=False, b_shift=0.0, norms_factor=1.0, seed=5):
    prob = _oracle(obj)
    norms = tsr.chi_norms(obj) * norms_factor
    if liouv:
        # (that rule's 0.02 is for the transmon Liouvillians, ||L_1|| ~ 1e2; here ||L_1|| ~ 1 and the dissipator in the
        # control is weak: ||chi|| = 1.2 lets a wrong adjoint move g_a, the smallest of the compared quantities, by > 1e-6)
        norms = np.full(obj.K, 1.2)
    chi_T = boundary_costates(obj, prob)
    kinds = choose_kinds(obj.pulses, b_shift)
    with hp.MemoExpm():
        chi = ko.backward_sweep(prob, chi_T, obj.pulses)
        so_inputs = second_order_inputs(obj, prob, seed) if so else None
        ref = restate_par(obj, prob, chi, norms, kinds, so_inputs)
    assert np.all(np.isfinite(ref['u_guess'])) and np.all(np.isfinite(ref['opt']))
    ref.update(obj=obj, prob=prob, norms=norms, chi_T=chi_T, chi=chi, kinds=kinds, so_inputs=so_inputs)
    return ref


_src_refs = {}


def source_inputs(obj, prob, seed=0):
    """(W, norms): W = -(lambda_b / T) s_b(t) D phi(t) on the forward states of a "previous iteration" (the guess pulses
    x (1 +- 10 %)), D random Hermitian, s_b = 0.5 + t / T; ||chi_k(T)|| in 0.2 ... 0.9 (never 1)."""
    rng = np.random.default_rng(prob.N + len(prob.tlist) + seed)
    older = [p * (1.0 + 0.1 * rng.standard_normal(np.shape(p))) for p in obj.pulses]
    states = ko.forward_propagation(prob, older, store=True)[1]
    D = cc.random_hermitian(prob.N, 31 + seed, 1.0)
    t0, t1 = prob.tlist[0], prob.tlist[-1]
    W = cc.source(D, cc.factors(LAMBDA_B * (1.0 + seed), prob.tlist, lambda t: 0.5 + (t - t0) / (t1 - t0)), states)
    return W, 0.2 + 0.7 * rng.random(prob.K)


def src_reference(base, how, variant=None):
    """The restated backward sweep with a source of a problem (computed once and shared)."""
    key = (base.replace('_noq2', ''), how, variant)
    if key not in _src_refs:
        _src_refs[key] = build_src_reference(problem(base, how, variant))
    return _src_refs[key]


def build_src_reference(obj, seed=0):
    prob = _oracle(obj)
    chi_T = boundary_costates(obj, prob)
    with hp.MemoExpm():
        W, norms = source_inputs(obj, prob, seed)
        chi = cc.backward_sweep(prob, chi_T, obj.pulses, W, norms)
        plain = ko.backward_sweep(prob, chi_T, obj.pulses)
    return dict(obj=obj, prob=prob, chi_T=chi_T, W=W, norms=norms, chi=chi, plain=plain)


# ---------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'id feature base how so variant mode')
CASES = collections.OrderedDict()


def add(group, feature, base, how, so=False, variant=None, mode='whole'):
    cid = '%s-%s-%s-%s%s%s%s' % (group, feature, base, '%s%s' % (how[0], ('%g' % how[1]).replace('.', 'p')),
                                 '-so' if so else '', '-' + variant if variant else '', '-' + mode if mode != 'whole' else '')
    assert cid not in CASES, cid
    CASES[cid] = Case(cid, feature, base, how, so, variant, mode)


ENGINE = ('ends', ENGINE_INTERVALS)
# 1. engine rows: first order and second order on every family the existing modules do not launch the features on
ENGINE_PAR = ('quad', 'tilex', 'coop', 'coop_L2', 'coop_c4_d9', 'ens', 'stream', 'ell', 'ellstream', 'gencsr', 'ellglobal')
ENGINE_SRC = ('ens', 'stream', 'tilex', 'ellstream', 'tile256_noq2', 'ellglobal')
for _b in ENGINE_PAR:
    for _so in (False, True):
        add('engine', 'par', _b, ENGINE, so=_so)
for _b in ENGINE_SRC:
    add('engine', 'src', _b, ENGINE)

# 2. axes: one row per distinct instantiation
AXES_PAR_TILE = ('q2', 'mini16', 'tile_L2', 'tile_L3', 'tile_L4', 'tile256')
AXES_PAR_GEN = ('tile128', 'coop', 'gencsr', 'mixed')
AXES_SRC = ('q2', 'mini16', 'quad', 'tile256', 'tile_L2', 'tile_L3', 'tile_L4', 'tile128', 'coop', 'gencsr')
THREE = ('ramp', 'pulse_ramp', 'tiny')


def _thetas(base):
    own = BASES[base].theta_max
    return (own,) if own == 1.0 else (own, 1.0)


# regimes.  Parametrized: every instantiation under the three regimes (the tile forms first and second order -- ten
# instantiations -- the generic ones first order, and second order under the ramp); at the engine's own theta_max and at 1
for _b in AXES_PAR_TILE:
    for _so in (False, True):
        for _r in THREE:
            add('regime', 'par', _b, (_r, 1.0), so=_so)
for _b in AXES_PAR_GEN:
    for _t in _thetas(_b):
        for _r in THREE:
            add('regime', 'par', _b, (_r, _t))
    add('regime', 'par', _b, ('ramp', BASES[_b].theta_max), so=True)
# source: the two-terms-per-phase engines hand their plan to a one-term-per-phase kernel -- the ramp on each of them; the
# other rows under the three regimes
for _b in AXES_SRC:
    for _t in _thetas(_b):
        for _r in (('ramp',) if _b in ('q2', 'mini16', 'quad', 'tile256') else THREE):
            add('regime', 'src', _b, (_r, _t))

# ends
for _b in AXES_PAR_TILE + AXES_PAR_GEN:
    for _I in (1, 2, 3):
        add('ends', 'par', _b, ('ends', _I))
        if _b != 'mini16':  # (its instantiations are the q2 row's)
            add('ends', 'par', _b, ('ends', _I), so=True)
for _I in (64, 65, 256):  # (first order: the adjoint-side store's 64- and 256-point tiles, the resident path)
    add('ends', 'par', 'tile128', ('ends', _I))
for _b in AXES_SRC:
    for _I in (1, 2, 3, 4, 65):
        add('ends', 'src', _b, ('ends', _I))
add('ends', 'src', 'tile128', ('ends', 256))

# an absent control (objective 0 and the last objective lack the last control), controls that are not self-adjoint
for _b in ('tile128', 'mixed', 'q2', 'tile_L2', 'tile_L4'):
    add('absent', 'par', _b, ENGINE, variant='absent')
    if _b != 'mixed':
        add('absent', 'src', _b, ENGINE, variant='absent')
for _b, _v in (('tile_L2', 'lower'), ('tile128', 'anti'), ('q2', 'liouv')):
    add('nsa', 'par', _b, ENGINE, variant=_v)
    add('nsa', 'src', _b, ENGINE, variant=_v)

CASE_IDS = list(CASES)


def reference(c):
    return par_reference(c.base, c.how, c.so, c.variant) if c.feature == 'par' else src_reference(c.base, c.how, c.variant)


def expected_kernel(c):
    if c.variant == 'liouv':  # (N = 25, one control)
        return TILE_PAR(1, 1, c.so) if c.feature == 'par' else TILE_SRC(1)
    return par_kernel(c.base, c.so) if c.feature == 'par' else BASES[c.base].src


# ---------------------------------------------------------------------------
# host
# ---------------------------------------------------------------------------
def test_tables_are_what_the_docstring_says():
    from krotov_amd import _lib

    names = _lib.kernel_instantiations()
    par = {expected_kernel(c) for c in CASES.values() if c.feature == 'par' and c.id.startswith('regime')}
    assert par == {n for n in names if '_par<' in n}  # ten tile forms and two generic ones, each under the regimes
    src = {expected_kernel(c) for c in CASES.values() if c.feature == 'src' and c.id.startswith('regime')}
    assert src == {n for n in names if '_src<' in n}
    for feature, rows in (('par', ENGINE_PAR), ('src', ENGINE_SRC)):
        assert {BASES[b].family for b in rows} >= {'ens64/mfma', 'tile64/stream', 'tile64x/512', 'ellstream/csr'}
    assert {BASES[b].family for b in ENGINE_PAR} >= {'mini4/wave', 'coop16/mfma', 'ell/csr', 'generic/csr'}
    for c in CASES.values():
        if c.how[0] != 'ends':
            assert c.how[1] in (1.0, BASES[c.base].theta_max)
        assert len(hp.regime_dt(problem(c.base, c.how, c.variant))) <= 65 or c.base == 'tile128'
        assert problem(c.base, c.how, c.variant).N <= (144 if c.base == 'ell' else 100)  # (the d = 12 Lindbladian)


_degree_tables = {}


def _tables(obj, theta_max, regime):
    cap = theta_max if theta_max > 2.0 else 2.0
    key = (cap, 3e-3 * (1e-7 if regime == 'tiny' else 1.0))
    if key not in _degree_tables:
        _degree_tables[key] = hp.series_degree_tables(*key)
    return _degree_tables[key]


@pytest.mark.parametrize('cid', CASE_IDS)
def test_witness(cid):
    """Host only, over the very table the GPU test runs.  Regime rows: the row enters its regime under the guess and
    (parametrized) under the restatement's updated pulses f(u_new).  Ends rows: the input conditions of
    ``helpers.grid_ends``.  Parametrized rows: the inverse is finite everywhere, f' != 0 on at least 90 % of the intervals
    of every control, the update moves the pulses by more than 1e-6.  Source rows: the source is no rounding matter.
    Absent / non-self-adjoint rows: filling the missing entry / taking H_l for H_l^dagger moves every compared quantity by
    more than 1e-6."""
    c = CASES[cid]
    obj = problem(c.base, c.how, c.variant)
    ref = reference(c)
    I = len(hp.regime_dt(obj))
    assert I == (c.how[1] if c.how[0] == 'ends' else REGIME_INTERVALS) and len(obj.tlist) == I + 1
    under = [np.array(obj.pulses)] + ([ref['opt']] if c.feature == 'par' else [])
    if c.how[0] == 'ends':
        hp.grid_ends_witness(obj, BASES[c.base].theta_max)
    else:
        for pulses in under:
            hp.regime_witness(obj, c.how[0], c.how[1], pulses, _tables(obj, c.how[1], c.how[0]))
    if c.feature == 'par':
        assert np.all(np.isfinite(ref['u_guess'])) and np.all(np.isfinite(ref['dfdu']))
        assert np.all(np.count_nonzero(ref['dfdu'], axis=1) >= 0.9 * I), np.count_nonzero(ref['dfdu'], axis=1)
        assert any(k is not None and k[0] in ('tanh', 'tanhsq') for k in ref['kinds'])
        assert len(ref['kinds']) < 2 or ref['kinds'][-1] is None or ref['kinds'][-1][0] == 'linear'
        move = np.abs(ref['opt'] - np.array(obj.pulses)).max()
        print('witness %s: kinds %s, pulse change %.1e' % (cid, [k and k[0] for k in ref['kinds']], move))
        assert move > 1e-6
        for l, k in enumerate(ref['kinds']):  # the bounded pulses stay inside their bounds
            if k is not None and k[0] == 'tanh':
                assert ref['opt'][l].min() > k[1] and ref['opt'][l].max() < k[2]
    else:
        moved = np.abs(ref['chi'] - ref['plain']).max()
        print('witness %s: the source moves the co-states by %.1e' % (cid, moved))
        assert moved > 1e-3 and np.all(np.abs(ref['norms'] - 1.0) > 1e-3)
    if c.variant is not None:
        for tag, wrong in _wrong_results(c, obj, ref).items():
            for what, d in wrong.items():
                print('witness %s (%s): %s moves by %.2e' % (cid, tag, what, d))
                assert d > 1e-6, (cid, tag, what, d)


def _distance(x, y):
    return float(np.abs(np.array(x) - np.array(y)).max())


def _wrong_results(c, obj, ref):
    """{mistake: {quantity: distance from the right result}} of a variant row."""
    import test_nonselfadjoint_controls as tnc

    out = {}
    if c.variant == 'absent':
        wrong_probs = {'filled': _oracle(tac._filled(obj))}
    else:  # the backward generator built from H_l for H_l^dagger
        wrong_probs = {'H_l for its adjoint': tnc._with_adjoints(ref['prob'], lambda o: o)}
    with hp.MemoExpm():
        for tag, prob in wrong_probs.items():
            if c.feature == 'src':
                out[tag] = dict(chi=_distance(cc.backward_sweep(prob, ref['chi_T'], obj.pulses, ref['W'], ref['norms']), ref['chi']))
                continue
            chi = ko.backward_sweep(prob, ref['chi_T'], obj.pulses)
            # (the update sweep of a wrong adjoint runs on the right forward operators and the wrong co-state store)
            fw = prob if c.variant == 'absent' else ref['prob']
            got = restate_par(obj, fw, chi, ref['norms'], ref['kinds'], ref['so_inputs'])
            out[tag] = {what: _distance(got[what], ref[what]) for what in ('opt', 'u', 'psi_T', 'g_a')}
            out[tag]['chi'] = _distance(chi, ref['chi'])
        if c.feature == 'par' and c.variant != 'absent':  # the update sums with H_l chi for H_l^dagger chi
            with tnc._Mu(lambda o: o.conj().T):
                got = restate_par(obj, ref['prob'], ref['chi'], ref['norms'], ref['kinds'], ref['so_inputs'])
            out['mu: H_l chi'] = {what: _distance(got[what], ref[what]) for what in ('opt', 'u', 'psi_T', 'g_a')}
    return out


def test_theta_from_u_would_plan_another_series():
    """A kernel that formed theta from u_new instead of f(u_new): on a ``TANH`` row whose bounds are not symmetric
    (b != 0, so |f(u)| > |u| where u is small) the restated planner picks another degree or sub-step count on at least one
    interval -- such a kernel would run another series there, and on the rows of this module the pulses are large against
    u (a pulse ramp spans |eps| up to 1e3), where the truncated series is off by far more than the tolerance."""
    for base, regime in (('q2', 'pulse_ramp'), ('tile_L2', 'ramp')):
        how = (regime, 1.0)
        ref = par_reference(base, how, False, b_shift=0.5)
        obj = ref['obj']
        tanh = [l for l, k in enumerate(ref['kinds']) if k is not None and k[0] == 'tanh']
        assert tanh and all(pc._ab(ref['kinds'][l])[1] != 0.0 for l in tanh)
        assert any(np.any(np.abs(ref['opt'][l]) > np.abs(ref['u'][l])) for l in tanh)
        tab = _tables(obj, 1.0, regime)['taylor']
        differs = 0
        for k in range(obj.K):
            right = hp.series_plan(hp.theta_sequence(obj, ref['opt'])[k], 1.0, tab)
            wrong = hp.series_plan(hp.theta_sequence(obj, ref['u'])[k], 1.0, tab)
            differs = max(differs, int(np.count_nonzero((right[0] != wrong[0]) | (right[1] != wrong[1]))))
        print('%s %s: the plan from u_new differs on %d of %d intervals' % (base, regime, differs, len(ref['opt'][0])))
        assert differs >= 1


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _nans(shape, dtype, device):
    import torch

    fill = complex(float('nan'), float('nan')) if dtype == torch.complex128 else float('nan')
    return torch.full(tuple(shape), fill, dtype=dtype, device=device)


def make_engine(base, obj, theta_max, family=True, **kw):
    eng = hp.regime_engine(obj, theta_max, **kw)
    assert eng.kernel, 'the engine names its kernel family'
    if family:
        assert eng.kernel == BASES[base].family, eng.kernel
    return eng


def device_kinds(kinds, pulses):
    """(kind, a, b) of the product's own classes (``PulseParameters``), whose u agrees with the restatement's inverse."""
    from krotov_amd.parametrization import PulseParameters

    par = PulseParameters([pc.to_product(k) for k in kinds], [np.array(p) for p in pulses])
    u = np.array([pc.inverse(k, p) for k, p in zip(kinds, pulses)])
    assert np.abs(np.array(par.u) - u).max() <= 1e-14 * max(1.0, np.abs(u).max())
    return par.device_kinds


def generic_grid(eng):
    """The clamp rule of ``update_generic<true>``: min(the engine's update grid, what the exchange takes) -- for every
    engine of this module min(K, #CUs, 256)."""
    return min(eng.K, eng._num_cus(), 256)


def run_par(eng, ref, so, mode='whole', chi=None, tensors=None):
    """One parametrized update sweep of ``ref`` on ``eng`` into NaN-filled outputs; returns (outputs on the host,
    deviations from the restatement, launched instantiations)."""
    import torch

    from krotov_amd import _lib

    obj, prob = ref['obj'], ref['prob']
    c128, f64, dv = torch.complex128, torch.float64, eng.device
    pulses, S, lam = np.array(obj.pulses), np.array(obj.shapes), ref['lambdas']
    L, I = pulses.shape
    dev = {}
    if chi is None:
        chi = eng.backward(ref['chi_T'], pulses, out=_nans((obj.K, I + 1, prob.N), c128, dv))
        dev['chi'] = _distance(chi.cpu().numpy(), ref['chi'])
    store = None
    if so:
        store = _nans((obj.K, I + 1, prob.N), c128, dv)
        eng.set_second_order(ref['so_inputs'][0], store, ref['so_inputs'][1])
    kind, a, b = device_kinds(ref['kinds'], obj.pulses)
    u_opt = _nans((L, I), f64, dv)
    eng.set_parametrization(kind, a, b, ref['u_guess'], ref['dfdu'], u_opt)
    _lib.forget_launched_kernels()
    if mode == 'whole':
        opt, psi_T, g_a = eng.forward_update(chi, ref['norms'], prob.init, pulses, S, lam,
                                             out=(_nans((L, I), f64, dv), _nans((obj.K, prob.N), c128, dv), _nans((L,), f64, dv)))
    else:
        # (the per-interval form takes no output tensors: it returns copies of buffers the engine keeps -- NaN-filled here
        # from its second call on; at the first call they are the engine's fresh allocations.  u_opt is NaN-filled always)
        for name in ('opt', 'psi_T', 'g_a'):
            if getattr(eng, '_sh', None) is not None:
                eng._sh[name].fill_(float('nan'))
        opt, psi_T, g_a = eng.forward_update_sharded(chi, ref['norms'], prob.init, pulses, S, lam, lambda x: None,
                                                     graph_chunk=int(mode))
    eng.check()
    launched = sorted(_lib.kernel_instantiations(launched_only=True))
    assert eng.stats()['intervals'] == I
    out = dict(opt=opt.cpu().numpy(), u=u_opt.cpu().numpy(), psi_T=psi_T.cpu().numpy(), g_a=g_a.cpu().numpy())
    if so:
        out['store'] = store.cpu().numpy()
        assert np.array_equal(out['store'][:, 0], np.asarray(prob.init, dtype=np.complex128)), 'slice 0 is the initial states'
    for what in out:
        scale = max(1.0, np.abs(ref[what]).max()) if what in ('opt', 'u', 'g_a') else 1.0
        dev[what] = _distance(out[what], ref[what]) / scale
    # the pulses the sweep propagated with are f(u) of the u it stored (tests/test_parametrization.py's check and its bound:
    # 4 ulp of max(1, |opt|) for the roundings of a, b, the product-sum and a tanh that differs between libraries by an ulp)
    for l, k in enumerate(ref['kinds']):
        assert np.abs(pc.f(k, out['u'][l]) - out['opt'][l]).max() <= 4e-15 * max(1.0, np.abs(out['opt'][l]).max())
    return out, dev, launched


def run_src(eng, ref, W=None, norms=None):
    import torch

    from krotov_amd import _lib

    obj, prob = ref['obj'], ref['prob']
    I = len(obj.pulses[0])
    _lib.forget_launched_kernels()
    got = eng.backward_source(ref['chi_T'], np.array(obj.pulses), ref['W'] if W is None else W,
                              ref['norms'] if norms is None else norms,
                              out=_nans((obj.K, I + 1, prob.N), torch.complex128, eng.device))
    eng.check()
    launched = sorted(_lib.kernel_instantiations(launched_only=True))
    assert eng.stats()['intervals'] == I
    got = got.cpu().numpy()
    assert np.array_equal(got[:, I], ref['chi_T']), 'chi[:, nt - 1] is chi_T'
    return got, launched


DEVIATIONS = {}  # row group: the largest deviation (printed for DESIGN.md)


def _record(c, worst):
    group = '%s/%s' % (c.id.split('-')[0], c.feature)
    DEVIATIONS[group] = max(DEVIATIONS.get(group, 0.0), worst) if np.isfinite(worst) else float('nan')
    return group, DEVIATIONS[group]


@pytest.mark.gpu
@pytest.mark.parametrize('cid', CASE_IDS)
def test_matrix(cid, monkeypatch):
    """One parametrized update sweep (u_opt, opt, psi(T), g_a, second order: the stored trajectory, slice 0 bit for bit
    the initial states) against ``pc.update_sweep``, or one backward sweep with a source and norms != 1 (the last slice
    bit for bit chi(T)) against ``cc.backward_sweep``; every output NaN-filled before the sweep, the kernel family and the
    launched instantiation asserted, ``stats()['intervals']`` the grid's, and -- on the generic parametrized form -- the
    grid that ran against the clamp rule of ``update_generic<true>``."""
    c = CASES[cid]
    b = BASES[c.base]
    for name, value in b.env.items():
        monkeypatch.setenv(name, value)
    ref = reference(c)
    obj = ref['obj']
    tol = tolerance(obj)
    want = expected_kernel(c)
    eng = make_engine(c.base, obj, engine_theta(c.base, c.how), family=c.variant in (None, 'absent'))
    try:
        if c.feature == 'par':
            _, dev, launched = run_par(eng, ref, c.so, c.mode)
            update = [n for n in launched if 'forward_update' in n]
            assert update == [want], (cid, want, launched)
            if want in (GEN_PAR, GEN_PAR_MIXED):
                assert eng.stats()['workgroups'] == generic_grid(eng), (eng.stats(), generic_grid(eng))
        else:
            got, launched = run_src(eng, ref)
            assert launched == [want], (cid, want, launched)
            dev = dict(chi=_distance(got, ref['chi']) / max(1.0, np.abs(ref['chi']).max()))
        kernel = eng.kernel
    finally:
        eng.close()
    worst = max(dev.values())
    group, so_far = _record(c, worst)
    print('bounded_constrained %s [%s]: %s; %s so far %.1e; launched: %s' % (
        cid, kernel, ' '.join('%s %.1e' % kv for kv in sorted(dev.items())), group, so_far, ', '.join(launched)))
    assert np.isfinite(worst) and worst < tol, dev


# ---------------------------------------------------------------------------
# GPU: refusals, with the error code and no sweep launched
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.no_oracle
def test_refusals(monkeypatch):
    """``set_parametrization`` on a split engine (``row_split > 1``) and on an engine whose vectors do not fit the generic
    kernels' LDS, and ``backward_source`` on the latter: KH_ERR_UNSUPPORTED with the library's message, and no sweep kernel
    launched.  ``ellglobal/csr`` forced at small N keeps ``gen_fits`` (it depends on N alone: N <= 2540), so the engine
    that refuses is the unforced one of tests/test_sparse_large.py, N = 4225; the forced one at small N accepts both
    features on the generic kernels (the ``ellglobal`` rows of ``test_matrix``)."""
    import torch

    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    def parametrize(eng):
        L, I = eng.L, eng.nt - 1
        u = torch.zeros((L, I), dtype=torch.float64, device=eng.device)
        eng.set_parametrization(np.full(L, 4, dtype=np.int32), np.full(L, 0.4), np.zeros(L), u, torch.ones_like(u),
                                torch.empty_like(u))

    _lib.forget_launched_kernels()
    monkeypatch.setenv('KH_KERNEL', 'ellsplit')
    monkeypatch.setenv('KH_ELL_SPLIT', '2')
    spec = tsr._banded(600, 21, nt=4, K=2)
    split = HipKrotovEngine(configs.sparse_ops(spec), np.diff(spec.tlist))
    assert split.kernel == 'ellsplit/csr' and split.row_split == 2
    with pytest.raises(_lib.KrotovHipError, match='split engine') as err:
        parametrize(split)
    assert err.value.code == _lib.KH_ERR_UNSUPPORTED
    assert split.set_row_split(1) == 1 and split.kernel == 'ellglobal/csr'
    parametrize(split)  # (row split 1: accepted)
    split.close()
    monkeypatch.delenv('KH_KERNEL')
    monkeypatch.delenv('KH_ELL_SPLIT')
    spec = configs.config_sparse_lindblad(d=65, nt=4, K=2)
    big = HipKrotovEngine(configs.sparse_ops(spec), np.diff(spec.tlist), is_super=True)
    assert big.kernel == 'ellglobal/csr' and big.N == 4225
    with pytest.raises(_lib.KrotovHipError, match='do not fit LDS') as err:
        parametrize(big)
    assert err.value.code == _lib.KH_ERR_UNSUPPORTED
    zeros = torch.zeros((big.K, big.nt, big.N), dtype=torch.complex128, device=big.device)
    with pytest.raises(_lib.KrotovHipError, match='do not fit LDS') as err:
        big.backward_source(zeros[:, 0].clone(), np.zeros((1, big.nt - 1)), zeros, None)
    assert err.value.code == _lib.KH_ERR_UNSUPPORTED
    big.check()
    big.close()
    assert _lib.kernel_instantiations(launched_only=True) == []


# ---------------------------------------------------------------------------
# one engine, changed inputs
# ---------------------------------------------------------------------------
REUSE = {'tile_L2': True, 'tile128': False, 'coop': False}  # base: second order (the generic row first order: its adjoint-side store)
_reuse = {}


def reuse_inputs(base):
    """(A, B, source A, source B): B differs from A in u_guess, f', the kinds and their bounds, the source W, the norms
    and (second order) sigma and the previous trajectory; the operators, the grid, the shapes and chi(T) stay."""
    if base not in _reuse:
        so = REUSE[base]
        A, src_A = par_reference(base, ENGINE, so), src_reference(base, ENGINE)
        obj_B = copy.copy(A['obj'])
        obj_B.pulses = [0.8 * np.asarray(p)[::-1].copy() for p in A['obj'].pulses]
        B = build_par_reference(obj_B, so, b_shift=0.1, norms_factor=0.7, seed=6)
        _reuse[base] = (A, B, src_A, build_src_reference(obj_B, seed=1))
    return _reuse[base]


@pytest.mark.parametrize('base', sorted(REUSE))
def test_reuse_inputs_differ(base):
    """Host only: every input of the two sets differs and so does every result -- a stale tensor would be told."""
    A, B, src_A, src_B = reuse_inputs(base)
    for what in ('u_guess', 'dfdu', 'norms', 'chi', 'lambdas', 'opt', 'u', 'psi_T', 'g_a'):
        assert _distance(A[what], B[what]) > 1e-6, what
    assert A['kinds'] != B['kinds']
    assert {k[0] for k in B['kinds'] if k is not None} >= {'tanh'} and all(k[1] != -k[2] for k in B['kinds'] if k and k[0] == 'tanh')
    for what in ('W', 'norms', 'chi'):
        assert _distance(src_A[what], src_B[what]) > 1e-6, what
    if REUSE[base]:
        assert _distance(A['so_inputs'][0], B['so_inputs'][0]) > 1e-6 and _distance(A['so_inputs'][1], B['so_inputs'][1]) > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('base', sorted(REUSE))
def test_one_engine_changed_inputs(base, monkeypatch):
    """One engine and one set of device tensors, overwritten in place (``copy_``): A parametrized, B parametrized, A again
    (bit for bit the first A run), parametrization off (bit for bit the engine's earlier plain sweep, on its own
    kernel), on again with B's kinds (bit for bit the B run), the source sweep with W_A and with W_B, and the plain
    ``backward()`` (bit for bit its first run).  Every run against its restatement."""
    import torch

    from krotov_amd import _lib

    so = REUSE[base]
    A, B, src_A, src_B = reuse_inputs(base)
    obj, prob = A['obj'], A['prob']
    tol = tolerance(obj)
    K, N, L, I = obj.K, prob.N, obj.L, len(obj.pulses[0])
    for name, value in BASES[base].env.items():
        monkeypatch.setenv(name, value)
    eng = make_engine(base, obj, BASES[base].theta_max)
    c128, f64, dv = torch.complex128, torch.float64, eng.device
    t = dict(pulses=_nans((L, I), f64, dv), norms=_nans((K,), f64, dv), lam=_nans((L,), f64, dv), u_guess=_nans((L, I), f64, dv),
             dfdu=_nans((L, I), f64, dv), u_opt=_nans((L, I), f64, dv), chi=_nans((K, I + 1, N), c128, dv),
             W=_nans((K, I + 1, N), c128, dv), src_norms=_nans((K,), f64, dv), prev=_nans((K, I + 1, N), c128, dv),
             sigma=_nans((I,), f64, dv), store=_nans((K, I + 1, N), c128, dv), src_out=_nans((K, I + 1, N), c128, dv))
    S, init, chi_T = eng.dev(np.array(obj.shapes), f64), eng.dev(prob.init, c128), eng.dev(A['chi_T'], c128)
    outs = (_nans((L, I), f64, dv), _nans((K, N), c128, dv), _nans((L,), f64, dv))

    def put(name, host):
        t[name].copy_(torch.from_numpy(np.ascontiguousarray(host)))

    def load(X, src):
        put('pulses', np.array(X['obj'].pulses)), put('norms', X['norms']), put('lam', X['lambdas'])
        put('u_guess', X['u_guess']), put('dfdu', X['dfdu']), put('W', src['W']), put('src_norms', src['norms'])
        if so:
            put('prev', X['so_inputs'][0]), put('sigma', X['so_inputs'][1])
        t['chi'].fill_(float('nan'))
        return eng.backward(chi_T, t['pulses'], out=t['chi']).cpu().numpy()

    def update(X=None):
        for x in outs + (t['u_opt'], t['store']):
            x.fill_(float('nan'))
        if X is not None:
            kind, a, b = device_kinds(X['kinds'], X['obj'].pulses)
            eng.set_parametrization(kind, a, b, t['u_guess'], t['dfdu'], t['u_opt'])
        _lib.forget_launched_kernels()
        eng.forward_update(t['chi'], t['norms'], init, t['pulses'], S, t['lam'], out=outs)
        eng.check()
        assert eng.stats()['intervals'] == I
        got = dict(opt=outs[0].cpu().numpy(), psi_T=outs[1].cpu().numpy(), g_a=outs[2].cpu().numpy())
        if X is not None:
            got['u'] = t['u_opt'].cpu().numpy()
        if so:
            got['store'] = t['store'].cpu().numpy()
        return got, sorted(n for n in _lib.kernel_instantiations(launched_only=True) if 'forward_update' in n)

    def deviation(got, X):
        return max(_distance(got[w], X[w]) / (max(1.0, np.abs(X[w]).max()) if w in ('opt', 'u', 'g_a') else 1.0) for w in got)

    def source(src):
        t['src_out'].fill_(float('nan'))
        _lib.forget_launched_kernels()
        got = eng.backward_source(chi_T, t['pulses'], t['W'], t['src_norms'], out=t['src_out']).cpu().numpy()
        eng.check()
        assert _lib.kernel_instantiations(launched_only=True) == [BASES[base].src]
        assert np.array_equal(got[:, I], src['chi_T'])
        return _distance(got, src['chi']) / max(1.0, np.abs(src['chi']).max())

    try:
        if so:
            eng.set_second_order(t['prev'], t['store'], t['sigma'])
        dev = {}
        chi_first = load(A, src_A)
        dev['chi'] = _distance(chi_first, A['chi'])
        plain_first, plain_kernels = update()
        assert plain_kernels and not any('_par<' in n for n in plain_kernels), plain_kernels
        a1, par_kernels = update(A)
        assert par_kernels == [par_kernel(base, so)], par_kernels
        dev['A'] = deviation(a1, A)
        load(B, src_B)
        b1, _ = update(B)
        dev['B'] = deviation(b1, B)
        assert _distance(a1['opt'], b1['opt']) > 1e-6
        load(A, src_A)
        a2, _ = update(A)
        for what in a1:
            assert np.array_equal(a1[what], a2[what]), 'A again: ' + what
        eng.set_parametrization(None)
        plain_again, kernels = update()
        assert kernels == plain_kernels, (kernels, plain_kernels)
        for what in plain_first:
            assert np.array_equal(plain_first[what], plain_again[what]), 'parametrization off: ' + what
        load(B, src_B)
        b2, kernels = update(B)
        assert kernels == par_kernels
        for what in b1:
            assert np.array_equal(b1[what], b2[what]), 'on again with the kinds of B: ' + what
        load(A, src_A)
        dev['source A'] = source(src_A)
        load(B, src_B)
        dev['source B'] = source(src_B)
        chi_last = load(A, src_A)
        assert np.array_equal(chi_first, chi_last), 'the plain backward sweep'
        kernel = eng.kernel
    finally:
        eng.close()
    print('bounded_constrained reuse %s [%s]: %s; update kernels %s / %s' % (
        base, kernel, ' '.join('%s %.1e' % kv for kv in dev.items()), plain_kernels, par_kernels))
    assert max(dev.values()) < tol, dev


# ---------------------------------------------------------------------------
# the graph replay of the per-interval form
# ---------------------------------------------------------------------------
GRAPH_CHUNK = 4
GRAPH_IDS = ['%s-I%d' % (b, I) for b in ('tile_L2', 'tile128') for I in (8, 9, 10)]


@pytest.mark.parametrize('gid', GRAPH_IDS)
def test_graph_witness(gid):
    base, I = gid.rsplit('-I', 1)
    obj = problem(base, ('ends', int(I)))
    hp.grid_ends_witness(obj, 1.0)
    ref = par_reference(base, ('ends', int(I)), False)
    move = np.abs(ref['opt'] - np.array(obj.pulses)).max(axis=0)
    assert move[0] > 1e-6 and move[-1] > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('gid', GRAPH_IDS)
def test_graph_replay(gid, monkeypatch):
    """``forward_update_sharded(graph_chunk=4)`` of a parametrized engine (``u.n_dev != nullptr``: the interval index in
    device memory) on 8, 9 and 10 intervals: bit for bit the ``graph_chunk=0`` run, ``u_opt`` included, and within the
    project's bound of the restatement.  I = 2 chunk + 1 and 2 chunk + 2: the graph is there and no fallback warning was
    raised; I = 2 chunk: the engine's rule (``nt - 1 > 2 graph_chunk``) takes the plain loop, as in
    tests/test_grid_ends.py."""
    base, I = gid.rsplit('-I', 1)
    I = int(I)
    ref = par_reference(base, ('ends', I), False)
    obj = ref['obj']
    eng = make_engine(base, obj, BASES[base].theta_max)
    try:
        plain, dev0, launched0 = run_par(eng, ref, False, mode='0')
        assert eng._sh['graph'] is None
        chi = eng.backward(ref['chi_T'], np.array(obj.pulses))
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            got, dev, launched = run_par(eng, ref, False, mode=str(GRAPH_CHUNK), chi=chi)
        if I == 2 * GRAPH_CHUNK:
            assert eng._sh['graph'] is None
        else:
            assert eng._sh['graph'] is not None and eng._sh['graph_key'] == (chi.data_ptr(), GRAPH_CHUNK)
        kernel = eng.kernel
    finally:
        eng.close()
    print('bounded_constrained graph %s [%s]: %s; launched: %s' % (gid, kernel, ' '.join('%s %.1e' % kv for kv in sorted(dev.items())),
                                                                 ', '.join(launched)))
    assert [n for n in launched if 'forward_update' in n] == [GEN_PAR], launched  # (one launch per interval: the generic form)
    for what in got:
        assert np.array_equal(got[what], plain[what]), what
    assert max(dev.values()) < tolerance(obj) and max(dev0.values()) < tolerance(obj), (dev, dev0)


# ---------------------------------------------------------------------------
# a caller-set series tolerance (the three references of tests/test_series_tolerance.py)
# ---------------------------------------------------------------------------
# Tile rows whose engines run the one-term-per-phase kernels themselves, tile rows whose plain sweeps are the
# two-terms-per-phase or one-wave kernels' (they hand their plan to the parametrized and the source form), and the generic
# rows: theta_max 1, so the one-term-per-phase kernels evaluate the engine's general table (``deg_theta`` / ``ratios``:
# the Chebyshev form with cap 2 on Hermitian operators, Taylor's on the mixed row), one product per term -- the degree
# rule tests/series_oracle.py restates.  The co-state store of the update sweep is the exact one, uploaded, so that the
# update sweep's own series is what is measured.  The series oracle's update in u is ``pc.update_sweep`` inside the
# ``SeriesOracle`` context: it steps through ``ko._step``, which the context replaces.
TOLS, TOL_HOW = (1e-4, 1e-8), ('ramp', 1.0)
# every parametrized instantiation (the ten tile forms: q2 -- mini16 shares its pair --, tile512 with L = 2, 3, 4 and tile256,
# first and second order; the two generic forms) and every source form; feature 'par' / 'par-so' / 'src'
TOL_ROWS = [(b, f) for b in ('q2', 'tile_L2', 'tile_L3', 'tile_L4', 'tile256') for f in ('par', 'par-so', 'src')]
TOL_ROWS += [('mini16', 'par'), ('mini16', 'src'), ('tile128', 'par'), ('tile128', 'src'), ('mixed', 'par')]
TOL_CASES = [(b, f, t) for b, f in TOL_ROWS for t in TOLS]
TOL_IDS = ['%s-%s-tol%g' % c for c in TOL_CASES]
_tol_refs, _tol_series = {}, {}


def _table(tol, obj=None):
    """Hermitian operators: the Chebyshev-form table with cap 2; the mixed row (a Liouvillian among its objectives): Taylor's,
    as tests/test_series_tolerance.py names them."""
    import series_oracle as so

    if obj is not None and obj.fmt == 'mixed':
        return so.table('taylor', tol, 2.0)
    return so.table('real', tol, 2.0)


def _sup_dfdu(kind):
    """sup |f'| of a kind: |f(u + du) - f(u)| <= sup |f'| |du|."""
    if kind is None:
        return 1.0
    a = abs(pc._ab(kind)[0])
    return a * 4.0 / (3.0 * np.sqrt(3.0)) if kind[0] == 'tanhsq' else a


def par_bound(ref, tol):
    """``series_oracle.tolerance_bound`` for the update in u.  The error of u_new on interval n is S / lambda |c_n| x (the
    error of the update sum), c = f'(u_guess), and the pulse f(u_new) is off by at most sup |f'| times that: the bound's
    own derivation with the shape S_ln |c_ln| sup |f'_l| in the place of S_ln.  (Its g_a is that of the update in eps and
    is not used here.)"""
    import series_oracle as so

    obj, prob = ref['obj'], ref['prob']
    tab = _table(tol, obj)
    scaled = copy.copy(obj)
    scaled.shapes = [np.asarray(S) * np.abs(c) * _sup_dfdu(k) for S, c, k in zip(obj.shapes, ref['dfdu'], ref['kinds'])]
    scaled.lambdas = list(ref['lambdas'])
    theta, nsub_opt, _ = so.plan(obj, ref['opt'], TOL_HOW[1], tab)
    plans = dict(guess=so.plan(obj, obj.pulses, TOL_HOW[1], tab)[1], opt=nsub_opt,
                 tol_guess=so.step_errors(obj, prob, obj.pulses, TOL_HOW[1], tab, tol),
                 tol_opt=so.step_errors(obj, prob, ref['opt'], TOL_HOW[1], tab, tol, so.WIDEN), theta_opt=theta)
    return so.tolerance_bound(scaled, tol, plans, ref, ref['so_inputs'] is not None)


def src_bound(ref, tol):
    """(K, nt) bounds on the 2-norm error of the backward sweep with a source: the plain sweep's recursion of
    ``tolerance_bound`` with the vector an interval starts from, chi[n+1] + h_n W[n+1] (the source itself is added exactly)."""
    import series_oracle as so

    obj, prob = ref['obj'], ref['prob']
    tab = _table(tol, obj)
    dt = np.diff(prob.tlist)
    _, nsub, _ = so.plan(obj, obj.pulses, TOL_HOW[1], tab)
    err = so.step_errors(obj, prob, obj.pulses, TOL_HOW[1], tab, tol)
    g = np.exp(dt[None, :] * np.maximum(0.0, so._growth_rates(prob, [np.asarray(p) for p in obj.pulses])))
    out = np.zeros((prob.K, len(dt) + 1))
    for k in range(prob.K):
        for n in range(len(dt) - 1, -1, -1):
            start = ref['chi'][k, n + 1] + (0.5 * dt[n] / ref['norms'][k]) * ref['W'][k, n + 1]
            out[k, n] = so._substeps(out[k, n + 1], float(np.linalg.norm(start)), nsub[k, n], g[k, n] ** (1.0 / nsub[k, n]), err[k, n])
    return out


def tol_reference(base, feature):
    """The exact restatement of a tolerance row.  Parametrized: boundary co-states and ||chi_k|| as
    tests/test_series_tolerance.py's ``reference`` (chi_k(T) plus 2 (-i mu_k phi_k(T)) / ||mu_k phi_k(T)||, normalised, so that
    the update sums add up the way the bound's worst case does; ||chi_k|| shrunk by that module's CHI_SHRINK until the bound
    at 1e-4 is not empty -- that module's condition)."""
    import test_series_tolerance as tst

    if (base, feature) in _tol_refs:
        return _tol_refs[base, feature]
    obj = problem(base, TOL_HOW)
    if feature == 'src':
        ref = src_reference(base, TOL_HOW)
        _tol_refs[base, feature] = ref
        return ref
    so_row = feature == 'par-so'
    prob = _oracle(obj)
    with hp.MemoExpm():
        psi_T, states = ko.forward_propagation(prob, obj.pulses, store=True)
        chi_T = np.array(boundary_costates(obj, prob))
        for k in range(prob.K):
            m = ko._mu_apply(prob, k, 0, psi_T[k])
            chi_T[k] = chi_T[k] + 2.0 * (-1j) * m / np.linalg.norm(m)
        chi_T = chi_T / np.linalg.norm(chi_T, axis=1)[:, None]
        chi = ko.backward_sweep(prob, chi_T, obj.pulses)
        kinds = choose_kinds(obj.pulses)
        base_so = second_order_inputs(obj, prob) if so_row else None
        # (sigma feeds back the same way and shrinks with ||chi||; a second-order row gets one more step, sigma alone x 0.1:
        # with three controls the bound on the pulse error at the last step is 12 % of the pulse change, beyond that
        # module's 10 %)
        for shrink, sigma_shrink in [(x, x) for x in tst.CHI_SHRINK] + ([(tst.CHI_SHRINK[-1], 0.1 * tst.CHI_SHRINK[-1])] if so_row else []):
            norms = tsr.chi_norms(obj) * shrink
            so_inputs = (base_so[0], base_so[1] * sigma_shrink) if so_row else None
            ref = restate_par(obj, prob, chi, norms, kinds, so_inputs)
            ref.update(obj=obj, prob=prob, norms=norms, chi_T=chi_T, chi=chi, kinds=kinds, so_inputs=so_inputs, states=states)
            if so_row:
                ref.update(prev=so_inputs[0], sigma=so_inputs[1])
            if tst.bound_is_not_empty(par_bound(ref, TOLS[0]), np.abs(ref['opt'] - np.array(obj.pulses)).max()):
                break
    _tol_refs[base, feature] = ref
    return ref


def tol_series(base, feature, tol):
    """The series oracle's sweep of a tolerance row: every step ``nsub`` sub-steps of the exported polynomial of the planned
    degree (tests/series_oracle.py), the update in u through ``pc.update_sweep``."""
    import series_oracle as so

    key = (base, feature, tol)
    if key not in _tol_series:
        ref = tol_reference(base, feature)
        obj, prob = ref['obj'], ref['prob']
        with so.SeriesOracle(prob, hp.series_bounds(obj), _table(tol, obj), TOL_HOW[1]):
            if feature != 'src':
                _tol_series[key] = restate_par(obj, prob, ref['chi'], ref['norms'], ref['kinds'], ref['so_inputs'])
            else:
                _tol_series[key] = dict(chi=cc.backward_sweep(prob, ref['chi_T'], obj.pulses, ref['W'], ref['norms']))
    return _tol_series[key]


def planned_products(ref, tol, pulses):
    import series_oracle as so

    tab = _table(tol, ref['obj'])
    theta, nsub, deg = so.plan(ref['obj'], pulses, TOL_HOW[1], tab)
    assert so.threshold_distance(theta, nsub, TOL_HOW[1], tab) > 1e-9
    return so.products(tab, nsub, deg)


def _tol_compare(got, ref, feature):
    """(largest entry of the difference per quantity, pulses / u / g_a relative to max(1, max |.|); 2-norm errors of the
    states)."""
    names = ('chi',) if feature == 'src' else ('opt', 'u', 'psi_T', 'g_a') + (('store',) if feature == 'par-so' else ())
    dev = {w: _distance(got[w], ref[w]) / (max(1.0, np.abs(ref[w]).max()) if w in ('opt', 'u', 'g_a') else 1.0) for w in names}
    return dev


def _beyond(got, ref, feature, tol, slack):
    """The quantities beyond their derived bound (+ ``slack`` for rounding)."""
    if feature == 'src':
        checks = {'chi': (np.linalg.norm(got['chi'] - ref['chi'], axis=2), src_bound(ref, tol))}
    else:
        bound = par_bound(ref, tol)
        sup = np.array([_sup_dfdu(k) for k in ref['kinds']])[:, None]
        checks = {'opt': (np.abs(got['opt'] - ref['opt']), bound['opt']), 'u': (np.abs(got['u'] - ref['u']), bound['opt'] / sup),
                  'psi_T': (np.linalg.norm(got['psi_T'] - ref['psi_T'], axis=1), bound['upd'][:, -1])}
        if feature == 'par-so':
            checks['store'] = (np.linalg.norm(got['store'] - ref['store'], axis=2), bound['upd'])
    return {w: float((d - b).max()) for w, (d, b) in checks.items() if (d - b).max() > slack}


@pytest.mark.parametrize('tid', TOL_IDS)
def test_tolerance_witness(tid):
    """Host only, per (row, tol): the plan is in the regime (at 1e-4: three or more degrees, one of at most 2 and one of at
    least 5, sub-steps; at 1e-8: other degrees than at the default tolerance), no theta sits near a threshold, the bound is
    not empty (tests/test_series_tolerance.py's condition: below 1e-2 for the states, below 10 % of the pulse change) and
    the series oracle stays within it of the exact restatement -- while being more than 100 x the project's rounding
    tolerance away at 1e-4."""
    import series_oracle as so

    base, feature, tol = TOL_CASES[TOL_IDS.index(tid)]
    ref = tol_reference(base, feature)
    obj = ref['obj']
    tab = _table(tol, obj)
    for pulses in [obj.pulses] + ([ref['opt']] if feature != 'src' else []):
        theta, nsub, deg = so.plan(obj, pulses, TOL_HOW[1], tab)
        assert so.threshold_distance(theta, nsub, TOL_HOW[1], tab) > 1e-9
        k = int(np.argmax(theta.max(axis=1)))
        if tol == 1e-4:
            assert len(set(deg[k].tolist())) >= 3 and deg[k].min() <= 2 and deg[k].max() >= 5 and np.any(nsub[k] > 1), deg[k]
        else:
            assert np.all(deg[k] != so.plan(obj, pulses, TOL_HOW[1], so.at_tolerance(tab, 0.0))[2][k])
    ser = tol_series(base, feature, tol)
    dev = _tol_compare(ser, ref, feature)
    if feature != 'src':
        bound = par_bound(ref, tol)
        change = np.abs(ref['opt'] - np.array(obj.pulses)).max()
        worst, pulse = max(bound['states'].max(), bound['chi'].max(), bound['upd'].max()), bound['opt'].max()
        print('tolerance witness %s: series oracle off by %s; bound upd %.1e opt %.1e (pulse change %.1e)' % (
            tid, ' '.join('%s %.1e' % kv for kv in dev.items()), bound['upd'].max(), pulse, change))
        if tol == 1e-4:
            assert np.isfinite(worst) and worst < 1e-2 and pulse < 0.1 * change and change > 1e-6
            assert dev['psi_T'] > 100.0 * 1e-11
    else:
        worst = src_bound(ref, tol).max()
        print('tolerance witness %s: series oracle off by %.1e; bound %.1e' % (tid, dev['chi'], worst))
        if tol == 1e-4:
            assert np.isfinite(worst) and worst < 1e-2 and dev['chi'] > 100.0 * 1e-11
    assert not _beyond(ser, ref, feature, tol, 1e-11)


_tol_default = {}


def _tol_run(base, feature, tol):
    """One sweep of a tolerance row on an engine created with ``tol``, twice: (results, products, launched, kernel)."""
    import torch

    ref = tol_reference(base, feature)
    eng = make_engine(base, ref['obj'], TOL_HOW[1], tol=tol)
    try:
        runs = []
        for _ in range(2):
            if feature != 'src':
                got, _, launched = run_par(eng, ref, feature == 'par-so', chi=eng.dev(ref['chi'], torch.complex128))
            else:
                chi, launched = run_src(eng, ref)
                got = dict(chi=chi)
            runs.append((got, eng.stats()['matvecs']))
        for what in runs[0][0]:
            assert np.array_equal(runs[0][0][what], runs[1][0][what]), 'second run differs: ' + what
        assert runs[0][1] == runs[1][1]
        return runs[0][0], runs[0][1], launched, eng.kernel
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('tid', TOL_IDS)
def test_tolerance(tid, monkeypatch):
    """``tol`` = 1e-4 and 1e-8 against the three references of tests/test_series_tolerance.py: the series oracle (to that
    module's rounding bound -- 1e-11 in the ramp regime -- with exactly the planned products), the exact restatement
    within the derived bound, and, at 1e-4, more than 100 x the default run's deviation from it (an engine that ignored
    ``tol`` fails that); the same instantiation as at the default tolerance, fewer products, two runs bit for bit."""
    base, feature, tol = TOL_CASES[TOL_IDS.index(tid)]
    ptol = 1e-11  # (tests/test_series_tolerance.py: project_tol of a ramp row)
    ref, ser = tol_reference(base, feature), tol_series(base, feature, tol)
    if (base, feature) not in _tol_default:
        _tol_default[base, feature] = _tol_run(base, feature, 0.0)
    got0, count0, launched0, kernel0 = _tol_default[base, feature]
    got, count, launched, kernel = _tol_run(base, feature, tol)
    dev, dev0, sdev = _tol_compare(got, ref, feature), _tol_compare(got0, ref, feature), _tol_compare(got, ser, feature)
    pulses, pulses0 = (got['opt'], got0['opt']) if feature != 'src' else (ref['obj'].pulses, ref['obj'].pulses)
    planned, planned0 = planned_products(ref, tol, pulses), planned_products(ref, 0.0, pulses0)
    print('bounded_constrained tolerance %s [%s]: products %d (planned series %d; default tolerance %d, planned %d); from the '
          'series oracle %s; from the exact restatement %s (default: %s); launched: %s' % (
              tid, kernel, count, planned, count0, planned0, ' '.join('%s %.1e' % kv for kv in sdev.items()),
              ' '.join('%s %.1e' % kv for kv in dev.items()), ' '.join('%s %.1e' % kv for kv in dev0.items()), ', '.join(launched)))
    want = par_kernel(base, feature == 'par-so') if feature != 'src' else BASES[base].src
    assert want in launched and launched == launched0 and kernel == kernel0
    assert count < count0
    # the source sweep: the series alone; the update sweep: plus the products of the update sums, whatever the tolerance
    assert count - planned == count0 - planned0 and (count == planned if feature == 'src' else count >= planned), (
        count, planned, count0, planned0)
    assert max(sdev.values()) < ptol, sdev
    assert max(dev0.values()) < ptol, dev0
    assert not _beyond(got, ref, feature, tol, ptol)
    if tol == 1e-4:
        for what in (('psi_T',) if feature != 'src' else ('chi',)):
            assert dev[what] > 100.0 * dev0[what], (what, dev[what], dev0[what])


# ---------------------------------------------------------------------------
# tests/fuzz_parity.py --bounded-constrained
# ---------------------------------------------------------------------------
FUZZ_SEED, FUZZ_CASES = 3, 16


def test_fuzz_generator_is_its_own():
    """Host only: ``--bounded-constrained`` decides with a generator of its own -- the default stream draws the same problems
    with and without it -- and over the fixed-seed slice it draws every kind, bounds that are not symmetric, inputs inside
    the range of their kinds (finite u) and an update that moves the pulses."""
    import fuzz_parity

    plain, other = np.random.default_rng(FUZZ_SEED), np.random.default_rng(FUZZ_SEED)
    rng_bc = np.random.default_rng([FUZZ_SEED, 0xbc0d])
    seen = set()
    for _ in range(FUZZ_CASES):
        a, tag_a, fmt_a = fuzz_parity.draw(plain)
        b, tag_b, fmt_b = fuzz_parity.draw(other)
        assert (a.name, a.K, a.N, a.L, len(a.tlist), fmt_a, tag_a) == (b.name, b.K, b.N, b.L, len(b.tlist), fmt_b, tag_b)
        r = fuzz_parity.bounded_constrained_inputs(rng_bc, b)
        seen |= {'none' if k is None else k[0] for k in r['kinds']}
        assert np.all(np.isfinite(r['u_guess'])) and np.all(np.isfinite(r['opt'])) and np.all(np.isfinite(r['src_chi']))
        assert any(k is not None and k[0] == 'tanh' and k[1] != -k[2] for k in r['kinds']) or 'tanh' not in {k and k[0] for k in r['kinds']}
        assert np.all(np.abs(r['src_norms'] - 1.0) > 1e-3)
        with hp.MemoExpm():
            plain_chi = ko.backward_sweep(r['prob'], r['chi_T'], r['gp'])
        assert np.abs(r['src_chi'] - plain_chi).max() > 1e-6
    assert seen >= {'none', 'linear', 'tanh', 'tanhsq'}, seen
    assert plain.random() == other.random()


@pytest.mark.gpu
def test_fuzz_parity_bounded_constrained_fixed_seed():
    """A fixed-seed slice of ``tests/fuzz_parity.py --bounded-constrained``."""
    import fuzz_parity

    stats = {}
    done, failures = fuzz_parity.fuzz(FUZZ_SEED, cases=FUZZ_CASES, verbose=True, bounded_constrained=True, stats=stats)
    assert done == FUZZ_CASES and not failures, failures
    assert stats['no_parametrization'] == 0  # (N <= 144, no row split: every drawn engine takes both features and ran them)
