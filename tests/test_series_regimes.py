"""Every kernel family across the regimes of the per-interval series, against the oracle.

Each family carries its own copy of the series logic: the degree lookup, the sub-step loop, the reload of the coefficient
rows when the degree changes, the cached degree bracket and -- where the generator is advanced instead of rebuilt -- a
restart every 64 intervals.  The fixtures of the rest of the suite pin ``||H0|| dt = 0.4`` on a uniform grid, so almost all
of them take one sub-step at one degree for the whole sweep.  This module transforms the same base cases into

* ``ramp``        a non-uniform grid, theta_n from <= 1e-3 theta_max up to 2.9 theta_max and back (degrees rise and fall,
                  sub-steps 1 -> 3 -> 1),
* ``pulse_ramp``  a uniform grid and a guess pulse spanning the same range, exactly 0.0 on three or more intervals (the first
                  and the last one among them),
* ``tiny``        every operator x 1e-7 (degree 2),
* ``long``        140 intervals under a two-period pulse ramp (two restarts of an advanced generator),

(``tests/helpers.py``; none of them touches Hermiticity, sharing, ensemble scaling or sparsity, so the engine picks the
same family), proves on the host that every (case, regime) pair really is in its regime (``test_witness``: no GPU), and
compares the four sweeps of every row of the family x regime table with ``oracle/krotov_oracle.py`` on the GPU
(``test_matrix``).

Tolerances are the project's: 1e-12 in Hilbert space; 1e-11 in Liouville space and for the ``ramp``
regime (non-uniform grid with theta > 1: what test_nonuniform_grid_and_large_step_norms uses).

Base cases whose grid has fewer than eleven intervals are built with eleven (a ramp cannot rise and fall on three); no
base case is replaced or thinned.  ``||chi_k||`` is chosen by one rule for every row (``chi_norms``), not per case.
"""
import collections

import numpy as np
import pytest

import helpers as hp
from krotov_amd import configs
from oracle import krotov_oracle as ko

Row = collections.namedtuple('Row', 'id family base fmt regime theta_max theta_arg env so')

BASES = {}
ROWS = []


def _c5(**kw):
    return lambda: configs.config_c5(**kw)


def _different_norms(spec):
    """Per-objective operators of different norm (the one-wave kernels take the largest degree of their wave)."""
    f = 1.0 / (1.0 + 1.5 * np.arange(spec.K))
    spec.H0 = [f[k] * spec.H0[k] for k in range(spec.K)]
    spec.Hc = [[f[k] * h for h in spec.Hc[k]] for k in range(spec.K)]
    return spec


def _coherent(spec, d):
    """Initial density matrices with coherences, (|k> + |k+1>)(<k| + <k+1|) / 2: the ladder's control operator is diagonal,
    so on the populations the fixture starts from its commutator vanishes and -- to first order, which is all the tiny
    regime has -- the update would not move the pulses."""
    for k in range(spec.K):
        psi = np.zeros(d, dtype=np.complex128)
        psi[k] = psi[k + 1] = np.sqrt(0.5)
        spec.init[k] = np.outer(psi, psi.conj()).ravel(order='F')
    return spec


def _banded(N, bands, nt, K=2):
    import test_hip_parity

    return test_hip_parity._banded(N, bands, nt, K)


def _lindblad(make):
    import test_lindblad_form as tlf

    def build():
        case = make(tlf)
        case.pulses = tlf._pulses(case)
        case.shapes = [np.linspace(0.2, 1.0, len(case.dt)) for _ in range(case.L)]
        case.lambdas = [0.7 + 0.3 * l for l in range(case.L)]
        return case
    return build


for _name, _fn, _fmt in [
    # tile64/256: more objectives than CUs, one control, two workgroups per CU
    ('c5_k300', _c5(K=300, N=16, nt=21, distinct=True), 'dense'),
    # tile64/stream
    ('c5_k600_distinct', _c5(K=600, N=8, nt=16, distinct=True), 'dense'),
    ('c5_k520_n64_distinct', _c5(K=520, N=64, nt=12, distinct=True), 'dense'),
    ('c5_k264_n64_L2', _c5(K=264, N=64, nt=12, L=2, distinct=True), 'dense'),
    ('c5_k1100_L3', _c5(K=1100, N=6, nt=12, L=3), 'dense'),
    # tile64x
    ('L5_n64', _c5(K=4, N=64, nt=21, L=5), 'dense'),
    ('L6_n20', _c5(K=5, N=20, nt=31, L=6, distinct=True), 'dense'),
    ('L8_n64', _c5(K=4, N=64, nt=21, L=8, distinct=True), 'dense'),
    ('L5_k260', _c5(K=260, N=6, nt=12, L=5), 'dense'),
    # ens64/mfma
    ('k40_n64', _c5(K=40, N=64, nt=12), 'dense'),
    ('k37_n33', _c5(K=37, N=33, nt=12), 'dense'),
    ('k70_n64', _c5(K=70, N=64, nt=12), 'dense'),
    ('k100_n16', _c5(K=100, N=16, nt=12), 'dense'),
    ('k520_n8', _c5(K=520, N=8, nt=12), 'dense'),
    # coop16/mfma
    ('shared_n96_L2', lambda: configs.config_shared(K=20, N=96, nt=21, L=2), 'dense'),
    ('shared_n300', lambda: configs.config_shared(K=16, N=300, nt=12, L=1), 'dense'),
    ('shared_n96_long', lambda: configs.config_shared(K=8, N=96, nt=141, L=1), 'dense'),
    ('c4_d9', lambda: configs.config_c4(d=9, nt=41, n_logical=2), 'dense'),
    # tile128/512
    ('c5_n80', _c5(K=3, N=80, nt=31, L=2), 'dense'),
    ('c5_n100', _c5(K=4, N=100, nt=21, L=1, distinct=True), 'dense'),
    ('c5_n128', _c5(K=2, N=128, nt=12, L=1), 'dense'),
    ('c5_n80_long', _c5(K=3, N=80, nt=141, L=2), 'dense'),
    ('c5_n128_long', _c5(K=2, N=128, nt=141, L=1), 'dense'),
    # tile64q2/512
    ('c5_n64', _c5(K=8, N=64, nt=61), 'dense'),
    ('c5_n33', _c5(K=5, N=33, nt=41), 'dense'),
    ('c5_n64_long', _c5(K=8, N=64, nt=141), 'dense'),
    ('c5_n33_long', _c5(K=5, N=33, nt=141), 'dense'),
    # tile64/512
    ('c5_n64_L2', _c5(K=4, N=64, nt=41, L=2, distinct=True), 'dense'),
    ('c5_n12_L3', _c5(K=5, N=12, nt=81, L=3, distinct=True), 'dense'),
    ('c5_n24_L4', _c5(K=4, N=24, nt=21, L=4, distinct=True), 'dense'),
    # sparse operators
    ('lindblad', lambda: _coherent(configs.config_sparse_lindblad(nt=21), 12), 'csr'),
    ('lindblad_n625', lambda: _coherent(configs.config_sparse_lindblad(d=25, nt=12, K=2), 25), 'csr'),
    ('banded_n800', lambda: _banded(800, 11, nt=12), 'csr'),   # two rows per lane of 512 threads (N > 768, 8 < E <= 16)
    ('c5_n16_csr', _c5(K=6, N=16, nt=31), 'csr'),
    ('c5_n33_csr', _c5(K=5, N=33, nt=21), 'csr'),
    # generic
    ('L2_n160', _c5(K=2, N=160, nt=12, L=2, distinct=True), 'dense'),
    ('L5_n100', _c5(K=3, N=100, nt=13, L=5, distinct=True), 'dense'),
    # generic/mixed
    ('mixed_dims', lambda: configs.config_mixed('dims', nt=21), 'mixed'),
    ('mixed_wide', lambda: configs.config_mixed('wide', nt=21), 'mixed'),
    # lindblad/matrix (row blocking 1, 2, 4)
    ('d7', _lindblad(lambda t: t._random(7, 3, 1, 1, 12, 1)), 'lindblad'),
    ('c4_d20', _lindblad(lambda t: t._from_spec(configs.config_c4_lindblad(), 11)), 'lindblad'),
    ('d32_two_cops_two_controls', _lindblad(lambda t: t._random(32, 2, 2, 2, 12, 2)), 'lindblad'),
    # one-wave kernels
    ('c5_n16', _c5(K=6, N=16, nt=31), 'dense'),
    ('c3', lambda: configs.config_c3(nt=31), 'dense'),
    ('c5_n16_norms', lambda: _different_norms(configs.config_c5(K=6, N=16, nt=31, distinct=True)), 'dense'),
    ('c3_norms', lambda: _different_norms(configs.config_c3(nt=31)), 'dense'),
]:
    BASES[_name] = (_fn, _fmt)


def rows(family, names, regimes, theta_max, env=None, tag='', so=False, default_too=False):
    for name in names:
        for regime in regimes:
            rid = '%s-%s%s-%s' % (family, name, tag, regime)
            ROWS.append(Row(rid, family, name, BASES[name][1], regime, theta_max, theta_max, dict(env or {}), so))
        if default_too and name == names[0]:  # (one case per family with theta_max left to the engine)
            ROWS.append(Row('%s-%s%s-%s-default' % (family, name, tag, regimes[0]), family, name, BASES[name][1], regimes[0],
                            theta_max, 0.0, dict(env or {}), so))


THREE = ('ramp', 'pulse_ramp', 'tiny')
rows('tile64/256', ['c5_k300'], THREE, 1.0, default_too=True)
rows('tile64/stream', ['c5_k600_distinct', 'c5_k520_n64_distinct', 'c5_k264_n64_L2', 'c5_k1100_L3'], THREE, 1.0,
     default_too=True)
rows('tile64x/512', ['L5_n64', 'L6_n20', 'L8_n64', 'L5_k260'], THREE, 1.0, default_too=True)
for _b, _cg in (('k40_n64', '1'), ('k37_n33', '2'), ('k70_n64', '4'), ('k100_n16', '8')):
    rows('ens64/mfma', [_b], THREE, 1.0, env={'KH_ENS': '1', 'KH_ENS_NCG': _cg}, tag='_cg' + _cg, default_too=_cg == '1')
rows('ens64/mfma', ['k520_n8'], THREE, 1.0, tag='_ens2')                        # kh_ens2_* (A^2 chain) by itself
rows('ens64/mfma', ['k520_n8'], THREE, 1.0, env={'KH_ENS2': '0'}, tag='_ens2off')  # its term-by-term twin
for _cols in ('2', '4', '16'):
    rows('coop16/mfma', ['shared_n96_L2'], THREE, 4.0, env={'KH_COOP_COLS': _cols}, tag='_cols' + _cols,
         default_too=_cols == '4')
    for _nosq in ('0', '1'):
        rows('coop16/mfma', ['shared_n300'], THREE if _cols == '4' or _nosq == '0' else ('ramp',), 4.0,
             env={'KH_COOP_COLS': _cols, 'KH_COOP_NOSQ': _nosq}, tag='_cols%s_nosq%s' % (_cols, _nosq))
for _nosq in ('0', '1'):
    rows('coop16/mfma', ['shared_n96_long'], ('long',), 4.0, env={'KH_COOP_NOSQ': _nosq}, tag='_nosq' + _nosq)
rows('coop16/mfma', ['shared_n96_long'], ('long',), 4.0, env={'KH_COOP_COLS': '16'}, tag='_cols16')
rows('coop16/mfma', ['shared_n300'], ('ramp',), 4.0, tag='_so', so=True)
rows('coop16/mfma', ['c4_d9'], ('ramp',), 4.0, default_too=True)
rows('tile128/512', ['c5_n80', 'c5_n100', 'c5_n128'], ('ramp', 'tiny'), 1.0, default_too=True)
rows('tile128/512', ['c5_n80_long', 'c5_n128_long'], ('long',), 1.0)
rows('tile64q2/512', ['c5_n64_long', 'c5_n33_long'], ('long',), 1.0)
rows('tile64q2/512', ['c5_n64', 'c5_n33'], ('ramp',), 1.0, env={'KH_NO_ADJ': '1'}, tag='_noadj', default_too=True)
rows('tile64q2/512', ['c5_n64', 'c5_n33'], ('ramp',), 1.0, env={'KH_TAYLOR': '1'}, tag='_taylor')
rows('tile64q2/512', ['c5_n64'], ('ramp',), 1.0, tag='_so', so=True)
rows('tile64/512', ['c5_n64_L2', 'c5_n12_L3', 'c5_n24_L4'], ('ramp', 'tiny'), 1.0, default_too=True)
rows('ell/csr', ['lindblad', 'lindblad_n625', 'banded_n800', 'c5_n16_csr'], ('ramp', 'tiny'), 4.0)
# theta_max left to the engine: a Hermitian generator takes the Chebyshev form's cap in the padded-row kernels (KH_ELL_THETA_CAP)
rows('ell/csr', ['c5_n16_csr'], ('ramp',), 6.0, tag='_cap6', default_too=True)
rows('ellstream/csr', ['lindblad'], ('ramp', 'tiny'), 4.0, env={'KH_KERNEL': 'ellstream'}, tag='_forced')
rows('ellstream/csr', ['c5_n16_csr'], ('ramp',), 6.0, env={'KH_KERNEL': 'ellstream'}, tag='_forced_cap6', default_too=True)
rows('generic/csr', ['c5_n33_csr'], ('ramp', 'tiny'), 1.0, default_too=True)
rows('generic/csr', ['lindblad'], ('ramp', 'tiny'), 1.0, env={'KH_KERNEL': 'generic'}, tag='_forced')
for _adj in ('1', '0'):
    rows('generic', ['L2_n160', 'L5_n100'], ('ramp', 'tiny'), 1.0, env={'KH_KERNEL': 'generic', 'KH_GEN_ADJ': _adj},
         tag='_adj' + _adj, default_too=_adj == '1')
rows('generic/mixed', ['mixed_dims', 'mixed_wide'], ('ramp', 'tiny'), 1.0, default_too=True)
rows('lindblad/matrix', ['d7', 'c4_d20', 'd32_two_cops_two_controls'], ('ramp', 'tiny'), 1.0, default_too=True)
rows('mini16/wave', ['c5_n16'], ('tiny',), 1.0)
rows('mini16/wave', ['c5_n16_norms'], ('ramp',), 1.0, default_too=True)
rows('mini4/wave', ['c3'], ('tiny',), 1.0)
rows('mini4/wave', ['c3_norms'], ('ramp',), 1.0, default_too=True)

ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)

# the largest theta per sub-step the Chebyshev-form tables of a family are built for (krotov_hip.hip, plan_families)
SERIES_CAP = {'coop16/mfma': 4.0, 'ell/csr': 6.0, 'ellstream/csr': 6.0}

_problems = {}


def problem(row):
    """The regime problem of a row (cached: rows that differ in switches only share it, and its oracle sweeps)."""
    key = (row.base, row.regime, row.theta_max)
    if key not in _problems:
        fn, fmt = BASES[row.base]
        _problems[key] = hp.REGIMES[row.regime](hp.explicit(fn(), fmt), row.theta_max)
    return _problems[key]


def chi_norms(obj):
    """||chi_k|| of the update sweeps: small enough that the sequential update stays well conditioned (many objectives add
    up, many controls feed back: tests/fuzz_parity.py; ||H_1|| ~ 1e2 ... 1e3 with lambda_a = 1, 2 where the objectives share
    their operators: test_second_order_update_sweep), large enough that the update moves the pulses."""
    v = 0.3 * min(1.0, 8.0 / obj.K) * min(1.0, 4.0 / obj.L)
    if obj.fmt == 'dense' and (obj.is_super or obj.name.startswith('shared')):
        v *= 0.02
    return np.full(obj.K, v)


_references = {}


def reference(row, states=False):
    """The oracle's results of a row's problem: co-states and the update sweep (first or second order); with ``states`` the
    stored forward states too (the GPU test needs them, the witness does not)."""
    return oracle_sweeps(_references, (row.base, row.regime, row.theta_max, row.so), lambda: problem(row), row.so, states)


def oracle_sweeps(cache, key, problem_of, so, states=False):
    """``reference``'s recipe for any regime problem (``problem_of()``), cached in ``cache`` under ``key``
    (tests/test_grid_ends.py runs it on its own problems)."""
    if key in cache:
        ref = cache[key]
        if states and 'states' not in ref:
            with hp.MemoExpm():
                ref['psi_T'], ref['states'] = ko.forward_propagation(ref['prob'], problem_of().pulses, store=True)
        return ref
    obj = problem_of()
    prob = hp.regime_oracle(obj)
    norms = chi_norms(obj)
    # boundary co-states: the targets plus a random complex part (real operators between real states leave Im <chi| H_1
    # |phi> = 0 to first order, and the tiny regime has nothing beyond first order: the update would not move the pulses)
    rng = np.random.default_rng(17)
    chi_T = prob.target + 0.5 * (
        rng.standard_normal(prob.target.shape) + 1j * rng.standard_normal(prob.target.shape)) / np.sqrt(prob.N)
    if obj.fmt == 'mixed':
        for k, n in enumerate(obj.dims):
            chi_T[k, n:] = 0.0
    chi_T = chi_T / np.linalg.norm(chi_T, axis=1)[:, None]
    ref = dict(prob=prob, norms=norms, chi_T=chi_T)
    with hp.MemoExpm():
        if states:
            ref['psi_T'], ref['states'] = ko.forward_propagation(prob, obj.pulses, store=True)
        ref['chi'] = ko.backward_sweep(prob, chi_T, obj.pulses)
        kw = {}
        if so:
            rng = np.random.default_rng(5)
            older = [p * (1.0 + 0.2 * rng.standard_normal(p.shape)) for p in obj.pulses]
            ref['prev'] = ko.forward_propagation(prob, older, store=True)[1]
            ref['sigma'] = -(1.0 + rng.random(len(obj.pulses[0]))) * (1e-3 if getattr(obj, 'name', '').startswith('shared') else 1.0)
            kw = dict(sigma_vals=ref['sigma'], fw_prev=ref['prev'], store=True)
        out = ko.forward_update_sweep(prob, ref['chi'], norms, obj.pulses, obj.shapes, obj.lambdas, **kw)
    ref['opt'], ref['upd_T'], ref['g_a'] = np.array(out[0]), out[1], np.array(out[2])
    if so:
        ref['store'] = out[3]
    cache[key] = ref
    return ref


_tables = {}


def tables(family, regime):
    """Taylor, real-spectrum and defect tables; the defect (the Hermitian part of a weakly damped generator, 3e-3 as in
    tests/test_capi_symbols.py) shrinks with the operators in the tiny regime."""
    key = (SERIES_CAP.get(family, 2.0), 3e-3 * (1e-7 if regime == 'tiny' else 1.0))
    if key not in _tables:
        _tables[key] = hp.series_degree_tables(*key)
    return _tables[key]


# ---------------------------------------------------------------------------
# host: every (case, regime) pair really is in its regime
# ---------------------------------------------------------------------------
def test_table_lists_every_family_and_regime():
    want = {
        'tile64/256': set(THREE), 'tile64/stream': set(THREE), 'tile64x/512': set(THREE), 'ens64/mfma': set(THREE),
        'coop16/mfma': set(THREE) | {'long'}, 'tile128/512': {'ramp', 'tiny', 'long'}, 'tile64q2/512': {'ramp', 'long'},
        'tile64/512': {'ramp', 'tiny'}, 'ell/csr': {'ramp', 'tiny'}, 'ellstream/csr': {'ramp', 'tiny'},
        'generic/csr': {'ramp', 'tiny'}, 'generic': {'ramp', 'tiny'}, 'generic/mixed': {'ramp', 'tiny'},
        'lindblad/matrix': {'ramp', 'tiny'}, 'mini16/wave': {'ramp', 'tiny'}, 'mini4/wave': {'ramp', 'tiny'},
    }
    got = collections.defaultdict(set)
    for r in ROWS:
        got[r.family].add(r.regime)
    assert dict(got) == want
    for family in want:  # one case per family with theta_max left to the engine
        assert any(r.family == family and r.theta_arg == 0.0 for r in ROWS)


@pytest.mark.parametrize('rid', ROW_IDS)
def test_witness(rid):
    """Host only, over the very table the GPU test runs: under the guess pulses (what the plain sweeps see) and under the
    oracle's updated pulses (what the update sweep sees) the sequence theta_n of the row enters its regime -- whichever
    of the three coefficient tables the engine chose."""
    row = ROWS[ROW_IDS.index(rid)]
    obj = problem(row)
    tabs = tables(row.family, row.regime)
    ref = reference(row)
    for pulses in (obj.pulses, ref['opt']):
        theta, nsub, degrees = hp.regime_witness(obj, row.regime, row.theta_max, pulses, tabs)
    assert np.abs(ref['opt'] - np.array(obj.pulses)).max() > 1e-6  # the update sweep moves the pulses
    if row.regime == 'ramp' and (row.base.endswith('_norms') or row.base == 'mixed_dims'):
        # objectives of one launch at different degrees on the same interval
        th = hp.theta_sequence(obj)
        per_objective = np.array([hp.series_plan(th[k], row.theta_max, tabs['taylor'])[1] for k in range(obj.K)])
        assert np.any(per_objective.max(axis=0) - per_objective.min(axis=0) >= 2)


# ---------------------------------------------------------------------------
# GPU: the four sweeps of every row against the oracle
# ---------------------------------------------------------------------------
def _forced_instantiation(row, launched):
    """The forced column count of the cooperative / ensemble kernels shows in the instantiation that was launched."""
    if 'KH_COOP_COLS' in row.env:
        names = [n for n in launched if n.startswith('kh_coop_forward_update<')]
        assert names and all(n.split('<')[1].split(',')[1].strip() == row.env['KH_COOP_COLS'] for n in names), names
    if 'KH_ENS_NCG' in row.env:
        ncg = row.env['KH_ENS_NCG']
        assert any(n.startswith(('kh_ens_forward_update<%s,' % ncg, 'kh_ens2_forward_update<%s>' % ncg)) for n in launched), launched
    if row.id.split('-')[1].endswith('_ens2'):
        assert 'kh_ens2_forward_update<2>' in launched
    if row.id.split('-')[1].endswith('_ens2off'):
        assert 'kh_ens_forward_update<2, false>' in launched and 'kh_ens2_forward_update<2>' not in launched
    if row.base == 'banded_n800':  # two rows per lane of 512 threads
        assert 'kh_ell_forward_update<512, 2, 12, false, false>' in launched and 'kh_ell_sweep_store<512, 2, 12, false>' in launched, launched


@pytest.mark.gpu
@pytest.mark.parametrize('rid', ROW_IDS)
def test_matrix(rid, monkeypatch):
    """Forward sweep with storage, backward sweep, single-launch update sweep and -- where the engine offers it -- the
    per-interval form, against the oracle; the kernel family (and the forced column count) is asserted, the sweep
    covers every interval, and a ramp costs more products than its base case on the same engine shape."""
    import torch

    from krotov_amd import _lib

    row = ROWS[ROW_IDS.index(rid)]
    obj = problem(row)
    ref = reference(row, states=True)
    prob, norms = ref['prob'], ref['norms']
    for name, value in row.env.items():
        monkeypatch.setenv(name, value)
    liouville = obj.fmt == 'lindblad' or bool(np.any(obj.is_super))
    tol = 1e-11 if liouville or row.regime == 'ramp' else 1e-12
    pulses, S, lam = np.array(obj.pulses), np.array(obj.shapes), np.array(obj.lambdas)
    M = pulses.shape[1]
    _lib.forget_launched_kernels()
    eng = hp.regime_engine(obj, row.theta_arg)
    assert eng.kernel == row.family
    dev = {}
    psi_T, states = eng.forward(pulses, prob.init, store=True)
    stats = eng.stats()
    assert stats['intervals'] == M
    states = states.cpu().numpy()
    dev['states'] = np.abs(states - ref['states']).max()
    dev['psi_T'] = np.abs(psi_T.cpu().numpy() - ref['psi_T']).max()
    chi = eng.backward(ref['chi_T'], pulses)
    assert eng.stats()['intervals'] == M
    dev['chi'] = np.abs(chi.cpu().numpy() - ref['chi']).max()
    if row.so:
        store = torch.full((obj.K, M + 1, prob.N), float('nan'), dtype=torch.complex128, device=eng.device)
        eng.set_second_order(ref['prev'], store, ref['sigma'])
    opt, upd_T, g_a = eng.forward_update(chi, norms, prob.init, pulses, S, lam)
    eng.check()
    assert eng.stats()['intervals'] == M
    scale = max(1.0, np.abs(ref['opt']).max())
    ga_scale = max(1.0, np.abs(ref['g_a']).max())
    dev['opt'] = np.abs(opt.cpu().numpy() - ref['opt']).max() / scale
    dev['upd_T'] = np.abs(upd_T.cpu().numpy() - ref['upd_T']).max()
    dev['g_a'] = np.abs(g_a.cpu().numpy() - ref['g_a']).max() / ga_scale
    if row.so:
        dev['store'] = np.abs(store.cpu().numpy() - ref['store']).max()
    launched = _lib.kernel_instantiations(launched_only=True)
    if obj.fmt != 'lindblad' and not row.so:  # (Lindblad form: single launch on one GPU only)
        opt2, upd2, ga2 = eng.forward_update_sharded(chi, norms, prob.init, pulses, S, lam, lambda x: x)
        eng.check()
        dev['opt/step - opt'] = np.abs((opt2 - opt).cpu().numpy()).max() / scale
        dev['opt/step'] = np.abs(opt2.cpu().numpy() - ref['opt']).max() / scale
        dev['upd_T/step'] = np.abs(upd2.cpu().numpy() - ref['upd_T']).max()
        dev['g_a/step'] = np.abs(ga2.cpu().numpy() - ref['g_a']).max() / ga_scale
    first_bad = None
    if dev['states'] >= tol:  # the first interval beyond the tolerance and its (sub-steps, degree) from the witness
        per_n = np.abs(states - ref['states']).max(axis=(0, 2))
        n = int(np.argmax(per_n >= tol)) - 1
        theta, nsub, degrees = hp.regime_witness(obj, row.regime, row.theta_max, obj.pulses, tables(row.family, row.regime))
        first_bad = (n, float(theta[n]), int(nsub[n]), {k: int(v[n]) for k, v in degrees.items()})
    ramp_products = stats['matvecs']
    eng.close()
    print("series_regimes %s [%s]: %s%s" % (row.id, row.family, ' '.join('%s %.1e' % kv for kv in dev.items()),
                                           '' if first_bad is None else '  first interval off: %r' % (first_bad,)))
    _forced_instantiation(row, launched)
    if row.theta_arg == 0.0:
        # theta_max left to the engine: it spends what the engine given the family's documented default spends
        eng1 = hp.regime_engine(obj, row.theta_max)
        eng1.forward(pulses, prob.init, store=False)
        assert eng1.stats()['matvecs'] == ramp_products
        eng1.close()
    if row.regime == 'ramp':
        fn, fmt = BASES[row.base]
        plain = hp.explicit(fn(), fmt)
        # (a few base cases sub-step on every interval as they are -- theta 3 ... 64 for the transmon Liouvillians -- and
        # cost more than any ramp that crosses theta_max from below: their grid is shrunk uniformly to theta <= theta_max / 2,
        # the regime the rest of the suite's fixtures are pinned to, before the comparison)
        base_theta = hp.theta_sequence(plain).max()
        if base_theta > row.theta_max:
            hp._set_dt(plain, hp.regime_dt(plain) * (0.5 * row.theta_max / base_theta))
        eng0 = hp.regime_engine(plain, row.theta_arg)
        assert eng0.kernel == row.family
        eng0.forward(np.array(plain.pulses), prob.init, store=False)
        base_products = eng0.stats()['matvecs']
        eng0.close()
        assert ramp_products > base_products
    assert max(dev.values()) < tol, dev


@pytest.mark.gpu
def test_fuzz_parity_regimes_fixed_seed():
    """A fixed-seed slice of ``tests/fuzz_parity.py --regimes``: drawn problems (Lindblad-form and mixed ones among them)
    in randomly chosen regimes against the oracle."""
    import fuzz_parity

    done, failures = fuzz_parity.fuzz(3, cases=16, verbose=True, regimes=True)
    assert done == 16 and not failures, failures
