"""Every kernel family at the ends of its interval pipeline, against the oracle.

Every sweep kernel is a software pipeline over the time grid: while interval n is worked on, the co-state row, the pulse
value, the step width and (in some families) the operator tiles of interval n + 1 are in flight, switched by guards of the
form ``n + 1 < nt - 1``; the advanced generators of ``kh_q2_*``, ``kh_tn_*`` and ``kh_coop_*`` restart every 64 intervals
(the update sweeps at absolute indices, the backward sweeps in windows counted from the end); the adjoint-side pre-passes
cut the co-state store into 16-, 64- and 256-point tiles under ``n < nt`` masks; ``forward_update_sharded`` replays a graph
of ``graph_chunk`` intervals and relies on "calls past the last interval are no-ops".  The fixtures of the rest of the suite
use 11 ... 400 intervals, none of them at such an end.  This module runs the base cases of tests/test_series_regimes.py's
families, built with nt = I + 1, at

* SHORT  I = 1, 2, 3    (I = 1: the prologue is the epilogue, every look-ahead guard is false from the start),
* BLOCK  I = 63, 64, 65 (a restart window with 63 intervals, exactly one window, a window that holds a single interval;
                         nt = 64, 65, 66 are also the 64-point edges of the pre-passes),
* PRE    I = 256        (nt = 257: one valid point in the pre-pass's second block in time),

with interval values of its own (``helpers.grid_ends``: the fixtures' update shapes and guess pulses vanish at both ends,
which on three intervals is everywhere -- the update sweep would be a no-op), proves on the host that the oracle's update
moves the pulse on the first and on the last interval of every (row, I) (``test_witness``: no GPU), and compares the sweeps
with ``oracle/krotov_oracle.py`` on the GPU (``test_matrix``, ``test_replicas``), the kernel family and the launched
instantiations asserted.  Further: the graph replay of the per-interval form at I = 2 chunk, 2 chunk + 1, 2 chunk + 2;
engines without controls (L = 0); a fixed-seed slice of ``tests/fuzz_parity.py --short-grids``.

Tolerances are the project's: 1e-12 in Hilbert space, 1e-11 in Liouville space; pulses and g_a
relative to max(1, scale).  ||chi_k||, lambda_a and chi_k(T) follow tests/test_series_regimes.py (``chi_norms``,
``oracle_sweeps``).
"""
import collections
import re
import warnings

import numpy as np
import pytest

import helpers as hp
import test_series_regimes as tsr
from krotov_amd import configs
from oracle import krotov_oracle as ko

SHORT, BLOCK, PRE = (1, 2, 3), (63, 64, 65), (256,)

# want / forbid: regular expressions over the launched instantiations (each ``want`` must match one, no ``forbid`` any)
End = collections.namedtuple('End', 'id family base fmt theta_max env so lengths want forbid split')

BASES = {}  # name: (builder(nt), fmt)
ROWS = []


def _c5(**kw):
    return lambda nt: configs.config_c5(nt=nt, **kw)


def _lindblad_d7(nt):
    import test_lindblad_form as tlf

    case = tlf._random(7, 3, 1, 1, nt, 1)
    case.lambdas = [0.7 + 0.3 * l for l in range(case.L)]
    case.pulses = tlf._pulses(case)  # (replaced by helpers.grid_ends)
    case.shapes = [np.ones(len(case.dt)) for _ in range(case.L)]
    return case


for _name, _fn, _fmt in [
    ('c3', lambda nt: configs.config_c3(nt=nt), 'dense'),
    ('c5_n16', _c5(K=6, N=16), 'dense'),
    ('c5_n33', _c5(K=5, N=33), 'dense'),
    ('c5_n24_L4', _c5(K=4, N=24, L=4, distinct=True), 'dense'),
    ('c5_n64_L2', _c5(K=4, N=64, L=2, distinct=True), 'dense'),
    ('c5_k300', _c5(K=300, N=16, distinct=True), 'dense'),
    ('c5_k600', _c5(K=600, N=8, distinct=True), 'dense'),
    ('L6_n20', _c5(K=5, N=20, L=6, distinct=True), 'dense'),
    ('k40_n64', _c5(K=40, N=64), 'dense'),
    ('k37_n33', _c5(K=37, N=33), 'dense'),
    ('shared_n96', lambda nt: configs.config_shared(K=8, N=96, nt=nt, L=1), 'dense'),
    ('shared_n96_L2', lambda nt: configs.config_shared(K=20, N=96, nt=nt, L=2), 'dense'),
    ('c4_d9', lambda nt: configs.config_c4(d=9, nt=nt, n_logical=2), 'dense'),
    ('c5_n80_L2', _c5(K=3, N=80, L=2), 'dense'),
    ('c5_n100', _c5(K=4, N=100, L=1, distinct=True), 'dense'),
    ('c5_n96', _c5(K=2, N=96, L=1), 'dense'),
    ('L2_n20', _c5(K=3, N=20, L=2, distinct=True), 'dense'),
    ('L2_n160', _c5(K=2, N=160, L=2, distinct=True), 'dense'),
    ('c5_n33_csr', _c5(K=5, N=33), 'csr'),
    ('c5_n16_csr', _c5(K=6, N=16), 'csr'),
    ('lindblad_d12', lambda nt: tsr._coherent(configs.config_sparse_lindblad(d=12, nt=nt), 12), 'csr'),
    ('banded_n600', lambda nt: tsr._banded(600, 21, nt=nt, K=2), 'csr'),
    ('mixed_dims', lambda nt: configs.config_mixed('dims', nt=nt), 'mixed'),
    ('d7', _lindblad_d7, 'lindblad'),
]:
    BASES[_name] = (_fn, _fmt)


def rows(family, base, lengths, want, theta_max=1.0, env=None, tag='', so=False, forbid=(), split=None):
    rid = '%s-%s%s' % (family, base, tag)
    ROWS.append(End(rid, family, base, BASES[base][1], theta_max, dict(env or {}), so, tuple(lengths), tuple(want), tuple(forbid),
                    split))


_ADJ, _STEP1 = r'kh_gen_adjoint_side$', r'kh_tile_forward_update<1, 1, false, false>$'
rows('mini4/wave', 'c3', SHORT, [r'kh_quad_sweep_store$', r'kh_quad_forward_update<false>$'])
rows('mini16/wave', 'c5_n16', SHORT, [r'kh_mini_sweep_store$', r'kh_mini_forward_update<false>$'])
# two terms per phase: <second order, sums on the adjoint side, single GPU>; the generator is advanced, restart every 64
_Q2 = 'c5_n33'
rows('tile64q2/512', _Q2, SHORT + BLOCK, [r'kh_q2_sweep_store$', r'kh_q2_forward_update<false, true, true>$', _STEP1])
rows('tile64q2/512', _Q2, SHORT + BLOCK, [r'kh_q2_sweep_store$', r'kh_q2_forward_update<false, false, true>$'],
     env={'KH_NO_ADJ': '1'}, tag='_noadj', forbid=[r'kh_q2_forward_update<false, true, '])
rows('tile64q2/512', _Q2, SHORT + BLOCK, [r'kh_q2_sweep_store$', r'kh_q2_forward_update<false, (true|false), true>$'],
     env={'KH_TAYLOR': '1'}, tag='_taylor')
rows('tile64q2/512', _Q2, SHORT + BLOCK, [r'kh_q2_sweep_store$', r'kh_q2_forward_update<true, false, true>$'], tag='_so', so=True)
# one term per phase: <rows per thread, controls, second order, single GPU>
rows('tile64/512', 'c5_n24_L4', SHORT, [r'kh_tile_sweep_store<1, 4>$', r'kh_tile_forward_update<1, 4, false, true>$',
                                        r'kh_tile_forward_update<1, 4, false, false>$'])
rows('tile64/512', 'c5_n24_L4', SHORT, [r'kh_tile_sweep_store<1, 4>$', r'kh_tile_forward_update<1, 4, true, true>$'], tag='_so',
     so=True)
rows('tile64/512', 'c5_n64_L2', SHORT, [r'kh_tile_sweep_store<1, 2>$', r'kh_tile_forward_update<1, 2, false, true>$'])
# (its plain sweeps run kh_q2_sweep_store with objectives in turns)
rows('tile64/256', 'c5_k300', SHORT + (64, 65), [r'kh_q2_sweep_store$', r'kh_tile_forward_update<2, 1, false, true>$'])
rows('tile64/stream', 'c5_k600', SHORT + (65,), [r'kh_stream_forward_update<1, false, false>$'])
rows('tile64x/512', 'L6_n20', SHORT + (63, 64) + PRE, [r'kh_tx_sweep_store<6>$', r'kh_tx_forward_update<6>$', _ADJ])
rows('ens64/mfma', 'k40_n64', SHORT, [r'kh_ens_forward_update<1, false>$'], env={'KH_ENS': '1', 'KH_ENS_NCG': '1'}, tag='_cg1')
rows('ens64/mfma', 'k37_n33', SHORT + PRE, [r'kh_ens2_forward_update<2>$', _ADJ], env={'KH_ENS': '1', 'KH_ENS_NCG': '2'},
     tag='_ens2')
# cooperative kernels: <slots, objectives per workgroup, second order, sums on the adjoint side, A^2 chain, cross-GPU stage>
_COOP = r'kh_coop_forward_update<8, %s, %s, %s, %s, \w+>$'
_CADJ = r'kh_coop_adjoint_side$'
rows('coop16/mfma', 'shared_n96', SHORT + BLOCK + PRE, [r'kh_coop_sweep_store<', _COOP % (r'\d+', 'false', 'true', 'true'), _CADJ],
     theta_max=4.0)
rows('coop16/mfma', 'shared_n96', SHORT + BLOCK, [_COOP % (r'\d+', 'false', 'false', 'false')], theta_max=4.0,
     env={'KH_COOP_NOSQ': '1'}, tag='_nosq', forbid=[_CADJ, _COOP % (r'\d+', 'false', r'\w+', 'true')])
rows('coop16/mfma', 'shared_n96', SHORT + BLOCK, [r'kh_coop_sweep_store<8, 16, ', _COOP % ('16', 'false', 'true', 'true'), _CADJ],
     theta_max=4.0, env={'KH_COOP_COLS': '16'}, tag='_cols16')
rows('coop16/mfma', 'shared_n96', SHORT + BLOCK, [_COOP % (r'\d+', 'false', 'false', 'true')], theta_max=4.0,
     env={'KH_COOP_NO_ADJ': '1'}, tag='_noadj', forbid=[_CADJ])
rows('coop16/mfma', 'shared_n96', SHORT + BLOCK, [_COOP % (r'\d+', 'true', 'false', 'true')], theta_max=4.0, tag='_so', so=True,
     forbid=[_CADJ])
rows('coop16/mfma', 'shared_n96_L2', SHORT, [r'kh_coop_sweep_store<', _COOP % (r'\d+', 'false', 'false', 'false')], theta_max=4.0)
rows('coop16/mfma', 'c4_d9', SHORT, [r'kh_coop_sweep_store<', r'kh_coop_forward_update<'], theta_max=4.0)
# the generator in registers: <elements per lane, second order, H1 in registers>
rows('tile128/512', 'c5_n80_L2', SHORT + BLOCK + PRE, [r'kh_tn_sweep_store<20, false>$', r'kh_tn_forward_update<20, false, false>$',
                                                       _ADJ])
rows('tile128/512', 'c5_n100', SHORT + BLOCK, [r'kh_tn_sweep_store<28, false>$', r'kh_tn_forward_update<28, false, false>$'])
rows('tile128/512', 'c5_n96', SHORT + BLOCK, [r'kh_tn_sweep_store<24, true>$', r'kh_tn_forward_update<24, false, true>$'])
_GEN = [r'kh_gen_sweep_store<false>$', r'kh_gen_forward_update<false>$']
rows('generic', 'L2_n20', SHORT + (63, 64) + PRE, _GEN + [_ADJ], env={'KH_KERNEL': 'generic', 'KH_GEN_ADJ': '1'}, tag='_adj1')
rows('generic', 'L2_n20', SHORT + (63, 64) + PRE, _GEN, env={'KH_KERNEL': 'generic', 'KH_GEN_ADJ': '0'}, tag='_adj0', forbid=[_ADJ])
rows('generic', 'L2_n20', SHORT + (63, 64) + PRE, _GEN, env={'KH_KERNEL': 'generic'}, tag='_so', so=True, forbid=[_ADJ])
rows('generic', 'L2_n160', SHORT, _GEN)  # (the generator in the global scratch matrix)
rows('generic/csr', 'c5_n33_csr', SHORT, _GEN)
for _base in ('lindblad_d12', 'c5_n16_csr'):
    rows('ell/csr', _base, SHORT, [r'kh_ell_sweep_store<\d+, \d+, \d+, false>$', r'kh_ell_forward_update<\d+, \d+, \d+, false, false>$'],
         theta_max=4.0)
    rows('ellstream/csr', _base, SHORT, [r'kh_ell_sweep_store<\d+, \d+, \d+, true>$',
                                         r'kh_ell_forward_update<\d+, \d+, \d+, false, true>$'],
         theta_max=4.0, env={'KH_KERNEL': 'ellstream'}, tag='_forced')
rows('ellglobal/csr', 'banded_n600', SHORT, [r'kh_ellg_sweep_store<512>$', r'kh_ellg_forward_update<512, false>$'], theta_max=4.0,
     env={'KH_KERNEL': 'ellglobal'}, tag='_forced')
rows('ellglobal/csr', 'banded_n600', SHORT, [r'kh_ellg_sweep_store<512>$', r'kh_ellg_forward_update<512, true>$'], theta_max=4.0,
     env={'KH_KERNEL': 'ellglobal'}, tag='_forced_so', so=True)
for _s in (2, 3):
    rows('ellsplit/csr', 'banded_n600', SHORT, [r'kh_ellgs_sweep_store<512>$', r'kh_ellgs_forward_update<512, false>$'],
         theta_max=4.0, env={'KH_KERNEL': 'ellsplit', 'KH_ELL_SPLIT': str(_s)}, tag='_forced_s%d' % _s, split=_s)
rows('generic/mixed', 'mixed_dims', SHORT, [r'kh_gen_sweep_store<true>$', r'kh_gen_forward_update<true>$'])
rows('lindblad/matrix', 'd7', SHORT, [r'kh_lind_sweep_store<1>$', r'kh_lind_forward_update<1>$'])

ROW_OF = {r.id: r for r in ROWS}
assert len(ROW_OF) == len(ROWS)
CASES = [(r.id, I) for r in ROWS for I in r.lengths]
CASE_IDS = ['%s-I%d' % c for c in CASES]

_problems, _references = {}, {}


def problem(row, I):
    """The ``grid_ends`` problem of a row on I intervals (cached: rows that differ in switches only share it)."""
    key = (row.base, I, row.theta_max)
    if key not in _problems:
        fn, fmt = BASES[row.base]
        _problems[key] = hp.grid_ends(hp.explicit(fn(I + 1), fmt), row.theta_max)
    return _problems[key]


def reference(row, I, states=False):
    return tsr.oracle_sweeps(_references, (row.base, I, row.theta_max, row.so), lambda: problem(row, I), row.so, states)


def tolerance(obj):
    return 1e-11 if obj.fmt == 'lindblad' or bool(np.any(obj.is_super)) else 1e-12


# ---------------------------------------------------------------------------
# host
# ---------------------------------------------------------------------------
def test_table_lists_every_family_and_length():
    families = {r.family for r in tsr.ROWS} | {'ellglobal/csr', 'ellsplit/csr'}
    got = collections.defaultdict(set)
    for r in ROWS:
        got[r.family] |= set(r.lengths)
    assert set(got) == families
    for family, lengths in got.items():
        assert set(SHORT) <= lengths, family
    for family in ('tile64q2/512', 'coop16/mfma', 'tile128/512'):  # an advanced generator: every edge of a restart window
        assert set(BLOCK) <= got[family], family
    for family in ('tile64x/512', 'ens64/mfma', 'coop16/mfma', 'tile128/512', 'generic'):  # an adjoint-side store
        assert set(PRE) <= got[family], family
        assert any(set(PRE) <= set(r.lengths) and any('adjoint_side' in w for w in r.want) for r in ROWS if r.family == family)
    assert {'63', '64'} <= {str(I) for r in ROWS if r.family in ('tile64x/512', 'generic') for I in r.lengths}
    assert {64, 65} <= got['tile64/256'] and 65 in got['tile64/stream']
    for r in ROWS:
        assert r.want, r.id  # every row names the instantiations it is there for
        if set(PRE) <= set(r.lengths):
            assert any('adjoint_side' in w for w in r.want) or r.so or r.env.get('KH_GEN_ADJ') == '0', r.id
    assert {r.split for r in ROWS if r.family == 'ellsplit/csr'} == {2, 3}
    assert any(r.so for r in ROWS if r.family in ('tile64q2/512', 'tile64/512', 'coop16/mfma', 'generic', 'ellglobal/csr'))


@pytest.mark.parametrize('cid', CASE_IDS)
def test_witness(cid):
    """Host only, over the very table the GPU test runs: the input conditions hold (no update shape is zero, the guess
    differs between intervals and controls and is non-zero at both ends, the grid is non-uniform, one sub-step on the short
    grids, decades of |eps| inside a restart window on the long ones), and under the oracle the update moves the pulse by
    more than 1e-6 on the first and on the last interval."""
    rid, I = CASES[CASE_IDS.index(cid)]
    row = ROW_OF[rid]
    obj = problem(row, I)
    assert len(hp.regime_dt(obj)) == I and len(obj.tlist) == I + 1
    hp.grid_ends_witness(obj, row.theta_max)
    ref = reference(row, I)
    move = np.abs(ref['opt'] - np.array(obj.pulses)).max(axis=0)
    print('grid_ends witness %s: pulse change on the first / last interval %.1e / %.1e' % (cid, move[0], move[-1]))
    assert move[0] > 1e-6 and move[-1] > 1e-6, (move[0], move[-1])
    assert np.allclose(np.linalg.norm(ref['chi_T'], axis=1), 1.0)


# ---------------------------------------------------------------------------
# GPU: the sweeps of every (row, I) against the oracle
# ---------------------------------------------------------------------------
def _nans(shape, dtype, device):
    import torch

    fill = complex(float('nan'), float('nan')) if dtype == torch.complex128 else float('nan')
    return torch.full(tuple(shape), fill, dtype=dtype, device=device)


def _check_launched(row, launched, cid):
    for want in row.want:
        assert any(re.match(want, n) for n in launched), (cid, want, sorted(launched))
    for forbid in row.forbid:
        assert not any(re.match(forbid, n) for n in launched), (cid, forbid, sorted(launched))


DEVIATIONS = {}  # row id: largest deviation over its lengths (printed for DESIGN.md)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', CASE_IDS)
def test_matrix(cid, monkeypatch):
    """Forward sweep with and without storage (psi_T bit for bit the same), backward sweep (its last slice bit for bit
    chi_T), single-launch update sweep into NaN-filled tensors (second order: the stored trajectory too, slice 0 bit for
    bit the initial states) and -- where the family offers it -- one launch per interval, against the oracle."""
    import torch

    from krotov_amd import _lib

    rid, I = CASES[CASE_IDS.index(cid)]
    row = ROW_OF[rid]
    obj = problem(row, I)
    ref = reference(row, I, states=True)
    prob, norms = ref['prob'], ref['norms']
    for name, value in row.env.items():
        monkeypatch.setenv(name, value)
    tol = tolerance(obj)
    pulses, S, lam = np.array(obj.pulses), np.array(obj.shapes), np.array(obj.lambdas)
    assert pulses.shape[1] == I
    _lib.forget_launched_kernels()
    eng = hp.regime_engine(obj, row.theta_max)
    try:
        assert eng.kernel == row.family and eng.nt == I + 1
        if row.split:
            assert eng.row_split == row.split
        c128, f64, dv = torch.complex128, torch.float64, eng.device
        dev = {}
        psi_T, states = eng.forward(pulses, prob.init, store=True,
                                    out=(_nans((obj.K, prob.N), c128, dv), _nans((obj.K, I + 1, prob.N), c128, dv)))
        assert eng.stats()['intervals'] == I
        plain_T = eng.forward(pulses, prob.init, store=False, out=_nans((obj.K, prob.N), c128, dv))
        assert eng.stats()['intervals'] == I
        assert torch.equal(plain_T, psi_T), 'psi_T with and without storage'
        dev['states'] = np.abs(states.cpu().numpy() - ref['states']).max()
        dev['psi_T'] = np.abs(psi_T.cpu().numpy() - ref['psi_T']).max()
        chi = eng.backward(ref['chi_T'], pulses, out=_nans((obj.K, I + 1, prob.N), c128, dv))
        assert eng.stats()['intervals'] == I
        chi_host = chi.cpu().numpy()
        assert np.array_equal(chi_host[:, I], ref['chi_T']), 'chi[:, nt - 1] is chi_T'
        dev['chi'] = np.abs(chi_host - ref['chi']).max()
        if row.so:
            store = _nans((obj.K, I + 1, prob.N), c128, dv)
            eng.set_second_order(ref['prev'], store, ref['sigma'])
        opt, upd_T, g_a = eng.forward_update(chi, norms, prob.init, pulses, S, lam,
                                             out=(_nans((obj.L, I), f64, dv), _nans((obj.K, prob.N), c128, dv),
                                                  _nans((obj.L,), f64, dv)))
        eng.check()
        assert eng.stats()['intervals'] == I
        scale = max(1.0, np.abs(ref['opt']).max())
        ga_scale = max(1.0, np.abs(ref['g_a']).max())
        dev['opt'] = np.abs(opt.cpu().numpy() - ref['opt']).max() / scale
        dev['upd_T'] = np.abs(upd_T.cpu().numpy() - ref['upd_T']).max()
        dev['g_a'] = np.abs(g_a.cpu().numpy() - ref['g_a']).max() / ga_scale
        if row.so:
            store_host = store.cpu().numpy()
            assert np.array_equal(store_host[:, 0], np.asarray(prob.init, dtype=np.complex128)), 'slice 0 is init'
            dev['store'] = np.abs(store_host - ref['store']).max()
        if obj.fmt != 'lindblad' and not row.so:  # (Lindblad form: single launch only; second order: as its neighbours)
            opt2, upd2, ga2 = eng.forward_update_sharded(chi, norms, prob.init, pulses, S, lam, lambda x: x, graph_chunk=0)
            eng.check()
            dev['opt/step'] = np.abs(opt2.cpu().numpy() - ref['opt']).max() / scale
            dev['upd_T/step'] = np.abs(upd2.cpu().numpy() - ref['upd_T']).max()
            dev['g_a/step'] = np.abs(ga2.cpu().numpy() - ref['g_a']).max() / ga_scale
        launched = sorted(_lib.kernel_instantiations(launched_only=True))
    finally:
        eng.close()
    worst = max(dev.values())
    DEVIATIONS[rid] = max(DEVIATIONS.get(rid, 0.0), worst) if np.isfinite(worst) else float('nan')
    print('grid_ends %s [%s]: %s; row so far %.1e; launched: %s' % (cid, row.family, ' '.join('%s %.1e' % kv for kv in dev.items()),
                                                                   DEVIATIONS[rid], ', '.join(launched)))
    _check_launched(row, launched, cid)
    assert np.isfinite(worst) and worst < tol, dev


# ---------------------------------------------------------------------------
# GPU: replica engines (tests/test_replicas.py's two-control batch, every replica its own step widths)
# ---------------------------------------------------------------------------
_replica_batches = {}


def replica_batch(I):
    import test_replicas as tr

    if I not in _replica_batches:
        reps = []
        for b in range(4):
            r = hp.grid_ends(tr._replica(tr._c5(b, 2, 7, I + 1, L=2, seed0=20), b), 1.0)
            r.chi_norms = tsr.chi_norms(r)
            reps.append(r)
        _replica_batches[I] = reps
    return _replica_batches[I]


def replica_reference(I, b, so):
    """tests/test_series_regimes.py's recipe on replica ``b``."""
    r = replica_batch(I)[b]
    r.fmt = 'dense'
    return tsr.oracle_sweeps(_references, ('replica', b, I, so), lambda: r, so, states=True)


REPLICA_CASES = [(so, I) for so in (False, True) for I in SHORT]
REPLICA_IDS = ['%s-I%d' % ('second' if so else 'first', I) for so, I in REPLICA_CASES]


@pytest.mark.parametrize('cid', REPLICA_IDS)
def test_replica_witness(cid):
    so, I = REPLICA_CASES[REPLICA_IDS.index(cid)]
    reps = replica_batch(I)
    dts = np.array([np.diff(r.tlist) for r in reps])
    assert len({tuple(d.tolist()) for d in dts}) == len(reps)  # every replica its own step widths
    for b, r in enumerate(reps):
        hp.grid_ends_witness(r, 1.0)
        ref = replica_reference(I, b, so)
        move = np.abs(ref['opt'] - np.array(r.pulses)).max(axis=0)
        assert move[0] > 1e-6 and move[-1] > 1e-6, (b, move)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', REPLICA_IDS)
def test_replicas(cid):
    import torch

    import test_replicas as tr
    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    so, I = REPLICA_CASES[REPLICA_IDS.index(cid)]
    reps = replica_batch(I)
    refs = [replica_reference(I, b, so) for b in range(len(reps))]
    a = tr._inputs(reps)
    a['chi_T'] = np.concatenate([ref['chi_T'] for ref in refs])
    nB, Kr, N, L = len(reps), reps[0].K, reps[0].N, reps[0].L
    _lib.load()
    _lib.forget_launched_kernels()
    eng = HipKrotovEngine(a['ops'], a['dt'], is_super=False, replicas=nB, theta_max=1.0)
    try:
        assert eng.kernel == 'replica16/wave' and eng.nt == I + 1
        c128, f64, dv = torch.complex128, torch.float64, eng.device
        psi_T, states = eng.forward(a['pulses'], a['init'], store=True,
                                    out=(_nans((nB * Kr, N), c128, dv), _nans((nB * Kr, I + 1, N), c128, dv)))
        assert eng.stats()['intervals'] == I
        plain_T = eng.forward(a['pulses'], a['init'], out=_nans((nB * Kr, N), c128, dv))
        assert torch.equal(plain_T, psi_T)
        chi = eng.backward(a['chi_T'], a['pulses'], out=_nans((nB * Kr, I + 1, N), c128, dv))
        assert eng.stats()['intervals'] == I
        if so:
            store = _nans((nB * Kr, I + 1, N), c128, dv)
            eng.set_second_order_replicas(np.concatenate([ref['prev'] for ref in refs]), store,
                                          np.array([ref['sigma'] for ref in refs]))
        opt, upd_T, g_a = eng.forward_update(chi, a['chi_norms'], a['init'], a['pulses'], a['shapes'], a['lambdas'],
                                             out=(_nans((nB, L, I), f64, dv), _nans((nB * Kr, N), c128, dv), _nans((nB, L), f64, dv)))
        eng.check()
        assert eng.stats()['intervals'] == I
        launched = sorted(_lib.kernel_instantiations(launched_only=True))
        got = dict(states=states, psi_T=psi_T, chi=chi, opt=opt, upd_T=upd_T, g_a=g_a)
        if so:
            got['store'] = store
        got = {k: v.cpu().numpy() for k, v in got.items()}
    finally:
        eng.close()
    assert np.array_equal(got['chi'][:, I], a['chi_T'])
    if so:
        assert np.array_equal(got['store'][:, 0], a['init'])
    worst = 0.0
    for b, ref in enumerate(refs):
        rws = slice(b * Kr, (b + 1) * Kr)
        dev = {'states': np.abs(got['states'][rws] - ref['states']).max(), 'psi_T': np.abs(got['psi_T'][rws] - ref['psi_T']).max(),
               'chi': np.abs(got['chi'][rws] - ref['chi']).max(),
               'opt': np.abs(got['opt'][b] - ref['opt']).max() / max(1.0, np.abs(ref['opt']).max()),
               'upd_T': np.abs(got['upd_T'][rws] - ref['upd_T']).max(),
               'g_a': np.abs(got['g_a'][b] - ref['g_a']).max() / max(1.0, np.abs(ref['g_a']).max())}
        if so:
            dev['store'] = np.abs(got['store'][rws] - ref['store']).max()
        print('grid_ends replica16/wave %s replica %d: %s' % (cid, b, ' '.join('%s %.1e' % kv for kv in dev.items())))
        worst = max(worst, max(dev.values()))
        assert max(dev.values()) < 1e-12, (b, dev)
    print('grid_ends replica16/wave %s: largest deviation %.1e; launched: %s' % (cid, worst, ', '.join(launched)))
    for want in ('kh_rep_sweep_store<2>', 'kh_rep_forward_update_so<2>' if so else 'kh_rep_forward_update<2>'):
        assert want in launched, (want, launched)


# ---------------------------------------------------------------------------
# GPU: the ends of the graph replay of the per-interval form
# ---------------------------------------------------------------------------
GRAPH_CHUNK = 4
BASES['graph_q2_n17'] = (_c5(K=5, N=17, distinct=True), 'dense')
BASES['graph_generic'] = (_c5(K=4, N=33, distinct=True), 'dense')
GRAPH_ROWS = {
    'q2_n17': End('graph-q2_n17', 'tile64q2/512', 'graph_q2_n17', 'dense', 1.0, {}, False, (8, 9, 10), [_STEP1], (), None),
    'generic': End('graph-generic', 'generic', 'graph_generic', 'dense', 1.0, {'KH_KERNEL': 'generic'}, False, (8, 9, 10),
                   [r'kh_gen_forward_update<false>$', _ADJ], (), None),
    'mixed': End('graph-mixed', 'generic/mixed', 'mixed_dims', 'mixed', 1.0, {}, False, (8, 9, 10),
                 [r'kh_gen_forward_update<true>$'], (), None),
}
GRAPH_IDS = ['%s-I%d' % (name, I) for name in sorted(GRAPH_ROWS) for I in (8, 9, 10)]


def test_graph_rows_are_those_of_the_reuse_module():
    import test_engine_reuse as ter

    assert sorted(GRAPH_ROWS) == sorted(ter.GRAPH_CASES) and GRAPH_CHUNK == ter.GRAPH_CHUNK
    for name, g in ter.GRAPH_CASES.items():
        assert GRAPH_ROWS[name].family == g.kernel and GRAPH_ROWS[name].env == g.env
        for I in GRAPH_ROWS[name].lengths:
            obj = problem(GRAPH_ROWS[name], I)
            hp.grid_ends_witness(obj, 1.0)
            ref = reference(GRAPH_ROWS[name], I)
            move = np.abs(ref['opt'] - np.array(obj.pulses)).max(axis=0)
            assert move[0] > 1e-6 and move[-1] > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('cid', GRAPH_IDS)
def test_graph_replay_ends(cid, monkeypatch):
    """I = 2 chunk: the plain loop (no graph); I = 2 chunk + 1: nt - 2 = 8, two replays and no launch behind the last
    interval; I = 2 chunk + 2: three replays, three no-op launches.  Each against the oracle and, bit for bit, against the
    ``graph_chunk=0`` run; a failed capture (which falls back with a warning) is an error here."""
    from krotov_amd import _lib

    name, I = cid.rsplit('-I', 1)
    row, I = GRAPH_ROWS[name], int(I)
    obj = problem(row, I)
    ref = reference(row, I)
    for key, value in row.env.items():
        monkeypatch.setenv(key, value)
    pulses, S, lam = np.array(obj.pulses), np.array(obj.shapes), np.array(obj.lambdas)
    _lib.forget_launched_kernels()
    eng = hp.regime_engine(obj, row.theta_max)
    try:
        assert eng.kernel == row.family
        chi = eng.backward(ref['chi_T'], pulses)
        args = (chi, ref['norms'], ref['prob'].init, pulses, S, lam, lambda x: x)
        plain = [x.cpu().numpy() for x in eng.forward_update_sharded(*args, graph_chunk=0)]
        eng.check()
        assert eng._sh['graph'] is None
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            got = [x.cpu().numpy() for x in eng.forward_update_sharded(*args, graph_chunk=GRAPH_CHUNK)]
        eng.check()
        if I == 2 * GRAPH_CHUNK:
            assert eng._sh['graph'] is None
        else:
            assert eng._sh['graph'] is not None and eng._sh['graph_key'] == (chi.data_ptr(), GRAPH_CHUNK)
        launched = sorted(_lib.kernel_instantiations(launched_only=True))
    finally:
        eng.close()
    scale, ga_scale = max(1.0, np.abs(ref['opt']).max()), max(1.0, np.abs(ref['g_a']).max())
    dev = {'opt': np.abs(got[0] - ref['opt']).max() / scale, 'upd_T': np.abs(got[1] - ref['upd_T']).max(),
           'g_a': np.abs(got[2] - ref['g_a']).max() / ga_scale}
    print('grid_ends graph %s: %s; launched: %s' % (cid, ' '.join('%s %.1e' % kv for kv in dev.items()), ', '.join(launched)))
    _check_launched(row, launched, cid)
    for x, y, what in zip(got, plain, ('opt', 'psi_T', 'g_a')):
        assert np.array_equal(x, y), what
    assert max(dev.values()) < tolerance(obj), dev


# ---------------------------------------------------------------------------
# engines without controls (L = 0): plain sweeps only
# ---------------------------------------------------------------------------
def _no_controls(name, I):
    """(ops, c_ops, dt, oracle problem, is_super) of an L = 0 engine on I non-uniform intervals."""
    import scipy.sparse as sp
    import test_lindblad_form as tlf

    rng = np.random.default_rng(11)
    dense = {'n5': (3, 5), 'n64': (2, 64), 'n100': (2, 100), 'n160': (2, 160)}

    def states(K, N):
        x = rng.standard_normal((2, K, N)) + 1j * rng.standard_normal((2, K, N))
        x /= np.linalg.norm(x, axis=2)[:, :, None]
        return x[0], x[1]

    c_ops, is_super = None, False
    if name in dense:
        K, N = dense[name]
        ops = [[configs.herm(rng, N, 1.0)] for _ in range(K)]
        init, target = states(K, N)
        prob_ops = ops
    elif name == 'shared_n96':
        K, N = 8, 96
        H0 = configs.herm(rng, N, 1.0)
        ops = prob_ops = [[H0]] * K
        init, target = states(K, N)
    elif name == 'csr':
        spec = configs.config_sparse_lindblad(d=5, nt=I + 1, K=3)
        K, N, is_super = spec.K, spec.N, spec.is_super
        prob_ops = [[spec.H0[k]] for k in range(K)]
        ops = [[sp.csr_matrix(spec.H0[k])] for k in range(K)]
        init, target = spec.init, spec.target
    elif name == 'lindblad':
        case = tlf._random(5, 2, 0, 1, I + 1, 3)
        assert case.L == 0 and all(len(c) == 1 for c in case.C)
        ops, c_ops, is_super = case.H, case.C, True
        full = case.oracle()
        K, N, prob_ops, init, target = case.K, full.N, full.ops, full.init, full.target
    else:
        raise KeyError(name)
    norm = max(np.linalg.norm(np.asarray(row[0]), 2) for row in prob_ops)
    dt = 0.5 * np.resize([1.0, 0.6, 0.85, 0.55, 0.7], I) / norm  # theta <= 0.5: one sub-step
    tlist = np.concatenate([[0.0], np.cumsum(dt)])
    prob = ko.OracleProblem([list(row) for row in prob_ops], np.array(init), np.array(target), tlist, is_super)
    return ops, c_ops, dt, prob, is_super


NO_CONTROL_ENGINES = ('n5', 'n64', 'n100', 'n160', 'shared_n96', 'csr', 'lindblad')
NO_CONTROL_IDS = ['%s-I%d' % (name, I) for name in NO_CONTROL_ENGINES for I in (1, 12)]


def test_header_states_the_contract_without_controls():
    import os

    header = open(os.path.join(os.path.dirname(hp.GOLDEN), os.pardir, 'include', 'krotov_hip.h')).read()
    text = re.sub(r'[\s*/]+', ' ', header)
    assert ('L = 0 (no controls) is accepted by every constructor except kh_engine_create_replicas (KH_ERR_UNSUPPORTED'
            in text)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', NO_CONTROL_IDS)
def test_no_controls(cid):
    """L = 0 is accepted by the C ABI: forward sweep with storage and backward sweep against the oracle; the update sweeps
    and the parametrization answer KH_ERR_INVALID."""
    import ctypes

    import torch

    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    name, I = cid.rsplit('-I', 1)
    I = int(I)
    ops, c_ops, dt, prob, is_super = _no_controls(name, I)
    with hp.MemoExpm():
        ref_T, ref_states = ko.forward_propagation(prob, [], store=True)
        chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
        ref_chi = ko.backward_sweep(prob, chi_T, [])
    kw = dict(c_ops=c_ops) if c_ops is not None else dict(is_super=is_super)
    eng = HipKrotovEngine(ops, dt, **kw)
    try:
        assert eng.L == 0 and eng.nt == I + 1
        none = np.zeros((0, I))
        psi_T, states = eng.forward(none, prob.init, store=True)
        assert eng.stats()['intervals'] == I
        assert torch.equal(eng.forward(none, prob.init), psi_T)
        chi = eng.backward(chi_T, none)
        assert eng.stats()['intervals'] == I
        eng.check()
        dev = {'states': np.abs(states.cpu().numpy() - ref_states).max(), 'psi_T': np.abs(psi_T.cpu().numpy() - ref_T).max(),
               'chi': np.abs(chi.cpu().numpy() - ref_chi).max()}
        print('grid_ends no controls %s [%s]: %s' % (cid, eng.kernel, ' '.join('%s %.1e' % kv for kv in dev.items())))
        assert np.array_equal(chi.cpu().numpy()[:, I], chi_T)
        assert max(dev.values()) < (1e-11 if is_super else 1e-12), dev
        if name in ('n5', 'n64', 'n100', 'n160'):
            lib, h = eng._lib, eng._handle
            one = torch.zeros(max(1, I), dtype=torch.float64, device=eng.device)  # (non-NULL stand-ins: the refusal is about L)
            other = torch.zeros(max(1, I), dtype=torch.float64, device=eng.device)
            p, q, st = one.data_ptr(), other.data_ptr(), eng._stream()
            norms = torch.ones(eng.K, dtype=torch.float64, device=eng.device)
            init = eng._c(prob.init, (eng.K, eng.N))
            out_T = torch.empty_like(init)
            assert lib.kh_forward_update(h, chi.data_ptr(), norms.data_ptr(), init.data_ptr(), p, p, p, q, out_T.data_ptr(), q,
                                         st) == _lib.KH_ERR_INVALID
            assert b'no controls' in lib.kh_last_error()
            assert lib.kh_update_begin(h, chi.data_ptr(), norms.data_ptr(), init.data_ptr(), p, q, q, q, st) == _lib.KH_ERR_INVALID
            assert b'no controls' in lib.kh_last_error()
            kind = (ctypes.c_int32 * 1)(0)
            ab = (ctypes.c_double * 1)(0.0)
            assert lib.kh_set_parametrization(h, kind, ab, ab, p, p, q) == _lib.KH_ERR_INVALID
            assert b'no controls' in lib.kh_last_error()
            eng.check()
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_replica_engine_refuses_no_controls():
    """The one constructor that refuses L = 0 (include/krotov_hip.h): KH_ERR_UNSUPPORTED, no engine."""
    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    rng = np.random.default_rng(3)
    ops = [[configs.herm(rng, 5, 1.0)] for _ in range(4)]
    with pytest.raises(_lib.KrotovHipError) as err:
        HipKrotovEngine(ops, np.full(3, 0.1), replicas=2)
    assert err.value.code == _lib.KH_ERR_UNSUPPORTED and '1..4 controls' in str(err.value)


# ---------------------------------------------------------------------------
# GPU: a fixed-seed slice of tests/fuzz_parity.py --short-grids
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_fuzz_parity_short_grids_fixed_seed():
    import fuzz_parity

    done, failures = fuzz_parity.fuzz(5, cases=16, verbose=True, short_grids=True)
    assert done == 16 and not failures, failures
