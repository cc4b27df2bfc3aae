"""The two-terms-per-phase kernels (kh_tile64q2.h) at the sizes that matter to the row-broadcast lane map
(kh_tile64.h: KhLanesR16), against the oracle.

The backward direction of ``kh_q2_sweep_store`` runs on that map; its forward direction and ``kh_q2_forward_update``
keep the previous one.  Every case runs them all, so the same cases hold for whichever map a
kernel is on.

Under this map lane i of a 16-lane DPP row holds matrix row 16 rb + i and 8 adjacent columns, a wave covers 16 rows x 32
columns and the wave pair (rb, 0), (rb, 1) the full rows; every vector in LDS is two partial vectors (one per column
half) that are added where they are read.  What can go wrong depends on where N falls against the DPP row of 16, the
column half of 32 and the zero-padded rows and columns, so every case runs at

    N in {2, 15, 16, 17, 31, 32, 33, 63, 64},  K = 3,  nt = 6 and nt = 131 grid points

(130 intervals cross the restart of the resident tiles after KH_Q2_REFRESH = 64 intervals twice), on

* ``kh_q2_sweep_store`` forward (with storage) and backward,
* the update sweep with the sums on the adjoint side, ``kh_q2_forward_update<false, true, *>`` (problem ``herm``),
* second order, ``<true, false, *>`` (``herm``),
* the sums on the forward side, ``<false, false, *>``: under KH_NO_ADJ=1 (``herm``) and by detection, with a control
  that is neither plus nor minus its adjoint (``lower``: Hermitian plus a strictly lower-triangular complex part, as in
  tests/test_nonselfadjoint_controls.py),
* Liouville space (``liouv``: ``is_super``, f real; anti-Hermitian generators, so the states stay bounded),
* each of them in the form for one GPU (``*, true>``) and, under KH_Q2_SINGLE=0, in the form that keeps the cross-GPU
  stage of the exchange (``*, false>``).  That is one rank: the two-ranks-on-one-GPU set-up of
  tests/test_hip_parity.py (``test_two_ranks_sharded_on_one_gpu[c5]``, N = 64) is not repeated here at other sizes --
  its problems are a fixed table in that file, the update kernels it exercises across ranks are unchanged, and the
  kernel on the new map, the backward sweep, runs per rank on the rank's own objectives with nothing crossing ranks.

Problems are tests/test_q2_odd_degrees.py's: Hermitian operators with ||H0|| = 1, a linear ramp as guess pulse, so that
theta = dt (1 + |eps| ||H1_k||) is known.  Regimes of the series (``herm``; the other kinds run the first):

* ``deg11_12``   theta from 0.93 to 1.07 x the table's threshold between degrees 11 and 12 (theta = 0.467 for Taylor's
                 table): every objective runs degree 11 -- the odd form, no B product in the last phase -- and then 12;
* ``one_phase``  theta across the threshold between degrees 1 and 2: one phase per step, with its extra barrier;
* ``substeps``   theta = 2.2 ... 2.4: three sub-steps per interval;
* ``odd_off``    ``deg11_12`` under KH_ODD_DEGREES=0 (degree 12 throughout).

``herm`` at nt = 6 runs all four, everything else ``deg11_12``.  Tolerances are the project's (DESIGN.md section 5,
tests/test_series_regimes.py, tests/test_q2_odd_degrees.py): 1e-12 in Hilbert space, 1e-11 in Liouville space and where
theta > 1.  The oracle's sweeps are computed once per problem and shared by the forms.

``test_lane_map_covers_the_operator_once`` (no GPU): the map as the kernels compute it (``kh_debug_q2_lane_map``) against a
NumPy restatement, and every element of the 64 x 64 operator held exactly once.
"""
import collections
import ctypes

import numpy as np
import pytest

import helpers
import test_q2_odd_degrees as tq
from krotov_amd import _lib
from oracle import krotov_oracle as ko

SIZES = (2, 15, 16, 17, 31, 32, 33, 63, 64)
GRIDS = (6, 131)  # grid points
K = 3
STORE = 'kh_q2_sweep_store'
FORM = 'kh_q2_forward_update<%s, %s, %s>'

Case = collections.namedtuple('Case', 'id kind N nt regime')


def _cases():
    out = []
    for N in SIZES:
        for nt in GRIDS:
            for kind in ('herm', 'lower', 'liouv'):
                regimes = ('deg11_12', 'one_phase', 'substeps', 'odd_off') if (kind == 'herm' and nt == 6) else ('deg11_12',)
                for regime in regimes:
                    out.append(Case('%s-n%d-nt%d-%s' % (kind, N, nt, regime), kind, N, nt, regime))
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


@pytest.fixture(scope='module')
def tabs():
    """(odd-capable thresholds, even-only thresholds) from the library's host code."""
    lib = _lib.load()
    th_o, c0, rows = (ctypes.c_double * 65)(), (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 32 * 2))()
    assert lib.kh_series_tables_odd(0.0, th_o, c0, rows) == 0
    th_e, ra = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
    assert lib.kh_series_tables(1, 0.0, th_e, ra) == 0
    return np.array(th_o), np.array(th_e)


_refs = {}


def _reference(case, tab_o):
    """The problem of (kind, N, nt, regime) -- ``odd_off`` shares ``deg11_12``'s -- and the oracle's sweeps, once."""
    regime = 'deg11_12' if case.regime == 'odd_off' else case.regime
    key = (case.kind, case.N, case.nt, regime)
    if key in _refs:
        return _refs[key]
    M = case.nt - 1
    dt = {'deg11_12': 0.93 * tab_o[11], 'one_phase': 0.93 * tab_o[1], 'substeps': 2.2}[regime]
    scales = (0.09, 0.07, 0.05) if regime == 'substeps' else tq.SCALES
    if case.kind == 'lower':
        # (a non-normal control lets the states grow: a tenth of the norm keeps e^(||G|| T) below 3 over 130 intervals)
        scales = tuple(0.1 * s for s in scales)
    p = tq._problem(case.N, M, K, dt, False, scales, seed=100 + case.N)
    is_super = case.kind == 'liouv'
    if case.kind == 'lower':
        rng = np.random.default_rng(5)
        ops = [[h0, helpers.nonselfadjoint_variant('lower', h1, rng)] for h0, h1 in p.ops]
    elif is_super:
        ops = [[-1j * h0, -1j * h1] for h0, h1 in p.ops]
    else:
        ops = p.ops
    if ops is not p.ops:
        tlist = np.concatenate([[0.0], np.cumsum(p.dt)])
        p = p._replace(ops=ops, prob=ko.OracleProblem(ops, p.init, p.prob.target, tlist, is_super=is_super))
    ref = {'p': p, 'is_super': is_super}
    ref['psi_T'], ref['states'] = ko.forward_propagation(p.prob, p.pulses, store=True)
    ref['chi'] = ko.backward_sweep(p.prob, p.chi_T, p.pulses)
    out = ko.forward_update_sweep(p.prob, ref['chi'], p.norms, p.pulses, p.shapes, p.lambdas)
    ref['opt'], ref['upd_T'], ref['g_a'] = np.array(out[0]), out[1], np.array(out[2])
    if case.kind != 'lower':
        rng = np.random.default_rng(5)
        older = [q * (1.0 + 0.2 * rng.standard_normal(q.shape)) for q in p.pulses]
        ref['prev'] = ko.forward_propagation(p.prob, older, store=True)[1]
        ref['sigma'] = -(1.0 + rng.random(M))
        out = ko.forward_update_sweep(p.prob, ref['chi'], p.norms, p.pulses, p.shapes, p.lambdas, sigma_vals=ref['sigma'],
                                      fw_prev=ref['prev'], store=True)
        ref['so_opt'], ref['so_T'], ref['so_g_a'], ref['so_store'] = np.array(out[0]), out[1], np.array(out[2]), out[3]
    _refs[key] = ref
    return ref


def _engine(ref):
    from krotov_amd.engine import HipKrotovEngine

    eng = HipKrotovEngine(ref['p'].ops, ref['p'].dt, is_super=ref['is_super'])
    assert eng.kernel == 'tile64q2/512'
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize('cid', CASE_IDS)
def test_q2_row_broadcast_sweeps(cid, tabs, monkeypatch):
    import torch

    case = CASES[CASE_IDS.index(cid)]
    tab_o, tab_e = tabs
    ref = _reference(case, tab_o)
    p = ref['p']
    pulses, S, lam = np.array(p.pulses), np.array(p.shapes), np.array(p.lambdas)
    M = case.nt - 1
    tol = 1e-11 if (case.kind == 'liouv' or case.regime == 'substeps') else 1e-12
    monkeypatch.setenv('KH_KERNEL', 'q2')  # (small N would otherwise go to the one-wave kernels)
    if case.regime == 'odd_off':
        monkeypatch.setenv('KH_ODD_DEGREES', '0')
    dev = {}
    want_forms = set()
    _lib.forget_launched_kernels()

    def update(eng, tag, so):
        if so:
            store = torch.full((K, M + 1, case.N), float('nan'), dtype=torch.complex128, device=eng.device)
            eng.set_second_order(ref['prev'], store, ref['sigma'])
        got = eng.forward_update(chi, p.norms, p.init, pulses, S, lam)
        eng.check()
        assert eng.stats()['intervals'] == M
        if so:
            dev.update(tq._update_devs(got, ref['so_opt'], ref['so_T'], ref['so_g_a'], tag))
            dev[tag + 'store'] = np.abs(store.cpu().numpy() - ref['so_store']).max()
            eng.set_second_order()
        else:
            dev.update(tq._update_devs(got, ref['opt'], ref['upd_T'], ref['g_a'], tag))
        return got

    # ---- plain sweeps and the update sweep in the form the engine picks ----
    eng = _engine(ref)
    psi_T, states = eng.forward(pulses, p.init, store=True)
    assert eng.stats()['intervals'] == M
    if case.kind == 'herm':
        # the witness: the degrees the regime is about, and the products they cost
        odd = case.regime != 'odd_off'
        want, deg, nsub = tq._products(eng.op_norms, p.dt, pulses[0], tab_o if odd else tab_e, odd)
        assert eng.stats()['matvecs'] == want
        degrees = {'deg11_12': {11, 12}, 'one_phase': {1, 2}, 'substeps': {13}, 'odd_off': {12}}[case.regime]
        assert set(np.unique(deg)) == degrees, deg
        assert nsub.min() == nsub.max() == (3 if case.regime == 'substeps' else 1)
    dev['states'] = np.abs(states.cpu().numpy() - ref['states']).max()
    dev['psi_T'] = np.abs(psi_T.cpu().numpy() - ref['psi_T']).max()
    chi = eng.backward(p.chi_T, pulses)
    dev['chi'] = np.abs(chi.cpu().numpy() - ref['chi']).max()
    first = update(eng, 'upd/', False)
    if case.kind == 'herm':
        want_forms.add(FORM % ('false', 'true', 'true'))
    elif case.kind == 'lower':
        want_forms.add(FORM % ('false', 'false', 'true'))
        assert np.abs(first[0].cpu().numpy() - pulses).max() > 1e-6  # the update sweep moves the pulse
    if case.kind != 'lower':
        update(eng, 'so/', True)
        want_forms.add(FORM % ('true', 'false', 'true'))
    eng.close()
    # ---- the form that keeps the cross-GPU stage of the exchange ----
    monkeypatch.setenv('KH_Q2_SINGLE', '0')
    eng = _engine(ref)
    update(eng, 'x/upd/', False)
    if case.kind != 'lower':
        update(eng, 'x/so/', True)
        want_forms.add(FORM % ('true', 'false', 'false'))
    if case.kind == 'herm':
        want_forms.add(FORM % ('false', 'true', 'false'))
    elif case.kind == 'lower':
        want_forms.add(FORM % ('false', 'false', 'false'))
    eng.close()
    # ---- a self-adjoint control with the sums on the forward side ----
    if case.kind == 'herm':
        monkeypatch.setenv('KH_NO_ADJ', '1')
        eng = _engine(ref)
        update(eng, 'x/fwd/', False)
        eng.close()
        monkeypatch.setenv('KH_Q2_SINGLE', '1')
        eng = _engine(ref)
        update(eng, 'fwd/', False)
        eng.close()
        want_forms |= {FORM % ('false', 'false', 'false'), FORM % ('false', 'false', 'true')}
    launched = _lib.kernel_instantiations(launched_only=True)
    print('q2_dpp_broadcast %s: %s' % (case.id, ' '.join('%s %.1e' % kv for kv in dev.items())))
    assert STORE in launched, launched
    for name in want_forms:
        assert name in launched, (name, launched)
    assert any(n.startswith('kh_q2_forward_update<') and n.endswith('false>') for n in launched), launched
    assert not any(n.startswith(('kh_tile_', 'kh_mini_', 'kh_quad_')) for n in launched), launched
    assert max(dev.values()) < tol, dev


# ---------------------------------------------------------------------------
# host: the lane map
# ---------------------------------------------------------------------------
def _map_restated(wave, lane):
    """KhLanesR16 in words: wave = (row block rb, column half); lane = 16 d + i, i the row inside the block, d the
    block of 8 columns inside the half.  v_mfma_f64_4x4x4 with a constant B operand adds its A operand over the lanes
    16 k + i and leaves the sum for i = 4 blk + r4 on lanes 16 r4 + 4 blk + (0 .. 3)."""
    rb, half, d, i = wave // 2, wave % 2, lane // 16, lane % 16
    blk, r4 = (lane // 4) % 4, lane // 16  # of an OUTPUT lane
    return dict(row_in=16 * rb + i, col0=8 * (d + 4 * half), x_index=8 * (d + 4 * half) + i % 8,
                landing_lane=16 * (i % 4) + 4 * (i // 4), row_out=16 * rb + 4 * blk + r4, writer=int(lane % 4 == 0), half=half)


def test_lane_map_covers_the_operator_once():
    lib = _lib.load()
    out = (ctypes.c_int32 * 7)()
    assert lib.kh_debug_q2_lane_map(8, 0, out) == -1 and lib.kh_debug_q2_lane_map(0, 64, out) == -1 and lib.kh_debug_q2_lane_map(-1, 0, out) == -1
    held = np.zeros((64, 64), dtype=int)
    written = np.zeros((2, 64), dtype=int)
    names = ('row_in', 'col0', 'x_index', 'landing_lane', 'row_out', 'writer', 'half')
    maps = {}
    for wave in range(8):
        for lane in range(64):
            assert lib.kh_debug_q2_lane_map(wave, lane, out) == 0
            got = dict(zip(names, list(out)))
            assert got == _map_restated(wave, lane), (wave, lane, got)
            maps[wave, lane] = got
            held[got['row_in'], got['col0']:got['col0'] + 8] += 1
            if got['writer']:
                written[got['half'], got['row_out']] += 1
    assert np.all(held == 1)     # all 64 x 64 elements, each exactly once
    assert np.all(written == 1)  # every row of either partial vector has one writer
    for (wave, lane), m in maps.items():
        # the element a lane fetches is the one product j = lane % 8 of its DPP row needs: column col0 + j
        assert m['x_index'] == m['col0'] + lane % 8 and m['col0'] // 32 == m['half']
        # the four lanes 16 k + i of a wave hold the same row; its sum lands on a writer lane that knows the row
        assert {maps[wave, 16 * k + lane % 16]['row_in'] for k in range(4)} == {m['row_in']}
        land = maps[wave, m['landing_lane']]
        assert land['writer'] == 1 and land['row_out'] == m['row_in']
        for c in range(4):  # (the sum is replicated over four lanes)
            assert maps[wave, m['landing_lane'] + c]['row_out'] == m['row_in']
