"""``kh_chi_local_invariants`` (krotov_amd/csrc/kh_chi_li.h) along the suite's axes, and the batch route around it.

1. Grid and dimension edges (GPU): more gates than one workgroup holds (``blockIdx.x > 0``, wave 3, a ragged last
   workgroup), N around the steps of the kernel's three loops (4 per lane group, 64 per wave), per-gate Bell bases and
   invariants on a dense engine, replica engines with one and with two gates per replica under the active mask, and the
   degenerate scalars (scale 0, w = 1, a NaN in one gate) -- against the host constructor at ``TOL``, as
   ``test_kernel_vs_host_constructor`` does.
2. A conditioning ladder U_B = Q1 diag(1, 1, 1, delta) Q2 down to delta = 4e-10 against a 60-digit reference
   (tests/golden/li_conditioning.npz, make_li_conditioning_goldens.py): per rung the kernel's error is at most 8 x that of
   the host constructor -- the other double-precision implementation -- on the same inputs; and both fall on the same
   side a factor 4 either way of the singular threshold.
3. ``optimize_pulses_batch``: ``.values`` over one batch, sub-batches and the sequential loop, early stops under the
   mask, on the oracle-backed doubles and end to end on the device with B = 9.

Every GPU case has a host-only witness here that shows its inputs do what the case claims."""
import functools
import logging
import os
import sys

import numpy as np
import pytest

import helpers
import test_local_invariants as tli
from test_local_invariants import (  # noqa: F401  (li_double: a fixture)
    E2E_BOUND, MODES, TOL, WEIGHTS, _case, _engine, bell_of, constructor, deviations, frame, li_double, noisy_gate,
    oracle_run, product_problem, product_sigma, states_of)

LI_WAVES = 4  # KH_LI_WAVES: gates per workgroup


def _show(line):
    print(line)


# ---------------------------------------------------------------------------
# 1. grid and dimension edges
# ---------------------------------------------------------------------------
GATE_COUNTS = (4, 5, 8, 9, 67)  # one full workgroup; ragged; two full; ragged; 17 workgroups, the last one ragged
DIMENSIONS = (4, 5, 7, 63, 64, 65, 128, 129, 200)

# name: (kind, M gates, N, B replicas or 0, per-gate Bell bases and invariants)
AXES_CASES = {}
for _N in (4, 9):
    for _M in GATE_COUNTS:
        AXES_CASES['uniform_M%d_N%d' % (_M, _N)] = ('uniform', _M, _N, 0, False)
for _N in DIMENSIONS:
    AXES_CASES['dense_M5_N%d' % _N] = ('dense', 5, _N, 0, False)
AXES_CASES['dense_M5_N9'] = ('dense', 5, 9, 0, False)  # (the degenerate scalars run on this one)
AXES_CASES['dense_M5_N9_per_gate'] = ('dense', 5, 9, 0, True)
AXES_CASES['replica_B9_Kr4_N4'] = ('dense', 9, 4, 9, False)
AXES_CASES['replica_B9_Kr4_N16'] = ('dense', 9, 16, 9, False)
AXES_CASES['replica_B3_Kr8_N9'] = ('dense', 6, 9, 3, False)
RAGGED = {name for name, c in AXES_CASES.items() if c[1] % LI_WAVES != 0}


@functools.lru_cache(maxsize=None)
def _built(name):
    """``_case`` of an ``AXES_CASES`` entry, once per session (read only)."""
    kind, M, N, B, per_gate = AXES_CASES[name]
    return _case(N, M, per_gate, seed=sum(map(ord, name)))


def _scale(name):
    kind, M, N, B, per_gate = AXES_CASES[name]
    return 1.0 if B else 1.0 / M


def _U_of(psi, bell, g):
    """U_B[i, k] = <B_i|phi_k> of gate g."""
    rows = bell[g] if bell.ndim == 3 else bell
    return rows.conj() @ psi[4 * g:4 * g + 4].T


def _run(eng, case, mode, w, scale, **kw):
    psi, bell, ref, inv = case
    return [x.cpu().numpy() for x in eng.chi_local_invariants(psi, bell, mode, inv, w, scale, **kw)]


def _against_host(name, eng, case, scale):
    """Every mode and weight against the host constructor at TOL; {(mode, w): (chi, norms, J)}."""
    ref = case[2]
    got, worst = {}, 0.0
    for mode in MODES:
        for w in WEIGHTS:
            chi, norms, J = got[mode, w] = _run(eng, case, mode, w, scale)
            want_chi, want_J = ref(mode, w, scale)
            errs = dict(chi=np.abs(chi * norms[:, None] - want_chi).max(), J=np.abs(J - want_J).max(),
                        norm=np.abs(np.linalg.norm(chi, axis=1) - 1).max())
            worst = max(worst, *errs.values())
            assert all(err < TOL for err in errs.values()), (name, mode, w, errs)
    _show("%s: largest deviation from the host constructor %.2e" % (name, worst))
    return got


@pytest.mark.parametrize('name', sorted(AXES_CASES))
def test_witness_the_cases_reach_the_edges_they_claim(name):
    """Host: whole gates, the workgroups / waves / loop steps a case is there for, well-conditioned inputs."""
    kind, M, N, B, per_gate = AXES_CASES[name]
    psi, bell, ref, inv = _built(name)
    K = psi.shape[0]
    assert K == 4 * M and K % 4 == 0 and psi.shape == (K, N)
    workgroups = -(-M // LI_WAVES)
    assert (name in RAGGED) == (M % LI_WAVES != 0) == (workgroups * LI_WAVES > M)
    assert M >= LI_WAVES  # (wave 3 runs)
    if name.startswith('uniform_M'):
        assert workgroups == {4: 1, 5: 2, 8: 2, 9: 3, 67: 17}[M] and K <= 268
    if name.startswith('dense_M5'):
        assert workgroups == 2 and M - LI_WAVES == 1  # blockIdx.x = 1 holds one gate, three waves leave at once
    if B:
        assert M % B == 0 and (M // B, K // B) in ((1, 4), (2, 8)) and N <= 16
    assert bell.shape == ((M, 4, N) if per_gate else (4, N)) and inv.shape == ((M, 3) if per_gate else (3,))
    for g in range(M):
        rows = bell[g] if per_gate else bell
        assert np.abs(rows.conj() @ rows.T - np.eye(4)).max() < 1e-13
        assert 0.3 < abs(np.linalg.det(_U_of(psi, bell, g))) < 3.0  # ("noisy gates": TOL is an absolute tolerance)
    if per_gate:  # CNOT, sqrt(iSWAP), CZ in turns: the invariants differ from gate to gate
        assert np.abs(inv[0] - inv[1]).max() > 0.1 and np.abs(inv[3] - inv[0]).max() < 1e-15


def test_witness_dimensions_sit_on_the_loop_steps():
    """The kernel's inner products step by 4 per lane group, its norm and row loops by 64 per wave: N on, one below and
    one above a multiple of each, one pass and several."""
    steps64 = {N: -(-N // 64) for N in DIMENSIONS}
    assert steps64 == {4: 1, 5: 1, 7: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 3, 200: 4}
    assert {N % 4 for N in DIMENSIONS} == {0, 1, 3} and {N % 64 for N in (63, 64, 65, 128, 129)} == {63, 0, 1}


def _unit_weight_closed_form(psi, bell, scale):
    """w = 1: chi_k = (scale / 4) sum_i U[i][k] B_i and J = 1 - ||U_B||_F^2 / 4, from the inner products alone."""
    M = psi.shape[0] // 4
    chi, J = [], []
    for g in range(M):
        U = _U_of(psi, bell, g)
        chi.append((scale / 4.0) * (U.T @ (bell[g] if bell.ndim == 3 else bell)))
        J.append(1.0 - np.sum(np.abs(U) ** 2) / 4.0)
    return np.concatenate(chi), np.array(J)


@pytest.mark.parametrize('N', DIMENSIONS)
def test_witness_host_constructor_has_the_unit_weight_closed_form(N):
    name = 'dense_M5_N%d' % N
    psi, bell, ref, inv = _built(name)
    for mode in MODES:
        chi, J = ref(mode, 1.0, _scale(name))
        want_chi, want_J = _unit_weight_closed_form(psi, bell, _scale(name))
        assert np.abs(chi - want_chi).max() < TOL and np.abs(J - want_J).max() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize('N', (4, 9))
@pytest.mark.parametrize('M', GATE_COUNTS)
def test_gate_counts_beyond_one_workgroup(M, N):
    """M = 4 ... 67 gates (K up to 268) on a dense engine of shared operator objects; no sweep is launched.  At M = 9
    every gate's chi, norms and J are, bit for bit, those of that gate alone on an M = 1 engine."""
    name = 'uniform_M%d_N%d' % (M, N)
    case, scale = _built(name), _scale(name)
    eng = _engine('uniform', 4 * M, N)
    try:
        got = _against_host(name, eng, case, scale)
    finally:
        eng.close()
    if M != 9:
        return
    psi, bell, ref, inv = case
    solo = _engine('uniform', 4, N)
    try:
        for (mode, w), (chi, norms, J) in got.items():
            for g in range(M):
                rows = slice(4 * g, 4 * g + 4)
                one = [x.cpu().numpy() for x in solo.chi_local_invariants(psi[rows], bell, mode, inv, w, scale)]
                assert np.array_equal(one[0], chi[rows]) and np.array_equal(one[1], norms[rows]) and one[2][0] == J[g], (
                    mode, w, g)
    finally:
        solo.close()


@pytest.mark.gpu
@pytest.mark.parametrize('N', DIMENSIONS)
def test_dimensions_around_the_loop_steps(N):
    name = 'dense_M5_N%d' % N
    eng = _engine('dense', 20, N)
    try:
        _against_host(name, eng, _built(name), _scale(name))
    finally:
        eng.close()


@pytest.mark.gpu
def test_per_gate_bell_bases_and_invariants_on_a_dense_engine():
    name = 'dense_M5_N9_per_gate'
    eng = _engine('dense', 20, 9)
    try:
        _against_host(name, eng, _built(name), _scale(name))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['replica_B9_Kr4_N4', 'replica_B9_Kr4_N16', 'replica_B3_Kr8_N9'])
def test_replica_engines_beyond_one_workgroup_and_one_gate(name):
    kind, M, N, B, per_gate = AXES_CASES[name]
    eng = _engine(kind, 4 * M, N, B)
    try:
        assert eng.K // eng.replicas == 4 * M // B
        _against_host(name, eng, _built(name), _scale(name))
    finally:
        eng.close()


MASK, FILL = [1, 0, 1], (7.25 - 3j, -7.25)


def test_witness_the_mask_case_has_two_gates_per_replica():
    kind, M, N, B, per_gate = AXES_CASES['replica_B3_Kr8_N9']
    assert (M // B, 4 * M // B) == (2, 8) and len(MASK) == B and MASK[1] == 0
    # gates 2 and 3 (rows 8..15) are replica 1's: active[gate / gates_per_replica] with gates_per_replica = 2
    assert [g // (M // B) for g in range(M)] == [0, 0, 1, 1, 2, 2]
    # no result of the unmasked call is the fill value: an unchanged slice shows that nothing wrote it
    for mode in MODES:
        chi, J = _built('replica_B3_Kr8_N9')[2](mode, 0.3, 1.0)
        assert not np.any(chi == FILL[0]) and not np.any(J == FILL[1])


@pytest.mark.gpu
def test_two_gates_per_replica_under_the_mask():
    """B = 3, K_r = 8, mask [1, 0, 1] into pre-filled ``out=`` tensors: replica 1's 8 rows, 8 norms and 2 J entries keep
    the fill values bit for bit, the other replicas equal the unmasked call bit for bit."""
    import torch

    name = 'replica_B3_Kr8_N9'
    case = _built(name)
    eng = _engine('dense', 24, 9, B=3)
    try:
        for mode in MODES:
            full = _run(eng, case, mode, 0.3, 1.0)
            eng.set_active_replicas(MASK)
            out = (torch.full((24, 9), FILL[0], dtype=torch.complex128, device='cuda'),
                   torch.full((24,), FILL[1], dtype=torch.float64, device='cuda'),
                   torch.full((6,), FILL[1], dtype=torch.float64, device='cuda'))
            got = _run(eng, case, mode, 0.3, 1.0, out=out)
            eng.set_active_replicas(None)
            assert np.all(got[0][8:16] == FILL[0]) and np.all(got[1][8:16] == FILL[1]) and np.all(got[2][2:4] == FILL[1])
            for rows, gates in ((slice(0, 8), slice(0, 2)), (slice(16, 24), slice(4, 6))):
                assert np.array_equal(got[0][rows], full[0][rows]) and np.array_equal(got[1][rows], full[1][rows])
                assert np.array_equal(got[2][gates], full[2][gates])
            _show("%s %s mask %s: replica 1 untouched, replicas 0 and 2 bitwise the unmasked call" % (name, mode, MASK))
    finally:
        eng.close()


DEGENERATE = 'dense_M5_N9'
NAN_GATE, NAN_AT = 2, (4 * 2 + 1, 3)  # gate 2 of 5: component 3 of its state 1


def _nan_case():
    psi, bell, ref, inv = _built(DEGENERATE)
    bad = psi.copy()
    bad[NAN_AT] = complex(float('nan'), 0.0)
    return bad, bell, ref, inv


def test_witness_degenerate_scalars_on_the_host():
    """scale = 0 leaves the host's J what it is and its co-states zero; a NaN component makes that gate -- and no other
    -- singular for the host constructor."""
    psi, bell, ref, inv = _built(DEGENERATE)
    for mode in MODES:
        chi0, J0 = ref(mode, 0.3, 0.0)
        assert not chi0.any() and np.array_equal(J0, ref(mode, 0.3, 1.0)[1]) and np.isfinite(J0).all()
    bad = _nan_case()[0]
    assert np.isnan(bad).sum() == 1 and NAN_AT[0] // 4 == NAN_GATE
    basis = frame(None, 9)
    for mode in MODES:
        for g in range(5):
            con = constructor(mode, basis, 0.3)
            if g == NAN_GATE:
                with pytest.raises(ValueError, match='linearly dependent'):
                    con(list(bad[4 * g:4 * g + 4]), None, None)
            else:
                con(list(bad[4 * g:4 * g + 4]), None, None)


@pytest.mark.gpu
def test_degenerate_scalars():
    """scale = 0, w = 1 and one NaN component in gate 2 of 5.  (scale and w belong to the call, not to a gate: for them
    "unchanged" is the J of the call -- which does not depend on scale -- and a plain call before and after.)"""
    case = _built(DEGENERATE)
    psi, bell, ref, inv = case
    scale = _scale(DEGENERATE)
    eng = _engine('dense', 20, 9)
    try:
        for mode in MODES:
            plain = _run(eng, case, mode, 0.3, scale)
            # scale = 0
            chi, norms, J = _run(eng, case, mode, 0.3, 0.0)
            assert not chi.any() and not norms.any() and np.isfinite(J).all() and not np.isnan(chi).any()
            assert np.array_equal(J, plain[2]) and np.abs(J - ref(mode, 0.3, 0.0)[1]).max() < TOL
            # w = 1: the closed form from the inner products
            chi, norms, J = _run(eng, case, mode, 1.0, scale)
            want_chi, want_J = _unit_weight_closed_form(psi, bell, scale)
            errs = (np.abs(chi * norms[:, None] - want_chi).max(), np.abs(J - want_J).max())
            _show("%s %s w=1 against the closed form: chi %.2e, J %.2e" % (DEGENERATE, mode, *errs))
            assert max(errs) < TOL
            # a NaN component in gate 2
            chi, norms, J = _run(eng, _nan_case(), mode, 0.3, scale)
            rows = slice(4 * NAN_GATE, 4 * NAN_GATE + 4)
            assert np.isnan(J[NAN_GATE]) and not chi[rows].any() and not norms[rows].any()
            others = np.ones(20, dtype=bool)
            others[rows] = False
            assert np.array_equal(chi[others], plain[0][others]) and np.array_equal(norms[others], plain[1][others])
            assert np.array_equal(np.delete(J, NAN_GATE), np.delete(plain[2], NAN_GATE))
            # nothing stays behind in the engine
            assert all(np.array_equal(a, b) for a, b in zip(_run(eng, case, mode, 0.3, scale), plain))
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 2. conditioning ladder against the extended-precision reference
# ---------------------------------------------------------------------------
MARGIN = 8.0  # the kernel's error against the host constructor's on the same rung
# The host constructor's error per rung as measured before the device ran (worst of a rung's draws): it grows like
# 2^-53 / delta.  The rungs 1e-1 and 1e-3 were not in that measurement: 1.4e-16 / delta, the trend of their neighbours.
HOST_TABLE = {1.0: 5.7e-16, 1e-1: 1.4e-15, 1e-2: 1.4e-14, 1e-3: 1.4e-13, 1e-4: 1.4e-12, 1e-6: 1.7e-10, 1e-8: 1.7e-8,
              4e-10: 6.0e-7}


@functools.lru_cache(maxsize=None)
def _goldens():
    data = np.load(os.path.join(helpers.GOLDEN, 'li_conditioning.npz'))
    return {key: data[key] for key in data.files}


def _maker():
    if helpers.GOLDEN not in sys.path:
        sys.path.insert(0, helpers.GOLDEN)
    import make_li_conditioning_goldens

    return make_li_conditioning_goldens


def _measure(D, J, D_ref, J_ref):
    return max(np.abs(D - D_ref).max() / max(1.0, np.abs(D_ref).max()), abs(J - J_ref) / max(1.0, abs(J_ref)))


@functools.lru_cache(maxsize=None)
def _host_ladder_errors():
    """Per rung the largest error of ``_li_gate_terms`` over the rung's draws, modes and weights."""
    from krotov_amd import functionals

    g = _goldens()
    target = tli.restated_target(tli.CNOT)
    errors = []
    for r in range(len(g['deltas'])):
        worst = 0.0
        for j in range(g['psi'].shape[1]):
            U_B = g['bell'].conj() @ g['psi'][r, j].T
            for m in range(2):
                for iw, w in enumerate(g['weights']):
                    J, D = functionals._li_gate_terms(U_B, m, target, float(w))
                    worst = max(worst, _measure(D, J, g['D'][r, j, m, iw], g['J'][r, j, m, iw]))
        errors.append(worst)
    return tuple(errors)


def test_conditioning_goldens_are_what_the_script_computes():
    """The committed file against a fresh 60-digit computation (where mpmath imports): the inputs of the recipe, and J
    and D from the committed inputs to 1e-15 relative."""
    pytest.importorskip('mpmath')
    mk, g = _maker(), _goldens()
    assert tuple(g['deltas']) == mk.DELTAS == tuple(sorted(HOST_TABLE, reverse=True)) and tuple(g['weights']) == WEIGHTS
    assert g['psi'].shape == (8, 6, 4, 9) and mk.DIGITS == 60
    psi, bell = mk.inputs()
    assert np.abs(psi - g['psi']).max() < 1e-13 and np.abs(bell - g['bell']).max() < 1e-13
    fresh = mk.compute(g['psi'], g['bell'])
    for key in ('J', 'D'):
        for r in range(8):
            for j in range(6):
                assert np.abs(fresh[key][r, j] - g[key][r, j]).max() <= 1e-15 * np.abs(g[key][r, j]).max(), (key, r, j)


def test_witness_ladder_inputs_and_host_error():
    """The inputs are what the ladder says -- singular values 1, 1, 1, delta to the rounding of the embedding -- and
    the host constructor's error per rung is within 4 x the figures measured for it before: that pins the inputs."""
    g = _goldens()
    assert np.abs(g['bell'].conj() @ g['bell'].T - np.eye(4)).max() < 1e-15
    for r, delta in enumerate(g['deltas']):
        for j in range(6):
            sv = np.linalg.svd(g['bell'].conj() @ g['psi'][r, j].T, compute_uv=False)
            assert np.abs(sv[:3] - 1).max() < 1e-14 and abs(sv[3] - delta) < 4e-15
    for delta, err in zip(g['deltas'], _host_ladder_errors()):
        _show("delta %-7.0e host constructor %.2e (measured before: %.1e)" % (delta, err, HOST_TABLE[float(delta)]))
        assert err <= 4 * HOST_TABLE[float(delta)], (delta, err)


@pytest.mark.gpu
def test_conditioning_ladder_kernel_against_host_constructor():
    """Per rung: the kernel's error against the 60-digit reference is at most 8 x the host constructor's.  D of the
    device is chi x norms mapped back through the Bell rows: D[i][k] = -<B_i|chi_k> (scale 1).

    Measured on an MI355X (DESIGN.md section 5 has the table): the ratio stays between 0.50 and 1.75, without a trend
    in 1 / delta."""
    g = _goldens()
    G_O, g3_O = tli.restated_target(tli.CNOT)
    bell, inv = g['bell'], np.array([G_O.real, G_O.imag, g3_O])
    host = _host_ladder_errors()
    eng = _engine('dense', 24, 9)
    rows = []
    try:
        for r, delta in enumerate(g['deltas']):
            psi = g['psi'][r].reshape(24, 9)
            worst = 0.0
            for m, mode in enumerate(MODES):
                for iw, w in enumerate(g['weights']):
                    chi, norms, J = (x.cpu().numpy() for x in eng.chi_local_invariants(psi, bell, mode, inv, float(w), 1.0))
                    assert np.isfinite(J).all() and norms.all()
                    for j in range(6):
                        D = -(bell.conj() @ (chi[4 * j:4 * j + 4] * norms[4 * j:4 * j + 4, None]).T)
                        worst = max(worst, _measure(D, J[j], g['D'][r, j, m, iw], g['J'][r, j, m, iw]))
            rows.append((float(delta), host[r], worst))
            _show("delta %-7.0e host %.2e  kernel %.2e  ratio %.2f" % (delta, host[r], worst, worst / host[r]))
    finally:
        eng.close()
    assert len(rows) == 8
    failed = [row for row in rows if not row[2] <= MARGIN * row[1]]
    assert not failed, failed


THRESHOLD_DRAWS = 3


def _threshold_delta():
    """|det Q| = 1: |det U_B| = delta and ||U_B||_F^2 = 3 + delta^2, so the singular test flips at
    delta* = LI_SINGULAR_RTOL ((3 + delta^2) / 4)^2 (delta^2 ~ 1e-21 does not reach the last bit of 3)."""
    from krotov_amd import functionals

    return functionals.LI_SINGULAR_RTOL * (3.0 / 4.0) ** 2


def _threshold_states(factor):
    """(24, 9) states of ``THRESHOLD_DRAWS`` gates at delta = factor x delta*, padded with well-conditioned gates."""
    mk = _maker()
    rng = np.random.default_rng(int(1000 * factor))
    basis = frame(rng, 9)
    gates = [mk.rank_losing_gate(rng, factor * _threshold_delta()) for _ in range(THRESHOLD_DRAWS)]
    gates += [noisy_gate(rng) for _ in range(6 - THRESHOLD_DRAWS)]
    return np.concatenate([states_of(rng, basis, U) for U in gates]), bell_of(basis)


def test_witness_threshold_points_fall_on_their_sides():
    """A factor 4 above the threshold the host constructor answers, a factor 4 below it raises: the determinant's
    rounding (1e-16 against 1e-11) cannot flip either."""
    from krotov_amd import functionals

    assert abs(_threshold_delta() - 5.625e-11) < 1e-24
    basis = frame(None, 9)
    for factor, singular in ((4.0, False), (0.25, True)):
        psi, bell = _threshold_states(factor)
        for g in range(THRESHOLD_DRAWS):
            U_B = bell.conj() @ psi[4 * g:4 * g + 4].T
            limit = functionals.LI_SINGULAR_RTOL * (np.sum(np.abs(U_B) ** 2) / 4.0) ** 2
            assert abs(abs(np.linalg.det(U_B)) / limit - factor) < 1e-3 * factor
            for mode in MODES:
                con = constructor(mode, basis, 0.3)
                if singular:
                    with pytest.raises(ValueError, match='linearly dependent'):
                        con(list(psi[4 * g:4 * g + 4]), None, None)
                else:
                    chis = np.array(con(list(psi[4 * g:4 * g + 4]), None, None))
                    assert np.isfinite(con.values).all() and np.isfinite(chis).all() and chis.any(axis=1).all()


@pytest.mark.gpu
def test_device_and_host_fall_on_the_same_side_of_the_threshold():
    eng = _engine('dense', 24, 9)
    inv = [0.0, 0.0, 1.0]
    try:
        for factor, singular in ((4.0, False), (0.25, True)):
            psi, bell = _threshold_states(factor)
            for mode in MODES:
                chi, norms, J = (x.cpu().numpy() for x in eng.chi_local_invariants(psi, bell, mode, inv, 0.3, 1.0))
                near, rest = slice(0, 4 * THRESHOLD_DRAWS), slice(4 * THRESHOLD_DRAWS, 24)
                if singular:
                    assert np.isnan(J[:THRESHOLD_DRAWS]).all() and not chi[near].any() and not norms[near].any()
                else:
                    assert np.isfinite(J[:THRESHOLD_DRAWS]).all() and chi[near].any(axis=1).all() and norms[near].all()
                assert np.isfinite(J[THRESHOLD_DRAWS:]).all() and norms[rest].all()
                _show("delta = %.2f delta* %s: %s" % (factor, mode, "J NaN, zero rows" if singular else "finite J, rows"))
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 3. the batch route
# ---------------------------------------------------------------------------
NT = 13
PER_REPLICA = 3 * 4 * NT * 4 * 16  # the co-state store and the two trajectories of one problem (batch.py), bytes


def _amplitudes(B):
    """B random guess amplitudes, as ``AMPLITUDES`` of test_local_invariants.py is made."""
    return tuple(0.3 * (0.7 + 0.6 * x) for x in np.random.default_rng(40 + B).random(B))


def _hook(con):
    return lambda **kw: con.J_T(kw['fw_states_T'], kw['objectives'])


def _solo(problem, con, sigma, iters, check=None):
    import krotov_amd

    return krotov_amd.optimize_pulses(
        problem['objectives'], problem['pulse_options'], problem['tlist'], propagator=krotov_amd.propagators.expm,
        chi_constructor=con, sigma=sigma, iter_stop=iters, store_all_pulses=True, check_convergence=check,
        info_hook=_hook(con))


def _batch(problems, con, sigmas, iters, check=None, hook=None):
    import krotov_amd

    return krotov_amd.optimize_pulses_batch(
        problems, propagator=krotov_amd.propagators.expm, chi_constructor=con, sigma=sigmas, iter_stop=iters,
        store_all_pulses=True, check_convergence=check, info_hook=_hook(con) if hook is None else hook)


def _stopping_rule(amps, freeze):
    """(limit, frozen): J after iteration 1 of the oracle runs, the ``freeze`` smallest below ``limit`` -- half way to
    the next one, the gap far above anything two double-precision runs differ by."""
    J1 = np.array([oracle_run('PE', NT, 1, a)['J'][1] for a in amps])
    order = np.argsort(J1)
    low, high = J1[order[freeze - 1]], J1[order[freeze]]
    assert high - low > 1e-4, (low, high)
    return 0.5 * (low + high), sorted(int(b) for b in order[:freeze])


def _same_run(res, sig, solo, solo_sig):
    from test_replicas import _same_result

    _same_result(res, solo)
    assert sig.history == solo_sig.history and len(sig.chi) == len(solo_sig.chi)
    assert all(np.array_equal(x, y) for x, y in zip(sig.chi, solo_sig.chi))


@pytest.mark.parametrize('route', ['one_batch', 'sub_batches', 'sequential'])
def test_values_hold_every_problem_whichever_route_ran(route, li_double, monkeypatch, caplog):
    """After ``optimize_pulses_batch`` returns, ``.values[b]`` is, bit for bit, the ``.values[0]`` the solo run of
    problem b leaves -- as one batch, in two sub-batches of two, and one problem after another (unequal nt)."""
    import krotov_amd.batch as batch_mod
    from replica_double import ReplicaEngineDouble

    amps = _amplitudes(4)
    nts = (NT, NT + 2, NT, NT + 2) if route == 'sequential' else (NT,) * 4
    built = [product_problem(nt, a) for nt, a in zip(nts, amps)]
    problems, con = [p for p, _ in built], built[0][1]
    if route == 'sub_batches':
        monkeypatch.setattr(batch_mod, '_free_device_bytes', lambda: 4 * (2 * PER_REPLICA + 1))  # a quarter holds two
    seen = []

    def hook(**kw):
        seen.append(None if con.values is None else con.values.shape)
        return con.J_T(kw['fw_states_T'], kw['objectives'])

    sigmas = [product_sigma() for _ in problems]
    with caplog.at_level(logging.INFO, logger='krotov'):
        results = _batch(problems, con, sigmas, 2, hook=hook)
    assert [e.replicas for e in ReplicaEngineDouble.created] == dict(
        one_batch=[4], sub_batches=[2, 2], sequential=[1, 1, 1, 1])[route]
    values = con.values.copy()
    assert values.shape == (4,) and values.dtype == np.float64
    messages = [rec.getMessage() for rec in caplog.records]
    assert any('sequential' in m for m in messages) == (route == 'sequential')
    assert any('sub-batches' in m for m in messages) == (route == 'sub_batches')
    if route != 'sequential':  # the index of a problem in the log is its index in the caller's list
        for b in range(4):
            assert messages.count("Finished Krotov iteration 1 of problem %d" % b) == 1
    # while it runs, a hook sees the running part only
    assert set(seen) <= {None, dict(one_batch=(4,), sub_batches=(2,), sequential=(1,))[route]}
    for b, (res, sig) in enumerate(zip(results, sigmas)):
        solo_sig = product_sigma()
        solo = _solo(problems[b], con, solo_sig, 2)
        assert con.values.shape == (1,) and con.values[0] == values[b], (route, b)
        assert abs(values[b] - res.info_vals[-2]) < 1e-13  # (J of the states iteration 2 started from)
        _same_run(res, sig, solo, solo_sig)


def test_values_of_a_batch_that_runs_no_iteration(li_double):
    """``iter_stop = 0``: no co-states are formed, ``.values`` stays what it was -- in a batch and in the sequential
    loop (unequal nt)."""
    for nts in ((NT, NT), (NT, NT + 2)):
        built = [product_problem(nt, a) for nt, a in zip(nts, _amplitudes(4))]
        con = built[0][1]
        assert con.values is None
        _batch([p for p, _ in built], con, [product_sigma(), product_sigma()], 0)
        assert con.values is None
        con.values = kept = np.array([0.25])
        _batch([p for p, _ in built], con, [product_sigma(), product_sigma()], 0)
        assert con.values is kept


def test_early_stop_under_the_mask(li_double):
    """4 problems, PE, second order; ``check_convergence`` freezes two of them after iteration 1.  Their Results,
    ``.values`` entries and sigma histories are those of their solo runs; so are the two that go on."""
    import krotov_amd
    from replica_double import ReplicaEngineDouble

    amps = _amplitudes(4)
    limit, frozen = _stopping_rule(amps, 2)
    check = krotov_amd.convergence.value_below(limit, name='J_T')
    built = [product_problem(NT, a) for a in amps]
    problems, con = [p for p, _ in built], built[0][1]
    sigmas = [product_sigma() for _ in problems]
    results = _batch(problems, con, sigmas, 3, check=check)
    eng = ReplicaEngineDouble.created[0]
    assert eng.replicas == 4
    masks = [m for name, m in eng.sweeps if name == 'update']
    assert masks[0] == [1] * 4 and masks[1] == [0 if b in frozen else 1 for b in range(4)]
    values = con.values.copy()
    assert values.shape == (4,)
    for b, (res, sig) in enumerate(zip(results, sigmas)):
        assert (res.iters == [0, 1]) == (b in frozen) and (b not in frozen or res.message.startswith('Reached convergence'))
        solo_sig = product_sigma()
        solo = _solo(problems[b], con, solo_sig, 3, check=check)
        assert con.values[0] == values[b]  # (a frozen one: the J of its last -- its only -- co-state construction)
        _same_run(res, sig, solo, solo_sig)


def _meddling(base, replica):
    """``base`` whose second ``chi_local_invariants`` call of a batch finds ``replica``'s states at T overwritten --
    state 2 a copy of state 0: U_B singular -- and, where that replica is masked out, a NaN in its J slot."""

    class Meddling(base):
        calls, masked = 0, None

        def chi_local_invariants(self, psi_T, bell, mode, invariants=None, unitarity_weight=0.0, scale=1.0, out=None):
            Meddling.calls += 1
            if Meddling.calls == 2:
                first = self._rows(replica).start
                psi_T[first + 2] = psi_T[first]
                Meddling.masked = not self.mask[replica]
                if Meddling.masked and out is not None:
                    out[2][replica] = float('nan')
            return super().chi_local_invariants(psi_T, bell, mode, invariants, unitarity_weight, scale, out=out)

    return Meddling


def test_a_replica_singular_while_inactive_raises_nothing_an_active_one_does(li_double, monkeypatch):
    import krotov_amd
    import krotov_amd.engine as engine_mod
    from test_replicas import _same_result

    amps = _amplitudes(4)
    limit, frozen = _stopping_rule(amps, 2)
    going = [b for b in range(4) if b not in frozen]
    check = krotov_amd.convergence.value_below(limit, name='J_T')
    built = [product_problem(NT, a) for a in amps]
    problems, con = [p for p, _ in built], built[0][1]
    plain = _batch(problems, con, [product_sigma() for _ in problems], 3, check=check)
    plain_values = con.values.copy()
    # the frozen replica: nothing is raised, nothing changes
    meddling = _meddling(li_double, frozen[0])
    monkeypatch.setattr(engine_mod, 'HipKrotovEngine', meddling)
    results = _batch(problems, con, [product_sigma() for _ in problems], 3, check=check)
    assert meddling.calls >= 2 and meddling.masked is True
    for b, (res, ref) in enumerate(zip(results, plain)):
        if b == frozen[0]:
            # (on the double ``psi_T.cpu().numpy()`` IS the buffer: the finished Result's states are views of the rows
            # overwritten above.  On the device the host copy is a copy.)
            assert np.array_equal(np.asarray(res.states[2]), np.asarray(res.states[0]))
            res.states = ref.states
        _same_result(res, ref)
    assert np.array_equal(con.values, plain_values)
    # a replica that goes on: the host constructor's error
    meddling = _meddling(li_double, going[0])
    monkeypatch.setattr(engine_mod, 'HipKrotovEngine', meddling)
    with pytest.raises(ValueError, match='linearly dependent'):
        _batch(problems, con, [product_sigma() for _ in problems], 3, check=check)
    assert meddling.calls == 2 and meddling.masked is False
    # set_device_values itself
    con.set_device_values([0.5, float('nan'), 0.25], active=[1, 0, 1])
    assert np.isnan(con.values[1]) and con.values[0] == 0.5
    with pytest.raises(ValueError, match='linearly dependent'):
        con.set_device_values([0.5, float('nan'), 0.25], active=[1, 1, 0])
    with pytest.raises(ValueError, match='linearly dependent'):
        con.set_device_values([0.5, float('nan'), 0.25])


@pytest.mark.gpu
def test_batch_of_nine_with_early_stops_end_to_end(monkeypatch):
    """B = 9 copies of notebook 07's problem on a 13-point grid, PE, second order, 2 iterations; the stopping rule
    freezes four of them after iteration 1.  Every ``results[b]`` is its solo ``optimize_pulses`` run bit for bit and
    within ``E2E_BOUND`` of its oracle run; in sub-batches of 3 the same bits again."""
    import krotov_amd
    import krotov_amd.batch as batch_mod
    from krotov_amd.engine import LAST_ENGINE
    from test_replicas import _same_result

    amps = _amplitudes(9)
    limit, frozen = _stopping_rule(amps, 4)
    check = krotov_amd.convergence.value_below(limit, name='J_T')
    built = [product_problem(NT, a) for a in amps]
    problems, con = [p for p, _ in built], built[0][1]
    sigmas = [product_sigma() for _ in problems]
    results = _batch(problems, con, sigmas, 2, check=check)
    assert LAST_ENGINE().kernel == 'replica16/wave' and LAST_ENGINE().replicas == 9
    values = con.values.copy()
    assert values.shape == (9,)
    worst = 0.0
    for b, (a, res, sig) in enumerate(zip(amps, results, sigmas)):
        assert res.iters == ([0, 1] if b in frozen else [0, 1, 2]), (b, res.iters)
        ref = oracle_run('PE', NT, len(res.iters) - 1, a)
        if sig.chi:
            d = deviations(res, sig, ref)[1]
        else:  # (frozen after iteration 1: sigma was never refreshed, there are no co-states to compare)
            d = max(np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() / max(1.0, np.abs(ref['all_pulses']).max()),
                    np.abs(np.array(res.info_vals) - ref['J']).max())
        worst = max(worst, d)
        assert d < E2E_BOUND, (b, d)
        solo_sig = product_sigma()
        solo = _solo(problems[b], con, solo_sig, 2, check=check)
        assert LAST_ENGINE().kernel == 'replica16/wave'
        assert con.values.shape == (1,) and con.values[0] == values[b]
        _same_run(res, sig, solo, solo_sig)
    _show("B = 9, %d frozen after iteration 1: largest deviation from the oracle runs %.2e" % (len(frozen), worst))
    # the same batch in sub-batches of 3
    monkeypatch.setattr(batch_mod, '_free_device_bytes', lambda: 4 * (3 * PER_REPLICA + 1))
    split_sigmas = [product_sigma() for _ in problems]
    split = _batch(problems, con, split_sigmas, 2, check=check)
    assert LAST_ENGINE().replicas == 3
    assert np.array_equal(con.values, values)
    for res, sig, ref, ref_sig in zip(split, split_sigmas, results, sigmas):
        _same_result(res, ref)
        assert sig.history == ref_sig.history and all(np.array_equal(x, y) for x, y in zip(sig.chi, ref_sig.chi))
