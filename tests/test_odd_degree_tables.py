"""kh_series_tables_odd (host code of the library, no GPU): the exactly-Hermitian Chebyshev-form tables with odd degrees,
which only the workgroup-per-objective two-terms-per-phase kernels are handed (kh_tile64q2.h).

* thresholds non-decreasing; every even entry (threshold, c_0, rows) equals the even-only table's bit for bit;
* an odd degree of the Chebyshev form serves strictly more than the even degree below it and strictly less than
  the one above;
* the polynomial of an odd degree m = 2P - 1, evaluated the way the kernel does (P - 1 products with A^2, then ONE
  product with A on s), reproduces exp(-i A) v at ||A|| = theta[m] within the bound the even degrees are held to in
  test_capi_symbols.test_series_tables_evaluate_the_exponential (6e-16) -- and the degree m - 1 polynomial misses that
  bound at the same norm: a table that served too much would be noticed;
* kh_series_tables / kh_series_tables_defect return what they returned before (even degrees only).
  ``golden/series_tables_even_only.npz`` holds this library's own kh_series_tables(0 / 1, tol = 2^-53) and
  kh_series_tables_defect(2^-53, 4, 3e-4) from before the odd-capable table existed: ``theta0/1/_d`` [65],
  ``ratios0/1/_d`` [65 * 65].
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg

from krotov_amd import _lib

ROWS = 32  # KH_Q2_ROWS
BOUND = 6e-16  # test_series_tables_evaluate_the_exponential's, same matrix size and normalisation
CAP = 2.0  # the Chebyshev form of the register-tile kernels ends here (Taylor beyond)


@pytest.fixture(scope='module')
def tables():
    lib = _lib.load()
    th_o, c0_o, rows_o = (ctypes.c_double * 65)(), (ctypes.c_double * 65)(), (ctypes.c_double * (65 * ROWS * 2))()
    assert lib.kh_series_tables_odd(0.0, th_o, c0_o, rows_o) == 0
    assert lib.kh_series_tables_odd(0.0, None, c0_o, rows_o) == -1
    th_e, ra_e = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
    assert lib.kh_series_tables(1, 0.0, th_e, ra_e) == 0
    return (np.array(th_o), np.array(c0_o), np.array(rows_o).reshape(65, ROWS, 2), np.array(th_e),
            np.array(ra_e).reshape(65, 65))


def test_thresholds_and_even_entries(tables):
    th_o, c0_o, rows_o, th_e, ra_e = tables
    assert np.all(np.diff(th_o) >= 0)
    assert th_o[0] == 0.0
    for m in range(0, 65, 2):
        assert th_o[m] == th_e[m], m  # bit for bit
    # the even-only table: odd entries repeat the even one below (no kernel that reads it ever lands on an odd degree)
    assert np.all(th_e[1::2] == th_e[0:64:2])
    cheb = [m for m in range(1, 64, 2) if th_o[m + 1] < CAP]  # odd degrees inside the Chebyshev form
    assert cheb[0] == 1 and cheb[-1] >= 13
    for m in cheb:
        assert th_o[m - 1] < th_o[m] < th_o[m + 1], m
    # ... and beyond it they repeat the even degree below, as in the even-only table
    for m in range(1, 64, 2):
        if th_e[m - 1] >= CAP:
            assert th_o[m] == th_o[m - 1], m
    # what config 5 runs at (theta = 0.40 ... 0.455): degree 11 instead of 12
    degree = lambda tab, th: int(np.argmax(tab >= th))  # noqa: E731
    assert degree(th_o, 0.40) == 11 and degree(th_o, 0.455) == 11
    assert degree(th_e, 0.40) == 12 and degree(th_e, 0.455) == 12
    assert degree(th_o, 0.5) == 12 and degree(th_o, 1.0) == 14


def test_even_rows_are_those_of_the_even_only_table(tables):
    """c_0 and the rows {r1_p, r2_p} of the even degrees, rebuilt from the even-only table's ratios in the same
    arithmetic order the library uses (long double quotients there: compare to one rounding)."""
    th_o, c0_o, rows_o, th_e, ra_e = tables
    for m in range(2, 40, 2):
        if not th_e[m] < CAP:
            continue
        assert c0_o[m] == ra_e[m, 0], m  # bit for bit
        c = np.cumprod(np.concatenate([[ra_e[m, 0], ra_e[m, 1] / ra_e[m, 0]], ra_e[m, 2:m + 1]]))
        assert rows_o[m, 0, 0] == ra_e[m, 1]
        for p in range(m // 2):
            den = 1.0 if p == 0 else c[2 * p]
            assert abs(rows_o[m, p, 0] - c[2 * p + 1] / den) <= 4e-16 * abs(rows_o[m, p, 0]), (m, p)
            assert abs(rows_o[m, p, 1] - c[2 * p + 2] / den) <= 4e-16 * abs(rows_o[m, p, 1]), (m, p)


def _kernel_form(rows, c0, m, A, v, odd):
    """kh_q2_expm_action: P = (m + 1) // 2 phases; an odd degree's last phase has no B product."""
    f, B = -1j, A @ A
    P = (m + 1) // 2
    s = rows[0, 0] * v
    state = c0 * v
    term = v
    for ph in range(P):
        last = ph + 1 == P
        if not (last and odd):
            term = rows[ph, 1] * (f * f) * (B @ term)
            state = state + term
            if not last:
                s = s + rows[ph + 1, 0] * term
    return state + f * (A @ s)


@pytest.mark.parametrize('m', [3, 5, 7, 9, 11, 13])
def test_odd_degree_evaluates_the_exponential(tables, m):
    th_o, c0_o, rows_o, th_e, ra_e = tables
    rng = np.random.default_rng(3)
    N = 24
    G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    Hm = (G + G.conj().T) / 2
    Hm /= np.linalg.norm(Hm, 2)
    v = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    v /= np.linalg.norm(v)
    A = Hm * th_o[m]
    ref = scipy.linalg.expm(-1j * A) @ v
    assert rows_o[m, m // 2, 1] == 0.0  # the row of the last phase: {r1_{P-1}, 0}
    err = np.linalg.norm(_kernel_form(rows_o[m], c0_o[m], m, A, v, odd=True) - ref)
    below = np.linalg.norm(_kernel_form(rows_o[m - 1], c0_o[m - 1], m - 1, A, v, odd=False) - ref)
    print('m = %d: theta %.6f, error %.2e, degree %d at the same norm %.2e' % (m, th_o[m], err, m - 1, below))
    assert err < BOUND, m
    assert below > BOUND, m  # the even degree below is NOT good enough at this norm


def test_even_only_tables_unchanged(tables):
    """kh_series_tables / kh_series_tables_defect still describe the even-only form every other kernel family reads."""
    th_o, c0_o, rows_o, th_e, ra_e = tables
    lib = _lib.load()
    th_d, ra_d = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
    assert lib.kh_series_tables_defect(0.0, 2.0, 0.0, th_d, ra_d) == 0
    assert np.array_equal(np.array(th_d), th_e) and np.array_equal(np.array(ra_d).reshape(65, 65), ra_e)
    assert lib.kh_series_tables_defect(0.0, 2.0, 1e-3, th_d, ra_d) == 0
    th_d = np.array(th_d)
    assert np.all(th_d[1::2] == th_d[0:64:2])  # the defect table stays even-only
    degree = lambda tab, th: int(np.argmax(tab >= th))  # noqa: E731
    assert degree(th_e, 0.5) == 12 and degree(th_e, 1.0) == 14
    # ... and hold the numbers they held before the odd-capable table existed (tests/golden; long double libm calls
    # behind them: compared to 1e-13, where a table with odd entries would differ in the first digit)
    import os

    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'series_tables_even_only.npz'))
    for rs in (0, 1):
        th, ra = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
        assert lib.kh_series_tables(rs, 0.0, th, ra) == 0
        assert np.allclose(np.array(th), gold['theta%d' % rs], rtol=1e-13, atol=0)
        assert np.allclose(np.array(ra), gold['ratios%d' % rs], rtol=1e-13, atol=0)
    th, ra = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
    assert lib.kh_series_tables_defect(0.0, 4.0, 3e-4, th, ra) == 0
    assert np.allclose(np.array(th), gold['theta_d'], rtol=1e-13, atol=0)
    assert np.allclose(np.array(ra), gold['ratios_d'], rtol=1e-13, atol=0)
    # odd rows of the even-only table's ratios are Taylor's, as before
    assert np.allclose(ra_e[11, 1:12], 1.0 / np.arange(1, 12), rtol=0, atol=0)
