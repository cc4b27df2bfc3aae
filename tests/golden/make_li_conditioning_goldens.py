#!/usr/bin/env python3
"""Generate tests/golden/li_conditioning.npz: the perfect-entangler / local-invariants functional J and its gradient
D = dJ / d conj U_B in 60-digit arithmetic (mpmath) on a ladder of gates that lose rank, for
tests/test_local_invariants_axes.py.

Inputs (fixed seed): U_B = Q1 diag(1, 1, 1, delta) Q2 with Haar-like unitaries Q from QR, six draws per rung, rungs
``DELTAS``; embedded into N = 9 states through ``states_of`` of tests/test_local_invariants.py (the logical subspace of
two qutrits plus population outside it).  The reference starts from the states and Bell rows AS DOUBLES -- what both
double-precision implementations are given --: U[i][k] = <B_i|phi_k> is formed in extended precision, so a
rounding of the smallest singular value by the embedding is part of the input, not of the reference's error.

The algebra restates the formula block at the top of krotov_amd/csrc/kh_chi_li.h with mpmath matrices:

    m = U^T U,  t = tr m,  d = det U,  G = t^2 / (16 d),  H = (t^2 - tr m^2) / (4 d),  g3 = Re H
    PE:  F = g3 |G| - Re G                   J_G = g3 conj(G) / (2 |G|) - 1/2,   J_H = |G| / 2
    LI:  F = |G - G_O|^2 + (g3 - g3_O)^2     J_G = conj(G - G_O),               J_H = g3 - g3_O
    J = (1 - w) F + w (1 - tr(U^+ U) / 4)
    dG/dU = t U / (4 d) - G U^-T,   dH/dU = (t U - U m) / d - H U^-T
    D = (1 - w) conj(J_G dG/dU + J_H dH/dU) - (w / 4) U

Arrays: ``deltas`` (R,), ``weights`` (2,), ``psi`` (R, DRAWS, 4, 9), ``bell`` (4, 9), ``J`` (R, DRAWS, mode, weight),
``D`` (R, DRAWS, mode, weight, 4, 4), rounded to double; mode 0 = PE, 1 = LI towards CNOT.

Needs mpmath; the test-suite reads the committed ``.npz`` (and recomputes it where mpmath imports).

Usage:  python tests/golden/make_li_conditioning_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for path in (os.path.dirname(TESTS), TESTS):
    if path not in sys.path:
        sys.path.insert(0, path)

DIGITS = 60
# the first of 1, 2, ... at which the host constructor's error on every rung stays within 4 x the figures measured for
# it before (HOST_TABLE of tests/test_local_invariants_axes.py): at small delta the error of a draw depends on how much
# cancels in it and varies tenfold between draws.  Chosen on the host constructor alone, before any device run.
SEED = 1
DRAWS = 6
N = 9
DELTAS = (1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-6, 1e-8, 4e-10)
WEIGHTS = (0.0, 0.3)
NAME = 'li_conditioning.npz'


def haar_like(rng):
    q, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
    return q


def rank_losing_gate(rng, delta):
    """U_B = Q1 diag(1, 1, 1, delta) Q2: singular values 1, 1, 1, delta, |det U_B| = delta."""
    return haar_like(rng) @ np.diag([1.0, 1.0, 1.0, delta]) @ haar_like(rng)


def inputs():
    """(psi (R, DRAWS, 4, N), bell (4, N)) of the ladder."""
    import test_local_invariants as tli

    rng = np.random.default_rng(SEED)
    basis = tli.frame(rng, N)
    psi = np.array([[tli.states_of(rng, basis, rank_losing_gate(rng, delta)) for _ in range(DRAWS)] for delta in DELTAS])
    return psi, tli.bell_of(basis)


def _mpc(z):
    from mpmath import mp

    return mp.mpc(mp.mpf(float(np.real(z))), mp.mpf(float(np.imag(z))))  # (a double is an exact mpf)


def target_invariants_of_cnot():
    """(G_O, g3_O) of CNOT from the Bell states of ``gate_objectives`` in extended precision."""
    from mpmath import mp

    s = 1 / mp.sqrt(2)
    bell = mp.matrix([[1, 0, 0, 1], [0, 1j, 1j, 0], [0, 1, -1, 0], [1j, 0, 0, -1j]]) * s
    cnot = mp.matrix([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]])
    U = bell.conjugate() * cnot * bell.T
    m = U.T * U
    t, d = sum(m[i, i] for i in range(4)), mp.det(U)
    m2 = m * m
    return t * t / (16 * d), mp.re((t * t - sum(m2[i, i] for i in range(4))) / (4 * d))


def reference(psi, bell, mode, w, target):
    """(J, D (4, 4)) of one gate as mpmath numbers from its states and the Bell rows (doubles)."""
    from mpmath import mp

    U = mp.matrix(4, 4)
    for i in range(4):
        for k in range(4):
            U[i, k] = sum(_mpc(np.conj(bell[i, n])) * _mpc(psi[k, n]) for n in range(bell.shape[1]))
    w = mp.mpf(float(w))
    m = U.T * U
    t, d = sum(m[i, i] for i in range(4)), mp.det(U)
    m2 = m * m
    G = t * t / (16 * d)
    H = (t * t - sum(m2[i, i] for i in range(4))) / (4 * d)
    g3 = mp.re(H)
    inv_T = mp.inverse(U).T
    dG = (t / (4 * d)) * U - G * inv_T
    dH = (t * U - U * m) * (1 / d) - H * inv_T
    if mode == 0:
        absG = abs(G)
        F = g3 * absG - mp.re(G)
        J_G = g3 * mp.conj(G) / (2 * absG) - mp.mpf(1) / 2
        J_H = absG / 2
    else:
        G_O, g3_O = target
        F = abs(G - G_O) ** 2 + (g3 - g3_O) ** 2
        J_G = mp.conj(G - G_O)
        J_H = g3 - g3_O
    fro2 = sum(abs(U[i, k]) ** 2 for i in range(4) for k in range(4))
    J = (1 - w) * F + w * (1 - fro2 / 4)
    D = (1 - w) * (J_G * dG + J_H * dH).conjugate() - (w / 4) * U
    return J, D


def compute(psi, bell):
    """dict(J (R, DRAWS, 2, 2), D (R, DRAWS, 2, 2, 4, 4)) rounded to double."""
    from mpmath import mp

    mp.dps = DIGITS
    target = target_invariants_of_cnot()
    R, draws = psi.shape[:2]
    J = np.zeros((R, draws, 2, len(WEIGHTS)))
    D = np.zeros((R, draws, 2, len(WEIGHTS), 4, 4), dtype=np.complex128)
    for r in range(R):
        for j in range(draws):
            for mode in (0, 1):
                for iw, w in enumerate(WEIGHTS):
                    val, grad = reference(psi[r, j], bell, mode, w, target)
                    J[r, j, mode, iw] = float(val)
                    D[r, j, mode, iw] = [[complex(grad[i, k]) for k in range(4)] for i in range(4)]
    return dict(J=J, D=D)


def main():
    psi, bell = inputs()
    out = dict(deltas=np.array(DELTAS), weights=np.array(WEIGHTS), psi=psi, bell=bell, **compute(psi, bell))
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))
    for r, delta in enumerate(DELTAS):
        print('delta %-7.0e max|J| %.3e  max|D| %.3e' % (delta, np.abs(out['J'][r]).max(), np.abs(out['D'][r]).max()))


if __name__ == '__main__':
    main()
