"""The exact gradient of the time-discretised J_T for the pulse values, restated in NumPy / SciPy on ``OracleProblem``
inputs (no GPU): what ``kh_pulse_gradient`` (krotov_amd/csrc/kh_grad.h) and ``krotov_amd.PulseGradient`` are compared with.

    A_kn = H0_k + sum_l eps_l[n] H_lk,   U_kn = exp(f A_kn dt_n),   f = -i (Hilbert) or 1 (Liouville)
    dJ_T/d eps_l[n] = -2 sum_k ||chi_k|| Re < chi^_k(t_{n+1}) | L_exp(f dt_n A_kn)[f dt_n H_lk] | phi_k(t_n) >

with the oracle's own forward and backward sweeps and ``scipy.linalg.expm_frechet``.  The sum over k runs in objective
order; an absent control contributes 0.
"""
import numpy as np
import scipy.linalg

from krotov_amd import configs
from oracle import krotov_oracle as ko

import helpers


def f_of(problem):
    return 1.0 + 0.0j if problem.is_super else -1.0j


def generator(problem, k, pulses, n):
    """A_kn (without f and dt)."""
    A = np.array(problem.ops[k][0], dtype=np.complex128)
    for l in range(problem.L):
        if problem.ops[k][1 + l] is not None:
            A = A + pulses[l][n] * problem.ops[k][1 + l]
    return A


def costates(problem, pulses, chi):
    """phi (K, nt, N) under ``pulses``, tau, the normalised co-states chi^ (K, nt, N) under the same pulses and their
    norms (K,) -- ``chi``: 're' | 'ss' | 'sm' | 'hs' or a callable ``(problem, fw_T, tau) -> (K, N)``."""
    with helpers.MemoExpm():
        fw_T, phi = ko.forward_propagation(problem, pulses, store=True)
        tau = ko.tau_vals(problem, fw_T)
        chi_T = (helpers.CHI[chi] if isinstance(chi, str) else chi)(problem, fw_T, tau)
        norms = np.array([np.linalg.norm(c) for c in chi_T])
        chi_hat_T = np.array([c / nrm if nrm > 0 else c for c, nrm in zip(chi_T, norms)])
        chi_hat = ko.backward_sweep(problem, chi_hat_T, pulses)
    return phi, tau, chi_hat, norms


def exact_gradient(problem, pulses, chi='ss', stores=None):
    """``(grad (L, nt-1), per_objective (K, L, nt-1))`` of the formula above; ``stores``: what :func:`costates` returned
    (computed when omitted)."""
    phi, _, chi_hat, norms = costates(problem, pulses, chi) if stores is None else stores
    dt = np.diff(problem.tlist)
    f = f_of(problem)
    nI = len(dt)
    per = np.zeros((problem.K, problem.L, nI))
    for k in range(problem.K):
        for n in range(nI):
            Z = f * dt[n] * generator(problem, k, pulses, n)
            for l in range(problem.L):
                H = problem.ops[k][1 + l]
                if H is None:
                    continue
                dU = scipy.linalg.expm_frechet(Z, f * dt[n] * H, compute_expm=False)
                per[k, l, n] = -2.0 * norms[k] * np.real(np.vdot(chi_hat[k, n + 1], dU @ phi[k, n]))
    grad = np.zeros((problem.L, nI))
    for k in range(problem.K):  # (objective order)
        grad = grad + per[k]
    return grad, per


def first_order_gradient(problem, pulses, chi='ss', stores=None):
    """Krotov's update sum as a gradient: -2 dt_n sum_k ||chi_k|| Im <chi^_k(t_n)| mu_lk phi_k(t_n)>, mu = H_l (Hilbert) or
    i H_l (Liouville) -- the first order in dt of :func:`exact_gradient`."""
    phi, _, chi_hat, norms = costates(problem, pulses, chi) if stores is None else stores
    dt = np.diff(problem.tlist)
    grad = np.zeros((problem.L, len(dt)))
    for k in range(problem.K):
        for l in range(problem.L):
            H = problem.ops[k][1 + l]
            if H is None:
                continue
            mu = (1j if problem.is_super else 1.0) * H
            for n in range(len(dt)):
                grad[l, n] += -2.0 * dt[n] * norms[k] * np.imag(np.vdot(chi_hat[k, n], mu @ phi[k, n]))
    return grad


def J_T(problem, pulses, kind):
    """J_T_ss = 1 - mean |tau_k|^2, J_T_re = 1 - mean Re tau_k of the oracle's forward propagation."""
    with helpers.MemoExpm():
        tau = ko.tau_vals(problem, ko.forward_propagation(problem, pulses))
    return 1.0 - np.mean(np.abs(tau) ** 2) if kind == 'ss' else 1.0 - np.mean(tau.real)


def central_differences(J, pulses, h):
    """(J(eps + h e) - J(eps - h e)) / 2h for every pulse value."""
    pulses = [np.array(p, dtype=np.float64) for p in pulses]
    out = np.zeros((len(pulses), len(pulses[0])))
    for l in range(len(pulses)):
        for n in range(len(pulses[0])):
            up = [p.copy() for p in pulses]
            dn = [p.copy() for p in pulses]
            up[l][n] += h
            dn[l][n] -= h
            out[l, n] = (J(up) - J(dn)) / (2.0 * h)
    return out


def frechet_of_polynomial(c, Z, E):
    """The derivative of p(Z) = sum_j c[j] Z^j in the direction E: sum_j c[j] sum_{i<j} Z^i E Z^(j-1-i), by the block
    recursion the kernel uses (P_j = Z^j, D_j = d Z^j = D_{j-1} Z + P_{j-1} E)."""
    n = Z.shape[0]
    P, D = np.eye(n, dtype=np.clongdouble), np.zeros((n, n), dtype=np.clongdouble)
    Z, E = Z.astype(np.clongdouble), E.astype(np.clongdouble)
    out = np.zeros((n, n), dtype=np.clongdouble)
    for j in range(1, len(c)):
        D = D @ Z + P @ E
        P = P @ Z
        out = out + np.longdouble(c[j]) * D
    return out


def random_spec(K=3, N=5, L=2, nt=9, is_super=False, seed=1, theta=0.5, dt_spread=True, chi='ss', shared=False, normalise=True):
    """A small random problem as a ``configs.ProblemSpec`` with explicit ``pulses`` (what ``helpers.regime_*`` take):
    Hermitian operators (Hilbert) or dense random complex ones (a Liouvillian that is nothing but a matrix), random
    normalised initial states and targets, a non-uniform grid, pulses of order 1 -- scaled so that the largest
    theta_n = dt_n (||H0|| + sum |eps| ||H_l||) is ``theta``."""
    rng = np.random.default_rng(seed)

    def op():
        G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        if not is_super:
            G = (G + G.conj().T) / 2
        return G / np.linalg.norm(G, 2) if normalise else (G if not is_super else 0.5 * G)

    if shared:
        h0, hl = op(), [op() for _ in range(L)]
        H0, Hc = [h0] * K, [list(hl) for _ in range(K)]
    else:
        H0, Hc = [op() for _ in range(K)], [[op() for _ in range(L)] for _ in range(K)]
    dt = rng.uniform(0.05, 0.2, size=nt - 1) if dt_spread else np.full(nt - 1, 0.1)
    pulses = [rng.standard_normal(nt - 1) for _ in range(L)]

    def unit(shape):
        v = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        return v / np.linalg.norm(v, axis=1)[:, None]

    spec = configs.ProblemSpec(name='gradient_K%d_N%d_L%d' % (K, N, L), H0=H0, Hc=Hc, is_super=is_super, init=unit((K, N)),
                               target=unit((K, N)), tlist=np.concatenate([[0.0], np.cumsum(dt)]),
                               controls=[None] * L, update_shape=None, lambda_a=1.0, chi=chi)
    spec.pulses, spec.shapes, spec.lambdas, spec.fmt = pulses, [np.ones(nt - 1)] * L, [1.0] * L, 'dense'
    if theta is not None:
        scale = theta / helpers.theta_sequence(spec).max()
        helpers._scale_operators(spec, scale)
    return spec


def engine_ops(spec):
    return [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
