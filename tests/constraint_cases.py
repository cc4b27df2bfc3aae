"""Yardstick and problems of tests/test_state_constraint.py (state-dependent constraints: a source term in the backward
sweep).

The functional is J_T + int g_b dt with the quadratic running cost

    g_b(t) = (lambda_b / T) s_b(t) sum_k <phi_k(t)|D_k|phi_k(t)>,      T = tlist[-1] - tlist[0],

the source W_k(t_n) = -d g_b / d <phi_k| = -(lambda_b / T) s_b(t_n) D_k phi_k(t_n) on the forward states of the previous
iteration, and the backward sweep, trapezoid in the source with the oracle's own per-interval step V_n (``ko._step`` on the
adjoint operators, ``backwards=True``),

    chi[nt-1] = chi(T);    chi[n] = V_n (chi[n+1] + h_n W[n+1]) + h_n W[n],    h_n = dt_n / 2 / ||chi_k(T)||.

Everything else of an iteration is the oracle's (``forward_propagation``, ``forward_update_sweep``, ``tau_vals``) or, with
a parametrization, tests/parametrization_cases.py's restatement of the update sweep.  The exact discrete identity

    d J_d / d eps_l[n] = -2 Re <lt_{n+1}| (d U_n / d eps_l) phi_n>,
    J_d = J_T(phi_{nt-1}) + sum_n omega_n g_b(phi_n, t_n),   lt_{n+1} = ||chi(T)|| (chi[n+1] + h_n W[n+1])

(omega_n: trapezoid weights) ties signs, half weights and the norm handling to finite differences of the oracle's own
propagator; written out here independently of ``krotov_amd.constraints``.
"""
import numpy as np

import parametrization_cases as pc
from oracle import krotov_oracle as ko

NORM = lambda prob, chi: float(np.linalg.norm(chi))  # noqa: E731


def trapezoid_weights(tlist):
    dt = np.diff(np.asarray(tlist, dtype=np.float64))
    w = np.zeros(len(tlist))
    w[0] = 0.5 * dt[0]
    w[-1] = 0.5 * dt[-1]
    for n in range(1, len(tlist) - 1):
        w[n] = 0.5 * (dt[n - 1] + dt[n])
    return w


def shape_values(shape, tlist):
    if shape is None:
        return np.ones(len(tlist))
    return np.array([float(shape(t)) for t in tlist])


def factors(lambda_b, tlist, shape=None):
    """-(lambda_b / T) s_b(t_n)."""
    return -(lambda_b / (tlist[-1] - tlist[0])) * shape_values(shape, tlist)


def per_objective(D, K):
    return list(D) if isinstance(D, (list, tuple)) else [D] * K


def source(D, fac, states):
    """W[k, n] = fac[n] D_k states[k, n]; zero where D_k is None."""
    K, nt, N = states.shape
    W = np.zeros((K, nt, N), dtype=np.complex128)
    for k, Dk in enumerate(per_objective(D, K)):
        if Dk is not None:
            for n in range(nt):
                W[k, n] = fac[n] * (Dk @ states[k, n])
    return W


def g_b_values(D, lambda_b, tlist, states, shape=None):
    """g_b(t_n) on the trajectories ``states`` (K, nt, N)."""
    K, nt, _ = states.shape
    s = shape_values(shape, tlist)
    T = tlist[-1] - tlist[0]
    g = np.zeros(nt)
    for k, Dk in enumerate(per_objective(D, K)):
        if Dk is not None:
            for n in range(nt):
                g[n] += (lambda_b / T) * s[n] * np.vdot(states[k, n], Dk @ states[k, n]).real
    return g


def integral(D, lambda_b, tlist, states, shape=None):
    return float(np.dot(trapezoid_weights(tlist), g_b_values(D, lambda_b, tlist, states, shape)))


def backward_sweep(problem, chi_T, pulses, W, chi_norms=None, variant=None):
    """The recursion of the module docstring; (K, nt, N) with ``[:, -1] = chi_T``.  ``chi_norms`` None: 1.
    ``variant`` -- wrong on purpose, for the test that shows the identity can fail: ``'flip'`` (W with the other sign),
    ``'full'`` (the full weight 2 h_n at W[n]), ``'substep'`` (the interval taken as two sub-steps of the propagator, the
    interval's source added at each of them)."""
    tl = problem.tlist
    nt = len(tl)
    adj = problem.adjoint_ops()
    out = np.empty((problem.K, nt, problem.N), dtype=np.complex128)
    sign = -1.0 if variant == 'flip' else 1.0
    for k in range(problem.K):
        state = chi_T[k].copy()
        out[k, nt - 1] = state
        nrm = 1.0 if chi_norms is None else chi_norms[k]
        for n in range(nt - 2, -1, -1):
            dt = tl[n + 1] - tl[n]
            h = 0.5 * dt / nrm
            eps = [np.conjugate(p[n]) for p in pulses]
            if variant == 'substep':
                for _ in range(2):
                    state = state + h * W[k, n + 1]
                    state = ko._step(problem, adj[k], eps, 0.5 * dt, state, True, False)
                    state = state + h * W[k, n]
            else:
                state = state + (sign * h) * W[k, n + 1]
                state = ko._step(problem, adj[k], eps, dt, state, True, False)
                state = state + (sign * h * (2.0 if variant == 'full' else 1.0)) * W[k, n]
            out[k, n] = state
    return out


# ---------------------------------------------------------------------------
# the discrete functional and its exact gradient
# ---------------------------------------------------------------------------
def J_T(chi_name, problem, fw_T):
    """The final-time functional whose chi_k(T) = -d J_T / d <phi_k| the oracle's constructor of that name returns
    (functionals.py: J_T_re = 1 - Re sum tau / K, J_T_ss = 1 - sum |tau|^2 / K; unit weights)."""
    tau = ko.tau_vals(problem, fw_T)
    if chi_name == 're':
        return 1.0 - float(np.sum(tau.real)) / problem.K
    if chi_name == 'ss':
        return 1.0 - float(np.sum(np.abs(tau) ** 2)) / problem.K
    raise ValueError(chi_name)


def J_d(chi_name, problem, pulses, D, lambda_b, shape=None):
    fw_T, states = ko.forward_propagation(problem, pulses, store=True)
    return J_T(chi_name, problem, fw_T) + integral(D, lambda_b, problem.tlist, states, shape)


def step_derivative(problem, k, eps, dt, l, state):
    """(d U_n / d eps_l) state for the oracle's forward step U_n = expm(f (H0 + sum eps H) dt): the Frechet derivative
    of the matrix exponential as the upper right block of expm([[A, E], [0, A]]), with the oracle's own ``expm_dense``."""
    f = ko._eqm_factor(problem.is_super, False)
    ops_k = problem.ops[k]
    N = problem.N
    A = f * ops_k[0]
    for j in range(1, len(ops_k)):
        if ops_k[j] is not None:
            A = A + (f * eps[j - 1]) * ops_k[j]
    E = np.zeros((N, N), dtype=np.complex128) if ops_k[1 + l] is None else f * ops_k[1 + l]
    big = np.zeros((2 * N, 2 * N), dtype=np.complex128)
    big[:N, :N] = A * dt
    big[N:, N:] = A * dt
    big[:N, N:] = E * dt
    return ko.expm_dense(big)[:N, N:] @ state


def identity_gradient(chi_name, problem, pulses, D, lambda_b, shape=None, variant=None):
    """-2 Re <lt_{n+1}| (d U_n / d eps_l) phi_n> for every (l, n), from the backward sweep above (``variant``: a wrong
    one); chi(T) from the oracle's constructor, normalised with the 2-norm as an optimisation does."""
    tl = problem.tlist
    nt, L = len(tl), len(pulses)
    fw_T, states = ko.forward_propagation(problem, pulses, store=True)
    tau = ko.tau_vals(problem, fw_T)
    chi_T = {'re': ko.chis_re, 'ss': ko.chis_ss}[chi_name](problem, fw_T, tau)
    norms = np.array([NORM(problem, chi_T[k]) for k in range(problem.K)])
    W = source(D, factors(lambda_b, tl, shape), states)
    chi = backward_sweep(problem, chi_T / norms[:, None], pulses, W, norms, variant=variant)
    grad = np.zeros((L, nt - 1))
    for n in range(nt - 1):
        dt = tl[n + 1] - tl[n]
        eps = [p[n] for p in pulses]
        for k in range(problem.K):
            h = 0.5 * dt / norms[k]
            sign = -1.0 if variant == 'flip' else 1.0
            lt = norms[k] * (chi[k, n + 1] + (sign * h) * W[k, n + 1])
            for l in range(L):
                grad[l, n] += -2.0 * np.vdot(lt, step_derivative(problem, k, eps, dt, l, states[k, n])).real
    return grad


def central_differences(chi_name, problem, pulses, D, lambda_b, h, shape=None):
    """(J_d(eps + h e_ln) - J_d(eps - h e_ln)) / 2h for every (l, n)."""
    L, M = len(pulses), len(pulses[0])
    fd = np.zeros((L, M))
    for l in range(L):
        for n in range(M):
            up = [np.array(p, dtype=np.float64) for p in pulses]
            dn = [np.array(p, dtype=np.float64) for p in pulses]
            up[l][n] += h
            dn[l][n] -= h
            fd[l, n] = (J_d(chi_name, problem, up, D, lambda_b, shape) - J_d(chi_name, problem, dn, D, lambda_b, shape)) / (2 * h)
    return fd


# ---------------------------------------------------------------------------
# the optimisation
# ---------------------------------------------------------------------------
def optimize(problem, guess_pulses, shapes, lambdas, chi_constructor, iter_stop, D, lambda_b, shape=None, sigma=None,
             kinds=None):
    """Iteration 0 + ``iter_stop`` iterations with the source term; chi normalised with the 2-norm.  ``sigma``: a constant
    (second-order update with that sigma(t)); ``kinds``: pulse parametrizations (tests/parametrization_cases.py (B)).
    Records as ``oracle.optimize``, plus ``g_b`` (int g_b dt per iteration, iteration 0 included), ``J_T_re`` and the
    last forward trajectories ``states``."""
    tl = problem.tlist
    pulses = [np.array(p, dtype=np.float64, copy=True) for p in guess_pulses]
    u = None if kinds is None else [pc.inverse(kinds[l], pulses[l]) for l in range(len(pulses))]
    fac = factors(lambda_b, tl, shape)
    fw_T, states = ko.forward_propagation(problem, pulses, store=True)
    tau = ko.tau_vals(problem, fw_T)
    all_pulses, taus, gas = [np.array(pulses)], [tau], [np.zeros(len(pulses))]
    gbs = [integral(D, lambda_b, tl, states, shape)]
    sig = None if sigma is None else [sigma] * (len(tl) - 1)
    for _ in range(iter_stop):
        chi_T = chi_constructor(problem, fw_T, tau)
        norms = np.array([NORM(problem, chi_T[k]) for k in range(problem.K)])
        chi_store = backward_sweep(problem, chi_T / norms[:, None], pulses, source(D, fac, states), norms)
        if kinds is None:
            pulses, fw_T, g_a, states = ko.forward_update_sweep(
                problem, chi_store, norms, pulses, shapes, lambdas, sigma_vals=sig, fw_prev=states, store=True)
        else:
            pulses, u, fw_T, g_a, states = pc.update_sweep(
                problem, chi_store, norms, u, kinds, shapes, lambdas, sigma_vals=sig, fw_prev=states, store=True)
        tau = ko.tau_vals(problem, fw_T)
        all_pulses.append(np.array(pulses))
        taus.append(tau)
        gas.append(g_a)
        gbs.append(integral(D, lambda_b, tl, states, shape))
    return dict(all_pulses=np.array(all_pulses), tau_vals=np.array(taus), g_a=np.array(gas), g_b=np.array(gbs),
                fw_T=fw_T, states=states)


# ---------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------
def projector(N, keep):
    """The projector onto the first ``keep`` basis states."""
    P = np.zeros((N, N), dtype=np.complex128)
    P[np.arange(keep), np.arange(keep)] = 1.0
    return P


def random_hermitian(N, seed, scale=1.0):
    from krotov_amd import configs

    return configs.herm(np.random.default_rng(seed), N, scale)


def nonuniform(spec, ratios):
    """``spec`` on a grid whose interval lengths are those of its own grid times ``ratios`` (cycled)."""
    dt = np.diff(spec.tlist)
    dt = dt * np.resize(np.asarray(ratios, dtype=np.float64), len(dt))
    spec.tlist = np.concatenate([[spec.tlist[0]], spec.tlist[0] + np.cumsum(dt)])
    return spec


def lambda_system(nt=41, T=5.0):
    """A three-level Lambda system |0> - |2> - |1>: pump and Stokes pulses couple the two ground states to the excited
    (forbidden) level |2>; the objective is |0> -> |1>.  Returns the spec, the projector onto the allowed subspace
    span(|0>, |1>) and the one onto the forbidden level."""
    from krotov_amd import configs

    H0 = np.diag([0.0, 0.2, 1.0]).astype(np.complex128)
    Hp = np.zeros((3, 3), dtype=np.complex128)
    Hp[0, 2] = Hp[2, 0] = 0.5
    Hs = np.zeros((3, 3), dtype=np.complex128)
    Hs[1, 2] = Hs[2, 1] = 0.5
    init = np.zeros((1, 3), dtype=np.complex128)
    init[0, 0] = 1.0
    target = np.zeros((1, 3), dtype=np.complex128)
    target[0, 1] = 1.0
    tlist = np.linspace(0.0, T, nt)

    def S(t):
        return ko.flattop(t, 0.0, T, 0.2 * T)

    controls = [lambda t, args: 1.2 * S(t), lambda t, args: 1.0 * S(t)]
    spec = configs.ProblemSpec(name='lambda3', H0=[H0], Hc=[[Hp, Hs]], is_super=False, init=init, target=target,
                               tlist=tlist, controls=controls, update_shape=S, lambda_a=None, chi='re', mu=None)
    spec.lambdas = [2.0, 2.0]
    allowed = projector(3, 2)
    return spec, allowed, np.eye(3, dtype=np.complex128) - allowed
