"""Yardstick and problems of tests/test_nonlinear_controls.py (non-linear controls: terms eps^p H in the update sweeps).

The reference cannot express H(eps) = H0 + sum_j eps_c(j)^p_j H_j, so there is no golden: this is a NumPy restatement of
``oracle.forward_update_sweep`` with the five lines of the update,

        w_j    = p_j eps_guess,c(j)[n]^(p_j - 1)
        D_c    = sum_{j in c} w_j D_j
        eps_c  = eps_guess,c[n] + (S_c[n] / lambda_c) D_c
        g_a,c += (S_c[n] / lambda_c) D_c^2 dt_n
        c_j    = eps_c^p_j                                   what interval n is propagated with

built from the oracle's own ``_mu_apply``, ``_step``, ``backward_sweep``, ``forward_propagation`` and ``tau_vals`` on an
``OracleProblem`` whose operator rows are ``[H0, T_1 .. T_J]``: one slot per TERM.  ``terms`` is a list of J pairs
``(control, power)``.  Powers are repeated products; nothing here imports ``krotov_amd.nonlinear``.
"""
import numpy as np

from oracle import krotov_oracle as ko

import parametrization_cases as pc


def power(e, p):
    out = e
    for _ in range(p - 1):
        out = out * e
    return out


def weight(e, p, linear_weights=False):
    """d(eps^p)/d eps; ``linear_weights``: the power-1 value (the wrong one the witnesses compare with)."""
    if p == 1 or linear_weights:
        return np.ones_like(np.asarray(e, dtype=np.float64))
    return p * power(e, p - 1)


def coefficients(terms, pulses):
    """The J coefficient pulses c_j[n] = eps_c(j)[n]^p_j of C pulses."""
    return [power(np.asarray(pulses[c], dtype=np.float64), p) for c, p in terms]


def update_sweep(problem, chi_store, chi_norms, guess, terms, shapes, lambdas, sigma_vals=None, fw_prev=None,
                 store=False, linear_weights=False, D_out=None):
    """``oracle.forward_update_sweep`` with the five lines above.  ``guess``: C arrays of eps.  Returns ``(opt, fw_T,
    g_a)`` (C rows) and, with ``store``, the (K, nt, N) forward states.  ``D_out``: a list that receives the J per-term
    sums of every interval."""
    tl = problem.tlist
    nt = len(tl)
    K, C, J = problem.K, len(guess), len(terms)
    assert problem.L == J
    guess = [np.asarray(g, dtype=np.float64) for g in guess]
    opt = [g.copy() for g in guess]
    w = [weight(guess[c], p, linear_weights) for c, p in terms]
    g_a = np.zeros(C)
    fw = [problem.init[k].copy() for k in range(K)]
    second_order = sigma_vals is not None
    out = np.empty((K, nt, problem.N), dtype=np.complex128) if store else None
    if store:
        out[:, 0] = problem.init
    delta = [np.zeros(problem.N, dtype=np.complex128) for _ in range(K)]
    for n in range(nt - 1):
        dt = tl[n + 1] - tl[n]
        D = np.zeros(J)
        for j in range(J):
            d = 0j
            for k in range(K):
                mu_psi = ko._mu_apply(problem, k, j, fw[k])
                update = np.vdot(chi_store[k, n], mu_psi)
                update *= chi_norms[k]
                if second_order:
                    update += 0.5 * sigma_vals[n] * np.vdot(delta[k], mu_psi)
                d += update
            D[j] = d.imag
        if D_out is not None:
            D_out.append(D.copy())
        for c in range(C):
            Dc = 0.0
            for j, (cj, _) in enumerate(terms):
                if cj == c:
                    Dc += w[j][n] * D[j]
            step = shapes[c][n] / lambdas[c]
            opt[c][n] = guess[c][n] + step * Dc
            g_a[c] += step * Dc * Dc * dt
        coef = [power(opt[c][n], p) for c, p in terms]
        for k in range(K):
            fw[k] = ko._step(problem, problem.ops[k], coef, dt, fw[k], False, False)
            if second_order:
                delta[k] = fw[k] - fw_prev[k, n + 1]
            if store:
                out[k, n + 1] = fw[k]
    if store:
        return opt, np.array(fw), g_a, out
    return opt, np.array(fw), g_a


# ---------------------------------------------------------------------------
# regime problems with a term table (tests/helpers.py: ``obj.terms``; tests/test_nonlinear_axes.py)
# ---------------------------------------------------------------------------
# by the number of slots J of a base case; J = 1: the two tables alternate over the single-slot bases of a kernel form
AXES_TABLES = {
    1: ([(0, 3)], [(0, 4)]),
    2: [(0, 2), (0, 1)],                                   # powers descending
    3: [(1, 1), (0, 2), (1, 3)],                           # slot 0 is not control 0; one control's terms are apart
    4: [(1, 4), (0, 1), (1, 1), (0, 3)],                   # the same, with power 4 and two controls interleaved
    6: [(0, 1), (1, 2), (2, 1), (0, 3), (1, 1), (2, 4)],   # three controls interleaved, beyond KH_MAX_L slots
}


def with_terms(obj, terms):
    """The explicit regime problem ``obj`` (``helpers.explicit``: L pulses for L slots) with the term table ``terms``:
    the slots stay, the pulses / shapes / lambdas are those of the first C controls."""
    import copy

    assert len(terms) == obj.L
    new = copy.copy(obj)
    C = n_controls(terms)
    new.terms = list(terms)
    new.pulses = [np.array(p, dtype=np.float64) for p in obj.pulses[:C]]
    new.shapes = [np.array(s, dtype=np.float64) for s in obj.shapes[:C]]
    new.lambdas = list(obj.lambdas[:C])
    return new


def coefficient_view(obj, pulses=None):
    """The linear regime problem the plain sweeps see: no table, the J coefficient pulses of ``pulses`` (default: the
    guess) as its pulses."""
    import copy

    new = copy.copy(obj)
    new.terms = None
    new.pulses = coefficients(obj.terms, obj.pulses if pulses is None else pulses)
    return new


def weights(terms, pulses, linear_weights=False):
    """(J, nt - 1): d c_j / d eps_c(j) under ``pulses`` -- the ``dcde`` of ``kh_set_nonlinear``."""
    return np.array([weight(np.asarray(pulses[c], dtype=np.float64), p, linear_weights) for c, p in terms])


def lambdas_in_eps(obj):
    """lambda_a of a regime problem with a table.  The update moves the coefficient c_j by about w_j^2 S / lambda Im D,
    w_j = p_j eps^(p_j - 1), and the regime transforms leave |eps| up to ~10 with w up to ~1e3: with the base case's
    lambda_a the first interval would throw the pulse (and theta with it) out of the regime.  lambda_c max(1, max_n (sum_{j
    in c} |w_j[n]|)^2) keeps the change of the coefficients what the regime helpers arranged for the linear update."""
    w = np.abs(weights(obj.terms, obj.pulses))
    out = []
    for c, lam in enumerate(obj.lambdas):
        tot = sum(w[j] for j, (cj, _) in enumerate(obj.terms) if cj == c)
        out.append(lam * max(1.0, float(tot.max()) ** 2))
    return out


def J_T_re(problem, tau):
    return 1.0 - float(np.mean(np.real(tau)))


def optimize(problem, guess, shapes, lambdas, terms, chi_constructor, iter_stop, linear_weights=False, norm=None):
    """Iteration 0 + ``iter_stop`` first-order iterations, chi normalised with the 2-norm (``norm(problem, chi)``
    otherwise).  Records as ``oracle.optimize``: ``all_pulses`` (iter_stop + 1, C, nt - 1), ``tau_vals``, ``g_a``."""
    pulses = [np.array(p, dtype=np.float64, copy=True) for p in guess]
    fw_T = ko.forward_propagation(problem, coefficients(terms, pulses))
    tau = ko.tau_vals(problem, fw_T)
    all_pulses, taus, gas = [np.array(pulses)], [tau], [np.zeros(len(pulses))]
    for _ in range(iter_stop):
        chi_T = chi_constructor(problem, fw_T, tau)
        if norm is None:
            chi_norms = np.array([float(np.linalg.norm(chi_T[k])) for k in range(problem.K)])
        else:
            chi_norms = np.array([norm(problem, chi_T[k]) for k in range(problem.K)])
        chi_T = chi_T / chi_norms[:, None]
        chi_store = ko.backward_sweep(problem, chi_T, coefficients(terms, pulses))
        pulses, fw_T, g_a = update_sweep(problem, chi_store, chi_norms, pulses, terms, shapes, lambdas,
                                         linear_weights=linear_weights)
        tau = ko.tau_vals(problem, fw_T)
        all_pulses.append(np.array(pulses))
        taus.append(tau)
        gas.append(g_a)
    return dict(all_pulses=np.array(all_pulses), tau_vals=np.array(taus), g_a=np.array(gas), fw_T=fw_T)


def optimize_kept_states(problem, guess, shapes, lambdas, terms, chi_constructor, iter_stop, sigma=None, D=None,
                         lambda_b=0.0):
    """The same with the trajectories kept: ``sigma`` (a constant: second-order update) and / or a state-dependent
    constraint with operator(s) ``D`` and weight ``lambda_b`` (tests/constraint_cases.py: its source and its backward
    sweep, on the coefficient pulses).  A constraint without sigma: sigma = 0."""
    import constraint_cases as cc

    tl = problem.tlist
    pulses = [np.array(p, dtype=np.float64, copy=True) for p in guess]
    fw_T, states = ko.forward_propagation(problem, coefficients(terms, pulses), store=True)
    tau = ko.tau_vals(problem, fw_T)
    all_pulses, taus, gas = [np.array(pulses)], [tau], [np.zeros(len(pulses))]
    sig = [0.0 if sigma is None else sigma] * (len(tl) - 1)
    for _ in range(iter_stop):
        chi_T = chi_constructor(problem, fw_T, tau)
        norms = np.array([float(np.linalg.norm(chi_T[k])) for k in range(problem.K)])
        coef = coefficients(terms, pulses)
        if D is None:
            chi_store = ko.backward_sweep(problem, chi_T / norms[:, None], coef)
        else:
            W = cc.source(D, cc.factors(lambda_b, tl), states)
            chi_store = cc.backward_sweep(problem, chi_T / norms[:, None], coef, W, norms)
        pulses, fw_T, g_a, states = update_sweep(problem, chi_store, norms, pulses, terms, shapes, lambdas,
                                                 sigma_vals=sig, fw_prev=states, store=True)
        tau = ko.tau_vals(problem, fw_T)
        all_pulses.append(np.array(pulses))
        taus.append(tau)
        gas.append(g_a)
    return dict(all_pulses=np.array(all_pulses), tau_vals=np.array(taus), g_a=np.array(gas), fw_T=fw_T)


# ---------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------
def n_controls(terms):
    return max(c for c, _ in terms) + 1


def problem(terms, K=3, N=5, nt=9, T=2.0, seed=12, bands=None, positive=False, absent=None):
    """``parametrization_cases.problem`` with one operator per term: K objectives with their own drift, J shared term
    operators (norm 1.5, scaled over the objectives), C guess pulses of amplitude <= 0.3.  ``positive``: every guess is
    the positive one (0.05 + 0.2 sin^2).  ``absent``: pairs (k, j) -- term j does not occur in objective k."""
    J, C = len(terms), n_controls(terms)
    spec = pc.problem(K=K, N=N, L=J, nt=nt, T=T, seed=seed, bands=bands)
    controls = spec.controls[:C]
    if positive:
        controls = [(lambda t, args, l=l: 0.05 + 0.2 * np.sin((l + 1) * np.pi * t / T) ** 2) for l in range(C)]
    spec.nl_controls = controls
    spec.nl_terms = list(terms)
    spec.nl_lambdas = [pc.LAMBDAS[c] for c in range(C)]
    spec.nl_absent = set(absent or ())
    return spec


def term_ops(spec):
    """Engine / oracle operator rows ``[H0, T_1 .. T_J]`` (None: the term is absent from the objective)."""
    return [[spec.H0[k]] + [None if (k, j) in spec.nl_absent else spec.Hc[k][j] for j in range(len(spec.nl_terms))]
            for k in range(spec.K)]


def oracle_side(spec):
    """(problem, guess_pulses, shapes, lambdas) through the oracle: C pulses, J operator slots."""
    prob = ko.OracleProblem(term_ops(spec), spec.init, spec.target, spec.tlist, spec.is_super, spec.weights)
    C = len(spec.nl_controls)
    _, gp, S = ko.initialize_controls(spec.nl_controls, [spec.update_shape] * C, spec.tlist)
    return prob, gp, S, list(spec.nl_lambdas)


def product_side(spec, wrap):
    """(objectives, pulse_options) for ``krotov_amd.optimize_pulses``: ``H = [H0, [T_j, wrap(control, p)], ...]`` with
    ``wrap(control, 1)`` the bare control; flat state vectors."""
    import krotov_amd

    objectives = []
    for k in range(spec.K):
        H = [spec.H0[k]]
        for j, (c, p) in enumerate(spec.nl_terms):
            if (k, j) in spec.nl_absent:
                continue
            H.append([spec.Hc[k][j], spec.nl_controls[c] if p == 1 else wrap(spec.nl_controls[c], p)])
        objectives.append(krotov_amd.Objective(initial_state=spec.init[k], target=spec.target[k], H=H))
    pulse_options = {c: dict(lambda_a=spec.nl_lambdas[i], update_shape=spec.update_shape)
                     for i, c in enumerate(spec.nl_controls)}
    return objectives, pulse_options
