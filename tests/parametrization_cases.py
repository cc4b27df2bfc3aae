"""Yardsticks and problems of tests/test_parametrization.py (pulse parametrizations eps = f(u), bounded controls).

(A) ``LINEAR`` eps = a u + b is the unparametrized update with lambda / a**2: the untouched ``oracle.optimize``.
(B) every other kind: a NumPy restatement of ``oracle.forward_update_sweep`` with the update in u,

        c = f'(u_old[n]);  D' = c D;  u_new = u_old[n] + (S[n] / lambda) D';  g_a += (S[n] / lambda) D'^2 dt;
        eps_new = f(u_new)

    built from the oracle's own ``_mu_apply``, ``_step``, ``backward_sweep``, ``forward_propagation`` and ``tau_vals``.
    f, f' and the inverse are written out here, by kind, independently of ``krotov_amd.parametrization``.
"""
import numpy as np

from oracle import krotov_oracle as ko

# a kind of (B): None (the control is its own parameter) or a tuple
#   ('linear', a, b)   ('square',)   ('tanhsq', eps_max)   ('tanh', eps_min, eps_max)


def _ab(kind):
    if kind[0] == 'tanh':
        return 0.5 * (kind[2] - kind[1]), 0.5 * (kind[2] + kind[1])
    if kind[0] == 'linear':
        return kind[1], kind[2]
    if kind[0] == 'tanhsq':
        return kind[1], 0.0
    return 0.0, 0.0


def f(kind, u):
    if kind is None:
        return u
    a, b = _ab(kind)
    if kind[0] == 'linear':
        return a * u + b
    if kind[0] == 'square':
        return u * u
    if kind[0] == 'tanhsq':
        t = np.tanh(u)
        return a * (t * t)
    return a * np.tanh(u) + b


def dfdu(kind, u):
    if kind is None:
        return np.ones_like(u)
    a, b = _ab(kind)
    if kind[0] == 'linear':
        return np.full(np.shape(u), a)
    if kind[0] == 'square':
        return 2.0 * u
    t = np.tanh(u)
    if kind[0] == 'tanhsq':
        return 2.0 * a * t * (1.0 - t * t)
    return a * (1.0 - t * t)


def inverse(kind, eps):
    eps = np.asarray(eps, dtype=np.float64)
    if kind is None:
        return eps.copy()
    a, b = _ab(kind)
    if kind[0] == 'linear':
        return (eps - b) / a
    if kind[0] == 'square':
        return np.sqrt(eps)
    if kind[0] == 'tanhsq':
        return np.arctanh(np.sqrt(eps / a))
    return np.arctanh((eps - b) / a)


def to_product(kind):
    """The product's object of a kind of (B)."""
    import krotov_amd

    if kind is None:
        return None
    cls = {'linear': krotov_amd.LinearParametrization, 'square': krotov_amd.SquareParametrization,
           'tanhsq': krotov_amd.TanhSqParametrization, 'tanh': krotov_amd.TanhParametrization}[kind[0]]
    return cls(*kind[1:])


def update_sweep(problem, chi_store, chi_norms, u_guess, kinds, shapes, lambdas, sigma_vals=None, fw_prev=None,
                 store=False, perturb=None):
    """(B): ``oracle.forward_update_sweep`` with the update in u.  ``u_guess``: L arrays.  Returns ``(eps_opt, u_opt,
    fw_T, g_a)`` and, with ``store``, the (K, nt, N) forward states.  ``perturb(l, n, value)``: applied to every f value
    (the ulp experiment of the tests' tolerance)."""
    tl = problem.tlist
    nt = len(tl)
    K, L = problem.K, len(u_guess)
    u_opt = [np.array(u, dtype=np.float64, copy=True) for u in u_guess]
    opt = [np.array(f(kinds[l], np.asarray(u_guess[l], dtype=np.float64)), dtype=np.float64) for l in range(L)]
    c = [dfdu(kinds[l], np.asarray(u_guess[l], dtype=np.float64)) for l in range(L)]
    g_a = np.zeros(L)
    fw = [problem.init[k].copy() for k in range(K)]
    second_order = sigma_vals is not None
    out = np.empty((K, nt, problem.N), dtype=np.complex128) if store else None
    if store:
        out[:, 0] = problem.init
    delta = [np.zeros(problem.N, dtype=np.complex128) for _ in range(K)]
    for n in range(nt - 1):
        dt = tl[n + 1] - tl[n]
        for l in range(L):
            d = 0j
            for k in range(K):
                mu_psi = ko._mu_apply(problem, k, l, fw[k])
                update = np.vdot(chi_store[k, n], mu_psi)
                update *= chi_norms[k]
                if second_order:
                    update += 0.5 * sigma_vals[n] * np.vdot(delta[k], mu_psi)
                d += update
            step = shapes[l][n] / lambdas[l]
            d1 = c[l][n] * d.imag
            u_opt[l][n] = u_guess[l][n] + step * d1
            g_a[l] += step * abs(d1) ** 2 * dt
            value = f(kinds[l], u_opt[l][n])
            opt[l][n] = value if perturb is None else perturb(l, n, value)
        eps = [p[n] for p in opt]
        for k in range(K):
            fw[k] = ko._step(problem, problem.ops[k], eps, dt, fw[k], False, False)
            if second_order:
                delta[k] = fw[k] - fw_prev[k, n + 1]
            if store:
                out[k, n + 1] = fw[k]
    if store:
        return opt, u_opt, np.array(fw), g_a, out
    return opt, u_opt, np.array(fw), g_a


def optimize(problem, guess_pulses, shapes, lambdas, chi_constructor, iter_stop, kinds, edit=None, perturb=None):
    """Iteration 0 + ``iter_stop`` iterations of (B), first order, chi normalised with the 2-norm; u is carried from
    iteration to iteration.  ``edit(iteration, pulses)``: what a ``modify_params_after_iter`` does to the pulses after an
    iteration (returns the controls it changed: their u is inverted again).  Records as ``oracle.optimize``, plus
    ``all_u``."""
    pulses = [np.array(p, dtype=np.float64, copy=True) for p in guess_pulses]
    u = [inverse(kinds[l], pulses[l]) for l in range(len(pulses))]
    fw_T = ko.forward_propagation(problem, pulses)
    tau = ko.tau_vals(problem, fw_T)
    all_pulses, all_u, taus, gas = [np.array(pulses)], [np.array(u)], [tau], [np.zeros(len(pulses))]
    for it in range(1, iter_stop + 1):
        chi_T = chi_constructor(problem, fw_T, tau)
        chi_norms = np.array([float(np.linalg.norm(chi_T[k])) for k in range(problem.K)])
        chi_T = chi_T / chi_norms[:, None]
        chi_store = ko.backward_sweep(problem, chi_T, pulses)
        pulses, u, fw_T, g_a = update_sweep(problem, chi_store, chi_norms, u, kinds, shapes, lambdas, perturb=perturb)
        tau = ko.tau_vals(problem, fw_T)
        if edit is not None:  # (the product records an iteration's pulses behind its hooks)
            for l in edit(it, pulses):
                u[l] = inverse(kinds[l], pulses[l])
        all_pulses.append(np.array(pulses))
        all_u.append(np.array(u))
        taus.append(tau)
        gas.append(g_a)
    return dict(all_pulses=np.array(all_pulses), all_u=np.array(all_u), tau_vals=np.array(taus), g_a=np.array(gas),
                fw_T=fw_T)


# ---------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------
BOUNDS = (-0.4, 0.45)  # the range of the bounded-control cases
LAMBDAS = (2.0, 3.0, 2.5, 3.5, 2.2, 2.8, 3.2, 2.4, 2.6)


def problem(K=3, N=5, L=2, nt=25, T=2.0, seed=12, bands=None):
    """K objectives with their own random Hermitian drift (norm 2) and L shared random Hermitian controls (norm 1.5,
    scaled 0.9 .. 1.1 over the objectives), flat-top update shapes, guess pulses of amplitude <= 0.3 (inside BOUNDS, and
    positive for the odd controls: inside the range of the kinds that are bounded below by zero), lambda_a = LAMBDAS[l].
    ``bands``: every operator keeps only that many diagonals on either side of the main one (a sparse problem)."""
    from krotov_amd import configs

    rng = np.random.default_rng(seed)
    tlist = np.linspace(0.0, T, nt)
    Hl = [configs.herm(rng, N, 1.5) for _ in range(L)]
    mu = np.linspace(0.9, 1.1, K) if K > 1 else np.array([1.0])
    H0 = [configs.herm(rng, N, 2.0) for _ in range(K)]
    if bands is not None:
        keep = np.abs(np.subtract.outer(np.arange(N), np.arange(N))) <= bands
        Hl = [h * keep for h in Hl]
        H0 = [h * keep for h in H0]
    Hc = [[mu[k] * Hl[l] for l in range(L)] for k in range(K)]
    init = np.zeros((K, N), dtype=np.complex128)
    init[:, 0] = 1.0
    target = np.zeros((K, N), dtype=np.complex128)
    target[:, 1] = 1.0

    def make_guess(l):
        if l % 2 == 0:
            return lambda t, args: 0.3 * np.sin((l + 2) * np.pi * t / T)  # (whole periods: both signs)
        return lambda t, args: 0.05 + 0.2 * np.sin((l + 1) * np.pi * t / T) ** 2

    def S(t):
        return ko.flattop(t, 0.0, T, 0.1 * T)

    spec = configs.ProblemSpec(
        name='par_K%d_N%d_L%d' % (K, N, L), H0=H0, Hc=Hc, is_super=False, init=init, target=target, tlist=tlist,
        controls=[make_guess(l) for l in range(L)], update_shape=S, lambda_a=None, chi='re', mu=mu)
    spec.lambdas = [LAMBDAS[l] for l in range(L)]
    return spec


def oracle_side(spec):
    """(problem, guess_pulses, shapes, lambdas) of a spec of :func:`problem` through the oracle."""
    ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    prob = ko.OracleProblem(ops, spec.init, spec.target, spec.tlist, spec.is_super, spec.weights)
    _, gp, S = ko.initialize_controls(spec.controls, [spec.update_shape] * spec.L, spec.tlist)
    return prob, gp, S, list(spec.lambdas)


def product_side(spec, kinds):
    """(objectives, pulse_options) for ``krotov_amd.optimize_pulses``: flat state vectors, ``parametrization`` set for
    every control whose kind is not None."""
    import krotov_amd
    from krotov_amd import configs

    objectives, _ = configs.spec_to_objectives(spec, krotov_amd, column_states=False)
    pulse_options = {}
    for l, c in enumerate(spec.controls):
        pulse_options[c] = dict(lambda_a=spec.lambdas[l], update_shape=spec.update_shape)
        if kinds is not None and kinds[l] is not None:
            pulse_options[c]['parametrization'] = to_product(kinds[l])
    return objectives, pulse_options
