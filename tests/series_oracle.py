"""A NumPy restatement of what the device's per-interval series computes, and a derived bound on what it may cost.

Test infrastructure, NumPy only (tests/test_series_tolerance.py).

``series_step`` applies, to one state over one interval, ``nsub`` sub-steps of the polynomial the library exports for the
degree that ``helpers.series_plan`` selects from the exported thresholds -- nothing else: no exponential, no remainder
estimate of its own.  ``SeriesOracle`` plugs it into the three sweeps of ``oracle/krotov_oracle.py`` in place of the exact
step (a context manager like ``helpers.MemoExpm``: the oracle is restored on exit).  An engine that uses the same table
must agree with these sweeps to rounding, at any truncation tolerance.

``tolerance_bound`` bounds the distance between such sweeps (or the device's) and the EXACT oracle from the tolerance, the
plan and the problem alone; nothing in it is fitted to a result.
"""
import collections

import numpy as np

import helpers as hp
from oracle import krotov_oracle as ko

# theta[m]: thresholds; coeff[m][:m + 1]: the polynomial of degree m; round_up: the two-terms-per-phase kernels evaluate an
# odd degree m of an even-only table (Taylor's thresholds are all distinct) as degree m + 1
Table = collections.namedtuple('Table', 'name theta coeff round_up tol cap defect')

_tables = {}


def table(name, tol=0.0, cap=2.0, defect=0.0, round_up=False):
    """'taylor' | 'real' (Chebyshev form, cap ``cap``) | 'defect' (the same with the margin for ``defect``) | 'odd' (the
    table of the two-terms-per-phase kernels) at the tolerance ``tol``, from the library's exported host code."""
    key = (name, tol, cap, defect, round_up)
    if key not in _tables:
        if name == 'taylor':
            theta, coeff = hp.series_taylor_coefficients(tol)
        elif name == 'odd':
            theta, coeff = hp.series_tables_odd(tol)
        elif name in ('real', 'defect'):
            theta, coeff = hp.series_coefficients(cap, tol, defect if name == 'defect' else 0.0)
        else:
            raise KeyError(name)
        _tables[key] = Table(name, theta, coeff, round_up, tol, cap, defect)
    return _tables[key]


def at_tolerance(tab, tol):
    """The same form of table at another tolerance."""
    return table(tab.name, tol, tab.cap, tab.defect, tab.round_up)


def polynomial(tab, m):
    """The coefficients c_0 ... c_m' of the polynomial a kernel evaluates where the plan says degree ``m``."""
    if tab.round_up and m % 2 == 1:
        m += 1
    return tab.coeff[m, :m + 1]


def products(tab, nsub, deg, two_terms=False):
    """Matrix-vector products of the series under a plan: one per term; the two-terms-per-phase kernels P + 1 per sub-step
    of degree 2P (or of 2P - 1 rounded up), P at degree 2P - 1 of the table with odd degrees
    (tests/test_q2_odd_degrees.py: _products)."""
    nsub, deg = np.asarray(nsub), np.asarray(deg)
    if not two_terms:
        return int((nsub * deg).sum())
    per = (deg + 1) // 2 + np.where((deg % 2 == 1) & (tab.name == 'odd'), 0, 1)
    return int((nsub * per).sum())


def series_step(ops, norms, eps, dt, v, table, theta_max, backwards, is_super=False, theta_of=None):
    """One interval: theta = dt (n_0 + sum_l |eps_l| n_l) from the norm bounds ``norms`` (1 + L), (nsub, degree) from
    ``helpers.series_plan``, then ``nsub`` times v <- sum_j c_j Z^j v (Horner, one product per term) with
    Z = f (H0 + sum_l eps_l H_l) dt / nsub.  ``theta_of(norms, eps, dt)``: a plan from outside -- the theta the series is
    planned with, whatever the generator (a witness evaluates what a wrongly planned kernel would compute)."""
    eps = np.asarray(eps, dtype=np.complex128).reshape(-1)
    theta = dt * (norms[0] + float(np.dot(np.abs(eps), norms[1:]))) if theta_of is None else float(theta_of(norms, eps, dt))
    nsub, deg = hp.series_plan([theta], theta_max, table.theta)
    nsub, c = int(nsub[0]), polynomial(table, int(deg[0]))
    f = ko._eqm_factor(is_super, backwards) * (dt / nsub)
    terms = [(ops[0], f)] + [(ops[l], f * eps[l - 1]) for l in range(1, len(ops)) if ops[l] is not None]

    def Z(x):
        out = terms[0][1] * (terms[0][0] @ x)
        for op, a in terms[1:]:
            out = out + a * (op @ x)
        return out

    v = np.asarray(v, dtype=np.complex128)
    for _ in range(nsub):
        out = c[-1] * v
        for cj in c[-2::-1]:
            out = Z(out) + cj * v
        v = out
    return v


class SeriesOracle:
    """Context manager: the sweeps of ``ko`` on ``prob`` take ``series_step`` (norm bounds ``bounds`` (K, 1 + L), ``table``,
    ``theta_max``) instead of the exact step.  ``ko.step`` and ``prob.adjoint_ops`` are restored on exit.  ``theta_of``:
    ``series_step``'s plan from outside."""

    def __init__(self, prob, bounds, table, theta_max, theta_of=None):
        self.prob, self.bounds, self.table, self.theta_max = prob, np.asarray(bounds), table, theta_max
        self.theta_of = theta_of

    def __enter__(self):
        prob = self.prob
        self._step = ko.step
        adj = prob.adjoint_ops()
        prob.adjoint_ops = lambda: adj  # (one list per objective that the step can recognise)
        who = {id(row): k for rows in (prob.ops, adj) for k, row in enumerate(rows)}
        self._keep = adj

        def step(ops_k, eps_n, dt, state, is_super=False, backwards=False, use_scipy=False):
            return series_step(ops_k, self.bounds[who[id(ops_k)]], eps_n, dt, state, self.table, self.theta_max, backwards,
                               is_super, self.theta_of)

        ko.step = step
        return self

    def __exit__(self, *exc):
        ko.step = self._step
        del self.prob.adjoint_ops
        return False


def plan(obj, pulses, theta_max, tab, bounds=None):
    """(theta, nsub, degree), each (K, M), of a regime problem under ``pulses``."""
    theta = hp.theta_sequence(obj, pulses, bounds)
    both = [hp.series_plan(row, theta_max, tab.theta) for row in theta]
    return theta, np.array([b[0] for b in both]), np.array([b[1] for b in both])


def threshold_distance(theta, nsub, theta_max, tab):
    """The smallest relative distance of any theta_n / nsub_n to a threshold of the table, and of theta_n / theta_max to
    the integer at which the sub-step count changes: beyond ~1e-13 the device's own rounding of theta cannot change
    the plan."""
    th = (np.asarray(theta) / nsub).ravel()
    edges = np.unique(tab.theta[1:])
    edges = edges[edges > 0.0]
    d = np.abs(th[:, None] - edges[None, :]) / edges[None, :]
    r = (np.asarray(theta) / theta_max).ravel()
    at = np.maximum(np.round(r), 1.0)
    return min(float(d.min()), float((np.abs(r - at) / at).min()))


# ---------------------------------------------------------------------------
# the derived bound
# ---------------------------------------------------------------------------
def _growth_rates(prob, pulses):
    """mu[k, n]: the largest eigenvalue of the Hermitian part of f A_kn (A = H0 + sum_l eps_ln H_l); exactly 0 where f = -i
    and every operator is Hermitian.  The adjoint generator f^* A^+ has the same Hermitian part."""
    K, M = prob.K, len(prob.tlist) - 1
    mu = np.zeros((K, M))
    f = ko._eqm_factor(prob.is_super, False)
    memo = {}
    for k in range(K):
        row = prob.ops[k]
        present = [op for op in row if op is not None]
        if not prob.is_super and all(np.array_equal(op, op.conj().T) for op in present):
            continue
        key = tuple(id(op) for op in row)
        for n in range(M):
            kn = key + tuple(float(p[n]) for p in pulses)
            if kn not in memo:
                A = f * row[0]
                for l in range(1, len(row)):
                    if row[l] is not None:
                        A = A + (f * pulses[l - 1][n]) * row[l]
                memo[kn] = float(np.linalg.eigvalsh(0.5 * (A + A.conj().T))[-1])
            mu[k, n] = memo[kn]
    return mu


WIDEN = 0.01  # the update sweep's refined step errors are taken on [-theta (1 + WIDEN), theta (1 + WIDEN)]


def step_errors(obj, prob, pulses, theta_max, tab, tol, widen=0.0):
    """(K, M) bounds on || p(Z) - exp(Z) || of one sub-step.  ``tol`` in general (the tables' own guarantee for every
    generator with ||Z|| <= theta).  Where f = -i and every operator of the objective is Hermitian, Z is normal with its
    spectrum in i [-theta, theta], so the distance is the largest |p(ix) - exp(ix)| over that interval -- often far below
    ``tol``, since a degree serves every theta up to its threshold: evaluated on a grid of 257 points in extended
    precision, with 2 % on top for the grid, never more than ``tol``.  ``widen``: on an interval that much wider (the
    update sweep of a run under test sees pulses that differ from the exact oracle's; ``tolerance_bound`` falls back to
    ``tol`` where its own bound on that difference moves theta by more)."""
    theta, nsub, deg = plan(obj, pulses, theta_max, tab)
    out = np.full(theta.shape, float(tol))
    x = np.linspace(-1.0, 1.0, 257).astype(np.clongdouble)
    memo = {}
    for k in range(prob.K):
        present = [op for op in prob.ops[k] if op is not None]
        if prob.is_super or not all(np.array_equal(op, op.conj().T) for op in present):
            continue
        for n in range(theta.shape[1]):
            key = (int(deg[k, n]), float(theta[k, n] / nsub[k, n]) * (1.0 + widen))
            if key not in memo:
                z = 1j * np.clongdouble(key[1]) * x
                p = hp.series_polynomial(polynomial(tab, key[0]), z, np.clongdouble)
                memo[key] = 1.02 * float(np.abs(p - np.exp(z)).max())
            out[k, n] = min(float(tol), memo[key])
    return out


def _substeps(e, x, nsub, g_sub, tol):
    """nsub sub-steps, each within ``tol`` (operator norm) of the exact one, whose norm is at most g_sub: the distance
    e_{j+1} <= g_sub e_j + tol (x_j + e_j) to the exact state (x_j <= g_sub^j x: its norm)."""
    for _ in range(int(nsub)):
        e = g_sub * e + tol * (x + e)
        x = g_sub * x
    return e


def tolerance_bound(obj, tol, plans, ref, so=False):
    """The derived bound: statement, derivation and arguments in ``_tolerance_bound`` below."""
    # (where the feedback term blows up the bound overflows to inf / nan: such a bound is empty, and the caller says so)
    with np.errstate(over='ignore', invalid='ignore'):
        return _tolerance_bound(obj, tol, plans, ref, so)


def _tolerance_bound(obj, tol, plans, ref, so):
    """Upper bounds on the 2-norm distance between sweeps whose every sub-step is within ``tol`` (operator norm) of the
    exact exponential and the exact oracle's sweeps ``ref`` (``tests/test_series_regimes.py: reference`` with states).

    Plain sweeps, per objective:  e_{n+1} <= g_n (e_n + nsub_n tol ||state_n||), g_n = exp(dt_n max(0, mu_n)) -- resolved
    per sub-step (``_substeps``), with ||state|| <= ||exact state|| + e.  mu_n: ``_growth_rates``.

    Update sweep: the pulse error of interval n is at most
        d_ln = S_ln / lambda_l sum_k h_kl [c_k (e^chi_kn ||phi_kn|| + (||chi_kn|| + e^chi_kn) e^phi_kn)
                                           + |sigma_n| / 2 e^phi_kn (||phi_kn|| + ||Delta phi_kn|| + e^phi_kn)]
    (h_kl >= ||H_kl||: the norm bounds; c_k: ``chi_norms``; the sigma term in second order only, and not at n = 0), it
    perturbs the generator of the step by at most E_kn = dt_n sum_l h_kl d_ln, and ||exp(Z + E) - exp(Z)|| <=
    ||E|| g_n exp(||E||).

    ``plans``: dict(guess=nsub (K, M) under the guess pulses, opt=nsub under the updated ones; optionally tol_guess,
    and tol_opt (with ``widen=WIDEN``) + theta_opt: ``step_errors`` in place of ``tol``).  Returns a dict of arrays: 'states', 'chi', 'upd' (K, M + 1),
    'opt' (L, M), 'g_a' (L,)."""
    tol_guess = plans.get('tol_guess', np.full(plans['guess'].shape, float(tol)))
    tol_opt = plans.get('tol_opt', np.full(plans['opt'].shape, float(tol)))
    prob = ref['prob']
    K, M, L = prob.K, len(prob.tlist) - 1, prob.L
    dt = np.diff(prob.tlist)
    h = hp.series_bounds(obj)  # (true upper bounds on the spectral norms)
    guess, opt = [np.asarray(p) for p in obj.pulses], [np.asarray(p) for p in ref['opt']]
    g_guess = np.exp(dt[None, :] * np.maximum(0.0, _growth_rates(prob, guess)))
    g_opt = np.exp(dt[None, :] * np.maximum(0.0, _growth_rates(prob, opt)))
    x_fw = np.linalg.norm(ref['states'], axis=2)
    x_bw = np.linalg.norm(ref['chi'], axis=2)
    out = {name: np.zeros((K, M + 1)) for name in ('states', 'chi', 'upd')}
    for k in range(K):
        for n in range(M):
            ns = plans['guess'][k, n]
            out['states'][k, n + 1] = _substeps(out['states'][k, n], x_fw[k, n], ns, g_guess[k, n] ** (1.0 / ns),
                                                tol_guess[k, n])
        for n in range(M - 1, -1, -1):
            ns = plans['guess'][k, n]
            out['chi'][k, n] = _substeps(out['chi'][k, n + 1], x_bw[k, n + 1], ns, g_guess[k, n] ** (1.0 / ns),
                                         tol_guess[k, n])
    # the update sweep: exact forward states under the updated pulses
    x_up = ref['store'] if so else None
    if x_up is None:
        with hp.MemoExpm():
            x_up = ko.forward_propagation(prob, opt, store=True)[1]
    x_un = np.linalg.norm(x_up, axis=2)
    delta = np.linalg.norm(x_up - ref['prev'], axis=2) if so else np.zeros((K, M + 1))
    sigma = np.abs(ref['sigma']) if so else np.zeros(M)
    S, lam, c = np.array(obj.shapes), np.array(obj.lambdas), np.asarray(ref['norms'])
    e_chi, e = out['chi'], np.zeros(K)
    out['opt'], out['g_a'] = np.zeros((L, M)), np.zeros(L)
    d_exact = np.abs(np.array(opt) - np.array(guess))  # S / lambda |Im D| of the exact sweep
    for n in range(M):
        per_k = c * (e_chi[:, n] * x_un[:, n] + (x_bw[:, n] + e_chi[:, n]) * e)
        if so and n > 0:
            per_k = per_k + 0.5 * sigma[n] * e * (x_un[:, n] + delta[:, n] + e)
        for l in range(L):
            d = S[l, n] / lam[l] * float(np.dot(h[:, 1 + l], per_k))
            out['opt'][l, n] = d
            if S[l, n] > 0.0:  # g_a = sum_n S / lambda |Im D|^2 dt = sum_n lambda / S (delta eps)^2 dt
                out['g_a'][l] += lam[l] / S[l, n] * dt[n] * d * (2.0 * d_exact[l, n] + d)
        for k in range(K):
            E = dt[n] * float(np.dot(h[k, 1:], out['opt'][:, n]))
            g = g_opt[k, n]
            ns = plans['opt'][k, n]
            refined = 'theta_opt' in plans and E <= WIDEN * plans['theta_opt'][k, n]
            series = _substeps(0.0, x_un[k, n] + e[k], ns, (g * np.exp(E)) ** (1.0 / ns), tol_opt[k, n] if refined else tol)
            e[k] = series + E * g * np.exp(E) * (x_un[k, n] + e[k]) + g * e[k]
        out['upd'][:, n + 1] = e
    return out
