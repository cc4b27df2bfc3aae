"""Shared test helpers: golden loading and spec -> oracle conversion."""
import os

import numpy as np

from oracle import krotov_oracle as ko

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

CHI = {'re': ko.chis_re, 'ss': ko.chis_ss, 'sm': ko.chis_sm, 'hs': ko.chis_hs}

# name: builder of krotov_amd.configs -> spec; tests/test_reference_dump_compat.py and the fixtures
# make_reference_goldens.py dump_continue made for it
DUMP_CONTINUE_CASES = {
    'c1': lambda c: c.config_c1(nt=80),
    'c5_L3': lambda c: c.config_c5(K=3, N=6, nt=41, L=3, distinct=True),
}


# the reference-loop fixtures on two- and three-point grids (tests/golden/make_reference_goldens.py makes them; the GPU and
# the oracle tests rebuild the same specs): name -> (builder of krotov_amd.configs, guess amplitude)
SHORT_GRID_CASES = {
    'ref_c5_nt2': (lambda c: c.config_c5(K=6, N=16, nt=2, L=1), 0.5),
    'ref_c5_nt3': (lambda c: c.config_c5(K=6, N=16, nt=3, L=1), 0.5),
    'ref_c3_nt2': (lambda c: c.config_c3(nt=2), 0.3),
}


def short_grid_spec(name, configs):
    """A spec of SHORT_GRID_CASES: ``update_shape = 1`` and a guess control that is non-zero on the whole grid, amplitude x
    (0.4 + 0.6 t / T) -- the configs' own flat-tops and guesses vanish at both ends of the grid, which on one or two
    intervals leaves the update nothing to do."""
    builder, amplitude = SHORT_GRID_CASES[name]
    spec = builder(configs)
    T = float(spec.tlist[-1])
    spec.update_shape = lambda t: 1.0
    spec.controls = [lambda t, args, l=l: amplitude * (1.0 + 0.5 * l) * (0.4 + 0.6 * t / T) for l in range(spec.L)]
    return spec


def golden(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def spec_to_oracle(spec):
    ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    return ko.OracleProblem(ops, spec.init, spec.target, spec.tlist, spec.is_super, spec.weights)


def oracle_controls(spec):
    """(guess_pulses, shape_arrays, lambdas) of a spec through the oracle."""
    _, gp, S = ko.initialize_controls(spec.controls, [spec.update_shape] * spec.L, spec.tlist)
    return gp, S, [spec.lambda_a] * spec.L


def oracle_optimize(spec, iter_stop, **kw):
    gp, S, lam = oracle_controls(spec)
    # numpy-mode reference runs pass norm=np.linalg.norm (notebook 09, cell 35)
    kw.setdefault('norm', lambda prob, chi: float(np.linalg.norm(chi)))
    return ko.optimize(spec_to_oracle(spec), gp, S, lam, CHI[spec.chi], iter_stop, **kw)


class SigmaA:
    """sigma(t) = -max(epsA, 2A + epsA) with A re-estimated every iteration (the
    reference's notebook 07, cell 30); oracle-side array form of the Sigma used
    for tests/golden/ref_so_c3.npz."""

    def __init__(self, A=0.0, epsA=2.0):
        self.A, self.epsA, self.history = A, epsA, []

    def __call__(self, t):
        return -max(self.epsA, 2 * self.A + self.epsA)

    def refresh(self, fw_T, fw_T0, chi_T, chi_norms, taus):
        J = lambda tau: 1 - abs(np.sum(tau) / len(tau)) ** 2  # noqa: E731  (J_T_sm)
        self.A = ko.numerical_estimate_A(fw_T, fw_T0, chi_T, chi_norms, J(taus[-1]) - J(taus[-2]))
        self.history.append(self.A)


def product_sigma(A=0.0, epsA=2.0):
    """The same sigma through the product's plugin surface: a
    ``krotov_amd.second_order.Sigma`` subclass whose ``refresh`` calls
    ``krotov_amd.second_order.numerical_estimate_A`` with Delta J_T (J_T_sm) taken
    from ``result.tau_vals``."""
    import krotov_amd
    from krotov_amd.second_order import Sigma, numerical_estimate_A

    class _Sigma(Sigma):
        def __init__(self):
            self.A, self.epsA, self.history, self.calls = A, epsA, [], []

        def __call__(self, t):
            return -max(self.epsA, 2 * self.A + self.epsA)

        def refresh(self, forward_states, forward_states0, chi_states, chi_norms, optimized_pulses, guess_pulses,
                    objectives, result):
            J = krotov_amd.functionals.J_T_sm
            dJ = J(None, objectives, tau_vals=result.tau_vals[-1]) - J(None, objectives, tau_vals=result.tau_vals[-2])
            self.A = numerical_estimate_A(forward_states, forward_states0, chi_states, chi_norms, dJ)
            self.history.append(self.A)
            self.calls.append((len(forward_states), len(forward_states[0]), guess_pulses is optimized_pulses))

    return _Sigma()


def numpy_plugins(is_super=False):
    """propagator / mu / overlap callables as in reference notebook 09."""

    def propagator(H, state, dt, c_ops=None, backwards=False, initialize=False):
        f = (1.0 + 0j) if is_super else -1j
        if backwards:
            f = f.conjugate()
        A = f * H[0]
        for part in H[1:]:
            A = A + (f * part[1]) * part[0]
        return ko.expm_dense(A * dt, use_scipy=False) @ state

    def mu(objs, i_obj, pulses, mapping, i_pulse, n):
        op = objs[i_obj].H[1 + i_pulse][0]
        return (lambda s: 1j * (op @ s)) if is_super else (lambda s: op @ s)

    def overlap(a, b):
        return complex(np.vdot(a, b))

    return propagator, mu, overlap


def check_infohook_chaining(**optimize_kwargs):
    """The scenario of reference tests/test_infohooks.py:15-72 (5-level transmon, two
    intervals, lambda_a halved after every iteration by modify_params_after_iter, two
    chained info_hooks) through ``krotov_amd.optimize_pulses(**optimize_kwargs)``."""
    import scipy.linalg

    import krotov_amd

    Ec, EjEc, nstates, T = 0.386, 45, 2, 10.0
    Ej = EjEc * Ec
    n = np.arange(-nstates, nstates + 1)
    up = np.diag(np.ones(2 * nstates), k=-1)
    H0 = (np.diag(4 * Ec * n**2) - Ej * (up + up.T) / 2.0).astype(complex)
    H1 = (-2 * np.diag(n)).astype(complex)
    eigenvals, eigenvecs = scipy.linalg.eig(H0)
    ndx = np.argsort(eigenvals.real)
    E, V = eigenvals[ndx].real, eigenvecs[:, ndx]
    w01 = E[1] - E[0]
    psi0, psi1 = V[:, 0].astype(complex), V[:, 1].astype(complex)
    eps0 = lambda t, args: 0.5 * np.exp(-40.0 * (t / T - 0.5) ** 2) * np.cos(8 * np.pi * w01 * t)  # noqa: E731
    H = [H0, [H1, eps0]]
    obj = krotov_amd.Objective(initial_state=psi0, target=psi1, H=H)
    tlist = np.array([0, 0.01, 0.02])
    printed = []

    def adjust_lambda_a(**args):
        before = args['lambda_vals'][0]
        args['lambda_vals'][0] *= 0.5
        args['shared_data'].setdefault('messages', []).append('λₐ: %s → %s' % (before, args['lambda_vals'][0]))

    def print_fidelity(**args):
        F_re = np.average(np.array(args['tau_vals']).real)
        printed.append("Iteration %d: \tF = %f" % (args['iteration'], F_re))
        return F_re

    def print_messages(**args):
        if 'messages' in args['shared_data']:
            message = "; ".join(args['shared_data']['messages'])
            printed.append("\tmsg: " + message)
            return message

    import io

    report = io.StringIO()

    def debug_information(**args):  # the full-signature hook works on whatever state containers the path hands out
        krotov_amd.info_hooks.print_debug_information(out=report, **args)

    res = krotov_amd.optimize_pulses(
        [obj], pulse_options={H[1][1]: dict(lambda_a=1, update_shape=1)}, tlist=tlist,
        chi_constructor=krotov_amd.functionals.chis_re,
        info_hook=krotov_amd.info_hooks.chain(print_fidelity, print_messages, debug_information),
        modify_params_after_iter=adjust_lambda_a, iter_stop=2, **optimize_kwargs)
    out = "\n".join(printed)
    assert report.getvalue().count('    storage (bw, fw, fw0): [1 * ') == 2  # iterations 1 and 2
    assert '    fw_states_T norm: 1.000000\n' in report.getvalue()
    assert len(res.info_vals) == 3
    assert isinstance(res.info_vals[1], tuple) and len(res.info_vals[1]) == 2
    assert abs(res.info_vals[1][0] - 0.001978333994757067) < 1e-8
    assert res.info_vals[1][1] == 'λₐ: 0.5 → 0.25'
    assert 'Iteration 0: \tF = 0.000000' in out
    assert 'msg: λₐ: 1.0 → 0.5' in out
    assert 'Iteration 1: \tF = 0.001978' in out
    assert 'msg: λₐ: 0.5 → 0.25' in out
    return res


# ---------------------------------------------------------------------------
# Regimes of the per-interval series (tests/test_series_regimes.py, tests/fuzz_parity.py --regimes)
# ---------------------------------------------------------------------------
# Pure NumPy.  A *regime problem* is a ProblemSpec (uniform or ``config_mixed``) or a Lindblad ``Case`` (anything with
# ``H`` / ``C`` / ``dt``) that carries its interval values explicitly -- ``pulses`` (L arrays of nt - 1 values), ``shapes``,
# ``lambdas`` -- because a non-uniform grid and pulse values of exactly 0.0 cannot be expressed through the
# callable -> mid-point -> interval conversion of ``oracle_controls``.  ``fmt``: 'dense' | 'csr' | 'mixed' | 'lindblad'.

# theta_n / theta_max along a ramp (log-linear between these levels): up through one, two and three sub-steps and down
# again through other values than on the way up, from <= 1e-3 to 2.9 and back
RAMP_LEVELS = (7e-4, 6e-2, 0.2, 1.5, 2.9, 2.6, 1.8, 0.5, 0.06, 2e-3, 5e-5)
RAMP_MIN_INTERVALS = len(RAMP_LEVELS)
PULSE_RAMP_DT = 0.02   # uniform grid of the pulse ramps: dt x this, so that the drift alone is at degree ~6
PULSE_RAMP_FLOOR = 1e-4  # smallest pulse amplitude of a pulse ramp relative to its largest (where the drift alone exceeds the level)


def _is_lindblad(obj):
    return hasattr(obj, 'C') and hasattr(obj, 'H')


def ramp_profile(M, periods=1):
    """theta_n / theta_max on M intervals: every level of RAMP_LEVELS (``periods`` times over) on an interval of its own,
    interpolated in the logarithm in between."""
    levels = np.log(np.array(RAMP_LEVELS * periods))
    at = np.round(np.arange(len(levels)) * (M - 1.0) / (len(levels) - 1.0))
    return np.exp(np.interp(np.arange(M), at, levels))


def explicit(obj, fmt=None):
    """A shallow copy of ``obj`` with explicit ``pulses`` / ``shapes`` / ``lambdas`` (those of ``oracle_controls`` unless
    it has them already) and ``fmt``."""
    import copy

    new = copy.copy(obj)
    if getattr(new, 'pulses', None) is None:
        gp, S, lam = oracle_controls(obj)
        new.pulses, new.shapes, new.lambdas = [np.array(p) for p in gp], [np.array(s) for s in S], list(lam)
    if fmt is not None or not hasattr(new, 'fmt'):
        new.fmt = fmt or ('lindblad' if _is_lindblad(obj) else 'mixed' if hasattr(obj, 'kinds') else 'dense')
    return new


def regime_dt(obj):
    return np.asarray(obj.dt, dtype=np.float64) if _is_lindblad(obj) else np.diff(obj.tlist)


def _set_dt(obj, dt):
    obj.tlist = np.concatenate([[0.0], np.cumsum(dt)])
    if _is_lindblad(obj):
        obj.dt = np.asarray(dt, dtype=np.float64)


def series_bounds(obj, norm=None, factor=1.0):
    """(K, 1 + L) norm bounds (n_0, n_l) with theta_n = dt_n (n_0 + sum_l |eps_l[n]| n_l): the formulas of
    ``HipKrotovEngine._create_dense`` (2-norm), ``_create_sparse`` (sqrt(||A||_1 ||A||_inf)) and ``_create_lindblad`` +
    ``kh_engine_create_lindblad`` (Hermitian Hamiltonian part: half the spread of its spectrum; n_0 = 2 ||H0|| +
    2 sum_j ||C_j||^2, n_l = 2 ||H_l||), restated.  ``norm='frobenius'``: what the library computes when it gets no
    bounds (``op_norms='frobenius'``); ``factor``: every operator's bound times this (a caller's loose bound)."""
    cache = {}

    def two(op):
        return float(np.linalg.norm(np.asarray(op), 2))

    def csr(op):
        a = np.abs(np.asarray(op))
        return float(np.sqrt(a.sum(axis=0).max() * a.sum(axis=1).max()))

    def ham(op):
        op = np.asarray(op)
        if np.array_equal(op, op.conj().T):
            ev = np.linalg.eigvalsh(op)
            return 0.5 * float(ev[-1] - ev[0])
        return two(op)

    def fro(op):
        return float(np.linalg.norm(np.asarray(op), 'fro'))

    def bound(op, fn):
        if op is None:
            return 0.0
        if norm == 'frobenius':
            fn = fro
        if id(op) not in cache:
            cache[id(op)] = (factor * fn(op), op)
        return cache[id(op)][0]

    if _is_lindblad(obj):
        out = np.zeros((obj.K, 1 + obj.L))
        for k in range(obj.K):
            out[k] = [2.0 * bound(h, ham) for h in obj.H[k]]
            out[k, 0] += 2.0 * sum(bound(c, two) ** 2 for c in obj.C[k] if c is not None)
        return out
    fn = csr if obj.fmt == 'csr' else two
    return np.array([[bound(obj.H0[k], fn)] + [bound(obj.Hc[k][l], fn) for l in range(obj.L)] for k in range(obj.K)])


def n_pulses(obj):
    """Rows of ``pulses`` / ``shapes`` / ``lambdas``: the L controls, or -- a problem with a term table ``obj.terms``, L
    pairs (control, power): slot j carries eps_c(j)^p_j H_j (tests/test_nonlinear_axes.py) -- its C controls."""
    terms = getattr(obj, 'terms', None)
    return obj.L if not terms else max(c for c, _ in terms) + 1


def theta_sequence(obj, pulses=None, bounds=None, terms=None):
    """theta[k, n] of a regime problem under ``pulses`` (default: its own guess) and the norm bounds ``bounds`` (default:
    ``series_bounds(obj)``).  With a term table (``terms``, default ``obj.terms``) the pulses are the C pulses eps_c and
    theta_n = dt_n (n_0 + sum_j |eps_c(j)[n]|^p_j n_j): what the series sees are the coefficient pulses."""
    b = series_bounds(obj) if bounds is None else bounds
    terms = getattr(obj, 'terms', None) if terms is None else terms
    eps = np.abs(np.array(obj.pulses if pulses is None else pulses, dtype=np.float64))
    if terms:
        eps = eps.reshape(max(c for c, _ in terms) + 1, -1)
        eps = np.array([eps[c] ** p for c, p in terms])
    eps = eps.reshape(obj.L, -1)
    return regime_dt(obj)[None, :] * (b[:, :1] + b[:, 1:] @ eps)


def _bisect(f, target, iterations=200):
    """The a >= 0 (an array, like ``target``) with f(a) = target for f monotone rising, f(0) <= target; to rounding."""
    target = np.asarray(target, dtype=np.float64)
    lo, hi = np.zeros_like(target), np.ones_like(target)
    for _ in range(1100):
        low = f(hi) < target
        if not np.any(low):
            break
        hi = np.where(low, 2.0 * hi, hi)
    assert not np.any(f(hi) < target), "no bracket: f stays below the target"
    for _ in range(iterations):
        mid = 0.5 * (lo + hi)
        low = f(mid) < target
        lo, hi = np.where(low, mid, lo), np.where(low, hi, mid)
    return 0.5 * (lo + hi)


def _scale_operators(obj, factor):
    """Every generator x ``factor``; objects shared between objectives stay shared (one scaled copy per distinct array)."""
    made = {}

    def s(op, f=factor):
        if op is None:
            return None
        if (id(op), f) not in made:
            made[id(op), f] = (f * op, op)
        return made[id(op), f][0]

    if _is_lindblad(obj):  # (the dissipator is quadratic in C)
        obj.H = [[s(h) for h in row] for row in obj.H]
        obj.C = [[s(c, np.sqrt(factor)) for c in row] for row in obj.C]
    else:
        obj.H0 = [s(h) for h in obj.H0]
        obj.Hc = [[s(h) for h in row] for row in obj.Hc]


def _largest(obj):
    """The objective with the largest theta under the guess pulses, and theta_n / dt_n of it."""
    rate = theta_sequence(obj) / regime_dt(obj)[None, :]
    k = int(np.argmax(rate.max(axis=1)))
    return k, rate[k]


def regime_ramp(obj, theta_max):
    """Non-uniform grid: dt_n such that theta_n of the objective with the largest norms follows ``ramp_profile`` under the
    guess pulses -- from <= 1e-3 theta_max up to 2.9 theta_max (three sub-steps) and back; the pulses keep their interval
    values."""
    new = explicit(obj)
    M = len(regime_dt(new))
    if M < RAMP_MIN_INTERVALS:
        raise ValueError("a ramp needs at least %d intervals" % RAMP_MIN_INTERVALS)
    _set_dt(new, theta_max * ramp_profile(M) / _largest(new)[1])
    return new


def regime_pulse_ramp(obj, theta_max, periods=1, zeros=True, steps=None):
    """Uniform grid (dt x PULSE_RAMP_DT: the drift alone sits at a low degree); every guess pulse is replaced by
    a_n (0.3 + |guess|) with a_n such that theta_n follows ``ramp_profile`` (a_n >= PULSE_RAMP_FLOOR max a where the drift
    alone is beyond the level), and is exactly 0.0 on the first and the last interval and on the first interval of the way
    down that needs no sub-steps.  ``zeros='inner'``: only the latter; ``steps``: step-width factors <= 1, repeated along
    the grid (a non-uniform grid under the same theta_n)."""
    new = explicit(obj)
    dt = regime_dt(new)
    M = len(dt)
    if M < RAMP_MIN_INTERVALS * periods:
        raise ValueError("a ramp needs at least %d intervals" % (RAMP_MIN_INTERVALS * periods))
    _set_dt(new, dt * PULSE_RAMP_DT * (1.0 if steps is None else np.resize(np.asarray(steps, dtype=np.float64), M)))
    new.pulses = [0.3 + np.abs(p) for p in new.pulses]
    k, rate = _largest(new)
    drift = series_bounds(new)[k, 0]
    if drift * regime_dt(new).max() >= theta_max:
        raise ValueError("the drift alone is beyond theta_max")
    profile = ramp_profile(M, periods)
    if getattr(new, 'terms', None):
        # a term table: dt_n (n_0 + sum_j |a_n e_c(j)[n]|^p_j n_j) = theta_max profile_n is monotone in a_n -- bisection;
        # the objective whose theta is the largest under the result (it may change with a: looked for again, twice)
        e = np.abs(np.array(new.pulses))
        for _ in range(3):
            b = series_bounds(new)[k]
            a = _bisect(lambda a: b[0] + sum(b[1 + j] * (a * e[c]) ** p for j, (c, p) in enumerate(new.terms)),
                        theta_max * profile / regime_dt(new))
            a = np.maximum(a, PULSE_RAMP_FLOOR * a.max())
            top = int(np.argmax(theta_sequence(new, a * e).max(axis=1)))
            if top == k:
                break
            k = top
    else:
        a = (theta_max * profile / regime_dt(new) - drift) / (rate - drift)
        a = np.maximum(a, PULSE_RAMP_FLOOR * a.max())
    new.pulses = [a * p for p in new.pulses]
    if zeros:
        falling = [n for n in range(1, M) if profile[n] < 1.0 <= profile[n - 1]]  # (one per period)
        for n in ([] if zeros == 'inner' else [0, M - 1]) + falling:
            for p in new.pulses:
                p[n] = 0.0
    return new


def regime_tiny(obj, factor=1e-7):
    """Every operator x 1e-7 (degree 2: one product per interval); lambda_a shrinks with it so that the update moves the
    pulses as much as in the base case."""
    new = explicit(obj)
    _scale_operators(new, factor)
    new.lambdas = [lam * factor for lam in new.lambdas]
    return new


def regime_long(obj, theta_max):
    """>= 130 intervals (two restarts of an advanced generator, one of them inside the grid) under a pulse ramp with two
    periods: |eps| spans the envelope's decades inside every 64-interval window."""
    if len(regime_dt(explicit(obj))) < 130:
        raise ValueError("the long regime needs at least 130 intervals")
    return regime_pulse_ramp(obj, theta_max, periods=2)


AMPLITUDE_COEFFICIENT, AMPLITUDE_LOW = 256.0, 0.4  # largest |eps^p| of a control's highest power; smallest |eps|


def regime_amplitude(obj, theta_max):
    """A ramp whose guess pulses straddle |eps| = 1 (problems with a term table: |eps|^p and |eps| part ways there).
    Control c keeps the envelope of its guess, rescaled to low_c + (top_c - low_c) |guess| / max |guess| with low_c =
    0.4 - c / 20 and top_c = (256 - 32 c)^(1 / p), p the highest power of the control's terms (1 without a table): the
    largest coefficient |eps^p| is the same whatever the table -- |eps| up to 4 with a power 4, up to 16 with a square --,
    so that a plan formed from |eps| with the powers ignored is short by a factor of several on every table, and where the
    envelope is above a quarter of its largest value the term eps^p H outweighs a drift of several times its norm.  The
    controls 0, 2, ... change sign in the middle of the grid.  Then ``regime_ramp``: dt_n such that theta_n follows
    ``ramp_profile`` under these pulses."""
    new = explicit(obj)
    M = len(regime_dt(new))
    if n_pulses(new) > 3:
        raise ValueError("the amplitude regime is laid out for up to three controls")
    terms = getattr(new, 'terms', None) or [(c, 1) for c in range(new.L)]
    half = np.where(np.arange(M) < M // 2, 1.0, -1.0)
    out = []
    for c, p in enumerate(new.pulses):
        top = (AMPLITUDE_COEFFICIENT - 32.0 * c) ** (1.0 / max(q for cj, q in terms if cj == c))
        low = AMPLITUDE_LOW - 0.05 * c
        out.append((half if c % 2 == 0 else 1.0) * (low + (top - low) * np.abs(p) / np.abs(p).max()))
    new.pulses = out
    return regime_ramp(new, theta_max)


REGIMES = {'ramp': regime_ramp, 'pulse_ramp': regime_pulse_ramp, 'tiny': lambda obj, theta_max: regime_tiny(obj),
           'long': regime_long, 'amplitude': regime_amplitude}


# ---- the ends of the interval pipeline (tests/test_grid_ends.py, tests/fuzz_parity.py --short-grids)
GRID_ENDS_SHORT = 3  # up to here: interval values of this module's own, one sub-step per interval
# theta_n / theta_max of the short grids (4 ... 10 intervals, the graph-replay cases: the last one repeated along the grid)
GRID_ENDS_THETA = {1: (0.5,), 2: (0.3, 0.8), 3: (0.25, 0.9, 0.45), 4: (0.25, 0.9, 0.45, 0.7)}
GRID_ENDS_STEPS = (1.0, 0.6, 0.85, 0.55, 0.7)  # step-width factors of the long grids (max / min = 1.8)


def grid_ends_pulses(obj, M):
    """Guess pulses of a short grid: eps_l[n] = a_l c[l, n] with 0.4 <= |c| <= 1 different on every interval and for every
    control, the sign changing from interval to interval and from control to control; a_l puts the L control terms together
    at the drift's norm bound (the objective with the largest drift bound), whatever the operators' scale."""
    b = series_bounds(obj)
    k = int(np.argmax(b[:, 0]))
    n, out = np.arange(M), []
    terms = getattr(obj, 'terms', None)
    for l in range(n_pulses(obj)):
        if terms:  # (a term table: the terms of control l together at their share of the drift's bound, sum_j a^p_j n_j)
            own = [(b[k, 1 + j], p) for j, (c, p) in enumerate(terms) if c == l and b[k, 1 + j] > 0.0]
            a = 1.0
            if own and b[k, 0] > 0.0:
                a = float(_bisect(lambda x: sum(nj * x ** p for nj, p in own), b[k, 0] * len(own) / obj.L))
        else:
            a = b[k, 0] / (obj.L * b[k, 1 + l]) if b[k, 1 + l] > 0.0 and b[k, 0] > 0.0 else 1.0
        out.append(a * (-1.0) ** (l + n) * (0.4 + 0.1 * ((3 * l + 5 * n + 1) % 7)))
    return out


def grid_ends(obj, theta_max):
    """The problem of ``obj`` (built with nt = I + 1) for a test of the ends of the sweeps' software pipeline:

    * update shapes S_l[n] = 0.2 + 0.8 (n + 1) / I -- the fixtures' flat-tops are 0 at both ends, which on one to three
      intervals is everywhere;
    * I <= 3 (and up to 10, for the graph-replay cases): ``grid_ends_pulses`` and step widths such that theta_n / theta_max
      of the objective with the largest theta is GRID_ENDS_THETA[I] (one sub-step; the steps differ by more than a factor
      1.5);
    * I >= 11: ``regime_pulse_ramp`` on a non-uniform grid (GRID_ENDS_STEPS), one period per 64 intervals (one up to
      I = 127: |eps| spans decades inside every restart window), exactly 0.0 on its inner intervals only -- not on the first
      and the last one."""
    new = explicit(obj)
    M = len(regime_dt(new))
    if M < RAMP_MIN_INTERVALS:
        new.pulses = grid_ends_pulses(new, M)
        _set_dt(new, theta_max * np.resize(GRID_ENDS_THETA[min(M, 4)], M) / _largest(new)[1])
    else:
        new = regime_pulse_ramp(new, theta_max, periods=max(1, M // 64), zeros='inner', steps=GRID_ENDS_STEPS)
    new.shapes = [0.2 + 0.8 * (np.arange(M) + 1.0) / M for _ in range(n_pulses(new))]
    return new


def grid_ends_witness(obj, theta_max):
    """Assert the input conditions of a ``grid_ends`` problem (host only); returns theta[k, n]."""
    C = n_pulses(obj)
    pulses, dt = np.array(obj.pulses, dtype=np.float64).reshape(C, -1), regime_dt(obj)
    M = len(dt)
    assert all(np.array_equal(s, 0.2 + 0.8 * (np.arange(M) + 1.0) / M) and np.all(s > 0.2) for s in obj.shapes)
    assert len(obj.shapes) == C and pulses.shape == (C, M)
    theta = theta_sequence(obj)
    if M >= 2:
        assert dt.max() / dt.min() >= 1.5
    if M < RAMP_MIN_INTERVALS:
        assert np.all(np.abs(pulses) >= 0.1 * np.abs(pulses).max())
        for l in range(C):
            assert len(set(pulses[l].tolist())) == M or M > GRID_ENDS_SHORT  # differ between intervals
        assert len({tuple(p.tolist()) for p in pulses}) == C  # and between controls
        top = theta.max(axis=0)
        assert np.all(top >= 0.1 * theta_max * (1 - 1e-12)) and np.all(top <= 0.9 * theta_max * (1 + 1e-12))
    else:
        assert np.all(pulses[:, 0] != 0.0) and np.all(pulses[:, -1] != 0.0)
        assert np.count_nonzero(pulses[0] == 0.0) >= 1  # (the inner zero stays)
        for start in range(0, M, 64):
            w = np.abs(pulses[0, start:start + 64])
            w = w[w > 0]
            if len(w) >= 32:
                assert np.log10(w.max() / w.min()) >= 2.0, "pulse spans %.1f decades" % np.log10(w.max() / w.min())
    return theta


def series_degree_tables(theta_cap=2.0, defect=3e-3, tol=0.0):
    """{'taylor' | 'real' | 'defect': theta thresholds per degree} at the truncation tolerance ``tol`` (0: the engine's
    default, 2^-53) from the library's exported host code (no GPU)."""
    import ctypes

    from krotov_amd import _lib

    lib = _lib.load()
    out = {}
    for name, call in (('taylor', lambda th, ra: lib.kh_series_tables(0, tol, th, ra)),
                       ('real', lambda th, ra: lib.kh_series_tables(1, tol, th, ra)),
                       ('defect', lambda th, ra: lib.kh_series_tables_defect(tol, theta_cap, defect, th, ra))):
        th, ra = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
        assert call(th, ra) == 0
        out[name] = np.array(th)
    return out


def _coefficients_of_ratios(ratios):
    """c[m][j] from ``ratios`` (c_0, c_1, c_j / c_{j-1}).  The rows of the degrees that stay with Taylor's coefficients are
    filled up to j = 64: the polynomial of degree m is c[m][:m + 1]."""
    ratios = np.array(ratios).reshape(65, 65)
    coeff = np.zeros((65, 65))
    coeff[:, :2] = ratios[:, :2]
    for j in range(2, 65):
        coeff[:, j] = coeff[:, j - 1] * ratios[:, j]
    return coeff


def series_coefficients(theta_cap=2.0, tol=0.0, defect=0.0):
    """(theta_b[m], c[m][j]) of the real-spectrum (Chebyshev-form) series with the cap ``theta_cap`` (and the margin for a
    Hermitian ``defect``) at the tolerance ``tol`` from the library's exported host code: the polynomial of degree m is
    sum_{j <= m} c[m][j] Z^j with Z = f A dt (``ratios``: c_0, c_1, c_j / c_{j-1})."""
    import ctypes

    from krotov_amd import _lib

    lib = _lib.load()
    th, ra = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
    assert lib.kh_series_tables_defect(tol, theta_cap, defect, th, ra) == 0
    return np.array(th), _coefficients_of_ratios(ra)


def series_taylor_coefficients(tol=0.0):
    """(theta[m], c[m][j] = 1 / j!) of the Taylor tables (``kh_series_tables(0, tol, ...)``)."""
    import ctypes

    from krotov_amd import _lib

    th, ra = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
    assert _lib.load().kh_series_tables(0, tol, th, ra) == 0
    return np.array(th), _coefficients_of_ratios(ra)


def series_tables_odd(tol=0.0):
    """(theta[m], c[m][j]) of ``kh_series_tables_odd``: the table the two-terms-per-phase kernels get where the series
    is the exactly-Hermitian Chebyshev form.  The export holds c_0 and the rows {r1_p, r2_p} (r1_0 = c_1, r2_0 = c_2;
    r1_p = c_{2p+1} / c_{2p}, r2_p = c_{2p+2} / c_{2p} for p >= 1; an odd degree m = 2P - 1 ends with {r1_{P-1}, 0}); the
    coefficients are rebuilt from them up to the degree."""
    import ctypes

    from krotov_amd import _lib

    th, c0, rows = (ctypes.c_double * 65)(), (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 32 * 2))()
    assert _lib.load().kh_series_tables_odd(tol, th, c0, rows) == 0
    c0, rows = np.array(c0), np.array(rows).reshape(65, 32, 2)
    coeff = np.zeros((65, 65))
    for m in range(1, 65):
        coeff[m, 0] = c0[m]
        for p in range((m + 1) // 2):
            even = 1.0 if p == 0 else coeff[m, 2 * p]
            coeff[m, 2 * p + 1] = rows[m, p, 0] * even
            if 2 * p + 2 <= m:
                coeff[m, 2 * p + 2] = rows[m, p, 1] * even
    return np.array(th), coeff


def series_polynomial(c, Z, dtype=np.complex128):
    """sum_j c[j] Z^j (Horner) for a matrix or an array of scalars ``Z`` (``dtype``: ``numpy.clongdouble`` where the
    rounding of the evaluation itself must stay below a truncation error that is being measured)."""
    Z = np.asarray(Z, dtype=dtype)
    one = np.eye(Z.shape[0], dtype=dtype) if Z.ndim == 2 else np.ones_like(Z)
    mul = (lambda a, b: a @ b) if Z.ndim == 2 else (lambda a, b: a * b)
    out = c[-1] * one
    for cj in c[-2::-1]:
        out = mul(Z, out) + cj * one
    return out


def series_plan(theta, theta_max, tab):
    """(nsub_n, degree_n) of a sequence theta_n: ``kh_degree_lookup`` restated (sub-steps beyond theta_max; the smallest
    degree m >= 1 whose threshold tab[m] serves theta_n / nsub_n)."""
    theta = np.asarray(theta, dtype=np.float64)
    nsub = np.where(theta > theta_max, np.ceil(theta / theta_max), 1.0).astype(int)
    th = theta / nsub
    deg = np.array([next((m for m in range(1, 64) if t <= tab[m]), 64) for t in th])
    return nsub, deg


def _changes(seq):
    return int(np.count_nonzero(np.diff(np.asarray(seq))))


def regime_witness(obj, regime, theta_max, pulses, tables):
    """Assert that ``obj`` under ``pulses`` (L, nt - 1) really is in ``regime`` (host only).  Evaluated for the objective
    with the largest theta; returns its (theta, nsub, {table: degrees}) for reports."""
    theta_all = theta_sequence(obj, pulses)
    k = int(np.argmax(theta_all.max(axis=1)))
    theta = theta_all[k]
    plans = {name: series_plan(theta, theta_max, tab) for name, tab in tables.items()}
    nsub = plans['taylor'][0]
    M = len(theta)
    if regime in ('ramp', 'pulse_ramp', 'long'):
        assert nsub.max() >= 3, "no interval with three sub-steps"
        assert np.all(theta_all.min(axis=1) <= theta_max), "no interval without sub-steps"
        assert theta.max() >= 2.5 * theta_max
        assert _changes(nsub) >= 4, "sub-step counts change %d times" % _changes(nsub)
        for name, (_, deg) in plans.items():
            steps = np.diff(deg)
            assert len(set(deg.tolist())) >= 4, "%s: degrees %s" % (name, sorted(set(deg.tolist())))
            assert steps.max() > 0 and steps.min() < 0, "%s: degrees do not rise and fall" % name
    if regime == 'ramp':
        assert theta.min() <= 1e-3 * theta_max
        assert np.ptp(regime_dt(obj)) > 0
    if regime in ('pulse_ramp', 'long'):
        eps = np.abs(np.asarray(pulses, dtype=np.float64)).reshape(n_pulses(obj), -1)
        assert np.ptp(regime_dt(obj)) < 1e-12 * regime_dt(obj).max()  # uniform grid
        guess = np.array(obj.pulses)
        assert np.all(guess[:, 0] == 0.0) and np.all(guess[:, -1] == 0.0) and np.count_nonzero(guess[0] == 0.0) >= 3
    if regime == 'tiny':
        for name, (ns, deg) in plans.items():
            assert ns.max() == 1 and deg.max() <= 4, "%s: degree %d" % (name, deg.max())
    if regime == 'long':
        assert M >= 130 and M % 64 != 0  # restarts at intervals 64 and 128, both inside the grid
        spans = []
        for start in range(0, M, 64):
            w = eps[0, start:start + 64]
            w = w[w > 0]
            spans.append(np.log10(w.max() / w.min()))
        assert max(spans) >= 2.5, "pulse spans %.1f decades inside a restart window" % max(spans)
    return theta, nsub, {name: p[1] for name, p in plans.items()}


def regime_oracle(obj):
    """The oracle problem of a regime problem: Liouvillian form of a Lindblad case, padded Hilbert form of a mixed one."""
    if obj.fmt == 'lindblad':
        return obj.oracle()
    if obj.fmt == 'mixed':  # zero-padded to the stride, Liouvillians L as i L (Hilbert form)
        S = obj.N

        def pad(a, shape):
            out = np.zeros(shape, dtype=np.complex128)
            out[tuple(slice(0, n) for n in a.shape)] = a
            return out

        def vec(state):
            arr = np.asarray(state, dtype=np.complex128)
            return arr.ravel(order='F') if arr.ndim == 2 and arr.shape[0] == arr.shape[1] and arr.shape[0] > 1 else arr.ravel()

        ops = [[pad((1j if obj.kinds[k] else 1.0) * op, (S, S)) for op in [obj.H0[k]] + list(obj.Hc[k])] for k in range(obj.K)]
        return ko.OracleProblem(ops, np.array([pad(vec(s), (S,)) for s in obj.init]),
                                np.array([pad(vec(s), (S,)) for s in obj.target]), obj.tlist, is_super=False)
    return spec_to_oracle(obj)


def regime_engine(obj, theta_max=0.0, tol=0.0, op_norms=None):
    """The engine of a regime problem (dense, CSR, mixed or Lindblad form); ``tol`` and ``op_norms`` as
    ``HipKrotovEngine`` takes them."""
    from krotov_amd import configs
    from krotov_amd.engine import HipKrotovEngine

    if obj.fmt == 'lindblad':
        return HipKrotovEngine(obj.H, obj.dt, c_ops=obj.C, theta_max=theta_max, tol=tol, op_norms=op_norms)
    if obj.fmt == 'csr':
        ops = configs.sparse_ops(obj)
    else:
        ops = [[obj.H0[k]] + [obj.Hc[k][l] for l in range(obj.L)] for k in range(obj.K)]
    return HipKrotovEngine(ops, regime_dt(obj), is_super=obj.is_super, theta_max=theta_max, tol=tol, op_norms=op_norms)


class MemoExpm:
    """Context manager: ``ko.expm_dense`` with a memo on its argument's bytes -- objectives sharing one operator list ask
    for the same exponential K times per interval.  The values are the oracle's own, bit for bit."""

    def __enter__(self):
        self._orig, memo = ko.expm_dense, {}

        def expm_dense(A, use_scipy=False):
            key = (A.shape, bool(use_scipy), hash(A.tobytes()))
            hit = memo.get(key)
            if hit is None or not np.array_equal(hit[0], A):
                if len(memo) >= 512:  # (per-objective operators never hit: keep the memo small)
                    memo.clear()
                hit = memo[key] = (np.array(A), self._orig(A, use_scipy))
            return hit[1]

        ko.expm_dense = expm_dense
        return self

    def __exit__(self, *exc):
        ko.expm_dense = self._orig
        return False


# ---------------------------------------------------------------------------
# Controls that are not self-adjoint (tests/test_nonselfadjoint_controls.py, tests/fuzz_parity.py --nonselfadjoint)
# ---------------------------------------------------------------------------
def _ladder_control(rng, N, scale, row_cols=None):
    """Entries on the super-diagonals 1 and 20 and one dense row (``row_cols`` entries of row N // 2): the non-zero 16 x 16
    blocks are (g, g), (g, g + 1), (g, g + 2) and a block row, those of the adjoint lie on the other side."""
    A = np.zeros((N, N), dtype=np.complex128)
    for off in (1, 20):
        if off < N:
            A += np.diag(rng.standard_normal(N - off) + 1j * rng.standard_normal(N - off), off)
    cols = N if row_cols is None else min(N, row_cols)
    A[N // 2, :cols] += rng.standard_normal(cols) + 1j * rng.standard_normal(cols)
    return scale * A / np.linalg.norm(A, 2)


def nonselfadjoint_variant(kind, H, rng, row_cols=None):
    """The control that replaces the Hermitian (or commutator) ``H``; the same spectral norm except ``lower`` (twice)."""
    N, scale = H.shape[0], np.linalg.norm(H, 2)
    if kind == 'lower':
        G = np.tril(rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)), -1)
        return H + G * (scale / np.linalg.norm(G, 2))
    if kind == 'ladder':
        return _ladder_control(rng, N, scale, row_cols)
    if kind == 'anti':
        return 1j * H
    raise KeyError(kind)
