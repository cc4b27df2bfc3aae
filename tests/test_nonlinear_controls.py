"""Non-linear controls: terms eps^p H of ONE control in the update sweeps (krotov_amd.nonlinear, kh_set_nonlinear).

Yardstick (tests/nonlinear_cases.py): a NumPy restatement of ``oracle.forward_update_sweep`` with the weights
w_j = p_j eps_guess^(p_j - 1) applied to the per-term sums -- the reference cannot express such a Hamiltonian, so there is
no golden.  What makes the restatement trustworthy is tested first, on the host: its weighted sum is the gradient of J_T
(central differences, second-order convergence in dt, and the weight-1 form is NOT), and it reduces to code that exists
(the untouched oracle for powers 1, the parametrization restatement with ``('square',)`` for one power 2).

Tolerances: the suite's 1e-12 against the restatement (1e-11 on Liouvillians).  The device forms eps^p and the weights by
the same repeated products as the restatement; a sum of up to four weighted terms adds roundings of relative 1e-16.
"""
import functools
import logging
import types

import numpy as np
import pytest

import constraint_cases as cc
import nonlinear_cases as nc
import parametrization_cases as pc
from helpers import numpy_plugins
from oracle import krotov_oracle as ko

import krotov_amd

TOL = 1e-12
TOL_LIOUVILLE = 1e-11
NORM = lambda prob, chi: float(np.linalg.norm(chi))  # noqa: E731

T1 = [(0, 2)]
T2 = [(0, 1), (0, 2)]
T3 = [(0, 1), (0, 2), (1, 1)]
T4 = [(0, 1), (0, 2), (0, 3), (1, 2)]
T9 = [(c, p) for c in range(3) for p in (1, 2, 3)]


# ---------------------------------------------------------------------------
# host 1: the weights are right
# ---------------------------------------------------------------------------
def _witness(nt):
    """Relative errors (right weights, weight 1) of Im<chi|sum_j w_j T_j|phi> at the midpoint states of the probed
    intervals against -(dJ_T / d eps[n]) / (2 dt) by central differences."""
    rng = np.random.default_rng(3)
    N, T, h = 4, 1.0, 1e-5

    def herm(norm):
        A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        H = 0.5 * (A + A.conj().T)
        return H * (norm / np.linalg.norm(H, 2))

    H0, H1, H2 = herm(6.0), herm(4.0), herm(3.0)
    tl = np.linspace(0.0, T, nt)
    eps = 0.3 + 0.5 * np.sin(np.pi * 0.5 * (tl[1:] + tl[:-1]) / T)
    e0, e1 = np.eye(N, dtype=np.complex128)[0], np.eye(N, dtype=np.complex128)[1]
    prob = ko.OracleProblem([[H0, H1, H2]], e0[None], e1[None], tl)

    def J_T(e):
        fw_T = ko.forward_propagation(prob, nc.coefficients(T2, [e]))
        return 1.0 - float(np.real(ko.tau_vals(prob, fw_T)[0]))

    coef = nc.coefficients(T2, [eps])
    _, fw = ko.forward_propagation(prob, coef, store=True)
    chi = ko.backward_sweep(prob, ko.chis_re(prob, None, None), coef)
    adj = prob.adjoint_ops()
    out = []
    for n in (nt // 5, nt // 2, 4 * nt // 5):
        dt = tl[n + 1] - tl[n]
        c = [x[n] for x in coef]
        phi = ko.step(prob.ops[0], c, 0.5 * dt, fw[0, n])
        x = ko.step(adj[0], c, 0.5 * dt, chi[0, n + 1], backwards=True)
        D = [np.vdot(x, prob.ops[0][1 + j] @ phi).imag for j in range(2)]
        up, down = eps.copy(), eps.copy()
        up[n] += h
        down[n] -= h
        want = -(J_T(up) - J_T(down)) / (2.0 * h) / (2.0 * dt)
        errs = []
        for linear in (False, True):
            got = sum(nc.weight(eps, p, linear)[n] * D[j] for j, (_, p) in enumerate(T2))
            errs.append(abs(got - want) / abs(want))
        out.append(errs)
    return np.array(out)  # (probe, [right, weight 1])


def test_the_weighted_sum_is_the_gradient_and_the_unweighted_one_is_not():
    errs = {nt: _witness(nt) for nt in (101, 201, 401)}
    for nt in sorted(errs):
        print(nt, 'right', errs[nt][:, 0], 'weight 1', errs[nt][:, 1])
    assert np.all(errs[401][:, 0] < 1e-3)
    for a, b in ((101, 201), (201, 401)):
        ratio = errs[a][:, 0] / errs[b][:, 0]
        assert np.all((ratio > 3.0) & (ratio < 5.0)), ratio
    for nt in errs:
        assert np.all(errs[nt][:, 1] > 10.0 * errs[nt][:, 0])


# ---------------------------------------------------------------------------
# host 2: reductions to code that exists
# ---------------------------------------------------------------------------
def test_two_linear_terms_are_the_oracle_on_the_summed_operator():
    spec = nc.problem([(0, 1), (0, 1)], K=2, N=5, nt=15)
    prob, gp, S, lam = nc.oracle_side(spec)
    summed = ko.OracleProblem([[row[0], row[1] + row[2]] for row in prob.ops], prob.init, prob.target, prob.tlist)
    ref = ko.optimize(summed, gp, S, lam, ko.chis_re, 3, norm=NORM)
    got = nc.optimize(prob, gp, S, lam, spec.nl_terms, ko.chis_re, 3)
    assert np.abs(got['all_pulses'] - ref['all_pulses']).max() < TOL
    assert np.abs(got['tau_vals'] - ref['tau_vals']).max() < TOL
    assert np.abs(got['g_a'] - ref['g_a']).max() < TOL


def test_one_square_term_is_the_square_parametrization_in_u():
    spec = nc.problem(T1, K=2, N=5, nt=15, positive=True)
    prob, gp, S, lam = nc.oracle_side(spec)
    assert min(p.min() for p in gp) > 0
    rng = np.random.default_rng(3)
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    norms = 0.2 + rng.random(prob.K)
    chi = ko.backward_sweep(prob, chi_T, nc.coefficients(T1, gp))
    got = nc.update_sweep(prob, chi, norms, gp, T1, S, lam)
    eps_opt, u_opt, fw_T, g_a = pc.update_sweep(prob, chi, norms, gp, [('square',)], S, lam)
    assert np.abs(np.array(got[0]) - np.array(u_opt)).max() < TOL
    assert np.abs(nc.power(np.array(got[0]), 2) - np.array(eps_opt)).max() < TOL
    assert np.abs(got[1] - fw_T).max() < TOL and np.abs(got[2] - g_a).max() < TOL


# ---------------------------------------------------------------------------
# host 3, 4: the host loop of optimize_pulses
# ---------------------------------------------------------------------------
def _host_run(spec, iters, **kw):
    prop, _, _ = numpy_plugins(spec.is_super)
    objectives, pulse_options = nc.product_side(spec, krotov_amd.Power)
    g_a = []
    res = krotov_amd.optimize_pulses(
        objectives, pulse_options, spec.tlist, propagator=prop, norm=np.linalg.norm,
        chi_constructor=krotov_amd.functionals.chis_re, iter_stop=iters, store_all_pulses=True,
        info_hook=lambda **args: g_a.append(np.array(args['g_a_integrals'])), **kw)
    res.g_a = np.array(g_a)
    return res


def _assert_matches(res, ref, tol=TOL):
    got = np.array(res.all_pulses)
    assert got.shape == ref['all_pulses'].shape
    d_p, d_t = np.abs(got - ref['all_pulses']).max(), np.abs(np.array(res.tau_vals) - ref['tau_vals']).max()
    print("max |d pulse| = %.3e  max |d tau| = %.3e" % (d_p, d_t))
    assert d_p < tol * max(1.0, np.abs(ref['all_pulses']).max())
    assert d_t < tol
    if hasattr(res, 'g_a'):
        assert np.abs(res.g_a - ref['g_a']).max() < tol * max(1.0, np.abs(ref['g_a']).max())


def test_host_loop_matches_the_restatement_and_rewraps_the_optimized_control():
    spec = nc.problem(T3, K=2, N=5, nt=9)
    prob, gp, S, lam = nc.oracle_side(spec)
    ref = nc.optimize(prob, gp, S, lam, T3, ko.chis_re, 3)
    res = _host_run(spec, 3)
    _assert_matches(res, ref)
    assert len(res.optimized_controls) == 2 and len(res.guess_controls) == 2
    new = res.optimized_objectives[0]
    assert new.H[1][1] is res.optimized_controls[0] and new.H[3][1] is res.optimized_controls[1]
    g = new.H[2][1]
    assert isinstance(g, krotov_amd.Power) and g.power == 2 and g.control is res.optimized_controls[0]
    assert res.objectives[0].H[2][1].control is spec.nl_controls[0]  # (the guess objectives keep theirs)
    from krotov_amd.conversions import control_onto_interval, extract_controls, extract_controls_mapping, plug_in_pulse_values
    ctrls = extract_controls([new])
    assert len(ctrls) == 2 and ctrls[0] is res.optimized_controls[0]
    mapping = extract_controls_mapping([new], ctrls)
    pulses = [control_onto_interval(c) for c in ctrls]
    H = plug_in_pulse_values(new.H, pulses, mapping[0][0], 4)
    assert H[1][1] == pulses[0][4] and H[2][1] == pulses[0][4] * pulses[0][4] and H[3][1] == pulses[1][4]


def _stark_lambda_system():
    """tests/constraint_cases.py's Lambda system with a Stark shift of the excited level driven by the pump: one more
    term eps_pump^2 H_2.  lambda_a = 5: the restatement alone is monotone there (checked in the test)."""
    spec, _, _ = cc.lambda_system(nt=41)
    H2 = np.diag([0.0, 0.0, 0.3]).astype(np.complex128)
    spec.Hc = [[spec.Hc[0][0], spec.Hc[0][1], H2]]
    spec.L = 3
    spec.nl_controls, spec.nl_terms, spec.nl_lambdas, spec.nl_absent = spec.controls, [(0, 1), (1, 1), (0, 2)], [5.0, 5.0], set()
    return spec


def _assert_monotone(taus, g_a):
    J_T = [1.0 - float(np.mean(np.real(t))) for t in taus]
    for i in range(1, len(J_T)):
        assert J_T[i] + float(np.sum(g_a[i])) < J_T[i - 1], (i, J_T, g_a)


def test_monotone_convergence_with_a_stark_term():
    spec = _stark_lambda_system()
    prob, gp, S, lam = nc.oracle_side(spec)
    ref = nc.optimize(prob, gp, S, lam, spec.nl_terms, ko.chis_re, 5)
    _assert_monotone(ref['tau_vals'], ref['g_a'])
    res = _host_run(spec, 5)
    _assert_matches(res, ref)
    _assert_monotone(np.array(res.tau_vals), res.g_a)


def test_user_defined_function_runs_the_host_loop(caplog):
    """A subclass with ``power None`` (here the same square) selects the host loop around the device's single steps when
    the device propagator is asked for -- logged; on a machine without a GPU that path cannot run, so the decision is
    what is tested: the plan says False."""
    from krotov_amd.conversions import extract_controls, extract_controls_mapping
    from krotov_amd.nonlinear import needs_host_loop, term_plan

    class Square(krotov_amd.ControlFunction):
        def value(self, eps):
            return eps * eps

        def derivative(self, eps):
            return 2.0 * eps

    spec = nc.problem(T2, K=2, N=5, nt=9)
    objectives, pulse_options = nc.product_side(spec, lambda c, p: Square(c))
    mapping = extract_controls_mapping(objectives, extract_controls(objectives))
    assert term_plan(objectives, mapping, 1) is False
    assert needs_host_loop(objectives) and not needs_host_loop(nc.product_side(spec, krotov_amd.Power)[0])
    prob, gp, S, lam = nc.oracle_side(spec)
    ref = nc.optimize(prob, gp, S, lam, T2, ko.chis_re, 2)
    prop, _, _ = numpy_plugins(False)
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, propagator=prop, norm=np.linalg.norm,
                                     chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2, store_all_pulses=True)
    _assert_matches(res, ref)


# ---------------------------------------------------------------------------
# the GPU cases (sweep level) and, on the host, their witnesses
# ---------------------------------------------------------------------------
SWEEPS = {}


def sweep(name, terms, expect, so=False, env=None, fmt='dense', mode='whole', reduced=0, kernel=None, **problem):
    SWEEPS[name] = dict(terms=terms, expect=expect, so=so, env=env or {}, fmt=fmt, mode=mode, reduced=reduced,
                        kernel=kernel, problem=problem)


TILE = 'kh_tile_forward_update_nl<%d, %d, %s>'
GEN = 'kh_gen_forward_update_nl<false>'
GENERIC = {'KH_KERNEL': 'generic'}
# ---- the register-tile kernel's non-linear form: <rows per thread, terms, second order>
for _terms in (T1, T2, T3, T4):
    for _so in (False, True):
        sweep('tile_J%d%s' % (len(_terms), '_so' if _so else ''), _terms,
              [TILE % (1, len(_terms), 'true' if _so else 'false')], so=_so, K=3, N=5 if len(_terms) % 2 else 8, nt=9,
              positive=_terms is T1)
for _so in (False, True):
    sweep('tile256_k257%s' % ('_so' if _so else ''), T1, [TILE % (2, 1, 'true' if _so else 'false')], so=_so,
          kernel='tile64/256', K=257, N=4, nt=8, positive=True)
# ---- the generic kernels' non-linear form
sweep('gen_generic_n6', T2, [GEN], env=GENERIC, K=3, N=6, nt=9)
sweep('gen_n70_tile128', T3, [GEN], kernel='tile128/512', K=2, N=70, nt=9)
sweep('gen_csr_n40', T2, [GEN], fmt='csr', K=2, N=40, nt=9, bands=3)
sweep('gen_9_terms', T9, [GEN], K=3, N=12, nt=9)
sweep('gen_so', T3, [GEN], so=True, env=GENERIC, K=3, N=6, nt=9)
# ---- the suite's axes, once per family (tile: K = 3, N = 5; generic: the same problem under KH_KERNEL=generic)
for _fam, _env, _exp in (('tile', None, [TILE % (1, 2, 'false')]), ('gen', GENERIC, [GEN])):
    # (the flat-top shape is zero on the first and the last interval: with one or two intervals nothing would move)
    sweep(_fam + '_nt2', T2, _exp, env=_env, K=3, N=5, nt=2, flat=True)
    sweep(_fam + '_nt3', T2, _exp, env=_env, K=3, N=5, nt=3, flat=True)
    sweep(_fam + '_nt131_wide', T2, _exp, env=_env, K=3, N=5, nt=131, guess='wide')
    sweep(_fam + '_nonuniform', T2, _exp, env=_env, K=3, N=5, nt=9, ratios=(0.5, 1.7, 1.0, 0.8))
    sweep(_fam + '_zero_square_only', T1, [e.replace(', 2, ', ', 1, ') for e in _exp], env=_env, K=3, N=5, nt=9, guess='zero')
    sweep(_fam + '_zero_both', T2, _exp, env=_env, K=3, N=5, nt=9, guess='zero')
    sweep(_fam + '_absent', T2, _exp, env=_env, K=3, N=5, nt=9, absent=((1, 1), (2, 0)))
    sweep(_fam + '_liouville', T2, _exp, env=_env, K=2, N=9, nt=9, liouville=True)
sweep('gen_stepwise', T3, [GEN], mode='stepwise', K=3, N=5, nt=9)
sweep('gen_stepwise_so', T2, [GEN], mode='stepwise', so=True, K=3, N=5, nt=9)
sweep('gen_reduced', T2, [GEN], reduced=4, K=6, N=5, nt=9)


def _build(case):
    """The spec of a case of SWEEPS."""
    from krotov_amd import configs

    kw = dict(case['problem'])
    guess, ratios, liouville = kw.pop('guess', None), kw.pop('ratios', None), kw.pop('liouville', False)
    flat = kw.pop('flat', False)
    if liouville:
        d = 3
        spec = nc.problem(case['terms'], K=kw['K'], N=d, nt=kw['nt'])
        rng = np.random.default_rng(4)
        c_op = 0.2 * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
        spec.H0 = [configs.liouvillian_dense(h, [c_op]) for h in spec.H0]
        spec.Hc = [[configs.liouvillian_dense(h, []) for h in row] for row in spec.Hc]
        rho0, rho1 = np.zeros((d, d), dtype=np.complex128), np.zeros((d, d), dtype=np.complex128)
        rho0[0, 0] = rho1[1, 1] = 1.0
        spec.init = np.array([rho0.ravel(order='F')] * spec.K)
        spec.target = np.array([rho1.ravel(order='F')] * spec.K)
        spec.is_super, spec.N = True, d * d
    else:
        spec = nc.problem(case['terms'], **kw)
    T = spec.tlist[-1]
    if flat:
        spec.update_shape = lambda t: 1.0
    if guess == 'zero':
        spec.nl_controls = [(lambda t, args: 0.0) for _ in spec.nl_controls]
    elif guess == 'wide':  # two orders of magnitude over the sweep: the series' generator is restarted on the way
        spec.nl_controls = [(lambda t, args, l=l: 0.004 * 10.0 ** (2.0 * t / T) * (1.0 if l % 2 == 0 else 0.5))
                            for l in range(len(spec.nl_controls))]
    if ratios is not None:
        cc.nonuniform(spec, ratios)
    return spec


@functools.lru_cache(maxsize=None)
def _reference(name, linear_weights=False):
    """(spec, problem, guess, shapes, lambdas, inputs, the restatement's sweep) of a case: computed once, shared."""
    case = SWEEPS[name]
    spec = _build(case)
    prob, gp, S, lam = nc.oracle_side(spec)
    rng = np.random.default_rng(17)
    nt = len(prob.tlist)
    coef = nc.coefficients(case['terms'], gp)
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    norms = (0.2 + rng.random(prob.K)) * min(1.0, 8.0 / prob.K)
    ref_chi = ko.backward_sweep(prob, chi_T, coef)
    kw = {}
    if case['so']:
        older = [p * (1.0 + 0.1 * rng.standard_normal(p.shape)) for p in gp]  # the "previous iteration"
        _, prev = ko.forward_propagation(prob, nc.coefficients(case['terms'], older), store=True)
        sigma_vals = -(1.0 + rng.random(nt - 1)) * min(1.0, 8.0 / prob.K)
        kw = dict(sigma_vals=sigma_vals, fw_prev=prev, store=True)
    ref = nc.update_sweep(prob, ref_chi, norms, gp, case['terms'], S, lam, linear_weights=linear_weights, **kw)
    return types.SimpleNamespace(spec=spec, prob=prob, gp=gp, S=S, lam=lam, coef=coef, chi_T=chi_T, norms=norms,
                                 ref_chi=ref_chi, kw=kw, ref=ref)


@pytest.mark.parametrize('name', sorted(SWEEPS))
def test_every_gpu_case_bites(name):
    """The restatement with every weight replaced by its power-1 value moves the case's optimized pulses by more than 1e3
    tolerances: a device that forgot the weights could not pass.  (The zero guess under eps^2 alone is the one case
    where the RIGHT pulse is the unmoved one.)"""
    right, wrong = _reference(name), _reference(name, True)
    moved = np.abs(np.array(right.ref[0]) - np.array(wrong.ref[0])).max()
    print(name, 'moved by %.3e' % moved)
    assert moved > 1e3 * (TOL_LIOUVILLE if right.prob.is_super else TOL)


# ---------------------------------------------------------------------------
# host 6, 7: validation, the ABI without a device
# ---------------------------------------------------------------------------
def test_power_validates_its_exponent():
    eps = lambda t, args: 0.1  # noqa: E731
    for p in (0, 5, 2.5, True):
        with pytest.raises(ValueError):
            krotov_amd.Power(eps, p)
    with pytest.raises(ValueError):
        krotov_amd.Power(krotov_amd.Power(eps, 2), 2)
    g = krotov_amd.Power(eps, 3)
    x = np.linspace(-1.0, 1.0, 7)
    assert np.array_equal(g.value(x), x * x * x) and np.array_equal(g.derivative(x), 3 * x * x)
    assert g.value(0.5) == 0.125 and krotov_amd.Power(eps, 1).derivative(0.5) == 1.0
    assert isinstance(g, krotov_amd.ControlFunction) and g.control is eps


def _small_objectives(c_ops=None):
    rng = np.random.default_rng(1)
    from krotov_amd import configs

    H0, H1, H2 = (configs.herm(rng, 3, 1.0) for _ in range(3))
    eps = lambda t, args: 0.1 + 0.1 * t  # noqa: E731
    psi = np.eye(3, dtype=np.complex128)
    obj = krotov_amd.Objective(initial_state=psi[0], target=psi[1], H=[H0, [H1, eps], [H2, krotov_amd.Power(eps, 2)]],
                               c_ops=c_ops)
    return obj, eps, (H0, H1, H2)


def test_a_control_function_in_c_ops_is_not_implemented():
    from krotov_amd.conversions import extract_controls, extract_controls_mapping
    from krotov_amd.mu import derivative_wrt_pulse

    obj, eps, (H0, H1, H2) = _small_objectives()
    obj.c_ops = [[[H1, krotov_amd.Power(eps, 2)]]]
    mapping = extract_controls_mapping([obj], extract_controls([obj]))
    with pytest.raises(NotImplementedError):
        derivative_wrt_pulse([obj], 0, [np.full(4, 0.2)], mapping, 0, 1)


def test_refusals_of_optimize_pulses_and_dump(tmp_path):
    obj, eps, _ = _small_objectives()
    tlist = np.linspace(0.0, 1.0, 5)
    opts = dict(lambda_a=2.0, update_shape=1)
    kw = dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1)
    with pytest.raises(ValueError, match='parametrization'):
        krotov_amd.optimize_pulses([obj], {eps: dict(opts, parametrization=krotov_amd.TanhParametrization(-1.0, 1.0))},
                                   tlist, **kw)
    with pytest.raises(ValueError, match='process_group'):
        krotov_amd.optimize_pulses([obj], {eps: opts}, tlist, process_group=object(), **kw)
    with pytest.raises(ValueError, match='pulse options'):  # (keyed by the wrapper instead of the control)
        krotov_amd.optimize_pulses([obj], {obj.H[2][1]: opts} if obj.H[2][1].__hash__ else {id(obj.H[2][1]): opts},
                                   tlist, **kw)
    prop, _, _ = numpy_plugins(False)
    res = krotov_amd.optimize_pulses([obj], {eps: opts}, tlist, propagator=prop, norm=np.linalg.norm,
                                     chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1)
    with pytest.raises(ValueError, match='non-linear'):
        res.dump(str(tmp_path / 'ref.dump'), reference=True)
    res.dump(str(tmp_path / 'own.dump'))  # (the function control inside the wrapper becomes a placeholder)
    back = krotov_amd.Result.load(str(tmp_path / 'own.dump'))
    g = back.objectives[0].H[2][1]
    assert isinstance(g, krotov_amd.Power) and g.power == 2 and isinstance(g.control, krotov_amd.result.ControlPlaceholder)
    assert g.control == back.objectives[0].H[1][1]


def test_without_a_control_function_nothing_changes():
    from krotov_amd import mixed
    from krotov_amd.conversions import extract_controls, extract_controls_mapping, plug_in_pulse_values
    from krotov_amd.mu import derivative_wrt_pulse
    from krotov_amd.nonlinear import has_control_function, term_plan

    obj, eps, (H0, H1, H2) = _small_objectives()
    eps2 = np.linspace(0.0, 1.0, 5)
    plain = krotov_amd.Objective(initial_state=obj.initial_state, target=obj.target, H=[H0, [H1, eps], [H2, eps2], [H2, eps]])
    controls = extract_controls([plain])
    assert len(controls) == 2 and controls[0] is eps and controls[1] is eps2
    mapping = extract_controls_mapping([plain], controls)
    assert mapping == [[[[1, 3], [2]]]]
    assert not has_control_function([plain]) and term_plan([plain], mapping, 2) is None
    pulses = [np.full(4, 0.25), np.full(4, 0.5)]
    mu = derivative_wrt_pulse([plain], 0, pulses, mapping, 0, 2)
    psi = np.arange(3) + 1j
    assert np.array_equal(mu(psi), (H1 + H2) @ psi)  # (the operators' own sum, no weights: bit for bit)
    assert plug_in_pulse_values(plain.H, pulses, mapping[0][0], 1)[3][1] == 0.25
    # ... and with one: one control, the wrapper unwrapped; the derivative at the pulse value
    controls = extract_controls([obj])
    assert len(controls) == 1 and controls[0] is eps
    mapping = extract_controls_mapping([obj], controls)
    assert mapping == [[[[1, 2]]]]
    mu = derivative_wrt_pulse([obj], 0, [np.full(4, 0.25)], mapping, 0, 2)
    assert np.abs(mu(psi) - (H1 + 0.5 * H2) @ psi).max() < 1e-15
    plan = term_plan([obj], mapping, 1)
    assert list(plan.term_control) == [0, 0] and list(plan.term_power) == [1, 2] and plan.mapping == [[[[1], [2]]]]
    rho = np.eye(3, dtype=np.complex128) / 3
    lind = krotov_amd.Objective(initial_state=rho, target=rho, H=obj.H, c_ops=[H1])
    assert mixed.lindblad_layout_of([lind], None, 1, False).matrix
    lay = mixed.lindblad_layout_of([lind], None, 1, False, False, True)
    assert not lay.matrix and 'non-linear' in lay.reason


def test_batch_runs_a_non_linear_problem_on_its_own():
    from krotov_amd import batch

    obj, eps, _ = _small_objectives()
    rep = types.SimpleNamespace(objectives=[obj], pulse_options={eps: dict(lambda_a=1.0, update_shape=1)})
    assert 'non-linear' in batch._batch_obstacle([], [rep], krotov_amd.propagators.expm)


def test_c_abi_declares_the_entry_point():
    import os

    from krotov_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'krotov_hip.h')).read()
    assert 'int kh_set_nonlinear(kh_engine *engine, int32_t C, const int32_t *term_control' in header
    assert 'kh_set_nonlinear' in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.kh_set_nonlinear(None, 1, None, None, None) == _lib.KH_ERR_INVALID == -1
    assert lib.kh_last_error().decode() != ''
    names = _lib.kernel_instantiations()
    want = ['kh_gen_forward_update_nl<false>', 'kh_gen_forward_update_nl<true>']
    want += [TILE % (1, j, so) for j in (1, 2, 3, 4) for so in ('false', 'true')]
    want += [TILE % (2, 1, 'false'), TILE % (2, 1, 'true')]
    assert sorted(n for n in names if '_nl<' in n) == sorted(want)


# ---------------------------------------------------------------------------
# GPU: sweep level, every new instantiation named and confirmed with kh_debug_launched
# ---------------------------------------------------------------------------
def _engine(spec, fmt, cls=None):
    from krotov_amd import configs
    from krotov_amd.engine import HipKrotovEngine

    ops = nc.term_ops(spec)
    if fmt == 'csr':
        import scipy.sparse as sp

        ops = [[None if o is None else sp.csr_matrix(o) for o in row] for row in ops]
    return (cls or HipKrotovEngine)(ops, np.diff(spec.tlist), is_super=spec.is_super)


def _tables(terms):
    return np.array([c for c, _ in terms], dtype=np.int32), np.array([p for _, p in terms], dtype=np.int32)


def _run_sweep(eng, case, r):
    """One non-linear update sweep on ``eng`` against the restatement ``r`` (``_reference``); returns the device outputs."""
    import torch

    from krotov_amd import _lib

    prob, gp, terms = r.prob, r.gp, case['terms']
    nt = len(prob.tlist)
    pulses, coef = np.array(gp), np.array(r.coef)
    chi = eng.backward(r.chi_T, coef)
    store = None
    if case['so']:
        store = torch.full((prob.K, nt, prob.N), float('nan'), dtype=torch.complex128, device=eng.device)
        eng.set_second_order(r.kw['fw_prev'], store, r.kw['sigma_vals'])
    tc, tp = _tables(terms)
    eng.set_nonlinear(tc, tp, np.array([nc.weight(gp[c], p) for c, p in terms]))
    if case['reduced']:
        assert eng.set_update_workgroups(case['reduced']) == case['reduced']
    _lib.forget_launched_kernels()
    if case['mode'] == 'stepwise':
        opt, psi_T, g_a = eng.forward_update_sharded(chi, r.norms, r.spec.init, pulses, np.array(r.S), np.array(r.lam),
                                                     lambda x: None, graph_chunk=0)
    else:
        opt, psi_T, g_a = eng.forward_update(chi, r.norms, r.spec.init, pulses, np.array(r.S), np.array(r.lam))
    eng.check()
    launched = _lib.kernel_instantiations(launched_only=True)
    ref = r.ref
    tol = TOL_LIOUVILLE if prob.is_super else TOL
    out = dict(opt=opt.cpu().numpy(), psi=psi_T.cpu().numpy(), g_a=g_a.cpu().numpy())
    assert out['opt'].shape == pulses.shape and out['g_a'].shape == (len(gp),)
    d = dict(chi=np.abs(chi.cpu().numpy() - r.ref_chi).max(), opt=np.abs(out['opt'] - np.array(ref[0])).max(),
             psi=np.abs(out['psi'] - ref[1]).max(), g_a=np.abs(out['g_a'] - ref[2]).max())
    print(' '.join('%s %.2e' % kv for kv in sorted(d.items())), '|', eng.kernel, [n for n in launched if 'update' in n])
    assert d['chi'] < tol
    assert d['opt'] < tol * max(1.0, np.abs(np.array(ref[0])).max())
    assert d['psi'] < tol
    assert d['g_a'] < tol * max(1.0, np.abs(ref[2]).max())
    if case['so']:
        assert np.abs(store.cpu().numpy() - ref[3]).max() < tol
    for want in case['expect']:
        assert want in launched, (want, launched)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SWEEPS))
def test_non_linear_sweep_vs_restatement(name, monkeypatch):
    case = SWEEPS[name]
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    r = _reference(name)
    eng = _engine(r.spec, case['fmt'])
    if case['kernel'] is not None:
        assert eng.kernel == case['kernel'], eng.kernel
    if case['fmt'] == 'csr':
        assert eng.kernel.endswith('/csr'), eng.kernel
    out = _run_sweep(eng, case, r)
    assert np.all(np.isfinite(out['opt'])) and np.all(np.isfinite(out['psi'])) and np.all(np.isfinite(out['g_a']))
    if name.endswith('_zero_square_only'):  # (weight 0: the pulse stays exactly 0)
        assert np.all(out['opt'] == 0.0) and np.all(out['g_a'] == 0.0)
    if name.endswith('_zero_both'):  # (the same guess with the linear term next to the square moves)
        assert np.abs(out['opt']).max() > 1e-6
    eng.close()


@pytest.mark.gpu
def test_mixed_dimensions_sweep_vs_restatement():
    """A 3-level ket, a 5-level ket and a qutrit rho under a Liouvillian, one control with {eps, eps^2}: the generic
    kernels' mixed form, whole and stepwise with second order."""
    from test_mixed_objectives import _engine_ops, _pad_vec, _vec, oracle_adapter, spec_controls

    from krotov_amd import configs
    from krotov_amd.engine import HipKrotovEngine

    spec = configs.config_mixed('dims', nt=11)
    spec.Hc = [[row[0], 0.6 * row[0]] for row in spec.Hc]
    gp, S, lam = spec_controls(spec)
    spec.L = 2
    prob = oracle_adapter(spec)
    eng = HipKrotovEngine(_engine_ops(spec), np.diff(spec.tlist), is_super=spec.kinds)
    assert eng.kernel == 'generic/mixed'
    init = np.array([_pad_vec(_vec(s), spec.N) for s in spec.init])
    for so, mode, seed in ((False, 'whole', 5), (True, 'stepwise', 6)):
        rng = np.random.default_rng(seed)
        gp = [np.array(p) for p in gp]
        coef = nc.coefficients(T2, gp)
        chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
        norms = 0.2 + rng.random(prob.K)
        kw = {}
        if so:
            _, prev = ko.forward_propagation(prob, nc.coefficients(T2, [p * 1.1 for p in gp]), store=True)
            kw = dict(sigma_vals=-(1.0 + rng.random(len(prob.tlist) - 1)), fw_prev=prev, store=True)
        r = types.SimpleNamespace(spec=types.SimpleNamespace(init=init), prob=prob, gp=gp, S=S, lam=list(lam), coef=coef,
                                  chi_T=chi_T, norms=norms, ref_chi=ko.backward_sweep(prob, chi_T, coef), kw=kw)
        r.ref = nc.update_sweep(prob, r.ref_chi, norms, gp, T2, S, list(lam), **kw)
        wrong = nc.update_sweep(prob, r.ref_chi, norms, gp, T2, S, list(lam), linear_weights=True, **kw)
        assert np.abs(np.array(r.ref[0]) - np.array(wrong[0])).max() > 1e3 * TOL_LIOUVILLE
        case = dict(terms=T2, so=so, reduced=0, mode=mode, expect=['kh_gen_forward_update_nl<true>'])
        _run_sweep(eng, case, r)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tile_J2', 'gen_n70_tile128'])
def test_set_run_clear_run_linear_is_the_engine_nothing_was_set_on(name):
    """After ``set_nonlinear()`` the engine's linear sweep is, bit for bit and on the same kernel, the sweep of an engine
    on which nothing was ever set; two non-linear sweeps give the same bits."""
    from krotov_amd import _lib

    case = SWEEPS[name]
    r = _reference(name)
    J = len(case['terms'])
    rng = np.random.default_rng(2)
    pulses_J = 0.2 * rng.standard_normal((J, len(r.prob.tlist) - 1))
    S_J, lam_J = np.array([r.S[0]] * J), np.full(J, 2.5)

    def linear(eng):
        chi = eng.backward(r.chi_T, pulses_J)
        _lib.forget_launched_kernels()
        out = [x.cpu().numpy() for x in eng.forward_update(chi, r.norms, r.spec.init, pulses_J, S_J, lam_J)]
        eng.check()
        return out, sorted(n for n in _lib.kernel_instantiations(launched_only=True) if 'forward_update' in n)

    fresh = _engine(r.spec, case['fmt'])
    want, kernels = linear(fresh)
    fresh.close()
    ref = ko.forward_update_sweep(r.prob, ko.backward_sweep(r.prob, r.chi_T, list(pulses_J)), r.norms, list(pulses_J),
                                  list(S_J), list(lam_J))
    assert np.abs(want[0] - np.array(ref[0])).max() < TOL and np.abs(want[1] - ref[1]).max() < TOL
    assert not any('_nl<' in n for n in kernels)
    eng = _engine(r.spec, case['fmt'])
    one = _run_sweep(eng, case, r)
    two = _run_sweep(eng, case, r)
    for key in one:
        assert np.array_equal(one[key], two[key]), key
    eng.set_nonlinear()
    got, kernels_after = linear(eng)
    assert kernels_after == kernels
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tile_J1', 'tile256_k257', 'gen_n70_square'])
def test_square_alone_is_the_square_parametrization_on_the_device(name):
    """{eps^2} against the existing device sweep with ``SquareParametrization`` on the coefficient pulse (u = eps_guess >
    0, f'(u) = 2 u): eps_new is its u_new, the states and g_a are the same, to 1e-12."""
    import torch

    if name == 'gen_n70_square':
        spec = nc.problem(T1, K=2, N=70, nt=9, positive=True)
        prob, gp, S, lam = nc.oracle_side(spec)
        rng = np.random.default_rng(17)
        chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
        r = types.SimpleNamespace(spec=spec, prob=prob, gp=gp, S=S, lam=lam, coef=nc.coefficients(T1, gp), chi_T=chi_T,
                                  norms=0.2 + rng.random(prob.K), kw={})
        r.ref_chi = ko.backward_sweep(prob, chi_T, r.coef)
        r.ref = nc.update_sweep(prob, r.ref_chi, r.norms, gp, T1, S, lam)
        case = dict(terms=T1, so=False, reduced=0, mode='whole', expect=[GEN], fmt='dense')
    else:
        case, r = SWEEPS[name], _reference(name)
    eng = _engine(r.spec, case['fmt'])
    out = _run_sweep(eng, case, r)
    eng.set_nonlinear()
    u_guess = np.array(r.gp)
    assert u_guess.min() > 0
    u_opt = torch.full(u_guess.shape, float('nan'), dtype=torch.float64, device=eng.device)
    eng.set_parametrization([2], [0.0], [0.0], u_guess, 2.0 * u_guess, u_opt)
    chi = eng.backward(r.chi_T, np.array(r.coef))
    opt, psi_T, g_a = eng.forward_update(chi, r.norms, r.spec.init, np.array(r.coef), np.array(r.S), np.array(r.lam))
    eng.check()
    u = u_opt.cpu().numpy()
    assert np.abs(out['opt'] - u).max() < TOL
    assert np.abs(out['opt'] * out['opt'] - opt.cpu().numpy()).max() < TOL
    assert np.abs(out['psi'] - psi_T.cpu().numpy()).max() < TOL
    assert np.abs(out['g_a'] - g_a.cpu().numpy()).max() < TOL * max(1.0, np.abs(out['g_a']).max())
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tile_J3_so', 'gen_csr_n40'])
def test_non_linear_sweep_on_guarded_buffers(name, monkeypatch):
    """Memory contract: every tensor the sweep sees -- operators, the engine's own buffers, inputs, outputs, ``dcde`` --
    carved from tests/guarded.py's arena; inputs bytewise unchanged, guard bands intact, results the restatement's."""
    import torch

    from guarded import GuardedEngine

    case, r = SWEEPS[name], _reference(name)
    prob, gp, terms = r.prob, r.gp, case['terms']
    K, N, nt, C, J = prob.K, prob.N, len(prob.tlist), len(gp), len(terms)
    eng = _engine(r.spec, case['fmt'], cls=GuardedEngine)
    arena = eng.arena
    c128, f64 = torch.complex128, torch.float64
    shapes = dict(chi_T=((K, N), c128), coef=((J, nt - 1), f64), chi=((K, nt, N), c128), norms=((K,), f64),
                  init=((K, N), c128), guess=((C, nt - 1), f64), S=((C, nt - 1), f64), lam=((C,), f64),
                  dcde=((J, nt - 1), f64), opt=((C, nt - 1), f64), psi_T=((K, N), c128), g_a=((C,), f64),
                  prev=((K, nt, N), c128), store=((K, nt, N), c128), sigma=((nt - 1,), f64))
    t = {k: arena.carve(k, s, d) for k, (s, d) in shapes.items()}
    host = dict(chi_T=r.chi_T, coef=np.array(r.coef), norms=r.norms, init=r.spec.init, guess=np.array(gp), S=np.array(r.S),
                lam=np.array(r.lam), dcde=np.array([nc.weight(gp[c], p) for c, p in terms]))
    if case['so']:
        host.update(prev=r.kw['fw_prev'], sigma=r.kw['sigma_vals'])
    for k, v in host.items():
        t[k].copy_(torch.as_tensor(np.ascontiguousarray(v), dtype=t[k].dtype))
    for k in ('opt', 'psi_T', 'g_a', 'store', 'chi'):
        t[k].fill_(float('nan'))
    arena.check_layout()
    arena.snapshot()
    try:
        eng.backward(t['chi_T'], t['coef'], out=t['chi'])
        torch.cuda.synchronize(eng.device)
        arena.verify('backward', [t['chi']])
        if case['so']:
            eng.set_second_order(t['prev'], t['store'], t['sigma'])
        tc, tp = _tables(terms)
        eng.set_nonlinear(tc, tp, t['dcde'])
        assert eng._nl[1] is t['dcde']
        torch.cuda.synchronize(eng.device)
        arena.verify('set_nonlinear')
        from krotov_amd import _lib
        _lib.forget_launched_kernels()
        eng.forward_update(t['chi'], t['norms'], t['init'], t['guess'], t['S'], t['lam'], out=(t['opt'], t['psi_T'], t['g_a']))
        eng.check()
        torch.cuda.synchronize(eng.device)
        arena.verify('non-linear update', [t['opt'], t['psi_T'], t['g_a']] + ([t['store']] if case['so'] else []))
        launched = _lib.kernel_instantiations(launched_only=True)
        for want in case['expect']:
            assert want in launched, (want, launched)
        ref = r.ref
        assert np.abs(t['chi'].cpu().numpy() - r.ref_chi).max() < TOL
        assert np.abs(t['opt'].cpu().numpy() - np.array(ref[0])).max() < TOL
        assert np.abs(t['psi_T'].cpu().numpy() - ref[1]).max() < TOL
        assert np.abs(t['g_a'].cpu().numpy() - ref[2]).max() < TOL * max(1.0, np.abs(ref[2]).max())
        if case['so']:
            assert np.abs(t['store'].cpu().numpy() - ref[3]).max() < TOL
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_engines_and_tables_that_are_refused_say_so():
    import torch

    from krotov_amd import _lib, configs
    from krotov_amd.engine import HipKrotovEngine

    rng = np.random.default_rng(2)
    d, nt = 4, 6

    def code(call):
        with pytest.raises(_lib.KrotovHipError) as exc:
            call()
        return exc.value.code

    ops = [[configs.herm(rng, d, 1.0), configs.herm(rng, d, 0.5), configs.herm(rng, d, 0.5)] for _ in range(2)]
    eng = HipKrotovEngine(ops, np.full(nt - 1, 0.1))
    w = torch.ones((2, nt - 1), dtype=torch.float64, device=eng.device)
    assert code(lambda: eng.set_nonlinear([0, 0], [1, 5], w)) == _lib.KH_ERR_INVALID
    assert code(lambda: eng.set_nonlinear([0, 0], [0, 1], w)) == _lib.KH_ERR_INVALID
    assert code(lambda: eng.set_nonlinear([0, -1], [1, 2], w)) == _lib.KH_ERR_INVALID
    assert code(lambda: eng.set_nonlinear([1, 1], [1, 2], w)) == _lib.KH_ERR_INVALID  # (control 0 without a term)
    u = torch.zeros((2, nt - 1), dtype=torch.float64, device=eng.device)
    eng.set_parametrization([4, 4], [0.4, 0.4], [0.0, 0.0], u, w, torch.empty_like(u))
    assert code(lambda: eng.set_nonlinear([0, 0], [1, 2], w)) == _lib.KH_ERR_INVALID
    eng.set_parametrization()
    eng.set_nonlinear([0, 0], [1, 2], w)
    assert code(lambda: eng.set_parametrization([4, 4], [0.4, 0.4], [0.0, 0.0], u, w, torch.empty_like(u))) == _lib.KH_ERR_INVALID
    eng.set_nonlinear()
    eng.close()
    rep = HipKrotovEngine(ops, np.full((1, nt - 1), 0.1), replicas=1)
    assert code(lambda: rep.set_nonlinear([0, 0], [1, 2], w)) == _lib.KH_ERR_UNSUPPORTED
    rep.close()
    rho_ops = [[configs.herm(rng, 3, 1.0), configs.herm(rng, 3, 0.5), configs.herm(rng, 3, 0.5)]]
    lind = HipKrotovEngine(rho_ops, np.full(nt - 1, 0.1), c_ops=[[0.1 * configs.herm(rng, 3, 1.0)]])
    assert code(lambda: lind.set_nonlinear([0, 0], [1, 2], w)) == _lib.KH_ERR_UNSUPPORTED
    lind.close()


# ---------------------------------------------------------------------------
# GPU: optimize_pulses, propagate_objectives
# ---------------------------------------------------------------------------
class ConstSigma(krotov_amd.second_order.Sigma):
    def __init__(self, value):
        self.value = value

    def __call__(self, t):
        return self.value

    def refresh(self, **kwargs):
        pass


def _device_run(spec, iters, **kw):
    objectives, pulse_options = nc.product_side(spec, krotov_amd.Power)
    g_a = []
    res = krotov_amd.optimize_pulses(
        objectives, pulse_options, spec.tlist, propagator=krotov_amd.propagators.expm, norm=np.linalg.norm,
        chi_constructor=krotov_amd.functionals.chis_re, iter_stop=iters, store_all_pulses=True,
        info_hook=lambda **args: g_a.append(np.array(args['g_a_integrals'])), **kw)
    res.g_a = np.array(g_a)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize('shape', ['tile_n5', 'generic_n70', 'sigma', 'constraint', 'constraint_generic'])
def test_optimize_pulses_on_the_device_vs_restatement(shape, monkeypatch):
    from krotov_amd import _lib

    if shape == 'constraint_generic':  # (the generic kernels' backward sweep with source and their non-linear update)
        monkeypatch.setenv('KH_KERNEL', 'generic')
    if shape == 'generic_n70':
        spec = nc.problem(T3, K=2, N=70, nt=9)
    else:
        spec = nc.problem(T3, K=3, N=5, nt=9)
    prob, gp, S, lam = nc.oracle_side(spec)
    _lib.forget_launched_kernels()
    if shape == 'sigma':
        ref = nc.optimize_kept_states(prob, gp, S, lam, T3, ko.chis_re, 2, sigma=-1.5)
        res = _device_run(spec, 2, sigma=ConstSigma(-1.5))
    elif shape.startswith('constraint'):
        D = cc.projector(5, 3)
        ref = nc.optimize_kept_states(prob, gp, S, lam, T3, ko.chis_re, 2, D=D, lambda_b=0.4)
        res = _device_run(spec, 2, state_dependent_constraint=krotov_amd.QuadraticStateConstraint(D, 0.4))
    else:
        ref = nc.optimize(prob, gp, S, lam, T3, ko.chis_re, 2)
        res = _device_run(spec, 2)
    wrong = nc.optimize(prob, gp, S, lam, T3, ko.chis_re, 2, linear_weights=True)
    assert np.abs(wrong['all_pulses'] - nc.optimize(prob, gp, S, lam, T3, ko.chis_re, 2)['all_pulses']).max() > 1e3 * TOL
    _assert_matches(res, ref)
    launched = _lib.kernel_instantiations(launched_only=True)
    want = GEN if 'generic' in shape else TILE % (1, 3, 'false' if shape == 'tile_n5' else 'true')
    assert want in launched, (want, launched)
    assert np.array(res.optimized_controls).shape == (2, len(spec.tlist))
    g = res.optimized_objectives[0].H[2][1]
    assert isinstance(g, krotov_amd.Power) and g.control is res.optimized_controls[0]


@pytest.mark.gpu
def test_propagate_objectives_honours_a_power_control():
    spec = nc.problem(T3, K=3, N=5, nt=9)
    objectives, _ = nc.product_side(spec, krotov_amd.Power)
    got = krotov_amd.propagate_objectives(objectives, spec.tlist, propagator=krotov_amd.propagators.expm)
    prop, _, _ = numpy_plugins(False)
    for k, obj in enumerate(objectives):
        want = obj.propagate(spec.tlist, propagator=prop)
        one = obj.propagate(spec.tlist, propagator=krotov_amd.propagators.expm)
        assert np.abs(np.array(got[k].states) - np.array(want.states)).max() < TOL
        assert np.abs(np.array(one.states) - np.array(want.states)).max() < TOL
    # (``propagate`` samples a control on the grid points, not at the interval mid-points as the optimisation does)
    prob, _, _, _ = nc.oracle_side(spec)
    gp = [ko.control_onto_interval(ko.discretize(c, spec.tlist, args=({},))) for c in spec.nl_controls]
    _, states = ko.forward_propagation(prob, nc.coefficients(T3, gp), store=True)
    assert np.abs(np.array([r.states for r in got]) - states).max() < TOL
    linear = ko.forward_propagation(prob, [gp[0], gp[0], gp[1]])
    assert np.abs(linear - states[:, -1]).max() > 1e3 * TOL  # (the squares matter in this problem)


@pytest.mark.gpu
def test_lindblad_form_with_a_power_control_runs_the_liouvillian(caplog):
    from krotov_amd import configs

    rng = np.random.default_rng(8)
    d, nt = 3, 7
    H0, H1, H2 = configs.herm(rng, d, 1.0), configs.herm(rng, d, 0.7), configs.herm(rng, d, 0.4)
    c_op = 0.2 * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
    eps = lambda t, args: 0.1 + 0.2 * np.sin(np.pi * t)  # noqa: E731
    rho0, rho1 = np.zeros((d, d), dtype=np.complex128), np.zeros((d, d), dtype=np.complex128)
    rho0[0, 0] = rho1[1, 1] = 1.0
    tlist = np.linspace(0.0, 1.0, nt)
    obj = krotov_amd.Objective(initial_state=rho0, target=rho1, H=[H0, [H1, eps], [H2, krotov_amd.Power(eps, 2)]], c_ops=[c_op])
    S = lambda t: ko.flattop(t, 0.0, 1.0, 0.2)  # noqa: E731
    with caplog.at_level(logging.INFO, logger='krotov'):
        res = krotov_amd.optimize_pulses(
            [obj], {eps: dict(lambda_a=2.0, update_shape=S)}, tlist, propagator=krotov_amd.propagators.LindbladExpm(),
            chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2, store_all_pulses=True, norm=np.linalg.norm)
    assert any('Liouvillian fallback (non-linear' in rec.getMessage() for rec in caplog.records)
    L = [configs.liouvillian_dense(H0, [c_op]), configs.liouvillian_dense(H1, []), configs.liouvillian_dense(H2, [])]
    prob = ko.OracleProblem([L], rho0.ravel(order='F')[None], rho1.ravel(order='F')[None], tlist, is_super=True)
    _, gp, shapes = ko.initialize_controls([eps], [S], tlist)
    ref = nc.optimize(prob, gp, shapes, [2.0], T2, ko.chis_re, 2)
    _assert_matches(res, ref, TOL_LIOUVILLE)
