"""Pulse parametrizations (bounded controls): eps = f(u), Krotov's update applied to u.

Yardsticks (tests/parametrization_cases.py): (A) ``LINEAR`` eps = a u + b against the untouched ``oracle.optimize`` with
lambda / a**2; (B) every other kind against a NumPy restatement of ``oracle.forward_update_sweep`` with the update in u.

Tolerance: the project's 1e-12 for Hilbert-space problems (1e-11 on Liouvillians).  f adds three roundings per value
(a, b, the product-sum) and a tanh that differs between libraries by an ulp; perturbing EVERY f value of the host problem
below by +-1 ulp moves the ``TANH`` pulses by < 1e-15 over eight iterations
(``test_ulp_sensitivity_of_the_bounded_case``), four orders of magnitude inside 1e-12: the device tanh needs no tolerance
of its own.
"""
import logging

import numpy as np
import pytest

import parametrization_cases as pc
from helpers import numpy_plugins
from oracle import krotov_oracle as ko

import krotov_amd

TOL = 1e-12
TANH = ('tanh',) + pc.BOUNDS
NORM = lambda prob, chi: float(np.linalg.norm(chi))  # noqa: E731


# ---------------------------------------------------------------------------
# host: classes
# ---------------------------------------------------------------------------
CLASSES = {
    'linear': (lambda: krotov_amd.LinearParametrization(0.7, 0.3), np.linspace(-3.0, 3.0, 41)),
    'square': (lambda: krotov_amd.SquareParametrization(), np.linspace(0.05, 2.0, 41)),
    'tanhsq': (lambda: krotov_amd.TanhSqParametrization(0.8), np.linspace(0.05, 2.5, 41)),
    'tanh': (lambda: krotov_amd.TanhParametrization(*pc.BOUNDS), np.linspace(-2.5, 2.5, 41)),
}


@pytest.mark.parametrize('name', sorted(CLASSES))
def test_classes_round_trip_and_derivative(name):
    make, u = CLASSES[name]
    par = make()
    assert isinstance(par, krotov_amd.Parametrization) and par.kind in (1, 2, 3, 4)
    eps = par.eps(u)
    # u -> eps -> u: the inverse amplifies the rounding of eps by 1 / |f'(u)| (>= 0.02 on these grids)
    assert np.abs(par.u(eps) - u).max() < 4 * np.finfo(float).eps * np.abs(eps).max() / np.abs(par.deps_du(u)).min()
    # central difference with step h: truncation h^2 |f'''| / 6 (|f'''| <= 4 |a| for these forms, a <= 1) plus rounding
    # eps_machine |f| / h (|f| <= 9 on the linear grid): h = 1e-5 gives 7e-11 + 2e-10
    h = 1e-5
    central = (par.eps(u + h) - par.eps(u - h)) / (2 * h)
    assert np.abs(central - par.deps_du(u)).max() < 5e-10
    # the module's own restatement in the tests agrees with the classes (the yardstick is independent code)
    kind = {'linear': ('linear', 0.7, 0.3), 'square': ('square',), 'tanhsq': ('tanhsq', 0.8), 'tanh': TANH}[name]
    assert np.abs(pc.f(kind, u) - eps).max() < 1e-15 and np.abs(pc.dfdu(kind, u) - par.deps_du(u)).max() < 1e-15
    assert (par.a, par.b) == pc._ab(kind) or name == 'square'


def test_classes_reject_values_outside_the_range():
    tanh = krotov_amd.TanhParametrization(*pc.BOUNDS)
    for bad in (0.45, -0.4, 0.5, -1.0, np.nan):
        with pytest.raises(ValueError, match='outside the range'):
            tanh.u(np.array([0.0, bad]))
    with pytest.raises(ValueError, match='index 1'):
        krotov_amd.SquareParametrization().u(np.array([0.0, -1e-3]))
    with pytest.raises(ValueError):
        krotov_amd.TanhSqParametrization(0.8).u(np.array([0.8]))
    # a value that rounding put on (or an ulp beyond) a bound is pulled inside when asked to; nothing further out is
    on = np.array([0.45, np.nextafter(0.45, 1.0), -0.4])
    u = tanh.u(on, pull=True)
    assert np.all(np.isfinite(u)) and u[0] > 15 and u[2] < -15
    with pytest.raises(ValueError):
        tanh.u(np.array([0.4500001]), pull=True)
    with pytest.raises(ValueError):
        krotov_amd.TanhParametrization(0.3, 0.3)
    with pytest.raises(ValueError):
        krotov_amd.LinearParametrization(0.0)


# ---------------------------------------------------------------------------
# host: optimize_pulses through the plugin path
# ---------------------------------------------------------------------------
def _host_run(spec, kinds, iters, **kw):
    prop, mu, overlap = numpy_plugins()
    objectives, pulse_options = pc.product_side(spec, kinds)
    kw.setdefault('store_all_pulses', True)
    g_a = []
    hook = kw.pop('info_hook', None)

    def record(**args):
        g_a.append(np.array(args['g_a_integrals']))
        return None if hook is None else hook(**args)

    res = krotov_amd.optimize_pulses(
        objectives, pulse_options, spec.tlist, propagator=prop, mu=mu, overlap=overlap, norm=np.linalg.norm,
        chi_constructor=krotov_amd.functionals.chis_re, iter_stop=iters, info_hook=record, **kw)
    res.g_a = np.array(g_a)
    return res


def _assert_matches(res, ref, tol=TOL):
    scale = max(1.0, np.abs(ref['all_pulses']).max())
    got = np.array(res.all_pulses)
    assert got.shape == ref['all_pulses'].shape
    print("max |d pulse| = %.3e  max |d tau| = %.3e" % (np.abs(got - ref['all_pulses']).max(),
                                                        np.abs(np.array(res.tau_vals) - ref['tau_vals']).max()))
    assert np.abs(got - ref['all_pulses']).max() < tol * scale
    assert np.abs(np.array(res.tau_vals) - ref['tau_vals']).max() < tol
    if hasattr(res, 'g_a'):
        assert np.abs(res.g_a - ref['g_a']).max() < tol * max(1.0, np.abs(ref['g_a']).max())


@pytest.mark.parametrize('a,b', [(2.0, 0.0), (0.7, 0.3)])
def test_linear_is_the_oracle_with_rescaled_lambda(a, b):
    """(A): eps = a u + b is the unparametrized update with lambda / a**2 -- pulses, tau and the u-space running cost
    (S / lambda') D^2 dt with lambda' = lambda / a**2 is what the oracle itself integrates."""
    spec = pc.problem()
    prob, gp, S, lam = pc.oracle_side(spec)
    ref = ko.optimize(prob, gp, S, [x / a ** 2 for x in lam], ko.chis_re, 5, norm=NORM)
    res = _host_run(spec, [('linear', a, b)] * 2, 5)
    _assert_matches(res, ref)
    # ... and the restatement (B) agrees with (A) too: the two yardsticks measure the same thing
    ref_b = pc.optimize(prob, gp, S, lam, ko.chis_re, 5, [('linear', a, b)] * 2)
    assert np.abs(ref_b['all_pulses'] - ref['all_pulses']).max() < 1e-14


@pytest.mark.parametrize('kinds', [[TANH, TANH], [TANH, None], [('square',), ('tanhsq', 0.8)]],
                         ids=['tanh', 'tanh_none', 'square_tanhsq'])
def test_bounded_kinds_match_the_restatement(kinds):
    """(B).  In the mixed lists control 1 keeps today's arithmetic (f = identity, c = 1); its guess is positive, so it is
    also inside the range of the kinds bounded below by zero."""
    spec = pc.problem()
    if kinds[0] == ('square',):
        spec.controls[0] = lambda t, args: 0.08 + 0.15 * np.cos(np.pi * t / 2.0) ** 2  # (a positive guess here too)
    prob, gp, S, lam = pc.oracle_side(spec)
    ref = pc.optimize(prob, gp, S, lam, ko.chis_re, 5, kinds)
    _assert_matches(_host_run(spec, kinds, 5), ref)


def _J_T_re(taus):
    return 1.0 - float(np.mean(np.real(taus)))


def test_the_case_bites_and_the_bounded_run_stays_inside():
    """Unparametrized, the pulses of this problem leave [-0.4, 0.45] within eight iterations; with TANH every iteration
    stays inside -- up to 2 ulp of max(|eps_min|, |eps_max|) for the three roundings in a, b and the product-sum -- and
    J_T falls monotonically, as does every iteration's running cost stay non-negative."""
    spec = pc.problem()
    lo, hi = pc.BOUNDS
    free = np.array(_host_run(spec, None, 8).all_pulses)
    print("unparametrized: %.3f ... %.3f" % (free.min(), free.max()))
    assert free.min() < lo - 0.05 and free.max() > hi + 0.05
    res = _host_run(spec, [TANH, TANH], 8)
    bounded = np.array(res.all_pulses)
    slack = 2 * np.spacing(max(abs(lo), abs(hi)))
    print("bounded:        %.6f ... %.6f" % (bounded.min(), bounded.max()))
    assert bounded.min() >= lo - slack and bounded.max() <= hi + slack
    assert not np.array_equal(bounded[-1], bounded[0])
    J = [_J_T_re(t) for t in res.tau_vals]
    assert all(J[i + 1] < J[i] for i in range(len(J) - 1)), J
    assert np.all(res.g_a >= 0.0) and np.all(res.g_a[1:].sum(axis=1) > 0.0)


def test_ulp_sensitivity_of_the_bounded_case():
    """The experiment behind the tolerance: every f value moved by +-1 ulp (alternating) moves the pulses of eight
    iterations by far less than 1e-13 = TOL / 10."""
    spec = pc.problem()
    prob, gp, S, lam = pc.oracle_side(spec)
    ref = pc.optimize(prob, gp, S, lam, ko.chis_re, 8, [TANH, TANH])
    moved = pc.optimize(prob, gp, S, lam, ko.chis_re, 8, [TANH, TANH],
                        perturb=lambda l, n, v: np.nextafter(v, np.inf if (l + n) % 2 else -np.inf))
    d = np.abs(moved['all_pulses'] - ref['all_pulses']).max()
    print("+-1 ulp on every f value: max |d pulse| = %.3e" % d)
    assert 0 < d < 1e-13


def test_an_edited_pulse_gets_its_parameter_inverted_again():
    """``modify_params_after_iter`` halves control 0 after iteration 1: iteration 2 starts from u = f^-1(edited pulse) for
    that control, and from the carried u for the other one."""
    spec = pc.problem()
    prob, gp, S, lam = pc.oracle_side(spec)

    def halve(**args):
        if args['iteration'] == 1:
            args['optimized_pulses'][0] *= 0.5

    def edit(it, pulses):
        if it == 1:
            pulses[0] *= 0.5
            return [0]
        return []

    res = _host_run(spec, [TANH, TANH], 3, modify_params_after_iter=halve)
    ref = pc.optimize(prob, gp, S, lam, ko.chis_re, 3, [TANH, TANH], edit=edit)
    _assert_matches(res, ref)
    # the witness: carrying the stale u instead gives other pulses
    stale = pc.optimize(prob, gp, S, lam, ko.chis_re, 3, [TANH, TANH], edit=lambda it, p: edit(it, p) and [])
    assert np.abs(stale['all_pulses'][2] - ref['all_pulses'][2]).max() > 1e-3


def test_continue_from_reproduces_the_uninterrupted_run():
    spec = pc.problem()
    whole = _host_run(spec, [TANH, TANH], 5)
    first = _host_run(spec, [TANH, TANH], 2)
    rest = _host_run(spec, [TANH, TANH], 5, continue_from=first)
    assert rest.iters == whole.iters
    assert np.abs(np.array(rest.all_pulses) - np.array(whole.all_pulses)).max() < TOL
    assert np.abs(np.array(rest.tau_vals) - np.array(whole.tau_vals)).max() < TOL
    # a stored pulse that rounding put on a bound does not stop the continuation
    on_bound = [np.array(p) for p in first.all_pulses[-1]]
    on_bound[0][3:5] = pc.BOUNDS[1]
    on_bound[1][7] = pc.BOUNDS[0]
    first.optimized_controls = [krotov_amd.conversions.pulse_onto_tlist(p) for p in on_bound]
    again = _host_run(spec, [TANH, TANH], 3, continue_from=first)
    lo, hi = pc.BOUNDS
    slack = 2 * np.spacing(max(abs(lo), abs(hi)))
    assert np.array(again.all_pulses).min() >= lo - slack and np.array(again.all_pulses).max() <= hi + slack


def test_guess_outside_the_range_names_control_and_interval():
    spec = pc.problem()
    prop, mu, overlap = numpy_plugins()
    objectives, pulse_options = pc.product_side(spec, [None, ('tanh', -0.1, 0.1)])
    _, gp, _, _ = pc.oracle_side(spec)
    n_bad = int(np.flatnonzero(~((gp[1] > -0.1) & (gp[1] < 0.1)))[0])
    with pytest.raises(ValueError, match=r'control 1.*index %d\b' % n_bad):
        krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, propagator=prop, mu=mu, overlap=overlap,
                                   chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1)
    pulse_options[spec.controls[0]]['parametrization'] = 'tanh'
    with pytest.raises(ValueError, match='Parametrization'):
        krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, propagator=prop, mu=mu, overlap=overlap,
                                   chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1)


def test_user_defined_subclass_runs_the_host_loop():
    """``kind = None``: evaluated on the host, the same five lines -- here a re-implementation of TANH, against (B)."""
    lo, hi = pc.BOUNDS
    a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)

    class Mine(krotov_amd.Parametrization):
        def eps(self, u):
            return a * np.tanh(u) + b

        def deps_du(self, u):
            return a * (1.0 - np.tanh(u) ** 2)

        def u(self, eps):
            return np.arctanh((np.asarray(eps) - b) / a)

    assert Mine().kind is None
    spec = pc.problem()
    prob, gp, S, lam = pc.oracle_side(spec)
    prop, mu, overlap = numpy_plugins()
    objectives, pulse_options = pc.product_side(spec, None)
    for c in spec.controls:
        pulse_options[c]['parametrization'] = Mine()
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, propagator=prop, mu=mu, overlap=overlap,
                                     norm=np.linalg.norm, chi_constructor=krotov_amd.functionals.chis_re, iter_stop=3,
                                     store_all_pulses=True)
    _assert_matches(res, pc.optimize(prob, gp, S, lam, ko.chis_re, 3, [TANH, TANH]))


def test_batch_runs_a_parametrized_problem_through_optimize_pulses(caplog):
    from krotov_amd import batch

    spec = pc.problem()
    prop, _, _ = numpy_plugins()
    objectives, pulse_options = pc.product_side(spec, [TANH, None])
    problems = [dict(objectives=objectives, pulse_options=pulse_options, tlist=spec.tlist)]
    kw = dict(propagator=prop, chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2, store_all_pulses=True)
    results = krotov_amd.optimize_pulses_batch(problems, **kw)
    alone = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, **kw)
    assert np.array_equal(np.array(results[0].all_pulses), np.array(alone.all_pulses))
    assert np.array_equal(np.array(results[0].tau_vals), np.array(alone.tau_vals))
    plain = krotov_amd.optimize_pulses(*pc.product_side(spec, None), spec.tlist, **kw)
    assert not np.array_equal(np.array(alone.all_pulses), np.array(plain.all_pulses))
    # with the device propagator the parametrization is what keeps the problem out of the batch (host-only decision)
    reps = [batch._Replica(p, krotov_amd.propagators.expm, kw['chi_constructor'], 2, True, None) for p in problems]
    assert 'parametrization' in batch._batch_obstacle(problems, reps, krotov_amd.propagators.expm)
    plain_problems = [dict(objectives=o, pulse_options=po, tlist=spec.tlist) for o, po in [pc.product_side(spec, None)]]
    reps = [batch._Replica(p, krotov_amd.propagators.expm, kw['chi_constructor'], 2, True, None) for p in plain_problems]
    assert batch._batch_obstacle(plain_problems, reps, krotov_amd.propagators.expm) is None


def test_process_group_with_a_parametrization_raises():
    spec = pc.problem()
    objectives, pulse_options = pc.product_side(spec, [TANH, None])
    with pytest.raises(ValueError, match='process_group'):
        krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, propagator=krotov_amd.propagators.expm,
                                   chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1, process_group=object())


def test_lindblad_layout_takes_a_parametrization_as_a_reason_to_fall_back():
    from krotov_amd import mixed

    rng = np.random.default_rng(3)
    d = 3
    H = [krotov_amd.configs.herm(rng, d, 1.0), [krotov_amd.configs.herm(rng, d, 1.0), lambda t, args: 0.1]]
    rho = np.diag([1.0, 0.0, 0.0]).astype(complex)
    objs = [krotov_amd.Objective(initial_state=rho, target=rho, H=H, c_ops=[0.1 * np.eye(d, k=1).astype(complex)])]
    assert mixed.lindblad_layout_of(objs, None, 1, False).matrix
    lay = mixed.lindblad_layout_of(objs, None, 1, False, True)
    assert not lay.matrix and 'parametrization' in lay.reason


def test_c_abi_declares_the_entry_point_and_the_kinds():
    import os

    from krotov_amd import _lib, parametrization

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'krotov_hip.h')).read()
    for name, value in (('NONE', 0), ('LINEAR', 1), ('SQUARE', 2), ('TANHSQ', 3), ('TANH', 4)):
        assert 'KH_PAR_%s = %d' % (name, value) in header
        assert getattr(parametrization, 'KH_PAR_' + name) == value
    lib = _lib.load()
    assert lib.kh_set_parametrization(None, None, None, None, None, None, None) == _lib.KH_ERR_INVALID
    names = _lib.kernel_instantiations()
    want = ['kh_gen_forward_update_par<false>', 'kh_gen_forward_update_par<true>']
    want += ['kh_tile_forward_update_par<1, %d, %s>' % (l, so) for l in (1, 2, 3, 4) for so in ('false', 'true')]
    want += ['kh_tile_forward_update_par<2, 1, false>', 'kh_tile_forward_update_par<2, 1, true>']
    assert sorted(n for n in names if '_par<' in n) == sorted(want)


# ---------------------------------------------------------------------------
# GPU: sweep level, every new instantiation named and confirmed with kh_debug_launched
# ---------------------------------------------------------------------------
def _kinds(L, shift=0):
    """Kinds mixed across the controls; odd controls have positive guesses (the kinds bounded below by zero sit there)."""
    out = []
    for l in range(L):
        if l % 2 == 0:
            out.append([TANH, None, ('linear', 0.7, 0.3)][(l // 2 + shift) % 3])
        else:
            out.append([('tanhsq', 0.8), ('square',)][(l // 2 + shift) % 2])
    return out


def _device_arrays(kinds, gp):
    from krotov_amd.parametrization import PulseParameters

    par = PulseParameters([pc.to_product(k) for k in kinds], gp)
    kind, a, b = par.device_kinds
    u_guess = np.array([pc.inverse(k, p) for k, p in zip(kinds, gp)])
    assert np.abs(np.array(par.u) - u_guess).max() < 1e-14
    return kind, a, b, u_guess, np.array([pc.dfdu(k, u) for k, u in zip(kinds, u_guess)])


SWEEPS = {}


def sweep(name, build, kinds, expect, so=False, env=None, fmt='dense', mode='whole', reduced=0, kernel=None):
    SWEEPS[name] = dict(build=build, kinds=kinds, expect=expect, so=so, env=env or {}, fmt=fmt, mode=mode,
                        reduced=reduced, kernel=kernel)


# ---- the register-tile kernel's parametrized form (kh_tile64.h): <rows per thread, controls, second order>; the q2, mini
# and quad engines of one control run it too
for _N in (5, 64):
    for _L in (1, 2, 3, 4):
        for _so in (False, True):
            sweep('tile_n%d_L%d%s' % (_N, _L, '_so' if _so else ''),
                  lambda N=_N, L=_L: pc.problem(K=3, N=N, L=L, nt=14), _kinds(_L, _N),
                  ['kh_tile_forward_update_par<1, %d, %s>' % (_L, 'true' if _so else 'false')], so=_so)
for _so in (False, True):
    sweep('tile256_k257%s' % ('_so' if _so else ''), lambda: pc.problem(K=257, N=4, L=1, nt=8), [TANH],
          ['kh_tile_forward_update_par<2, 1, %s>' % ('true' if _so else 'false')], so=_so, kernel='tile64/256')
# ---- the generic kernels' parametrized form (kh_generic.h): <mixed>; every other route of a parametrized engine
GEN = 'kh_gen_forward_update_par<false>'
sweep('gen_n70_tile128', lambda: pc.problem(K=2, N=70, L=2, nt=10), [TANH, ('tanhsq', 0.8)], [GEN], kernel='tile128/512')
sweep('gen_n70_tile128_so', lambda: pc.problem(K=2, N=70, L=2, nt=10), [TANH, ('square',)], [GEN], so=True)
sweep('gen_csr_n20', lambda: pc.problem(K=2, N=20, L=2, nt=12, bands=3), [TANH, ('tanhsq', 0.8)], [GEN], fmt='csr')
sweep('gen_L9', lambda: pc.problem(K=3, N=12, L=9, nt=10), _kinds(9), [GEN])
sweep('gen_stepwise', lambda: pc.problem(K=3, N=64, L=2, nt=12), [TANH, ('tanhsq', 0.8)], [GEN], mode='stepwise')
sweep('gen_stepwise_so', lambda: pc.problem(K=3, N=20, L=1, nt=12), [TANH], [GEN], mode='stepwise', so=True)
sweep('gen_reduced_n64', lambda: pc.problem(K=6, N=64, L=2, nt=12), [TANH, ('square',)], [GEN], reduced=4)
sweep('gen_one_objective', lambda: pc.problem(K=1, N=64, L=1, nt=12), [TANH], [GEN])
sweep('gen_linear_n80', lambda: pc.problem(K=2, N=80, L=2, nt=10), [('linear', 2.0, 0.0), ('linear', 0.7, 0.3)], [GEN])


def _engine(spec, fmt):
    from krotov_amd import configs
    from krotov_amd.engine import HipKrotovEngine

    if fmt == 'csr':
        ops = configs.sparse_ops(spec)
    else:
        ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    return HipKrotovEngine(ops, np.diff(spec.tlist), is_super=spec.is_super)


def _run_sweep(eng, case, prob, gp, S, lam, init, rng):
    """One parametrized update sweep on ``eng`` against (B); returns the device outputs (host arrays)."""
    import torch

    from krotov_amd import _lib

    kinds = case['kinds']
    nt = len(prob.tlist)
    pulses = np.array(gp)
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    norms = (0.2 + rng.random(prob.K)) * min(1.0, 8.0 / prob.K)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    chi = eng.backward(chi_T, pulses)
    kind, a, b, u_guess, dfdu = _device_arrays(kinds, gp)
    kw = {}
    store = None
    if case['so']:
        older = [p * (1.0 + 0.1 * rng.standard_normal(p.shape)) for p in gp]  # the "previous iteration"
        _, prev = ko.forward_propagation(prob, older, store=True)
        sigma_vals = -(1.0 + rng.random(nt - 1)) * min(1.0, 8.0 / prob.K)
        kw = dict(sigma_vals=sigma_vals, fw_prev=prev, store=True)
        store = torch.full((prob.K, nt, prob.N), float('nan'), dtype=torch.complex128, device=eng.device)
        eng.set_second_order(prev, store, sigma_vals)
    u_opt = torch.full((len(gp), nt - 1), float('nan'), dtype=torch.float64, device=eng.device)
    eng.set_parametrization(kind, a, b, u_guess, dfdu, u_opt)
    if case['reduced']:
        assert eng.set_update_workgroups(case['reduced']) == case['reduced']
    _lib.forget_launched_kernels()
    if case['mode'] == 'stepwise':
        opt, psi_T, g_a = eng.forward_update_sharded(chi, norms, init, pulses, np.array(S), np.array(lam),
                                                     lambda x: None, graph_chunk=0)
    else:
        opt, psi_T, g_a = eng.forward_update(chi, norms, init, pulses, np.array(S), np.array(lam))
    eng.check()
    launched = _lib.kernel_instantiations(launched_only=True)
    ref = pc.update_sweep(prob, ref_chi, norms, list(u_guess), kinds, S, lam, **kw)
    tol = 1e-11 if prob.is_super else TOL
    out = dict(opt=opt.cpu().numpy(), u=u_opt.cpu().numpy(), psi=psi_T.cpu().numpy(), g_a=g_a.cpu().numpy())
    d = dict(chi=np.abs(chi.cpu().numpy() - ref_chi).max(), opt=np.abs(out['opt'] - np.array(ref[0])).max(),
             u=np.abs(out['u'] - np.array(ref[1])).max(), psi=np.abs(out['psi'] - ref[2]).max(),
             g_a=np.abs(out['g_a'] - ref[3]).max())
    print(' '.join('%s %.2e' % kv for kv in sorted(d.items())), '|', eng.kernel, [n for n in launched if 'update' in n])
    assert d['chi'] < tol
    assert d['opt'] < tol * max(1.0, np.abs(np.array(ref[0])).max())
    assert d['u'] < tol * max(1.0, np.abs(np.array(ref[1])).max())
    assert d['psi'] < tol
    assert d['g_a'] < tol * max(1.0, np.abs(ref[3]).max())
    if case['so']:
        assert np.abs(store.cpu().numpy() - ref[4]).max() < tol
    for want in case['expect']:
        assert want in launched, (want, launched)
    # the pulses the sweep propagated with are f(u) of the u it stored, and a LINEAR control is (A)'s update
    for l, k in enumerate(kinds):
        assert np.abs(pc.f(k, out['u'][l]) - out['opt'][l]).max() < 1e-15 * max(1.0, np.abs(out['opt'][l]).max()) * 4
    return out, ref, (chi, norms, pulses)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SWEEPS))
def test_parametrized_sweep_vs_restatement(name, monkeypatch):
    case = SWEEPS[name]
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    spec = case['build']()
    prob, gp, S, lam = pc.oracle_side(spec)
    eng = _engine(spec, case['fmt'])
    if case['kernel'] is not None:
        assert eng.kernel == case['kernel'], eng.kernel
    if case['fmt'] == 'csr':
        assert eng.kernel.endswith('/csr'), eng.kernel
    _run_sweep(eng, case, prob, gp, S, lam, spec.init, np.random.default_rng(17))
    eng.close()


@pytest.mark.gpu
def test_linear_sweep_is_the_oracles_sweep_with_rescaled_lambda():
    """(A) at the sweep level: eps = a u + b against ``oracle.forward_update_sweep`` with lambda / a**2; g_a is the
    oracle's own integral (the cost in u)."""
    spec = pc.problem(K=3, N=64, L=2, nt=14)
    prob, gp, S, lam = pc.oracle_side(spec)
    kinds = [('linear', 2.0, 0.0), ('linear', 0.7, 0.3)]
    eng = _engine(spec, 'dense')
    case = dict(kinds=kinds, so=False, reduced=0, mode='whole', expect=['kh_tile_forward_update_par<1, 2, false>'])
    rng = np.random.default_rng(17)
    out, _, (chi, norms, pulses) = _run_sweep(eng, case, prob, gp, S, lam, spec.init, rng)
    ref = ko.forward_update_sweep(prob, ko.backward_sweep(prob, prob.target / np.linalg.norm(prob.target, axis=1)[:, None], gp),
                                  norms, gp, S, [lam[0] / 4.0, lam[1] / 0.49])
    assert np.abs(out['opt'] - np.array(ref[0])).max() < TOL
    assert np.abs(out['psi'] - ref[1]).max() < TOL
    assert np.abs(out['g_a'] - ref[2]).max() < TOL * max(1.0, np.abs(ref[2]).max())
    eng.close()


@pytest.mark.gpu
def test_mixed_dimensions_sweep_vs_restatement():
    """Objectives of dimension 3, 5 and 9 (a ket, a ket, a density matrix) under one TANH control: the generic kernels'
    mixed form."""
    from test_mixed_objectives import _engine_ops, _pad_vec, _vec, oracle_adapter, spec_controls

    from krotov_amd import configs
    from krotov_amd.engine import HipKrotovEngine

    spec = configs.config_mixed('dims', nt=41)
    prob = oracle_adapter(spec)
    gp, S, lam = spec_controls(spec)
    eng = HipKrotovEngine(_engine_ops(spec), np.diff(spec.tlist), is_super=spec.kinds)
    assert eng.kernel == 'generic/mixed'
    init = np.array([_pad_vec(_vec(s), spec.N) for s in spec.init])
    case = dict(kinds=[('tanh', -0.05, 0.3)], so=False, reduced=0, mode='whole', expect=['kh_gen_forward_update_par<true>'])
    _run_sweep(eng, case, prob, [np.array(p) for p in gp], S, list(lam), init, np.random.default_rng(5))
    case = dict(case, so=True, mode='stepwise')
    _run_sweep(eng, case, prob, [np.array(p) for p in gp], S, list(lam), init, np.random.default_rng(6))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tile_n64_L2', 'gen_n70_tile128', 'tile_n5_L1'])
def test_two_runs_are_bitwise_equal_and_switching_off_restores_the_engine(name):
    """Two parametrized sweeps give the same bits; after ``set_parametrization(None)`` the engine reproduces its earlier
    unparametrized sweep bit for bit, on its earlier kernel."""
    from krotov_amd import _lib

    case = SWEEPS[name]
    spec = case['build']()
    prob, gp, S, lam = pc.oracle_side(spec)
    eng = _engine(spec, case['fmt'])
    rng = np.random.default_rng(17)
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    pulses = np.array(gp)
    chi = eng.backward(chi_T, pulses)
    norms = 0.2 + rng.random(prob.K)

    def plain():
        _lib.forget_launched_kernels()
        out = [x.cpu().numpy() for x in eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))]
        eng.check()
        return out, sorted(n for n in _lib.kernel_instantiations(launched_only=True) if 'forward_update' in n)

    before, kernels_before = plain()
    ref = ko.forward_update_sweep(prob, ko.backward_sweep(prob, chi_T, gp), norms, gp, S, lam)
    assert np.abs(before[0] - np.array(ref[0])).max() < TOL and np.abs(before[1] - ref[1]).max() < TOL
    assert not any('_par<' in n for n in kernels_before)
    one, _, _ = _run_sweep(eng, case, prob, gp, S, lam, spec.init, np.random.default_rng(17))
    two, _, _ = _run_sweep(eng, case, prob, gp, S, lam, spec.init, np.random.default_rng(17))
    for key in one:
        assert np.array_equal(one[key], two[key]), key
    assert not np.array_equal(one['opt'], before[0])
    eng.set_parametrization(None)
    after, kernels_after = plain()
    assert kernels_after == kernels_before
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    eng.close()


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_engines_that_take_no_parametrization_say_so():
    import torch

    from krotov_amd import _lib, configs
    from krotov_amd.engine import HipKrotovEngine

    rng = np.random.default_rng(2)
    d, nt = 4, 6

    def refused(eng, L):
        kind = np.full(L, 4, dtype=np.int32)
        a, b = np.full(L, 0.4), np.zeros(L)
        u = torch.zeros((L, nt - 1), dtype=torch.float64, device=eng.device)
        with pytest.raises(_lib.KrotovHipError) as err:
            eng.set_parametrization(kind, a, b, u, torch.ones_like(u), torch.empty_like(u))
        assert err.value.code == _lib.KH_ERR_UNSUPPORTED

    H = [[configs.herm(rng, d, 1.0), configs.herm(rng, d, 0.5)] for _ in range(2)]
    c_ops = [[0.1 * np.eye(d, k=1).astype(complex)] for _ in range(2)]
    lind = HipKrotovEngine(H, np.full(nt - 1, 0.1), c_ops=c_ops)
    assert lind.kernel.startswith('lindblad')
    refused(lind, 1)
    lind.close()
    ops = [[configs.herm(rng, d, 1.0), configs.herm(rng, d, 0.5)] for _ in range(4)]
    rep = HipKrotovEngine(ops, np.full((2, nt - 1), 0.1), replicas=2)
    assert rep.replicas == 2
    refused(rep, 1)
    rep.close()
    # an unknown kind is an invalid argument, not a crash
    eng = HipKrotovEngine(ops, np.full(nt - 1, 0.1))
    u = torch.zeros((1, nt - 1), dtype=torch.float64, device=eng.device)
    with pytest.raises(_lib.KrotovHipError) as err:
        eng.set_parametrization([7], [1.0], [0.0], u, torch.ones_like(u), torch.empty_like(u))
    assert err.value.code == _lib.KH_ERR_INVALID
    with pytest.raises(_lib.KrotovHipError) as err:
        eng.set_parametrization([4], [1.0], [0.0], u, torch.ones_like(u), u)
    assert err.value.code == _lib.KH_ERR_INVALID
    eng.close()


# ---------------------------------------------------------------------------
# GPU: optimize_pulses on the device path
# ---------------------------------------------------------------------------
def _device_run(spec, kinds, iters, propagator=None, **kw):
    objectives, pulse_options = pc.product_side(spec, kinds)
    g_a = []

    def record(**args):
        g_a.append(np.array(args['g_a_integrals']))

    res = krotov_amd.optimize_pulses(
        objectives, pulse_options, spec.tlist, propagator=propagator or krotov_amd.propagators.expm,
        chi_constructor=krotov_amd.functionals.chis_re, iter_stop=iters, store_all_pulses=True, info_hook=record, **kw)
    res.g_a = np.array(g_a)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize('shape', ['tile_n5', 'tile_n64_L3', 'generic_n70'])
def test_optimize_pulses_on_the_device_vs_restatement(shape):
    from krotov_amd import _lib
    from krotov_amd.engine import LAST_ENGINE

    build, kinds, want = {
        'tile_n5': (lambda: pc.problem(), [TANH, ('tanhsq', 0.8)], 'kh_tile_forward_update_par<1, 2, false>'),
        'tile_n64_L3': (lambda: pc.problem(K=3, N=64, L=3, nt=20), [TANH, ('square',), None], 'kh_tile_forward_update_par<1, 3, false>'),
        'generic_n70': (lambda: pc.problem(K=2, N=70, L=2, nt=16), [TANH, None], 'kh_gen_forward_update_par<false>'),
    }[shape]
    spec = build()
    prob, gp, S, lam = pc.oracle_side(spec)
    _lib.forget_launched_kernels()
    res = _device_run(spec, kinds, 3)
    launched = _lib.kernel_instantiations(launched_only=True)
    assert want in launched, (want, LAST_ENGINE().kernel, launched)
    _assert_matches(res, pc.optimize(prob, gp, S, lam, ko.chis_re, 3, kinds))


@pytest.mark.gpu
def test_device_run_stays_inside_the_bounds_where_the_free_run_leaves_them():
    spec = pc.problem()
    lo, hi = pc.BOUNDS
    free = np.array(_device_run(spec, None, 8).all_pulses)
    assert free.min() < lo - 0.05 and free.max() > hi + 0.05
    res = _device_run(spec, [TANH, TANH], 8)
    bounded = np.array(res.all_pulses)
    slack = 2 * np.spacing(max(abs(lo), abs(hi)))
    print("device: unparametrized %.3f ... %.3f, bounded %.6f ... %.6f" % (free.min(), free.max(), bounded.min(), bounded.max()))
    assert bounded.min() >= lo - slack and bounded.max() <= hi + slack
    J = [_J_T_re(t) for t in res.tau_vals]
    assert all(J[i + 1] < J[i] for i in range(len(J) - 1)), J
    prob, gp, S, lam = pc.oracle_side(spec)
    _assert_matches(res, pc.optimize(prob, gp, S, lam, ko.chis_re, 8, [TANH, TANH]))


@pytest.mark.gpu
def test_device_edit_continue_and_batch():
    """An edited pulse is inverted again, a continued run reproduces the uninterrupted one, and the batch driver hands a
    parametrized problem to ``optimize_pulses`` -- all on the device path."""
    spec = pc.problem()
    prob, gp, S, lam = pc.oracle_side(spec)

    def halve(**args):
        if args['iteration'] == 1:
            args['optimized_pulses'][0] *= 0.5

    def edit(it, pulses):
        if it == 1:
            pulses[0] *= 0.5
            return [0]
        return []

    res = _device_run(spec, [TANH, TANH], 3, modify_params_after_iter=halve)
    _assert_matches(res, pc.optimize(prob, gp, S, lam, ko.chis_re, 3, [TANH, TANH], edit=edit))
    whole = _device_run(spec, [TANH, TANH], 4)
    rest = _device_run(spec, [TANH, TANH], 4, continue_from=_device_run(spec, [TANH, TANH], 2))
    assert np.abs(np.array(rest.all_pulses) - np.array(whole.all_pulses)).max() < TOL
    objectives, pulse_options = pc.product_side(spec, [TANH, TANH])
    batch = krotov_amd.optimize_pulses_batch(
        [dict(objectives=objectives, pulse_options=pulse_options, tlist=spec.tlist)] * 2,
        propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_re, iter_stop=4,
        store_all_pulses=True)
    for r in batch:
        assert np.array_equal(np.array(r.all_pulses), np.array(whole.all_pulses))


@pytest.mark.gpu
def test_lindblad_form_with_a_parametrization_runs_the_liouvillian(caplog):
    from test_lindblad_form import _oracle_of, _small_problem

    from krotov_amd import mixed
    from krotov_amd.engine import LAST_ENGINE

    ls = _small_problem(4, 3, 21, 2)
    kind = ('tanh', -0.6, 0.7)
    objectives, pulse_options = ls.objectives(krotov_amd)
    for c in ls.controls:
        pulse_options[c]['parametrization'] = pc.to_product(kind)
    kw = dict(chi_constructor=krotov_amd.functionals.chis_re, iter_stop=3, store_all_pulses=True)
    caplog.set_level(logging.INFO, logger='krotov')
    res = krotov_amd.optimize_pulses(objectives, pulse_options, ls.tlist, propagator=krotov_amd.propagators.LindbladExpm(), **kw)
    assert 'Liouvillian fallback' in caplog.text and 'parametrization' in caplog.text
    assert not LAST_ENGINE().kernel.startswith('lindblad')
    other = krotov_amd.optimize_pulses(mixed.LindbladLayout.liouvillian_objectives(objectives), pulse_options, ls.tlist,
                                       propagator=krotov_amd.propagators.HipExpm(), **kw)
    assert np.array_equal(np.array(res.all_pulses), np.array(other.all_pulses))
    prob, gp, S = _oracle_of(ls)
    ref = pc.optimize(prob, gp, S, [ls.lambda_a], ko.chis_re, 3, [kind])
    assert np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() < 1e-11
    assert np.abs(np.array(res.tau_vals) - ref['tau_vals']).max() < 1e-11
