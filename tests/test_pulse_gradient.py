"""The exact gradient of J_T for the pulse values: the NumPy / SciPy restatement (tests/gradient_cases.py) against central
differences of the oracle's J_T, and ``kh_pulse_gradient`` (krotov_amd/csrc/kh_grad.h) / ``krotov_amd.PulseGradient``
against the restatement.

Host tests first (``-m "not gpu"``): they test the restatement itself, the degree rule of the kernel's series and what
is refused without a device.  Every GPU test compares the device with the restatement at the sweeps' tolerances times
max(1, max |g|).
"""
import ctypes
import math

import numpy as np
import pytest
import scipy.linalg

import krotov_amd
from krotov_amd import _lib, configs
from krotov_amd.nonlinear import Power
from krotov_amd.propagators import expm
from oracle import krotov_oracle as ko

import gradient_cases as gc
import helpers
from test_absent_controls import TOL_HILBERT, TOL_LIOUVILLE

CHUNK = 64  # KH_GRAD_CHUNK of krotov_amd/csrc/kh_grad.h: intervals per workgroup
STEPS = (1e-3, 5e-4, 2.5e-4)


def _tol(spec):
    return TOL_LIOUVILLE if spec.is_super else TOL_HILBERT


def _script_spec(is_super, chi):
    """The inputs the formula was first checked on: K = 3, N = 5, L = 2, nt = 9, non-uniform dt in [0.05, 0.2], operators
    and pulses of order 1 (not normalised)."""
    return gc.random_spec(K=3, N=5, L=2, nt=9, is_super=is_super, seed=11, theta=None, chi=chi, normalise=False)


# ---------------------------------------------------------------------------------------------------------------------
# host: the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('is_super', [False, True], ids=['hilbert', 'liouville'])
@pytest.mark.parametrize('chi', ['ss', 're'])
def test_restatement_agrees_with_central_differences(is_super, chi):
    spec = _script_spec(is_super, chi)
    prob = helpers.spec_to_oracle(spec)
    g, _ = gc.exact_gradient(prob, spec.pulses, chi)
    errs = []
    for h in STEPS:
        fd = gc.central_differences(lambda p: gc.J_T(prob, p, chi), spec.pulses, h)
        errs.append(np.abs(fd - g).max() / np.abs(g).max())
    print('relative error of the central differences at h = %s: %s' % (STEPS, errs))
    assert errs[0] < 1e-6
    for a, b in zip(errs, errs[1:]):
        assert 3.5 < a / b < 4.5, errs


@pytest.mark.parametrize('is_super', [False, True], ids=['hilbert', 'liouville'])
@pytest.mark.parametrize('chi', ['ss', 're'])
def test_first_order_form_is_not_the_gradient(is_super, chi):
    spec = _script_spec(is_super, chi)
    prob = helpers.spec_to_oracle(spec)
    stores = gc.costates(prob, spec.pulses, chi)
    g, _ = gc.exact_gradient(prob, spec.pulses, chi, stores)
    first = gc.first_order_gradient(prob, spec.pulses, chi, stores)
    dev = np.abs(first - g).max() / np.abs(g).max()
    print('first-order form: relative deviation %.3f' % dev)
    assert dev > 0.05


@pytest.mark.parametrize('theta', [0.5, 1.0])
def test_degree_rule_one_above_the_table(theta):
    """The derivative of the Taylor polynomial of degree m + 1 (m: the table's degree for theta) meets 2^-53 ||E||; the
    one of degree m - 1 does not.  Sharp case: Z = theta 1 commutes with E, L_exp = e^theta E and the polynomial's
    derivative is p'(theta) E, which misses it by ||E|| sum_{i >= degree} theta^i / i! exactly (evaluated in extended
    precision).  Then a random non-normal Z of norm theta against ``expm_frechet``: the truncation bound plus the
    reference's own rounding, 32 eps ||E|| e^theta."""
    tab, coeff = helpers.series_taylor_coefficients()
    _, deg = helpers.series_plan([theta], 1.0, tab)
    m = int(deg[0])
    tol = 2.0 ** -53
    n = 4
    rng = np.random.default_rng(3)
    E = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    E /= np.linalg.norm(E, 2)
    Z = theta * np.eye(n, dtype=np.complex128)
    exact = np.exp(np.longdouble(theta)) * E.astype(np.clongdouble)

    def miss(degree):
        return float(np.linalg.norm((gc.frechet_of_polynomial(coeff[degree][:degree + 1], Z, E) - exact).astype(np.complex128), 2))

    print('theta %.1f: table degree %d; derivative misses L_exp by %.3e (m + 1), %.3e (m), %.3e (m - 1); tol %.3e' % (
        theta, m, miss(m + 1), miss(m), miss(m - 1), tol))
    assert miss(m + 1) <= tol
    assert miss(m - 1) > tol
    G = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    Zr = theta * G / np.linalg.norm(G, 2)
    ref = scipy.linalg.expm_frechet(Zr, E, compute_expm=False)
    got = gc.frechet_of_polynomial(coeff[m + 1][:m + 2], Zr, E).astype(np.complex128)
    assert np.linalg.norm(got - ref, 2) <= tol + 32 * np.finfo(float).eps * math.exp(theta)


def _power_problem(seed=5, K=2, N=4, nt=6):
    """H = H0 + eps H1 + eps^2 H2 as a two-term oracle problem; returns (spec with L = 2 term operators, eps)."""
    spec = gc.random_spec(K=K, N=N, L=2, nt=nt, seed=seed, theta=0.6)
    return spec, np.array(spec.pulses[0])


def test_chain_rule_of_a_power_term_against_central_differences():
    spec, eps = _power_problem()
    prob = helpers.spec_to_oracle(spec)
    terms = lambda e: [e, e * e]
    g, _ = gc.exact_gradient(prob, terms(eps), 'ss')
    chain = g[0] + 2.0 * eps * g[1]
    errs = []
    for h in STEPS:
        fd = gc.central_differences(lambda p: gc.J_T(prob, terms(p[0]), 'ss'), [eps], h)[0]
        errs.append(np.abs(fd - chain).max() / np.abs(chain).max())
    print('Power(eps, 2): relative error of the central differences %s' % errs)
    assert errs[0] < 1e-6
    for a, b in zip(errs, errs[1:]):
        assert 3.5 < a / b < 4.5, errs


# ---------------------------------------------------------------------------------------------------------------------
# host: refusals, symbols, instantiations
# ---------------------------------------------------------------------------------------------------------------------
def _objectives(spec, controls=None):
    spec.controls = controls or [lambda t, args, l=l: 0.3 + 0.1 * l for l in range(spec.L)]
    spec.update_shape = lambda t: 1.0
    return configs.spec_to_objectives(spec, krotov_amd)


def test_pulse_gradient_refuses_what_it_cannot_differentiate_without_a_device():
    from krotov_amd import functionals as F

    assert 'PulseGradient' in krotov_amd.__all__
    spec = gc.random_spec(K=2, N=4, L=1, nt=5)
    objs, opts = _objectives(spec)
    kw = dict(chi_constructor=F.chis_ss)

    def own_propagator(H, state, dt, c_ops=None, backwards=False, initialize=False):
        return state

    with pytest.raises(NotImplementedError, match='propagator'):
        krotov_amd.PulseGradient(objs, opts, spec.tlist, propagator=own_propagator, **kw)
    with pytest.raises(NotImplementedError, match='process_group'):
        krotov_amd.PulseGradient(objs, opts, spec.tlist, propagator=expm, process_group=object(), **kw)
    lind = [krotov_amd.Objective(initial_state=o.initial_state, target=o.target, H=o.H, c_ops=[np.eye(4)]) for o in objs]
    with pytest.raises(NotImplementedError, match='c_ops'):
        krotov_amd.PulseGradient(lind, opts, spec.tlist, propagator=expm, **kw)
    other = gc.random_spec(K=1, N=6, L=1, nt=5)
    other.controls = spec.controls
    mixed = objs + configs.spec_to_objectives(other, krotov_amd)[0]
    with pytest.raises(NotImplementedError, match='one dimension'):
        krotov_amd.PulseGradient(mixed, opts, spec.tlist, propagator=expm, **kw)
    big = gc.random_spec(K=1, N=97, L=1, nt=3, theta=None)
    with pytest.raises(NotImplementedError, match='N <= 96'):
        krotov_amd.PulseGradient(*_objectives(big), big.tlist, propagator=expm, **kw)
    five = gc.random_spec(K=1, N=4, L=5, nt=3)
    with pytest.raises(NotImplementedError, match='at most 4'):
        krotov_amd.PulseGradient(*_objectives(five), five.tlist, propagator=expm, **kw)

    class Sine(krotov_amd.ControlFunction):  # (power None: no integer power)
        def value(self, eps):
            return np.sin(eps)

        def derivative(self, eps):
            return np.cos(eps)

    o = objs[0]
    nl = [krotov_amd.Objective(initial_state=o.initial_state, target=o.target, H=[o.H[0], [o.H[1][0], Sine(spec.controls[0])]])]
    with pytest.raises(NotImplementedError, match='power None'):
        krotov_amd.PulseGradient(nl, opts, spec.tlist, propagator=expm, **kw)


def test_capi_limits_symbols_and_instantiations_without_a_device():
    lib = _lib.load()
    assert 'kh_pulse_gradient' in _lib.SYMBOLS and 'kh_pulse_gradient_limits' in _lib.SYMBOLS
    assert lib.kh_pulse_gradient(None, None, None, None, None, None, None, None) == _lib.KH_ERR_INVALID
    assert lib.kh_pulse_gradient_limits(None) == _lib.KH_ERR_INVALID

    def limits(K, N, L, nt):
        pr = _lib.kh_problem()
        pr.K, pr.N, pr.L, pr.nt = K, N, L, nt
        return lib.kh_pulse_gradient_limits(ctypes.byref(pr)), lib.kh_last_error().decode()

    assert limits(3, 96, 4, 9)[0] == _lib.KH_OK and limits(3, 1, 1, 2)[0] == _lib.KH_OK
    rc, text = limits(3, 5, 0, 9)
    assert rc == _lib.KH_ERR_INVALID and 'L = 0' in text
    rc, text = limits(3, 97, 1, 9)
    assert rc == _lib.KH_ERR_UNSUPPORTED and 'N <= 96' in text
    rc, text = limits(3, 5, 5, 9)
    assert rc == _lib.KH_ERR_UNSUPPORTED and 'L <= 4' in text
    names = _lib.kernel_instantiations()
    for L in (1, 2, 3, 4):
        for rows in (1, 2):
            assert 'kh_grad_items<%d, %d>' % (L, rows) in names
    assert 'kh_grad_reduce' in names
    assert len([n for n in names if n.startswith('kh_grad')]) == 9


# ---------------------------------------------------------------------------------------------------------------------
# GPU: kh_pulse_gradient against the restatement
# ---------------------------------------------------------------------------------------------------------------------
_REFERENCE = {}


def reference(key, spec, pulses=None, chi=None):
    """(grad, per_objective, stores) of the restatement, computed once per key and left unchanged."""
    if key not in _REFERENCE:
        prob = helpers.spec_to_oracle(spec)
        pulses = spec.pulses if pulses is None else pulses
        stores = gc.costates(prob, pulses, chi or spec.chi)
        g, per = gc.exact_gradient(prob, pulses, chi or spec.chi, stores)
        for x in (g, per) + tuple(stores):
            x.setflags(write=False)
        _REFERENCE[key] = (g, per, stores)
    return _REFERENCE[key]


def device_gradient(spec, stores, pulses=None, norms=True, engine=None, engine_class=None):
    """(grad, per_objective, engine) of ``kh_pulse_gradient`` on the engine's own forward and backward stores under
    ``pulses``, from the restatement's boundary co-states."""
    import torch
    from krotov_amd.engine import HipKrotovEngine

    _, _, chi_hat, chi_norms = stores
    pulses = np.array(spec.pulses if pulses is None else pulses, dtype=np.float64)
    eng = engine or (engine_class or HipKrotovEngine)(gc.engine_ops(spec), np.diff(spec.tlist), is_super=spec.is_super)
    _, fw = eng.forward(pulses, spec.init, store=True)
    chi = eng.backward(np.array(chi_hat[:, -1]), pulses)  # (copies: the shared reference is read-only)
    per = torch.full((spec.K, spec.L, len(spec.tlist) - 1), float('nan'), dtype=torch.float64, device=eng.device)
    g = eng.pulse_gradient(fw, chi, np.array(chi_norms) if norms else None, pulses, per_objective=per)
    torch.cuda.synchronize()
    return g.cpu().numpy(), per.cpu().numpy(), eng


def check(spec, g, per, ref_g, ref_per, what=''):
    bound = _tol(spec) * max(1.0, np.abs(ref_g).max())
    err, err_per = np.abs(g - ref_g).max(), np.abs(per - ref_per).max()
    print('%s kh_pulse_gradient: max |g| %.3e, error %.3e (per objective %.3e), bound %.1e' % (
        what, np.abs(ref_g).max(), err, err_per, bound))
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(per))
    assert err <= bound and err_per <= bound


def launched_instantiation(spec):
    return 'kh_grad_items<%d, %d>' % (spec.L, 1 if spec.N <= 64 else 2)


# N = 5 (odd, padded), 16, 17, 64, 96; L = 1, 2, 3, 4; nt = 2, 3, 9; nt - 1 = chunk - 1, chunk, chunk + 1; every
# instantiation kh_grad_items<L, 1> (N <= 64) and <L, 2> (N > 64)
SHAPES = [(5, 1, 2), (5, 2, 3), (5, 4, 9), (16, 1, 9), (16, 2, CHUNK), (17, 1, CHUNK + 1), (17, 4, CHUNK + 2), (17, 3, 9),
          (64, 1, 9), (64, 2, 9), (64, 4, 5), (96, 1, 5), (96, 2, 4), (96, 3, 3), (96, 4, 3),
          # G = 3 row blocks at a multiple of 16 and just above it (the register-operand path, kb < G); G = 5 (N = 65 .. 80:
          # only wave 0 owns a second block, the waves 1 .. 3 skip it)
          (48, 2, 9), (49, 3, 5), (65, 1, 5), (80, 2, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize('N,L,nt', SHAPES, ids=['N%d_L%d_nt%d' % s for s in SHAPES])
def test_shapes_against_the_restatement(N, L, nt):
    spec = gc.random_spec(K=3, N=N, L=L, nt=nt, seed=N + 7 * L + nt, theta=0.7)
    ref_g, ref_per, stores = reference(('shape', N, L, nt), spec)
    _lib.forget_launched_kernels()
    g, per, _ = device_gradient(spec, stores)
    launched = _lib.kernel_instantiations(launched_only=True)
    assert launched_instantiation(spec) in launched and 'kh_grad_reduce' in launched, launched
    check(spec, g, per, ref_g, ref_per, 'N %d L %d nt %d:' % (N, L, nt))


@pytest.mark.gpu
@pytest.mark.parametrize('grid', [2, 3])
def test_more_objectives_than_workgroup_columns(grid, monkeypatch):
    spec = gc.random_spec(K=7, N=5, L=2, nt=9, seed=21, theta=0.7)
    ref_g, ref_per, stores = reference('turns', spec)
    g0, per0, _ = device_gradient(spec, stores)
    monkeypatch.setenv('KH_GRAD_GRID', str(grid))  # (read when the engine is created)
    g, per, _ = device_gradient(spec, stores)
    check(spec, g, per, ref_g, ref_per, 'K 7 on %d workgroup columns:' % grid)
    assert g.tobytes() == g0.tobytes() and per.tobytes() == per0.tobytes()  # the result does not depend on the grid


def _regime(name):
    base = gc.random_spec(K=3, N=17, L=2, nt=13, seed=31, theta=0.5, dt_spread=False)
    if name == 'tiny':
        return helpers.regime_tiny(base)
    if name == 'half':
        return base
    if name == 'ramp':  # degree changes inside the grid, up to three sub-steps
        return helpers.regime_ramp(base, 1.0)
    if name == 'three':
        return gc.random_spec(K=3, N=17, L=2, nt=13, seed=31, theta=2.9, dt_spread=False)  # (not on a boundary of ceil)
    if name == 'zero':
        base.pulses = [np.zeros_like(p) for p in base.pulses]
        return base
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny', 'half', 'ramp', 'three', 'zero'])
def test_series_regimes(name):
    spec = _regime(name)
    theta = helpers.theta_sequence(spec)
    tab = helpers.series_degree_tables()['taylor']
    nsub, deg = helpers.series_plan(theta.max(axis=0), 1.0, tab)
    # host witness: the problem is in its regime ...
    if name == 'tiny':
        assert theta.max() < 2e-7 and deg.max() <= 4
    if name in ('half', 'zero'):
        assert nsub.max() == 1 and (name == 'zero' or abs(theta.max() - 0.5) < 1e-12)
    if name == 'ramp':
        assert len(set(deg.tolist())) >= 4 and nsub.max() >= 3 and nsub.min() == 1
    if name == 'three':
        assert nsub.max() == 3 and abs(theta.max() - 2.9) < 1e-9
    ref_g, ref_per, stores = reference(('regime', name), spec)
    # ... and a kernel without the derivative series (the first-order form) cannot pass
    if name != 'tiny':
        prob = helpers.spec_to_oracle(spec)
        first = gc.first_order_gradient(prob, spec.pulses, spec.chi, stores)
        assert np.abs(first - ref_g).max() > 1e3 * _tol(spec) * max(1.0, np.abs(ref_g).max())
    g, per, _ = device_gradient(spec, stores)
    check(spec, g, per, ref_g, ref_per, 'regime %s (theta <= %.3g, sub-steps <= %d, degrees %d..%d):' % (
        name, theta.max(), nsub.max(), deg.min(), deg.max()))


@pytest.mark.gpu
def test_a_control_absent_from_one_objective():
    spec = gc.random_spec(K=3, N=17, L=2, nt=9, seed=41, theta=0.7)
    spec.Hc[1][0] = None
    ref_g, ref_per, stores = reference('absent', spec)
    assert np.all(ref_per[1, 0] == 0.0) and np.abs(ref_per[1, 1]).max() > 0
    g, per, _ = device_gradient(spec, stores)
    check(spec, g, per, ref_g, ref_per, 'absent control:')
    assert per[1, 0].tobytes() == np.zeros_like(per[1, 0]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['lower', 'ladder'])
def test_controls_that_are_not_self_adjoint(kind):
    spec = gc.random_spec(K=3, N=33, L=2, nt=7, seed=51, theta=0.7)
    rng = np.random.default_rng(52)
    spec.Hc = [[helpers.nonselfadjoint_variant(kind, h, rng) for h in row] for row in spec.Hc]
    for row in spec.Hc:
        assert all(not np.allclose(h, h.conj().T) for h in row)
    ref_g, ref_per, stores = reference(('nsa', kind), spec)
    g, per, _ = device_gradient(spec, stores)
    check(spec, g, per, ref_g, ref_per, 'non-self-adjoint controls (%s):' % kind)


@pytest.mark.gpu
@pytest.mark.parametrize('N,L', [(16, 1), (25, 2), (81, 1)])
def test_a_random_dense_liouvillian(N, L):
    spec = gc.random_spec(K=3, N=N, L=L, nt=6, is_super=True, seed=61 + N, theta=0.8, chi='re')
    ref_g, ref_per, stores = reference(('super', N, L), spec)
    g, per, _ = device_gradient(spec, stores)
    check(spec, g, per, ref_g, ref_per, 'Liouvillian N %d L %d:' % (N, L))


@pytest.mark.gpu
def test_chi_norms_given_and_null():
    spec = gc.random_spec(K=3, N=16, L=2, nt=9, seed=71, theta=0.7, chi='ss')
    ref_g, ref_per, stores = reference('norms', spec)
    norms = stores[3]
    assert np.all(np.abs(norms - 1.0) > 0.1)
    g, per, eng = device_gradient(spec, stores)
    check(spec, g, per, ref_g, ref_per, 'norms given:')
    g1, per1, _ = device_gradient(spec, stores, norms=False, engine=eng)
    unit = ref_per / norms[:, None, None]
    check(spec, g1, per1, unit.sum(axis=0), unit, 'norms NULL:')


FAMILIES = [('q2', {}, dict(N=64, L=1)), ('tile512', {'KH_KERNEL': 'tile512'}, dict(N=33, L=1)),
            ('mini', {}, dict(N=16, L=1)), ('generic', {'KH_KERNEL': 'generic'}, dict(N=33, L=1))]


@pytest.mark.gpu
@pytest.mark.parametrize('family,env,shape', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_the_sweep_family_does_not_matter(family, env, shape, monkeypatch):
    spec = gc.random_spec(K=3, nt=9, seed=81, theta=0.7, **shape)
    ref_g, ref_per, stores = reference(('family', shape['N']), spec)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    g, per, eng = device_gradient(spec, stores)
    print('family %s: engine kernel %s' % (family, eng.kernel))
    assert {'q2': 'q2', 'tile512': 'tile64/', 'mini': 'mini', 'generic': 'generic'}[family] in eng.kernel
    check(spec, g, per, ref_g, ref_per, 'family %s:' % family)


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal_and_the_rows_sum_in_order():
    spec = gc.random_spec(K=5, N=17, L=2, nt=CHUNK + 3, seed=91, theta=0.7)
    ref_g, ref_per, stores = reference('repeat', spec)
    g, per, eng = device_gradient(spec, stores)
    g2, per2, _ = device_gradient(spec, stores, engine=eng)
    g3, per3, _ = device_gradient(spec, stores)  # a fresh engine
    check(spec, g, per, ref_g, ref_per, 'repeatability:')
    assert g.tobytes() == g2.tobytes() == g3.tobytes() and per.tobytes() == per2.tobytes() == per3.tobytes()
    acc = np.zeros_like(g)
    for k in range(spec.K):
        acc = acc + per[k]
    assert acc.tobytes() == g.tobytes()


@pytest.mark.gpu
def test_memory_contract_on_guarded_arenas():
    import torch
    from guarded import GuardedEngine

    spec = gc.random_spec(K=3, N=17, L=2, nt=CHUNK + 2, seed=101, theta=0.7)
    ref_g, ref_per, stores = reference('guarded', spec)
    K, N, L, nt = spec.K, spec.N, spec.L, len(spec.tlist)
    eng = GuardedEngine(gc.engine_ops(spec), np.diff(spec.tlist), is_super=spec.is_super)
    arena = eng.arena
    c128, f64 = torch.complex128, torch.float64
    t = {name: arena.carve(name, shape, dtype, role) for name, shape, dtype, role in (
        ('init', (K, N), c128, 'input'), ('chi_T', (K, N), c128, 'input'), ('pulses', (L, nt - 1), f64, 'input'),
        ('norms', (K,), f64, 'input'), ('psi_T', (K, N), c128, 'output'), ('fw', (K, nt, N), c128, 'output'),
        ('chi', (K, nt, N), c128, 'output'), ('grad', (L, nt - 1), f64, 'output'), ('per', (K, L, nt - 1), f64, 'output'))}
    arena.check_layout()
    t['init'].copy_(torch.from_numpy(spec.init))
    t['chi_T'].copy_(torch.from_numpy(np.ascontiguousarray(stores[2][:, -1])))
    t['pulses'].copy_(torch.from_numpy(np.array(spec.pulses)))
    t['norms'].copy_(torch.from_numpy(stores[3]))
    arena.snapshot()
    eng.forward(t['pulses'], t['init'], store=True, out=(t['psi_T'], t['fw']))
    torch.cuda.synchronize()
    arena.verify('forward', (t['psi_T'], t['fw']))
    eng.backward(t['chi_T'], t['pulses'], out=t['chi'])
    torch.cuda.synchronize()
    arena.verify('backward', (t['chi'],))
    eng.pulse_gradient(t['fw'], t['chi'], t['norms'], t['pulses'], out=t['grad'], per_objective=t['per'])
    torch.cuda.synchronize()
    arena.verify('pulse_gradient', (t['grad'], t['per']))  # guard bands and inputs bytewise unchanged
    check(spec, t['grad'].cpu().numpy(), t['per'].cpu().numpy(), ref_g, ref_per, 'guarded arena:')
    eng.pulse_gradient(t['fw'], t['chi'], None, t['pulses'], out=t['grad'])  # (the library's own workspace)
    torch.cuda.synchronize()
    arena.verify('pulse_gradient, workspace', (t['grad'],))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: PulseGradient end to end
# ---------------------------------------------------------------------------------------------------------------------
def _small_config():
    spec = configs.config_c5(K=3, N=6, nt=12, L=2, distinct=True, T=1.1)
    spec.chi = 'ss'
    return spec


def _pulse_gradient(spec, chi='ss'):
    from krotov_amd import functionals as F

    objs, opts = configs.spec_to_objectives(spec, krotov_amd)
    return krotov_amd.PulseGradient(objs, opts, spec.tlist, propagator=expm, chi_constructor=getattr(F, 'chis_' + chi),
                                    J_T=getattr(F, 'J_T_' + chi))


@pytest.mark.gpu
def test_pulse_gradient_end_to_end():
    spec = _small_config()
    prob = helpers.spec_to_oracle(spec)
    guess, _, _ = helpers.oracle_controls(spec)
    pg = _pulse_gradient(spec)
    res = pg()
    ref_g, _ = gc.exact_gradient(prob, guess, 'ss')
    bound = TOL_HILBERT * max(1.0, np.abs(ref_g).max())
    g = np.array(res.gradient)
    print('PulseGradient: max |g| %.3e, error %.3e, J_T %.6f' % (np.abs(ref_g).max(), np.abs(g - ref_g).max(), res.J_T))
    assert np.abs(g - ref_g).max() <= bound
    assert abs(res.J_T - gc.J_T(prob, guess, 'ss')) <= bound
    assert np.abs(np.asarray(res.tau_vals) - ko.tau_vals(prob, ko.forward_propagation(prob, guess))).max() <= bound
    # g . v against central differences of the device's own J_T
    rng = np.random.default_rng(7)
    v = [rng.standard_normal(len(p)) for p in guess]
    gv = sum(float(np.dot(a, b)) for a, b in zip(res.gradient, v))
    errs = []
    for h in STEPS[:2]:
        up = pg([p + h * d for p, d in zip(guess, v)]).J_T
        dn = pg([p - h * d for p, d in zip(guess, v)]).J_T
        errs.append(abs((up - dn) / (2 * h) - gv))
    print('g.v %.6e, central differences miss it by %s' % (gv, errs))
    assert 3.5 < errs[0] / errs[1] < 4.5
    # a reused object with changed pulses equals a fresh one, bit for bit
    other = [p + 0.05 * d for p, d in zip(guess, v)]
    again, fresh = pg(other), _pulse_gradient(spec)(other)
    assert np.array(again.gradient).tobytes() == np.array(fresh.gradient).tobytes()
    # the flat form L-BFGS-B takes
    J, flat = pg.value_and_gradient(np.concatenate(other))
    assert J == again.J_T and flat.tobytes() == np.concatenate(again.gradient).tobytes()


@pytest.mark.gpu
def test_pulse_gradient_of_a_power_problem():
    from krotov_amd import functionals as F

    spec, eps = _power_problem()
    prob = helpers.spec_to_oracle(spec)
    T = spec.tlist[-1]
    mid = 0.5 * (spec.tlist[1:] + spec.tlist[:-1])
    control = lambda t, args: float(np.interp(t, mid, eps))
    objs = [krotov_amd.Objective(initial_state=spec.init[k], target=spec.target[k],
                                 H=[spec.H0[k], [spec.Hc[k][0], control], [spec.Hc[k][1], Power(control, 2)]])
            for k in range(spec.K)]
    opts = {control: dict(lambda_a=1.0, update_shape=lambda t: 1.0)}
    pg = krotov_amd.PulseGradient(objs, opts, spec.tlist, propagator=expm, chi_constructor=F.chis_ss, J_T=F.J_T_ss)
    res = pg([eps])
    g, _ = gc.exact_gradient(prob, [eps, eps * eps], 'ss')
    chain = g[0] + 2.0 * eps * g[1]
    bound = TOL_HILBERT * max(1.0, np.abs(chain).max())
    print('Power problem: max |g| %.3e, error %.3e' % (np.abs(chain).max(), np.abs(res.gradient[0] - chain).max()))
    assert len(res.gradient) == 1 and np.abs(res.gradient[0] - chain).max() <= bound
    assert T > 0
