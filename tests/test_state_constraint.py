"""State-dependent constraints: a running cost g_b(phi(t)) as a source term in the backward sweep
(``optimize_pulses(state_dependent_constraint=...)``, ``kh_backward_store_source``, ``kh_apply_store``).

Yardstick: tests/constraint_cases.py -- the recursion chi[n] = V_n (chi[n+1] + h_n W[n+1]) + h_n W[n] restated in NumPy on
the oracle's own per-interval propagator and update sweep, tied to finite differences of the discrete functional by an
exact identity (tests 2 and 3 below).

Tolerances: the project's 1e-12 relative to max(1, max|.|) for Hilbert-space sweeps, 1e-11 on Liouvillians; the identity
is checked to 10 x |FD(h) - FD(h/2)|, the central difference's own error estimate; ``kh_apply_store`` to the rounding
bound of an N-term complex dot product.

``kh_apply_store`` at nt = 1: an engine cannot be created with fewer than two time points (``kh_engine_create`` answers
KH_ERR_INVALID, asserted below), and the entry point takes nt from its engine -- the smallest grid it can be called with
is nt = 2, which is what the test runs in that place.
"""
import numpy as np
import pytest

import constraint_cases as cc
import helpers as hp
import parametrization_cases as pc
from helpers import numpy_plugins
from oracle import krotov_oracle as ko

import krotov_amd
from krotov_amd.constraints import QuadraticStateConstraint, StateDependentConstraint

TOL = 1e-12
LAMBDA_B = -1.5
GEN = 'kh_gen_sweep_store_src<false>'
APPLY = 'kh_gen_apply_store'


def TILE(L):
    return 'kh_tile_sweep_store_src<1, %d>' % L


# ---------------------------------------------------------------------------
# host: the yardstick itself
# ---------------------------------------------------------------------------
def _identity_problem():
    spec = cc.nonuniform(pc.problem(K=2, N=4, L=2, nt=6), [1.0, 0.6, 1.4, 0.8, 1.2])
    prob, gp, S, lam = pc.oracle_side(spec)
    assert np.ptp(np.diff(prob.tlist)) > 0.1 * np.diff(prob.tlist).mean()
    # guess pulses that are non-zero on every interval (the fixture's vanish at the ends of the grid)
    gp = [np.array(p) + 0.15 * (1 + l) * np.cos(1.3 * np.arange(len(p)) + l) for l, p in enumerate(gp)]
    D = [cc.random_hermitian(4, 21, 1.0), cc.random_hermitian(4, 22, 0.7)]
    shape = lambda t: 0.5 + t / prob.tlist[-1]  # noqa: E731
    return prob, gp, D, shape


def test_zero_source_is_the_oracles_backward_sweep():
    """(1) The restated sweep with W = 0 is ``oracle.backward_sweep``, bit for bit."""
    prob, gp, D, shape = _identity_problem()
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    W = np.zeros((prob.K, len(prob.tlist), prob.N), dtype=np.complex128)
    for norms in (None, np.array([0.3, 1.7])):
        assert cc.backward_sweep(prob, chi_T, gp, W, norms).tobytes() == ko.backward_sweep(prob, chi_T, gp).tobytes()


_fd = {}


def _finite_differences(chi_name):
    """FD(h), FD(h/2) of J_d for every (l, n), computed once per functional."""
    if chi_name not in _fd:
        prob, gp, D, shape = _identity_problem()
        h = 1e-3
        _fd[chi_name] = (cc.central_differences(chi_name, prob, gp, D, LAMBDA_B, h, shape),
                         cc.central_differences(chi_name, prob, gp, D, LAMBDA_B, 0.5 * h, shape))
    return _fd[chi_name]


@pytest.mark.parametrize('chi_name', ['re', 'ss'])
def test_discrete_identity(chi_name):
    """(2) d J_d / d eps_l[n] = -2 Re <lt_{n+1}| (d U_n / d eps_l) phi_n> for every (l, n): N = 4, K = 2, L = 2, nt = 6,
    non-uniform dt, against central differences at h and h / 2; tolerance 10 |FD(h) - FD(h/2)|."""
    prob, gp, D, shape = _identity_problem()
    fd_h, fd_h2 = _finite_differences(chi_name)
    grad = cc.identity_gradient(chi_name, prob, gp, D, LAMBDA_B, shape)
    tol = 10.0 * np.abs(fd_h - fd_h2)
    print("max |grad - FD(h/2)| = %.3e, tolerances %.3e .. %.3e, max |grad| = %.3e" % (
        np.abs(grad - fd_h2).max(), tol.min(), tol.max(), np.abs(grad).max()))
    assert tol.max() < 1e-5 and np.abs(grad).max() > 1e-3  # (the estimate is small against what is measured)
    assert np.all(np.abs(grad - fd_h2) <= tol)
    # the source matters here: without it the identity fails
    without = cc.identity_gradient(chi_name, prob, gp, D, 0.0, shape)
    assert np.any(np.abs(without - fd_h2) > 100 * tol)


@pytest.mark.parametrize('variant', ['flip', 'full', 'substep'])
@pytest.mark.parametrize('chi_name', ['re', 'ss'])
def test_wrong_recursions_violate_the_identity(chi_name, variant):
    """(3) A flipped sign of W, a full instead of a half weight at n, a source added per sub-step: each misses (2) by more
    than its tolerance."""
    prob, gp, D, shape = _identity_problem()
    fd_h, fd_h2 = _finite_differences(chi_name)
    grad = cc.identity_gradient(chi_name, prob, gp, D, LAMBDA_B, shape, variant=variant)
    excess = np.abs(grad - fd_h2) / (10.0 * np.abs(fd_h - fd_h2))
    print("%s: |grad - FD| / tolerance up to %.3e" % (variant, excess.max()))
    assert excess.max() > 100.0


# ---------------------------------------------------------------------------
# host: the classes
# ---------------------------------------------------------------------------
def test_quadratic_constraint_against_the_restatement():
    prob, gp, D, shape = _identity_problem()
    tl = prob.tlist
    _, states = ko.forward_propagation(prob, gp, store=True)
    con = QuadraticStateConstraint(D, LAMBDA_B, shape=shape)
    assert isinstance(con, StateDependentConstraint)
    assert np.array_equal(con.factors(tl), cc.factors(LAMBDA_B, tl, shape))
    assert np.abs(con.source(states, tl) - cc.source(D, cc.factors(LAMBDA_B, tl, shape), states)).max() < 1e-15
    assert abs(con.integral(states, tl) - cc.integral(D, LAMBDA_B, tl, states, shape)) < 1e-15
    # one operator for all objectives, None for an unconstrained one, an array shape, column states
    one = QuadraticStateConstraint(D[0], LAMBDA_B, shape=cc.shape_values(shape, tl))
    assert np.abs(one.source(states, tl) - cc.source(D[0], cc.factors(LAMBDA_B, tl, shape), states)).max() < 1e-15
    ops = one.operators([None, None])
    assert ops[0] is ops[1]
    part = QuadraticStateConstraint([None, D[1]], LAMBDA_B)
    assert np.all(part.source(states, tl)[0] == 0.0)
    assert abs(part.integral(states, tl) - cc.integral([None, D[1]], LAMBDA_B, tl, states)) < 1e-15
    cols = [[s.reshape(-1, 1) for s in states[k]] for k in range(prob.K)]
    assert np.array_equal(con.source(cols, tl), con.source(states, tl))
    with pytest.raises(ValueError):
        QuadraticStateConstraint(np.ones((3, 4)), 1.0)
    with pytest.raises(ValueError):
        QuadraticStateConstraint([D[0]], 1.0).operators([None, None])
    assert np.abs(krotov_amd.constraints.trapezoid_weights(tl) - cc.trapezoid_weights(tl)).max() < 1e-16


# ---------------------------------------------------------------------------
# host: optimize_pulses through the plugin path
# ---------------------------------------------------------------------------
class _ConstSigma(krotov_amd.second_order.Sigma):
    def __init__(self, value):
        self.value = value

    def __call__(self, t):
        return self.value

    def refresh(self, **kwargs):
        pass


def _run(spec, constraint, iters, kinds=None, device=False, sigma=None, hook=None, **kw):
    objectives, pulse_options = pc.product_side(spec, kinds)
    record = dict(g_a=[], g_b=[], kept=[])

    def info_hook(**args):
        record['g_a'].append(np.array(args['g_a_integrals']))
        record['kept'].append((args['forward_states'] is not None, args['forward_states0'] is not None))
        if constraint is not None and args['forward_states'] is not None:
            record['g_b'].append(constraint.integral(args['forward_states'], spec.tlist))
        if hook is not None:
            hook(**args)

    if device:
        plugins = dict(propagator=krotov_amd.propagators.expm)
    else:
        prop, mu, overlap = numpy_plugins()
        plugins = dict(propagator=prop, mu=mu, overlap=overlap, norm=np.linalg.norm)
    if constraint is not None:
        kw['state_dependent_constraint'] = constraint
    res = krotov_amd.optimize_pulses(
        objectives, pulse_options, spec.tlist, chi_constructor=krotov_amd.functionals.chis_re, iter_stop=iters,
        store_all_pulses=True, info_hook=info_hook, sigma=None if sigma is None else _ConstSigma(sigma), **plugins, **kw)
    res.g_a, res.g_b, res.kept = np.array(record['g_a']), np.array(record['g_b']), record['kept']
    return res


def _assert_matches(res, ref, tol=TOL):
    scale = max(1.0, np.abs(ref['all_pulses']).max())
    got = np.array(res.all_pulses)
    assert got.shape == ref['all_pulses'].shape
    d = dict(pulse=np.abs(got - ref['all_pulses']).max(), tau=np.abs(np.array(res.tau_vals) - ref['tau_vals']).max(),
             g_a=np.abs(res.g_a - ref['g_a']).max(), g_b=np.abs(res.g_b - ref['g_b']).max())
    print(' '.join('%s %.2e' % kv for kv in sorted(d.items())))
    assert d['pulse'] < tol * scale
    assert d['tau'] < tol
    assert d['g_a'] < tol * max(1.0, np.abs(ref['g_a']).max())
    assert d['g_b'] < tol * max(1.0, np.abs(ref['g_b']).max())


def _constraint_of(spec, per_objective=True):
    """D: the projector onto the first N // 2 + 1 basis states -- for all objectives, or per objective with one left
    unconstrained and the others sharing one array."""
    P = cc.projector(spec.N, spec.N // 2 + 1)
    if not per_objective:
        return P
    return [P if k != 1 else None for k in range(spec.K)] if spec.K > 2 else [P, cc.projector(spec.N, 2)]


@pytest.mark.parametrize('case', ['first_order', 'sigma', 'shape_nonuniform'])
def test_plugin_path_matches_the_restatement(case):
    """(4) ``optimize_pulses(state_dependent_constraint=...)`` through the host loop with the NumPy propagator, three
    iterations, against the restatement; tolerance of tests/test_parametrization.py's host-loop comparison (1e-12)."""
    spec = pc.problem()
    shape = None
    if case == 'shape_nonuniform':
        spec = cc.nonuniform(spec, [1.0, 0.7, 1.3])
        shape = lambda t: 0.25 + 0.5 * t  # noqa: E731
    prob, gp, S, lam = pc.oracle_side(spec)
    D = _constraint_of(spec)
    sigma = -1.5 if case == 'sigma' else None
    ref = cc.optimize(prob, gp, S, lam, ko.chis_re, 3, D, LAMBDA_B, shape=shape, sigma=sigma)
    res = _run(spec, QuadraticStateConstraint(D, LAMBDA_B, shape=shape), 3, sigma=sigma)
    _assert_matches(res, ref)
    assert all(kept == (True, True) for kept in res.kept)  # forward_states / forward_states0 as in second-order runs
    # the constraint moves the pulses by far more than the tolerance
    free = ko.optimize(prob, gp, S, lam, ko.chis_re, 3, norm=cc.NORM) if sigma is None else None
    if free is not None:
        assert np.abs(free['all_pulses'] - ref['all_pulses']).max() > 1e-4


def test_plugin_path_with_a_parametrization_and_a_source_of_ones_own():
    spec = pc.problem()
    prob, gp, S, lam = pc.oracle_side(spec)
    D = _constraint_of(spec)
    kinds = [('tanh',) + pc.BOUNDS, None]
    ref = cc.optimize(prob, gp, S, lam, ko.chis_re, 3, D, LAMBDA_B, kinds=kinds)

    class Mine(QuadraticStateConstraint):
        calls = 0

        def source(self, forward_states, tlist):
            Mine.calls += 1
            return super().source(forward_states, tlist)

    _assert_matches(_run(spec, Mine(D, LAMBDA_B), 3, kinds=kinds), ref)
    assert Mine.calls == 3


def test_the_case_bites():
    """(5) A three-level Lambda system, D the projector onto the allowed subspace, lambda_b < 0, five iterations: the
    population integral of the forbidden level ends lower than in the unconstrained run, and J_T + int g_b dt falls in
    every iteration."""
    spec, allowed, forbidden = cc.lambda_system()
    lambda_b = -4.0
    con = QuadraticStateConstraint(allowed, lambda_b)
    trajectories = {}

    def keep(name):
        def hook(**args):
            if args['forward_states'] is not None:
                trajectories[name] = np.array([[np.asarray(s).ravel() for s in traj] for traj in args['forward_states']])
        return hook

    res = _run(spec, con, 5, hook=keep('constrained'))
    # (the unconstrained run keeps no trajectories: a zero-weight constraint makes it hand them to the hook)
    free = _run(spec, QuadraticStateConstraint(allowed, 0.0), 5, hook=keep('free'))
    prob, gp, S, lam = pc.oracle_side(spec)
    plain = ko.optimize(prob, gp, S, lam, ko.chis_re, 5, norm=cc.NORM)
    assert np.abs(np.array(free.all_pulses) - plain['all_pulses']).max() < TOL  # lambda_b = 0 is the unconstrained run

    def forbidden_population(states):
        return cc.integral(forbidden, 1.0, spec.tlist, states) * (spec.tlist[-1] - spec.tlist[0])

    pop_c, pop_f = forbidden_population(trajectories['constrained']), forbidden_population(trajectories['free'])
    J = 1.0 - np.real(np.array(res.tau_vals)).mean(axis=1) + res.g_b
    print("int <P_forbidden> dt: constrained %.4f, free %.4f; J_T + int g_b dt: %s" % (pop_c, pop_f, J))
    assert pop_c < 0.9 * pop_f
    assert np.all(np.diff(J) < 0.0)


def test_refusals_come_before_any_engine(monkeypatch):
    """(6) Refused with a clear error, host-only: no engine is created."""
    from krotov_amd import engine

    def no_engine(*args, **kwargs):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(engine.HipKrotovEngine, '__init__', no_engine)
    spec = pc.problem()
    objectives, pulse_options = pc.product_side(spec, None)
    con = QuadraticStateConstraint(cc.projector(spec.N, 3), LAMBDA_B)
    common = dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_re, iter_stop=1)
    with pytest.raises(ValueError, match='process_group'):
        krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, state_dependent_constraint=con,
                                   process_group=object(), **common)
    with pytest.raises(ValueError, match='skip_initial_forward_propagation'):
        krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, state_dependent_constraint=con,
                                   skip_initial_forward_propagation=True, **common)
    with pytest.raises(ValueError, match='StateDependentConstraint'):
        krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, state_dependent_constraint=np.eye(5), **common)
    lossy = [krotov_amd.Objective(initial_state=o.initial_state, target=o.target, H=o.H,
                                  c_ops=[0.1 * np.eye(spec.N, k=1).astype(complex)]) for o in objectives]
    for prop in (krotov_amd.propagators.expm, numpy_plugins()[0]):
        with pytest.raises(NotImplementedError, match='c_ops'):
            krotov_amd.optimize_pulses(lossy, pulse_options, spec.tlist, state_dependent_constraint=con,
                                       **dict(common, propagator=prop))
    small = pc.problem(K=1, N=3, L=2)
    small.controls = spec.controls  # (the same control callables: one pulse_options dict serves both)
    other, _ = pc.product_side(small, None)
    with pytest.raises(ValueError, match='one dimension and kind'):
        krotov_amd.optimize_pulses(objectives + other, pulse_options, spec.tlist, state_dependent_constraint=con, **common)
    # the keyword is keyword-only and None leaves the call as it was
    import inspect

    par = inspect.signature(krotov_amd.optimize_pulses).parameters['state_dependent_constraint']
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    assert 'state_dependent_constraint' not in inspect.signature(krotov_amd.optimize_pulses_batch).parameters


def test_c_abi_declares_and_exports_both_entry_points():
    import os

    from krotov_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'krotov_hip.h')).read()
    lib = _lib.load()
    for name in ('kh_backward_store_source', 'kh_apply_store'):
        assert 'int %s(kh_engine *engine' % name in header
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    contract = header[header.index('Memory contract'):header.index('#ifndef KROTOV_HIP_H')]
    assert 'kh_backward_store_source' in contract and 'kh_apply_store' in contract and 'src_store_dev' in contract
    names = _lib.kernel_instantiations()
    for want in [TILE(L) for L in (1, 2, 3, 4)] + [GEN, APPLY]:
        assert want in names, want
    assert not any(n.startswith('kh_tile_sweep_store_src<2') for n in names)  # (only what can be dispatched)


# ---------------------------------------------------------------------------
# GPU: kh_apply_store
# ---------------------------------------------------------------------------
def _dense_engine(spec, cls=None, **kw):
    from krotov_amd.engine import HipKrotovEngine

    ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    return (cls or HipKrotovEngine)(ops, np.diff(spec.tlist), is_super=spec.is_super, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('nt', [2, 256, 257])
@pytest.mark.parametrize('N', [5, 64, 70])
def test_apply_store_against_numpy(N, nt):
    """(7) out[k][n] = c[n] Op_k in[k][n]: N below, at and above the 16 x 16 blocks' multiples; one workgroup's 256 time
    points and the next one's first (nt = 2: module docstring); a NULL entry gives exact zeros, a shared pointer is
    accepted; with factors and with NULL factors.  Bound: the rounding of an N-term complex dot product and of the
    factor, 4 (N + 2) 2^-53 |c| (|Op| |in|) elementwise."""
    import torch

    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    rng = np.random.default_rng(100 * N + nt)
    K = 3
    ops = [[cc.random_hermitian(N, 7 + k, 1.0), cc.random_hermitian(N, 3, 0.5)] for k in range(K)]
    eng = HipKrotovEngine(ops, np.full(nt - 1, 0.01))
    D = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))  # (any operator: Hermitian or not)
    table = [D, None, D]
    x = rng.standard_normal((K, nt, N)) + 1j * rng.standard_normal((K, nt, N))
    c = rng.standard_normal(nt)
    x_dev = eng.dev(x, torch.complex128)
    for fac in (c, None):
        _lib.forget_launched_kernels()
        out = torch.full((K, nt, N), float('nan'), dtype=torch.complex128, device=eng.device)
        got = eng.apply_store(table, fac, x_dev, out=out).cpu().numpy()
        assert APPLY in _lib.kernel_instantiations(launched_only=True)
        f = np.ones(nt) if fac is None else fac
        ref = cc.source(table, f, x)
        bound = 4 * (N + 2) * 2.0 ** -53 * np.abs(f)[None, :, None] * np.einsum('ij,knj->kni', np.abs(D), np.abs(x))
        print("N %d nt %d: max |d| %.2e, bound up to %.2e" % (N, nt, np.abs(got - ref).max(), bound.max()))
        assert np.all(np.abs(got - ref)[[0, 2]] <= bound[[0, 2]])
        assert np.all(got[1] == 0.0) and not np.signbit(got[1].real).any() and not np.signbit(got[1].imag).any()
    assert np.array_equal(x_dev.cpu().numpy(), x)
    # refusals: a null argument, input == output
    with pytest.raises(_lib.KrotovHipError) as err:
        _lib.check(eng._lib.kh_apply_store(eng._handle, None, None, x_dev.data_ptr(), out.data_ptr(), eng._stream()))
    assert err.value.code == _lib.KH_ERR_INVALID
    with pytest.raises(_lib.KrotovHipError) as err:
        _lib.check(eng._lib.kh_apply_store(eng._handle, eng._apply_table.data_ptr(), None, x_dev.data_ptr(), x_dev.data_ptr(),
                                           eng._stream()))
    assert err.value.code == _lib.KH_ERR_INVALID
    eng.close()


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_an_engine_needs_two_time_points():
    """Why (7) runs nt = 2 in the place of nt = 1."""
    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    ops = [[cc.random_hermitian(5, 1, 1.0), cc.random_hermitian(5, 2, 1.0)]]
    with pytest.raises(_lib.KrotovHipError) as err:
        HipKrotovEngine(ops, np.zeros(0))
    assert err.value.code == _lib.KH_ERR_INVALID


# ---------------------------------------------------------------------------
# GPU: kh_backward_store_source
# ---------------------------------------------------------------------------
# theta_n / theta_max of the regime cases' eight intervals: sub-steps on two of them, five decades of theta
RAMP = (0.01, 0.2, 0.9, 2.3, 0.5, 0.05, 1.2, 0.3)
THETA_MAX = 1.0


def _ramped(spec):
    """``spec`` (nt = 9) on a non-uniform grid on which theta_n of the objective with the largest norms follows RAMP."""
    obj = hp.explicit(spec, 'dense')
    _, rate = hp._largest(obj)
    hp._set_dt(obj, THETA_MAX * np.array(RAMP) / rate)
    return obj


def _shared(K, N, L):
    return hp.explicit(krotov_amd.configs.config_shared(K=K, N=N, nt=9, L=L), 'dense')


def _liouville():
    return hp.explicit(krotov_amd.configs.config_sparse_lindblad(d=9, nt=9, K=3), 'dense')


def _banded():
    return hp.explicit(pc.problem(K=2, N=40, L=2, nt=9, bands=3), 'csr')


def _dense(**kw):
    return hp.explicit(pc.problem(**kw), 'dense')


# name: (builder, expected kernel, engine family or None, engine keyword arguments[, environment])
CASES = {
    # the register-tile form: engines whose plain sweeps are the q2 (mini and quad included) or the 512-thread tile kernels
    'tile_n64_L1': (lambda: _dense(K=3, N=64, L=1, nt=9), TILE(1), 'tile64q2/512', {}),
    'tile_n64_L2': (lambda: _dense(K=3, N=64, L=2, nt=9), TILE(2), 'tile64/512', {}),
    'tile_n64_L3': (lambda: _dense(K=3, N=64, L=3, nt=9), TILE(3), 'tile64/512', {}),
    'tile_n64_L4': (lambda: _dense(K=3, N=64, L=4, nt=9), TILE(4), 'tile64/512', {}),
    'tile_n33': (lambda: _dense(K=3, N=33, L=1, nt=9), TILE(1), 'tile64q2/512', {}),
    'tile_n5_mini': (lambda: _dense(K=3, N=5, L=1, nt=9), TILE(1), 'mini16/wave', {}),
    'tile_n4_quad': (lambda: _dense(K=2, N=4, L=1, nt=9), TILE(1), 'mini4/wave', {}),
    # the tile256 engine (more objectives than compute units): with one control its plain sweeps are the q2 kernel's,
    # so the register-tile form takes it
    'tile_k300_tile256': (lambda: _dense(K=300, N=16, L=1, nt=9), TILE(1), 'tile64/256', {}),
    # the generic form: every other engine the generic kernels hold
    'gen_n70_tile128': (lambda: _dense(K=3, N=70, L=1, nt=9), GEN, 'tile128/512', {}),
    'gen_n100_L6': (lambda: _dense(K=2, N=100, L=6, nt=6), GEN, None, {}),
    'gen_n200_scratch': (lambda: _dense(K=2, N=200, L=1, nt=5), GEN, None, {}),
    'gen_n81_coop': (lambda: _shared(4, 81, 1), GEN, 'coop16/mfma', {}),
    # (more objectives than twice the compute units: the workgroups take objectives in turns)
    'gen_k600_turns': (lambda: _dense(K=600, N=8, L=1, nt=5), GEN, 'generic', {}, {'KH_KERNEL': 'generic'}),
    'gen_csr_n40': (_banded, GEN, '/csr', {}),
    'gen_liouville': (_liouville, GEN, None, {}),
    # regimes (witnessed on the host from the exported planner: test_regime_cases_enter_their_regime)
    'tile_ramp': (lambda: _ramped(pc.problem(K=3, N=64, L=2, nt=9)), TILE(2), 'tile64/512', dict(theta_max=THETA_MAX)),
    'gen_ramp': (lambda: _ramped(pc.problem(K=3, N=70, L=1, nt=9)), GEN, 'tile128/512', dict(theta_max=THETA_MAX)),
    'tile_nt2': (lambda: _dense(K=3, N=64, L=2, nt=2, T=0.3), TILE(2), 'tile64/512', {}),
    'gen_nt2': (lambda: _dense(K=3, N=70, L=1, nt=2, T=0.3), GEN, 'tile128/512', {}),
}
_refs = {}


def _reference(name):
    """The case's problem and its restated sweep, computed once and shared (the tests do not write to it)."""
    if name not in _refs:
        obj = CASES[name][0]()
        prob = hp.spec_to_oracle(obj)
        rng = np.random.default_rng(len(name) + prob.N)
        nt = len(prob.tlist)
        pulses = [np.array(p) + 0.05 * np.cos(1.7 * np.arange(nt - 1) + l) for l, p in enumerate(obj.pulses)]
        older = [p * (1.0 + 0.1 * rng.standard_normal(p.shape)) for p in pulses]  # the "previous iteration"
        _, states = ko.forward_propagation(prob, older, store=True)
        D = cc.random_hermitian(prob.N, 31, 1.0)
        W = cc.source(D, cc.factors(LAMBDA_B, prob.tlist, lambda t: 0.5 + t / prob.tlist[-1]), states)
        chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
        norms = (0.2 + rng.random(prob.K))
        ref = cc.backward_sweep(prob, chi_T, pulses, W, norms)
        plain = ko.backward_sweep(prob, chi_T, pulses)
        assert np.abs(ref - plain).max() > 1e-3  # (the source is no rounding matter)
        _refs[name] = dict(obj=obj, prob=prob, pulses=np.array(pulses), W=W, chi_T=chi_T, norms=norms, ref=ref)
    return _refs[name]


def _case_engine(name, cls=None):
    from krotov_amd.engine import HipKrotovEngine

    obj = _reference(name)['obj']
    _, _, family, kw = CASES[name][:4]
    ops = krotov_amd.configs.sparse_ops(obj) if obj.fmt == 'csr' else \
        [[obj.H0[k]] + [obj.Hc[k][l] for l in range(obj.L)] for k in range(obj.K)]
    eng = (cls or HipKrotovEngine)(ops, np.diff(obj.tlist), is_super=obj.is_super, **kw)
    if family is not None:
        assert eng.kernel.endswith(family) if family.startswith('/') else eng.kernel == family, eng.kernel
    return eng


def _tol(prob):
    return 1e-11 if prob.is_super else TOL


def test_regime_cases_enter_their_regime():
    """Host-only witnesses of (8)'s regimes, from the library's exported planner tables."""
    tables = hp.series_degree_tables()
    for name in ('tile_ramp', 'gen_ramp'):
        obj = CASES[name][0]()
        dt = np.diff(obj.tlist)
        assert dt.max() > 20 * dt.min()  # non-uniform dt
        # (the sweep runs under pulses shifted by <= 0.05: the plan is taken under those)
        pulses = [np.array(p) + 0.05 * np.cos(1.7 * np.arange(len(dt)) + l) for l, p in enumerate(obj.pulses)]
        theta = hp.theta_sequence(obj, pulses)
        k = int(np.argmax(theta.max(axis=1)))
        for tab_name, tab in tables.items():
            nsub, deg = hp.series_plan(theta[k], THETA_MAX, tab)
            assert nsub.max() >= 2 and nsub.min() == 1, (name, tab_name, nsub)  # an interval with sub-steps, one without
            assert hp._changes(deg) >= 4 and len(set(deg.tolist())) >= 3, (name, tab_name, deg)  # degree changes
    for name in ('tile_nt2', 'gen_nt2'):
        assert len(CASES[name][0]().tlist) == 2


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_backward_sweep_with_source_vs_restatement(name, monkeypatch):
    """(8) Every case asserts through the launch registry which kernel ran; chi_norms != 1 everywhere."""
    from krotov_amd import _lib

    for key, value in (CASES[name][4] if len(CASES[name]) > 4 else {}).items():
        monkeypatch.setenv(key, value)
    r = _reference(name)
    eng = _case_engine(name)
    _lib.forget_launched_kernels()
    got = eng.backward_source(r['chi_T'], r['pulses'], r['W'], r['norms']).cpu().numpy()
    launched = _lib.kernel_instantiations(launched_only=True)
    scale = max(1.0, np.abs(r['ref']).max())
    print("%s: max |d chi| = %.3e (max |chi| %.3f) on %s, %s" % (name, np.abs(got - r['ref']).max(), scale, eng.kernel, launched))
    assert launched == [CASES[name][1]], launched
    assert np.abs(got - r['ref']).max() < _tol(r['prob']) * scale
    assert np.array_equal(got[:, -1], r['chi_T'])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tile_n64_L2', 'gen_n70_tile128'])
def test_null_norms_are_ones(name):
    """(8) ``chi_norms`` NULL: the source is divided by 1 -- the sweep with norms of one, bit for bit, and the restatement's."""
    r = _reference(name)
    eng = _case_engine(name)
    none = eng.backward_source(r['chi_T'], r['pulses'], r['W'], None).cpu().numpy()
    ones = eng.backward_source(r['chi_T'], r['pulses'], r['W'], np.ones(r['prob'].K)).cpu().numpy()
    assert np.array_equal(none, ones)
    ref = cc.backward_sweep(r['prob'], r['chi_T'], list(r['pulses']), r['W'], None)
    assert np.abs(none - ref).max() < TOL * max(1.0, np.abs(ref).max())
    assert np.abs(none - r['ref']).max() > 1e-4  # (the norms of the main case are not 1)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('kernel,name,plain,src', [
    ('tile512', 'tile_n64_L2', 'kh_tile_sweep_store<1, 2>', TILE(2)),
    ('tile512', 'tile_n64_L1', 'kh_tile_sweep_store<1, 1>', TILE(1)),
    ('generic', 'gen_n70_tile128', 'kh_gen_sweep_store<false>', GEN),
    ('generic', 'tile_n64_L2', 'kh_gen_sweep_store<false>', GEN),
])
def test_zero_source_equals_the_plain_backward_sweep(kernel, name, plain, src, monkeypatch):
    """(9) W = 0 under KH_KERNEL=tile512 and under KH_KERNEL=generic: ``kh_backward_store`` of the same engine, bit for
    bit, whatever the norms (chi + h 0 is chi; a component that is exactly -0.0 would come out as +0.0: none is here)."""
    from krotov_amd import _lib

    monkeypatch.setenv('KH_KERNEL', kernel)
    r = _reference(name)
    obj = r['obj']
    eng = _dense_engine(obj)
    _lib.forget_launched_kernels()
    want = eng.backward(r['chi_T'], r['pulses']).cpu().numpy()
    got = eng.backward_source(r['chi_T'], r['pulses'], np.zeros_like(r['W']), r['norms']).cpu().numpy()
    assert sorted(_lib.kernel_instantiations(launched_only=True)) == sorted([plain, src])
    assert got.tobytes() == want.tobytes()
    assert np.abs(want - ko.backward_sweep(r['prob'], r['chi_T'], list(r['pulses']))).max() < TOL
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tile_n64_L3', 'tile_n5_mini', 'gen_n70_tile128', 'gen_csr_n40'])
def test_two_runs_are_bitwise_equal(name):
    """(10)"""
    r = _reference(name)
    eng = _case_engine(name)
    one = eng.backward_source(r['chi_T'], r['pulses'], r['W'], r['norms']).cpu().numpy()
    two = eng.backward_source(r['chi_T'], r['pulses'], r['W'], r['norms']).cpu().numpy()
    assert one.tobytes() == two.tobytes()
    assert np.abs(one - r['ref']).max() < TOL * max(1.0, np.abs(r['ref']).max())
    eng.close()


@pytest.mark.gpu
def test_refusals_of_the_entry_point():
    """(10) Replica, Lindblad-form and mixed engines answer KH_ERR_UNSUPPORTED; a null source and a source aliasing the
    output KH_ERR_INVALID."""
    import torch

    from krotov_amd import _lib, configs
    from krotov_amd.engine import HipKrotovEngine

    rng = np.random.default_rng(2)
    d, nt = 4, 6

    def call(eng, src=True, alias=False):
        K, N = eng.K, eng.N
        chi_T = torch.zeros((K, N), dtype=torch.complex128, device=eng.device)
        pulses = torch.zeros(eng._pulse_shape(), dtype=torch.float64, device=eng.device)
        W = torch.zeros((K, nt, N), dtype=torch.complex128, device=eng.device)
        out = W if alias else torch.empty_like(W)
        return eng._lib.kh_backward_store_source(eng._handle, chi_T.data_ptr(), pulses.data_ptr(),
                                                 W.data_ptr() if src else None, None, out.data_ptr(), eng._stream())

    H = [[configs.herm(rng, d, 1.0), configs.herm(rng, d, 0.5)] for _ in range(2)]
    lind = HipKrotovEngine(H, np.full(nt - 1, 0.1), c_ops=[[0.1 * np.eye(d, k=1).astype(complex)] for _ in range(2)])
    assert lind.kernel.startswith('lindblad') and call(lind) == _lib.KH_ERR_UNSUPPORTED
    lind.close()
    ops = [[configs.herm(rng, d, 1.0), configs.herm(rng, d, 0.5)] for _ in range(4)]
    rep = HipKrotovEngine(ops, np.full((2, nt - 1), 0.1), replicas=2)
    assert rep.replicas == 2 and call(rep) == _lib.KH_ERR_UNSUPPORTED
    rep.close()
    mixed_ops = [[configs.herm(rng, n, 1.0), configs.herm(rng, n, 0.5)] for n in (3, 5)]
    mixed = HipKrotovEngine(mixed_ops, np.full(nt - 1, 0.1))
    assert mixed.kernel == 'generic/mixed' and call(mixed) == _lib.KH_ERR_UNSUPPORTED
    with pytest.raises(_lib.KrotovHipError) as err:
        mixed.apply_store([None, None], None, torch.zeros((2, nt, 5), dtype=torch.complex128, device=mixed.device))
    assert err.value.code == _lib.KH_ERR_UNSUPPORTED
    mixed.close()
    eng = HipKrotovEngine(ops, np.full(nt - 1, 0.1))
    assert call(eng) == _lib.KH_OK
    assert call(eng, src=False) == _lib.KH_ERR_INVALID
    assert call(eng, alias=True) == _lib.KH_ERR_INVALID
    eng.check()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tile_n33', 'gen_n70_tile128'])
def test_guarded_buffers(name):
    """(11) One tile and one generic case of (8) with every tensor carved from tests/guarded.py's arena: guard bands and
    the source store are byte-identical afterwards (as is every other input); the trajectory W is formed from, too."""
    import torch

    from guarded import GuardedEngine

    from krotov_amd import _lib

    r = _reference(name)
    prob = r['prob']
    K, N, nt, L = prob.K, prob.N, len(prob.tlist), len(r['pulses'])
    eng = _case_engine(name, cls=GuardedEngine)
    a = eng.arena
    c128, f64 = torch.complex128, torch.float64
    t = dict(chi_T=a.carve('sdc_chi_T', (K, N), c128), pulses=a.carve('sdc_pulses', (L, nt - 1), f64),
             W=a.carve('sdc_W', (K, nt, N), c128), norms=a.carve('sdc_norms', (K,), f64),
             out=a.carve('sdc_out', (K, nt, N), c128, 'output'), states=a.carve('sdc_states', (K, nt, N), c128),
             fac=a.carve('sdc_factors', (nt,), f64), W2=a.carve('sdc_W2', (K, nt, N), c128, 'output'))
    a.check_layout()
    rng = np.random.default_rng(4)
    states = rng.standard_normal((K, nt, N)) + 1j * rng.standard_normal((K, nt, N))
    fac = rng.standard_normal(nt)
    for key, host in (('chi_T', r['chi_T']), ('pulses', r['pulses']), ('W', r['W']), ('norms', r['norms']),
                      ('states', states), ('fac', fac)):
        t[key].copy_(torch.from_numpy(np.ascontiguousarray(host)))
    t['out'].fill_(float('nan'))
    t['W2'].fill_(float('nan'))
    a.snapshot()
    _lib.forget_launched_kernels()
    got = eng.backward_source(t['chi_T'], t['pulses'], t['W'], t['norms'], out=t['out'])
    torch.cuda.synchronize(eng.device)
    assert got.data_ptr() == t['out'].data_ptr()
    a.verify('kh_backward_store_source', [t['out']])
    assert _lib.kernel_instantiations(launched_only=True) == [CASES[name][1]]
    assert np.abs(got.cpu().numpy() - r['ref']).max() < TOL * max(1.0, np.abs(r['ref']).max())
    D = cc.random_hermitian(N, 5, 1.0)
    table = [D] + [None] * (K - 2) + [D]
    W2 = eng.apply_store(table, t['fac'], t['states'], out=t['W2'])  # (its operator and pointer table are carved too)
    torch.cuda.synchronize(eng.device)
    a.verify('kh_apply_store', [t['W2']])
    assert np.abs(W2.cpu().numpy() - cc.source(table, fac, states)).max() < TOL * N
    eng.close()


# ---------------------------------------------------------------------------
# GPU: optimize_pulses on the device path
# ---------------------------------------------------------------------------
TANH = ('tanh',) + pc.BOUNDS
DEVICE_RUNS = {
    # name: (problem, kinds, sigma, a source() of the user's own, the source kernel)
    'n5_L1': (lambda: pc.problem(K=3, N=5, L=1, nt=14), None, None, False, TILE(1)),
    'n64_L3': (lambda: pc.problem(K=3, N=64, L=3, nt=12), None, None, False, TILE(3)),
    'n70': (lambda: pc.problem(K=2, N=70, L=2, nt=10), None, None, False, GEN),
    'n5_L2_sigma': (lambda: pc.problem(K=3, N=5, L=2, nt=14), None, -1.5, False, TILE(2)),
    'n70_sigma': (lambda: pc.problem(K=2, N=70, L=2, nt=10), None, -1.5, False, GEN),
    'n64_L3_tanh': (lambda: pc.problem(K=3, N=64, L=3, nt=12), [TANH, ('square',), None], None, False, TILE(3)),
    'n70_tanh': (lambda: pc.problem(K=2, N=70, L=2, nt=10), [TANH, None], None, False, GEN),
    'n5_L1_own_source': (lambda: pc.problem(K=3, N=5, L=1, nt=14), None, None, True, TILE(1)),
}
_device_refs = {}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(DEVICE_RUNS))
def test_optimize_pulses_on_the_device_vs_restatement(name):
    """(12) Three iterations: N = 5 with L = 1, N = 64 with L = 3, N = 70; first order, with ``sigma=``, with a
    ``TanhParametrization``; a subclass overriding ``source()`` gives the built-in class's result (the same reference);
    ``constraint.integral`` on the device trajectories (``HipKrotovEngine.expect``) equals the host trapezoid."""
    from krotov_amd import _lib

    build, kinds, sigma, own, kernel = DEVICE_RUNS[name]
    spec = build()
    prob, gp, S, lam = pc.oracle_side(spec)
    D = _constraint_of(spec)
    key = name.replace('_own_source', '')
    if key not in _device_refs:
        _device_refs[key] = cc.optimize(prob, gp, S, lam, ko.chis_re, 3, D, LAMBDA_B, sigma=sigma, kinds=kinds)
    ref = _device_refs[key]

    class Mine(QuadraticStateConstraint):
        calls = 0

        def source(self, forward_states, tlist):
            Mine.calls += 1
            return cc.source(D, cc.factors(LAMBDA_B, np.asarray(tlist)), np.asarray(forward_states))

    con = (Mine if own else QuadraticStateConstraint)(D, LAMBDA_B)
    _lib.forget_launched_kernels()
    res = _run(spec, con, 3, kinds=kinds, device=True, sigma=sigma)
    launched = _lib.kernel_instantiations(launched_only=True)
    print(launched)
    assert kernel in launched and (APPLY in launched) == (not own), launched
    assert any(n.startswith('kh_expect') for n in launched), launched  # (constraint.integral in the hook)
    assert Mine.calls == (3 if own else 0)
    _assert_matches(res, ref)
    assert all(kept == (True, True) for kept in res.kept)
    assert len(res.g_b) == 4  # (iteration 0 included)
