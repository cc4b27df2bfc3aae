"""Host-side logic on CPU: conversions, shapes, functionals, objectives and the
plugin path of optimize_pulses (driven by user callables -- here NumPy closures
built on the oracle's single-step function, the reference's "numpy mode").

KAT sources: reference tests/test_structural_conversions.py, test_shapes.py,
test_functionals.py, test_mu.py, test_overlap.py, test_krotov.py, and the TLS
dump of tests/test_result_serialization.
"""
import copy
import os

import numpy as np
import pytest

import krotov_amd
from krotov_amd import configs, conversions, functionals, shapes
from oracle import krotov_oracle as ko

from helpers import golden, numpy_plugins


def test_controls_roundtrip_and_boundaries():
    rng = np.random.default_rng(0)
    c = rng.standard_normal(50)
    p = conversions.control_onto_interval(c)
    assert len(p) == 49 and p[0] == c[0] and p[-1] == c[-1]
    back = conversions.pulse_onto_tlist(p)
    assert np.abs(back[:-2] - c[:-2]).max() < 1e-12  # the recurrence inverts the averaging
    assert np.abs(conversions.control_onto_interval(back) - p).max() < 1e-12  # pulse -> control -> pulse = id
    assert back[0] == c[0] and back[-1] == p[-1]
    # matches the oracle's restatement bit for bit
    assert np.array_equal(p, ko.control_onto_interval(c))
    assert np.array_equal(back, ko.pulse_onto_tlist(p))


def test_discretize_rejects_complex_and_wrong_length():
    tl = np.linspace(0, 1, 11)
    with pytest.raises(TypeError):
        conversions.discretize(lambda t, a: 1j * t, tl)
    with pytest.raises(ValueError):
        conversions.discretize(np.zeros(5), tl)
    with pytest.raises(TypeError):
        conversions.discretize("nope", tl)
    vals = conversions.discretize(lambda t, a: t**2, tl, via_midpoints=True)
    assert len(vals) == 11 and vals[0] == 0.0


def test_shapes_match_oracle_bitwise():
    for t in np.linspace(-0.5, 5.5, 241):
        for func in ('blackman', 'sinsq'):
            assert shapes.flattop(t, 0, 5, 0.3, func=func) == ko.flattop(t, 0, 5, 0.3, func=func)
        assert shapes.blackman(t, 1.0, 4.0) == ko.blackman(t, 1.0, 4.0)
    assert abs(shapes.flattop(0.0, 0, 5, 0.3)) < 1e-16 and shapes.flattop(2.5, 0, 5, 0.3) == 1.0
    with pytest.raises(ValueError):
        shapes.flattop(1.0, 0, 5, 0.3, func='nope')
    cb = shapes.qutip_callback(shapes.flattop, t_start=0, t_stop=5, t_rise=0.3)
    assert cb(2.5, None) == 1.0 and cb(2.5, {'func': 'sinsq'}) == 1.0


def test_mapping_and_plug_in(dummy_objectives):
    X, Y, Z = np.eye(2), 2 * np.eye(2), 3 * np.eye(2)
    u1, u2 = np.zeros(3), np.ones(3)
    o1 = krotov_amd.Objective(initial_state=None, target=None, H=[X, [Y, u1], [Z, u1]])
    o2 = krotov_amd.Objective(initial_state=None, target=None, H=[X, [Y, u2]])
    controls = conversions.extract_controls([o1, o2])
    assert len(controls) == 2 and controls[0] is u1 and controls[1] is u2
    mapping = conversions.extract_controls_mapping([o1, o2], controls)
    assert mapping == [[[[1, 2], []]], [[[], [1]]]]
    H = conversions.plug_in_pulse_values(['X', ['X', None], ['Y', None], ['Z', None]],
                                         [np.array([0, 10, 0]), np.array([0, 20, 0])], [[1, 2], [3]], 1)
    assert H == ['X', ['X', 10], ['Y', 10], ['Z', 20]]
    with pytest.raises(ValueError):
        conversions.pulse_options_dict_to_list({}, controls)


def test_functionals_known_answers():
    """reference tests/test_functionals.py: J_T_ss=0.25? -> values on fixed taus."""
    class O:
        def __init__(self, target):
            self.target = target
    objs = [O(np.array([1, 0], dtype=complex)), O(np.array([0, 1], dtype=complex))]
    taus = np.array([0.5, 1.0], dtype=complex)
    assert abs(functionals.F_ss(None, objs, taus) - (0.25 + 1.0) / 2) < 1e-14
    assert abs(functionals.F_sm(None, objs, taus) - 0.75**2) < 1e-14
    assert abs(functionals.F_re(None, objs, taus) - 0.75) < 1e-14
    assert abs(functionals.J_T_re(None, objs, taus) - 0.25) < 1e-14
    for name in ('re', 'ss', 'sm', 'hs'):
        fn = getattr(functionals, 'chis_' + name)
        fw = [np.array([0.6, 0.8j]), np.array([0.1, 0.9])]
        listed = np.array(fn(fw, objs, taus))
        stacked = functionals.chi_stacked(fn, np.array([o.target for o in objs]), None, np.array(fw), taus)
        assert np.abs(listed - stacked).max() < 1e-15, name
        c, d = functionals.chi_coefficients(fn, None, taus, 2)  # what kh_chi_boundary is fed
        combined = c[:, None] * np.array([o.target for o in objs]) + d[:, None] * np.array(fw)
        assert np.abs(listed - combined).max() < 1e-15, name
    assert functionals.chi_coefficients(functionals.chis_ss, None, [None, None], 2) is None
    assert functionals.chi_coefficients(lambda **kw: None, None, taus, 2) is None
    objs[0].weight, objs[1].weight = 0.5, 1.5
    listed = np.array(functionals.chis_sm(None, objs, taus))
    stacked = functionals.chi_stacked(functionals.chis_sm, np.array([o.target for o in objs]),
                                      np.array([0.5, 1.5]), None, taus)
    assert np.abs(listed - stacked).max() < 1e-15
    c, d = functionals.chi_coefficients(functionals.chis_sm, np.array([0.5, 1.5]), taus, 2)
    assert np.abs(listed - c[:, None] * np.array([o.target for o in objs])).max() < 1e-15 and not d.any()


def test_overlap_and_mu(dummy_objectives):
    from krotov_amd.mu import derivative_wrt_pulse
    from krotov_amd.second_order import _overlap

    a = np.array([[1, 2j], [0, 1]], dtype=complex)  # non-Hermitian: must use a^dagger
    b = np.array([[0.5, 1], [1j, 2]], dtype=complex)
    assert abs(_overlap(a, b) - np.trace(a.conj().T @ b)) < 1e-14
    assert _overlap('PE', b) is None
    sp = np.array([[0, 1], [0, 0]], dtype=complex)
    sm = sp.T.copy()
    u = np.zeros(3)
    obj = krotov_amd.Objective(initial_state=None, target=None, H=[np.eye(2), [sp, u], [sm, u]])
    mapping = conversions.extract_controls_mapping([obj], [u])
    mu = derivative_wrt_pulse([obj], 0, [u], mapping, 0, 0)
    v = np.array([0.3, 0.7j])
    assert np.abs(mu(v) - (sp + sm) @ v).max() < 1e-15  # repeated control: sum of terms
    other = np.ones(3)
    mapping2 = conversions.extract_controls_mapping([obj], [u, other])
    zero = derivative_wrt_pulse([obj], 0, [u, other], mapping2, 1, 0)
    assert np.all(zero(v) == 0)


def test_objective_copy_eq_adjoint_and_constructors():
    H0 = np.diag([1.0, -1.0]).astype(complex)
    H1 = np.array([[0, 1j], [-1j, 0]])
    u = lambda t, args: 1.0  # noqa: E731
    psi = np.array([1, 0], dtype=complex)
    obj = krotov_amd.Objective(initial_state=psi, target=psi[::-1].copy(), H=[H0, [H1 * 1j, u]])
    obj.weight = 0.7
    c = copy.copy(obj)
    assert c == obj and c.H is not obj.H and c.H[1] is not obj.H[1] and c.H[1][0] is obj.H[1][0]
    assert c.weight == 0.7
    adj = obj.adjoint()
    assert np.array_equal(adj.H[1][0], (H1 * 1j).conj().T) and adj.H[1][1] is u and adj.weight == 0.7
    d = copy.deepcopy(obj)
    assert d == obj
    d.weight = 0.1
    assert d != obj
    # gate objectives: X gate on a qubit reuses the basis objects
    basis = [np.array([1, 0], dtype=complex), np.array([0, 1], dtype=complex)]
    X = np.array([[0, 1], [1, 0]])
    objs = krotov_amd.gate_objectives(basis, X, [H0, [H1, u]])
    assert len(objs) == 2 and objs[0].target is basis[1] and objs[1].target is basis[0]
    o3 = krotov_amd.gate_objectives(basis, X, [H0, [H1, u]], liouville_states_set='3states', weights=[20, 1, 1])
    assert len(o3) == 3 and abs(sum(o.weight for o in o3) - 3) < 1e-12
    assert abs(np.trace(o3[0].initial_state) - 1) < 1e-14
    full = krotov_amd.gate_objectives(basis, X, [H0, [H1, u]], liouville_states_set='full')
    assert len(full) == 4
    with pytest.raises(ValueError):
        krotov_amd.gate_objectives(basis, 'nope', [H0])
    ens = krotov_amd.ensemble_objectives(objs, [[H0, [0.9 * H1, u]], [H0, [1.1 * H1, u]]])
    assert len(ens) == 6 and ens[2].initial_state is basis[0]
    L = krotov_amd.objectives.liouvillian([H0, [H1, u]], c_ops=[np.array([[0, 1], [0, 0]])])
    assert L[0].shape == (4, 4) and L[1][1] is u
    assert np.abs(L[1][0] - configs.liouvillian_dense(H1)).max() == 0


def _run_plugin(spec, iters, **kw):
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    prop, mu, overlap = numpy_plugins(spec.is_super)
    return krotov_amd.optimize_pulses(
        objectives, pulse_options, spec.tlist, propagator=prop,
        chi_constructor=getattr(krotov_amd.functionals, 'chis_' + spec.chi),
        mu=mu, overlap=overlap, norm=np.linalg.norm, iter_stop=iters, store_all_pulses=True, **kw)


def test_plugin_path_reproduces_tls_dump():
    """Config 1 (plumbing, no GPU): the host loop with NumPy plugins vs the
    reference's shipped TLS result, all pulses of the first 6 iterations."""
    g = golden('dump_tls_ss')
    res = _run_plugin(configs.config_c1(), 6)
    got = np.array([np.array(p) for p in res.all_pulses])
    assert np.abs(got[0] - g['all_pulses'][0]).max() == 0.0
    assert np.abs(got - g['all_pulses'][:7]).max() < 1e-9
    assert np.abs(np.array(res.tau_vals)[:, 0] - g['tau_vals'][:7, 0]).max() < 1e-9
    assert res.iters == list(range(7)) and res.message == "Reached 6 iterations"
    assert len(res.optimized_controls[0]) == len(g['tlist'])
    assert np.abs(res.optimized_controls[0] - conversions.pulse_onto_tlist(got[-1][0])).max() == 0


@pytest.mark.parametrize('name,builder', [
    ('ref_c2_liouville', lambda: configs.config_c2_liouville()),
    ('ref_c5_small_L3', lambda: configs.config_c5(K=5, N=12, nt=151, L=3, distinct=True)),
])
def test_plugin_path_matches_reference_loop(name, builder):
    g = golden(name)
    res = _run_plugin(builder(), int(g['iter_stop']))
    got = np.array([np.array(p) for p in res.all_pulses])
    assert np.abs(got - g['all_pulses']).max() < 1e-11
    assert np.abs(np.array(res.tau_vals) - g['tau_vals']).max() < 1e-11


def test_plugin_path_second_order_matches_reference_loop():
    """sigma= through the host loop (reference optimize.py:429-442, 451-452, 468-469,
    492-500, 566-577) vs the reference's own loop on the same problem."""
    from helpers import product_sigma

    g = golden('ref_so_c3')
    spec = configs.config_c3(nt=201)
    spec.lambda_a = 20.0
    sig = product_sigma(0.0, 2.0)
    seen = []

    def hook(**kw):
        seen.append((kw['iteration'], kw['forward_states'] is not None, kw['forward_states0'] is not None))

    res = _run_plugin(spec, int(g['iter_stop']), sigma=sig, info_hook=hook)
    got = np.array([np.array(p) for p in res.all_pulses])
    assert np.abs(got - g['all_pulses']).max() < 1e-11
    assert np.abs(np.array(res.tau_vals) - g['tau_vals']).max() < 1e-11
    # refresh after every iteration but the last, with the full trajectories, and
    # (like the reference) after guess_pulses was advanced to the optimized ones
    assert np.abs(np.array(sig.history) - g['A_history']).max() < 1e-10
    assert sig.calls == [(len(g['tau_vals'][0]), len(spec.tlist), True)] * 2
    assert seen == [(i, True, True) for i in range(4)]
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    prop, mu, overlap = numpy_plugins(spec.is_super)
    with pytest.raises(ValueError, match='skip_initial_forward_propagation'):
        krotov_amd.optimize_pulses(
            objectives, pulse_options, spec.tlist, propagator=prop, mu=mu, overlap=overlap,
            chi_constructor=krotov_amd.functionals.chis_sm, sigma=sig, iter_stop=1,
            skip_initial_forward_propagation=True)


def test_numerical_estimate_A_known_answers():
    """reference second_order.py:148-164 on hand-checkable vectors."""
    from krotov_amd.second_order import numerical_estimate_A

    fw0 = [[None, np.array([1.0, 0.0], dtype=complex)], [None, np.array([0.0, 1.0], dtype=complex)]]
    fw = [[None, np.array([1.0, 0.5j], dtype=complex)], [None, np.array([0.5, 1.0], dtype=complex)]]
    chis = [np.array([0.0, 1.0j]), np.array([1.0, 0.0], dtype=complex)]
    # dphi = (0, .5j), (.5, 0): denominator .5; numerator 2*2*Re(conj(1j)*.5j) + 2*3*.5 - .25 = 2 + 3 - .25
    assert abs(numerical_estimate_A(fw, fw0, chis, [2.0, 3.0], -0.25) - 9.5) < 1e-14
    assert numerical_estimate_A(fw0, fw0, chis, [2.0, 3.0], -0.25) == 0


def test_continue_from_equals_uninterrupted():
    """reference tests/test_krotov.py:426-432: continuation == one long run (1e-10)."""
    spec = configs.config_c1(nt=120)
    full = _run_plugin(spec, 4)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    prop, mu, overlap = numpy_plugins()
    kw = dict(propagator=prop, chi_constructor=krotov_amd.functionals.chis_ss, mu=mu, overlap=overlap,
              norm=np.linalg.norm, store_all_pulses=True)
    first = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, iter_stop=2, **kw)
    cont = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, iter_stop=4, continue_from=first, **kw)
    assert cont.iters == [0, 1, 2, 3, 4]
    assert np.abs(cont.optimized_controls[0] - full.optimized_controls[0]).max() < 1e-10
    with pytest.raises(ValueError):
        krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist[:-1], iter_stop=3, continue_from=first, **kw)
    with pytest.raises(ValueError):
        krotov_amd.optimize_pulses(objectives[:0] + objectives + objectives, pulse_options, spec.tlist,
                                   iter_stop=3, continue_from=first, **kw)


def test_validation_errors():
    """reference tests/test_krotov.py:22-134, test_pulse_options.py."""
    spec = configs.config_c1(nt=30)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    prop, mu, overlap = numpy_plugins()
    kw = dict(propagator=prop, chi_constructor=krotov_amd.functionals.chis_re, mu=mu, overlap=overlap,
              norm=np.linalg.norm, iter_stop=1)
    ctrl = spec.controls[0]
    with pytest.raises(ValueError, match='lambda_a'):
        krotov_amd.optimize_pulses(objectives, {ctrl: dict(update_shape=1)}, spec.tlist, **kw)
    with pytest.raises(ValueError, match='update_shape'):
        krotov_amd.optimize_pulses(objectives, {ctrl: dict(lambda_a=1.0)}, spec.tlist, **kw)
    with pytest.raises(ValueError, match=r'range \[0, 1\]'):
        krotov_amd.optimize_pulses(objectives, {ctrl: dict(lambda_a=1.0, update_shape=lambda t: 2.0)}, spec.tlist, **kw)
    with pytest.raises(ValueError, match='real-valued'):
        krotov_amd.optimize_pulses(objectives, {ctrl: dict(lambda_a=1.0, update_shape=lambda t: 1j)}, spec.tlist, **kw)
    with pytest.raises(ValueError, match='pulse options'):
        krotov_amd.optimize_pulses(objectives, {}, spec.tlist, **kw)
    # complex control
    H = [spec.H0[0], [spec.Hc[0][0], lambda t, args: 1j]]
    objs = [krotov_amd.Objective(initial_state=spec.init[0], target=spec.target[0], H=H)]
    with pytest.raises(ValueError, match='real-valued'):
        krotov_amd.optimize_pulses(objs, {H[1][1]: dict(lambda_a=1.0, update_shape=1)}, spec.tlist, **kw)


def test_info_hook_and_convergence_contract():
    spec = configs.config_c1(nt=60)
    seen = []

    def hook(**kwargs):
        needed = {'objectives', 'adjoint_objectives', 'backward_states', 'forward_states', 'forward_states0',
                  'guess_pulses', 'optimized_pulses', 'g_a_integrals', 'lambda_vals', 'shape_arrays',
                  'fw_states_T', 'tlist', 'tau_vals', 'start_time', 'stop_time', 'iteration', 'info_vals',
                  'shared_data', 'propagator', 'chi_constructor', 'mu', 'sigma', 'iter_start', 'iter_stop'}
        assert needed <= set(kwargs)
        seen.append(kwargs['iteration'])
        return 1 - abs(kwargs['tau_vals'][0]) ** 2

    def halve(**kwargs):
        kwargs['lambda_vals'][:] *= 0.5

    def converged(result):
        return "done" if len(result.iters) > 2 else None

    res = _run_plugin(spec, 10, info_hook=hook, modify_params_after_iter=halve, check_convergence=converged)
    assert seen == [0, 1, 2] and res.message == "Reached convergence: done"
    assert len(res.info_vals) == 3 and res.info_vals[2] < res.info_vals[0]


def test_sparse_ingestion_and_ode_propagator_surface():
    """to_sparse: SciPy matrices, QuTiP-4-like objects (sparse .data), dense arrays; the
    DensityMatrixODEPropagator drop-in keeps the reference's constructor (propagators.py:180-205)."""
    import scipy.sparse as sp

    from krotov_amd._ingest import to_sparse
    from krotov_amd.optimize import _use_device_path
    from krotov_amd.propagators import DensityMatrixODEPropagator, HipExpm

    a = np.array([[0, 2j, 0], [0, 0, 0], [1, 0, 3]], dtype=complex)

    class QobjLike:
        def __init__(self, arr):
            self.data = sp.csr_matrix(arr)

        def full(self):
            return self.data.toarray()

    for src in (a, sp.coo_matrix(a), sp.csc_matrix(a), QobjLike(a)):
        m = to_sparse(src)
        assert sp.isspmatrix_csr(m) and m.dtype == np.complex128 and np.array_equal(m.toarray(), a)
    with pytest.raises(ValueError):
        to_sparse(np.zeros((2, 3)))
    p = DensityMatrixODEPropagator(method='bdf', order=5, atol=1e-10, rtol=1e-8, nsteps=10, reentrant=True)
    assert (p.method, p.order, p.atol, p.rtol, p.nsteps, p.reentrant) == ('bdf', 5, 1e-10, 1e-8, 10, True)
    assert p.sparse and p.liouville is True and isinstance(p, HipExpm) and not HipExpm().sparse

    class Obj:
        c_ops = []

    assert _use_device_path(p, None, None, None, 'array', [Obj()])
    assert _use_device_path([p, HipExpm()], None, None, None, 'array', [Obj(), Obj()])
    assert not _use_device_path(lambda *a, **k: None, None, None, None, 'array', [Obj()])


def test_device_path_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    spec = configs.config_c1(nt=20)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist,
                                   propagator=krotov_amd.propagators.expm,
                                   chi_constructor=krotov_amd.functionals.chis_ss, iter_stop=1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        krotov_amd.propagators.expm([spec.H0[0], [spec.Hc[0][0], 0.1]], spec.init[0], 0.01)


def test_bench_starts_its_own_ranks(monkeypatch):
    """``python bench.py --gpus N`` without a launcher (no WORLD_SIZE): bench.self_launch re-executes the same command
    line under torch.distributed.run -- one rank per GPU, rendezvous on 127.0.0.1 with a free port -- and hands the
    launcher's return code on (the driver's multi-GPU command is exactly this form)."""
    import importlib
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    bench = importlib.import_module('bench')
    seen = {}

    class Done:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen['cmd'], seen['env'] = list(cmd), dict(env)
        return Done()

    monkeypatch.setattr(subprocess, 'run', fake_run)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '3', '--warmup', '1'])
    assert bench.self_launch(4) == 7
    cmd = seen['cmd']
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert cmd[cmd.index('--nproc-per-node') + 1] == '4' and '--nnodes=1' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert 1024 < int(cmd[cmd.index('--master-port') + 1]) < 65536
    tail = cmd[cmd.index(os.path.join(root, 'bench.py')) + 1:]
    assert tail == ['--gpus', '4', '--steps', '3', '--warmup', '1']
    assert seen['env'].get('HSA_ENABLE_IPC_MODE_LEGACY') == '0'


def test_bench_dump_outputs_writes_what_the_caller_received(tmp_path):
    """``bench.py --dump-outputs DIR`` (bench.dump_outputs): the optimized controls, the last iteration's tau values and
    the forward states at T of a result, as float64 .npy files with complex values split into (real, imaginary);
    beyond the size limit a seeded sample of rows, the same one every time, with its row indices beside it."""
    import importlib
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    bench = importlib.import_module('bench')
    spec = configs.config_c5(K=40, N=16, nt=21, L=2, distinct=True)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    prop, mu, overlap = numpy_plugins(spec.is_super)
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, propagator=prop,
                                     chi_constructor=krotov_amd.functionals.chis_re, mu=mu, overlap=overlap,
                                     norm=np.linalg.norm, iter_stop=2)
    bench.dump_outputs(res, str(tmp_path / 'all'))
    got = {n: np.load(str(tmp_path / 'all' / (n + '.npy'))) for n in ('optimized_controls', 'tau_vals', 'states')}
    assert sorted(os.listdir(str(tmp_path / 'all'))) == ['optimized_controls.npy', 'states.npy', 'tau_vals.npy']
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got['optimized_controls'], np.array(res.optimized_controls, dtype=np.float64))
    tau = np.asarray(res.tau_vals[-1])
    assert got['tau_vals'].shape == (40, 2) and np.array_equal(got['tau_vals'][:, 0] + 1j * got['tau_vals'][:, 1], tau)
    states = np.array([np.asarray(s).ravel() for s in res.states])
    assert got['states'].shape == (40, 16, 2) and np.array_equal(got['states'][..., 0] + 1j * got['states'][..., 1], states)

    limit = sum(a.nbytes for a in got.values()) // 2
    for run in ('a', 'b'):
        bench.dump_outputs(res, str(tmp_path / run), limit=limit)
    files = sorted(os.listdir(str(tmp_path / 'a')))
    assert sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in files) <= limit
    for f in files:
        assert np.array_equal(np.load(str(tmp_path / 'a' / f)), np.load(str(tmp_path / 'b' / f)))
    for name in ('tau_vals', 'states'):
        rows = np.load(str(tmp_path / 'a' / (name + '_rows.npy'))).astype(int)
        assert 1 <= len(rows) < 40 and np.all(np.diff(rows) > 0)
        assert np.array_equal(np.load(str(tmp_path / 'a' / (name + '.npy'))), got[name][rows])


def test_update_sweep_retry_ladder_on_the_host(monkeypatch, caplog):
    """``_HipBackend.iterate`` after KH_ERR_TIMEOUT (the single-launch update sweep's workgroups were not all resident):
    half the workgroups, then an eighth, through ``set_update_workgroups`` -- two rungs at most, each costs a timed-out
    sweep --; only then (or when the engine has no smaller grid) one launch per interval; a reduced grid that got through
    is kept, the full one probed again after ``_FULL_GRID_PROBE_EVERY`` sweeps in a row.  Driven on the
    CPU with the oracle-backed engine double, whose single-launch sweep "times out" above a scripted number of
    workgroups; the pulses must be the oracle's whatever path was taken."""
    import logging

    import krotov_amd
    import krotov_amd.engine as engine_mod
    from helpers import oracle_optimize
    from krotov_amd import _lib, configs
    from oracle_engine_double import OracleEngineDouble

    script = {'fits': 2, 'floor': 1, 'calls': [], 'stepwise': 0}

    class Flaky(OracleEngineDouble):
        grid = None  # None: the engine's own (K workgroups)

        def set_update_workgroups(self, g=0):
            script['calls'].append(g)
            if g == 0:
                self.grid = None
                return self.K
            if g < script['floor']:
                raise _lib.KrotovHipError("no such grid", _lib.KH_ERR_UNSUPPORTED)
            self.grid = g
            return g

        def forward_update(self, *a):
            if (self.grid or self.K) > script['fits']:
                raise _lib.KrotovHipError("timed out", _lib.KH_ERR_TIMEOUT)
            return super().forward_update(*a)

        def forward_update_sharded(self, *a, **kw):
            script['stepwise'] += 1 if kw.get('graph_chunk') == 0 else 0
            return super().forward_update_sharded(*a, **kw)

    monkeypatch.setattr(engine_mod, 'HipKrotovEngine', Flaky)
    caplog.set_level(logging.WARNING, logger='krotov')
    spec = configs.config_c5(K=8, N=4, nt=9, L=1, distinct=True)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    kw = dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_re, store_all_pulses=True)
    ref = oracle_optimize(spec, 5)

    # 8 workgroups never fit, 2 do: 8 -> 4 (times out) -> 1 (an eighth: two rungs at most) in the first iteration; the
    # grid that got through is kept: no further call, no further timed-out sweep
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, iter_stop=5, **kw)
    assert np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() < 1e-12
    assert script['stepwise'] == 0
    assert script['calls'] == [0, 4, 0, 1]  # (query the full grid, ask for half; query, ask for an eighth)
    assert caplog.text.count('repeating it on 4 workgroups') == 1 and caplog.text.count('repeating it on 1 workgroups') == 1

    # ... and after _FULL_GRID_PROBE_EVERY sweeps in a row on it the full grid gets one more chance (the co-tenant may
    # be gone); the reduced grid of the last time is then asked for directly
    import krotov_amd._update_ladder as optimize_mod

    monkeypatch.setattr(optimize_mod, '_FULL_GRID_PROBE_EVERY', 2)
    script.update(fits=4, calls=[])
    caplog.clear()
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, iter_stop=5, **kw)
    assert np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() < 1e-12
    # it 1: 8 -> 4 fits; it 2: kept; it 3: probe (reset 0), times out, back to 4 at once; it 4: kept; it 5: probe again
    assert script['calls'] == [0, 4] + [0, 0, 4] * 2
    monkeypatch.setattr(optimize_mod, '_FULL_GRID_PROBE_EVERY', 16)

    # no grid fits and the engine refuses anything below 4: half (times out), an eighth (refused) -> one launch per
    # interval and the engine's own grid again; for good after three such sweeps
    script.update(fits=0, floor=4, calls=[], stepwise=0)
    caplog.clear()
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, iter_stop=5, **kw)
    assert np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() < 1e-12
    assert script['stepwise'] == 5
    assert caplog.text.count('one launch per interval') == 3 and 'staying with that form' in caplog.text
    assert script['calls'] == [0, 4, 0, 1, 0] * 3  # (4 is tried and times out, 1 is refused: reset) -- then never again


def _ladder_rig(K, fits, code=None, floor=1, invalid=(), row_split=None):
    """``krotov_amd._update_ladder.UpdateLadder`` on a scripted engine of K workgroups that refuses grids below ``floor``
    (KH_ERR_UNSUPPORTED) or in ``invalid`` (KH_ERR_INVALID), and a sweep that answers ``code`` (KH_ERR_TIMEOUT if None)
    while more than ``script['fits']`` workgroups are in force or the rows are still split.  Returns the engine -- its
    ``calls`` are the arguments of ``set_update_workgroups``, ``splits`` those of ``set_row_split`` --, the script and
    ``run()``: 'single' if the single launch got through, 'intervals' if the per-interval form ran."""
    from krotov_amd import _lib
    from krotov_amd._update_ladder import UpdateLadder

    class Engine:
        grid = None  # None: the engine's own (K workgroups)

        def __init__(self):
            self.calls, self.splits = [], []
            if row_split is not None:  # (the engine double has no such attribute: the ladder must not need it)
                self.row_split = row_split

        def set_update_workgroups(self, g=0):
            self.calls.append(g)
            if g == 0:
                self.grid = None
                return K
            if g in invalid:
                raise _lib.KrotovHipError("no such argument", _lib.KH_ERR_INVALID)
            if g < floor:
                raise _lib.KrotovHipError("no such grid", _lib.KH_ERR_UNSUPPORTED)
            self.grid = g
            return g

        def set_row_split(self, S):
            self.splits.append(S)
            self.row_split = S

    eng = Engine()
    script = {'fits': fits, 'code': _lib.KH_ERR_TIMEOUT if code is None else code, 'sweeps': 0}

    def sweep():
        script['sweeps'] += 1
        if getattr(eng, 'row_split', 1) > 1 or (eng.grid or K) > script['fits']:
            raise _lib.KrotovHipError("did not get through", script['code'])
        return 'single'

    ladder = UpdateLadder(eng)
    return eng, script, lambda: ladder.run(sweep, lambda: 'intervals')


def test_update_ladder_sweep_that_cannot_be_resident(caplog):
    """A sweep that answers KH_ERR_UNSUPPORTED (the device cannot hold the grid at all) walks the same rungs as one that
    timed out; if no grid gets through, the single launch is given up for good AT ONCE -- no strike count, no further
    engine call, no further attempt --; a grid that gets through is kept like any other."""
    import logging

    from krotov_amd import _lib

    caplog.set_level(logging.WARNING, logger='krotov')
    eng, script, run = _ladder_rig(8, fits=0, code=_lib.KH_ERR_UNSUPPORTED)
    assert run() == 'intervals'
    assert eng.calls == [0, 4, 0, 1, 0] and script['sweeps'] == 3
    assert caplog.text.count('one launch per interval (and staying with that form)') == 1
    assert [run(), run()] == ['intervals'] * 2
    assert eng.calls == [0, 4, 0, 1, 0] and script['sweeps'] == 3

    eng, script, run = _ladder_rig(8, fits=4, code=_lib.KH_ERR_UNSUPPORTED)
    assert [run(), run(), run()] == ['single'] * 3
    assert eng.calls == [0, 4] and eng.grid == 4 and script['sweeps'] == 4


def test_update_ladder_passes_real_errors_on():
    """Codes other than KH_ERR_TIMEOUT / KH_ERR_UNSUPPORTED are not the ladder's: from the sweep they propagate with no
    engine call and nothing remembered, from ``set_update_workgroups`` after the calls made so far."""
    from krotov_amd import _lib

    eng, script, run = _ladder_rig(8, fits=0, code=_lib.KH_ERR_HIP)
    with pytest.raises(_lib.KrotovHipError) as err:
        run()
    assert err.value.code == _lib.KH_ERR_HIP and eng.calls == [] and script['sweeps'] == 1
    script.update(fits=8, code=_lib.KH_ERR_TIMEOUT)
    assert run() == 'single' and eng.calls == []
    script.update(fits=4)  # ... and the first timeout after it is a first one: half the full grid
    assert run() == 'single' and eng.calls == [0, 4]

    eng, script, run = _ladder_rig(8, fits=0, invalid=(4,))
    with pytest.raises(_lib.KrotovHipError) as err:
        run()
    assert err.value.code == _lib.KH_ERR_INVALID and eng.calls == [0, 4] and script['sweeps'] == 1


def test_update_ladder_second_rung_below_the_engine_floor():
    """TODAY'S BEHAVIOUR, AS RECORDED -- and the finding of ADVICE.md (first item): 16 workgroups, the engine refuses
    fewer than 4, and 4 would fit.  Half (8) times out, the second rung asks for 8 // 4 = 2, which is refused, and the
    sweep goes to one launch per interval in every run; the grid of 4 that would have got through is never asked for.
    This is the one case that a change of the policy will edit."""
    eng, script, run = _ladder_rig(16, fits=4, floor=4)
    assert [run(), run(), run()] == ['intervals'] * 3
    assert eng.calls == [0, 8, 0, 2, 0] * 3 and 4 not in eng.calls
    assert script['sweeps'] == 2 * 3  # (the refused rung costs no sweep)


def test_update_ladder_strikes_are_consecutive():
    """Three sweeps IN A ROW that needed one launch per interval make that form permanent: one that got through in
    between starts the count again."""
    eng, script, run = _ladder_rig(8, fits=0)
    assert [run(), run()] == ['intervals'] * 2
    script.update(fits=8)
    assert run() == 'single'
    script.update(fits=0)
    assert [run(), run()] == ['intervals'] * 2
    before = script['sweeps']
    assert run() == 'intervals' and script['sweeps'] == before + 3  # (still tried: the third strike in a row)
    calls = list(eng.calls)
    assert run() == 'intervals' and script['sweeps'] == before + 3 and eng.calls == calls  # ... and now for good


def test_update_ladder_leaves_the_row_split_first(caplog):
    """A timed-out update sweep of an engine with ``row_split`` > 1: one workgroup per objective again -- once, logged at
    INFO, no grid asked for, no rung used up --; a timeout after that goes on to the rungs."""
    import logging

    caplog.set_level(logging.INFO, logger='krotov')
    eng, script, run = _ladder_rig(8, fits=8, row_split=2)
    assert run() == 'single' and eng.splits == [1] and eng.calls == [] and script['sweeps'] == 2
    info = [rec for rec in caplog.records if 'row split 2: the update sweep timed out' in rec.getMessage()]
    assert len(info) == 1 and info[0].levelno == logging.INFO and len(caplog.records) == 1

    eng, script, run = _ladder_rig(8, fits=4, row_split=2)
    assert run() == 'single' and eng.splits == [1] and eng.calls == [0, 4] and script['sweeps'] == 3
    assert run() == 'single' and eng.splits == [1] and eng.calls == [0, 4]


@pytest.mark.parametrize('second_order', [False, True])
def test_no_upload_between_the_backward_and_the_update_sweep(monkeypatch, second_order):
    """Every host-to-device upload of an iteration is issued BEFORE the backward sweep is launched (a copy from pageable
    memory is ordered behind the kernels in the stream and would keep the update sweep's launch back): between the
    return of ``engine.backward`` and the entry of ``engine.forward_update`` the backend hands no host array to
    ``engine.dev``, in three iterations of a first- and of a second-order run on the engine double (what the double
    uploads to itself inside its own methods happens outside that window)."""
    import torch

    import krotov_amd.engine as engine_mod
    from helpers import product_sigma
    from oracle_engine_double import OracleEngineDouble

    seen = {'window': False, 'uploads': [], 'sweeps': 0}

    class Watched(OracleEngineDouble):
        def dev(self, x, dtype):
            if seen['window'] and not isinstance(x, torch.Tensor):
                seen['uploads'].append(np.shape(x))
            return super().dev(x, dtype)

        def backward(self, *a, **kw):
            out = super().backward(*a, **kw)
            seen['window'] = True
            return out

        def forward_update(self, *a):
            seen['window'] = False
            seen['sweeps'] += 1
            return super().forward_update(*a)

    monkeypatch.setattr(engine_mod, 'HipKrotovEngine', Watched)
    spec = configs.config_c5(K=3, N=4, nt=9, L=2, distinct=True)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, propagator=krotov_amd.propagators.expm,
                               chi_constructor=krotov_amd.functionals.chis_re, iter_stop=3,
                               sigma=product_sigma() if second_order else None)
    assert seen['sweeps'] == 3 and seen['uploads'] == []


def test_bench_leg_traffic_is_keyed_on_the_build_and_scaled_per_interval(tmp_path, monkeypatch):
    """bench.py's ``pmc_traffic_leg``: counters of another build of the kernels are refused, bytes = (2 x FETCH_SIZE +
    WRITE_SIZE) x 1024 (the one convention), scaled from the profiled run's intervals to the leg's; the
    instantiation with the largest traffic stands for a kernel name without template arguments."""
    import json

    import bench

    prof = tmp_path / 'profiles'
    prof.mkdir()
    rec = {'_build': 'B1', '_convention': 'x',
           'K1024': {'_config': {'K': 1024, 'N': 64, 'nt': 501, 'L': 1, 'command': 'perf_sweeps.py 1024 64 501 1'},
                     'kh_ens_forward_update<2, false>': {'FETCH_SIZE': {'avg_per_launch': 1000.0, 'launches': 3},
                                                         'WRITE_SIZE': {'avg_per_launch': 48.0, 'launches': 3}},
                     'kh_ens_forward_update<2, true>': {'FETCH_SIZE': {'avg_per_launch': 10.0, 'launches': 1},
                                                        'WRITE_SIZE': {'avg_per_launch': 1.0, 'launches': 1}},
                     'kh_q2_sweep_store': {'FETCH_SIZE': {'avg_per_launch': 7.0, 'launches': 3}}}}
    (prof / 'pmc_tile_latest.json').write_text(json.dumps(rec))
    monkeypatch.setattr(bench, 'ROOT', str(tmp_path))
    monkeypatch.setattr(bench, 'build_id', lambda: 'B1')
    t, src = bench.pmc_traffic_leg('K1024', 'kh_ens_forward_update', 4000)
    assert t == (2 * 1000.0 + 48.0) * 1024.0 * 4000 / 500 and 'scaled to 4000' in src
    assert bench.pmc_traffic_leg('K1024', 'kh_q2_sweep_store', 4000)[0] is None  # (no WRITE_SIZE pass of that kernel)
    assert bench.pmc_traffic_leg('L4', 'kh_tile_forward_update', 4000)[0] is None
    monkeypatch.setattr(bench, 'build_id', lambda: 'B2')
    t, src = bench.pmc_traffic_leg('K1024', 'kh_ens_forward_update', 4000)
    assert t is None and 'another build' in src
    assert bench.pmc_traffic_leg('config4', 'kh_coop_forward_update', 1000) == (None, 'no profiles/pmc_config4_latest.json')


# ---- the run record both drivers keep (krotov_amd/_run.py), under scripted hooks and with no engine ------------------


def _record(iter_stop, **kw):
    from krotov_amd._run import RunRecord

    return RunRecord(dict(
        objectives=['objective'], adjoint_objectives=['adjoint'], lambda_vals=np.ones(1), shape_arrays=[np.ones(3)],
        tlist=np.linspace(0.0, 1.0, 4), propagator=None, chi_constructor=None, mu=None, sigma=None, iter_start=0,
        iter_stop=iter_stop), **kw)


def _drive(run, tau=lambda iteration: np.array([0.5 + 0.1j * iteration])):
    """The drivers' loop around ``run``: every iteration adds 1 to the one pulse; returns the Result."""
    guess = [np.zeros(3)]
    optimized = copy.deepcopy(guess)
    run.record_initial(['control'], 'mapping', guess, optimized, np.zeros(1), ['phi0'], tau(0), None, 0.0, 0.0)
    iteration = run.iter_start
    go_on = run.verdict(iteration)
    while go_on:
        iteration += 1
        assert iteration < 50, "the record never ends the run"
        optimized = [p + 1.0 for p in guess]
        run.record_iteration(iteration, None, None, None, ['phi%d' % iteration], guess, optimized, np.zeros(1),
                             tau(iteration), 0.0, 0.0)
        go_on = run.verdict(iteration, run.convergence())
        guess = optimized
    run.finish(optimized)
    return run.result


def test_run_record_lowered_iter_stop_ends_the_run_there():
    def lower(**kwargs):
        if kwargs['iteration'] == 1:
            run.static_args['iter_stop'] = 3

    run = _record(7, info_hook=lower)
    res = _drive(run)
    assert res.iters == [0, 1, 2, 3] and res.message == "Reached 3 iterations"
    assert run.range_stop == 7

    def lift(**kwargs):  # (the loop's own bound is the one fixed at the start, whatever a hook raises static_args to)
        run.static_args['iter_stop'] = 9

    run = _record(2, info_hook=lift)
    res = _drive(run)
    assert res.iters == [0, 1, 2] and res.message == "Reached 2 iterations"


@pytest.mark.parametrize('answer, message', [("tau is fine", "Reached convergence: tau is fine"),
                                             (True, "Reached convergence")])
def test_run_record_convergence_message(answer, message):
    res = _drive(_record(7, check_convergence=lambda result: answer if result.iters[-1] == 2 else None))
    assert res.iters == [0, 1, 2] and res.message == message
    assert len(res.optimized_controls[0]) == 4 and np.all(res.optimized_controls[0] == 2.0)  # (finish: on the time grid)


def test_run_record_iteration_count_goes_before_convergence():
    calls = []

    def hook(**kwargs):
        calls.append(('hook', kwargs['iteration']))

    def converged(result):
        calls.append(('check', result.iters[-1]))
        return "converged as well" if result.iters[-1] == 2 else None

    res = _drive(_record(2, info_hook=hook, check_convergence=converged))
    assert res.message == "Reached 2 iterations" and res.iters == [0, 1, 2]
    assert calls == [('hook', 0), ('hook', 1), ('check', 1), ('hook', 2), ('check', 2)]


def test_run_record_empty_loop_of_a_continued_run():
    first = _drive(_record(3, store_all_pulses=True))
    assert first.iters == [0, 1, 2, 3] and len(first.all_pulses) == 4
    seen = []

    def hook(**kwargs):
        seen.append((kwargs['iteration'], list(kwargs['info_vals'])))
        return 'never recorded'

    for iter_stop, said in [(3, 3), (2, 3)]:  # (the message: max(iter_start, iter_stop), iter_start the last one run)
        del seen[:]
        run = _record(iter_stop, continue_from=first, store_all_pulses=True, info_hook=hook)
        res = _drive(run)
        assert run.iter_start == 3 and res.message == "Reached %d iterations" % said
        assert res.iters == [0, 1, 2, 3] and len(res.all_pulses) == 4 and len(res.iter_seconds) == 4
        assert res.info_vals == [] and seen == [(0, [])]
    assert first.message == "Reached 3 iterations" and res is not first  # (the record works on a copy)
    # ... and one that does go on appends from the iteration after
    res = _drive(_record(5, continue_from=first, store_all_pulses=True))
    assert res.iters == [0, 1, 2, 3, 4, 5] and res.message == "Reached 5 iterations"


def test_run_record_tau_vals_and_info_vals_skip_none():
    res = _drive(_record(2, info_hook=lambda **kwargs: None if kwargs['iteration'] == 1 else kwargs['iteration']),
                 tau=lambda iteration: np.array([None, None]))
    assert res.tau_vals == [] and res.info_vals == [0, 2] and res.iters == [0, 1, 2]
    res = _drive(_record(2), tau=lambda iteration: np.array([None, 0.25 * iteration], dtype=object))
    assert [t[1] for t in res.tau_vals] == [0.0, 0.25, 0.5]  # (only ALL-None values are left out)


def test_run_record_store_all_pulses():
    run = _record(2, store_all_pulses=True)
    guess, first, second = [np.zeros(3)], [np.ones(3)], [np.full(3, 2.0)]
    run.record_initial(['control'], 'mapping', guess, copy.deepcopy(guess), np.zeros(1), ['phi'], np.array([0.5]), None,
                       0.0, 0.0)
    run.record_iteration(1, None, None, None, ['phi'], guess, first, np.zeros(1), np.array([0.5]), 0.0, 0.0)
    run.record_iteration(2, None, None, None, ['phi'], first, second, np.zeros(1), np.array([0.5]), 0.0, 0.0)
    stored = run.result.all_pulses
    assert len(stored) == 3 and stored[0] is guess  # (iteration 0: the guess itself)
    assert stored[1] is not first and stored[1][0] is not first[0] and np.array_equal(stored[1][0], first[0])
    first[0][:] = 7.0
    assert np.all(stored[1][0] == 1.0) and np.all(stored[2][0] == 2.0)
    assert run.result.optimized_controls is second
    assert _drive(_record(2)).all_pulses == []


def test_host_costates_norm_and_dimension():
    from krotov_amd._run import default_norm, host_costates

    asked = []

    def constructor(**kwargs):
        asked.append(list(kwargs))
        return [np.array([3.0, 4.0j]), np.array([0.0, 2.0])]

    def to_vector(chi, k):
        return chi if len(chi) == 2 else None

    chis, norms, vecs = host_costates(constructor, default_norm, to_vector, fw_states_T='phi', objectives='objs',
                                      tau_vals='tau')
    assert asked == [['fw_states_T', 'objectives', 'tau_vals']] and norms == [5.0, 2.0]
    assert np.array_equal(chis[0], np.array([3.0, 4.0j]) / 5.0) and np.array_equal(vecs[1], [0.0, 1.0])
    assert abs(np.linalg.norm(chis[0]) - 1.0) < 1e-15  # (a handful of roundings at 1.1e-16 each)
    chis, norms, _ = host_costates(constructor, lambda chi: 2.0, to_vector, fw_states_T='phi', objectives='objs',
                                   tau_vals='tau')
    assert norms == [2.0, 2.0] and np.array_equal(chis[0], [1.5, 2.0j])
    with pytest.raises(ValueError, match="chi_constructor returned states that do not match the state dimension"):
        host_costates(constructor, default_norm, lambda chi, k: None if k == 1 else chi, fw_states_T='phi',
                      objectives='objs', tau_vals='tau')

    class WithNorm:  # (a state type that brings its own norm)
        def norm(self):
            return 4.0

    assert default_norm(WithNorm()) == 4.0
