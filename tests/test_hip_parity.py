"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle,
the committed reference goldens, and size-independent properties at the full
BASELINE sizes.  fp64 tolerances: 1e-12 relative on pulses / 1e-12
on tau vs the oracle after 1-2 iterations of the small cases, 1e-9 vs dump goldens.
"""
import os

import numpy as np
import pytest

import krotov_amd
from krotov_amd import configs
from oracle import krotov_oracle as ko

import helpers
from helpers import CHI, golden, oracle_controls, oracle_optimize, spec_to_oracle

pytestmark = pytest.mark.gpu


def _engine(spec, **kw):
    from krotov_amd.engine import HipKrotovEngine

    ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    return HipKrotovEngine(ops, np.diff(spec.tlist), is_super=spec.is_super, **kw)


SMALL = {
    'c1': lambda: configs.config_c1(nt=200),
    'c2h': lambda: configs.config_c2_hilbert(nt=150),
    'c2l': lambda: configs.config_c2_liouville(nt=150),
    'c3': lambda: configs.config_c3(nt=301),
    'c4_d5': lambda: configs.config_c4(d=5, nt=101, n_logical=2),
    'c5_n16': lambda: configs.config_c5(K=6, N=16, nt=101),
    'c5_n12_L3': lambda: configs.config_c5(K=5, N=12, nt=81, L=3, distinct=True),
    'c5_n64': lambda: configs.config_c5(K=8, N=64, nt=61),
    'c5_n64_L2': lambda: configs.config_c5(K=4, N=64, nt=41, L=2, distinct=True),
    # per-objective operators with 64 < N <= 128: the generator in registers, N / 4 elements per lane (kh_tilen.h)
    'c5_n80': lambda: configs.config_c5(K=3, N=80, nt=31, L=2),
    'c5_n100': lambda: configs.config_c5(K=4, N=100, nt=21, L=1, distinct=True),
    'c5_n128': lambda: configs.config_c5(K=2, N=128, nt=11, L=1),
    'c5_n33': lambda: configs.config_c5(K=5, N=33, nt=41),
    # more objectives than CUs: two 256-thread workgroups per CU
    'c5_k300': lambda: configs.config_c5(K=300, N=16, nt=21, distinct=True),
    'c5_k300_ens': lambda: configs.config_c5(K=300, N=16, nt=21),  # one drift, scaled control operators: the ensemble kernel
    # more objectives than can be co-resident (one control: > 2 per CU; several controls: > 1 per CU): the update
    # sweep runs the streaming register-tile kernel (kh_tile64s.h: every workgroup walks through several objectives
    # per interval; 600 = 512 + 88: some workgroups own one objective, some two; 1100 with three controls: five and four)
    'c5_k600_distinct': lambda: configs.config_c5(K=600, N=8, nt=16, distinct=True),
    # ... the same at N = 64 (the instantiations with the immediate-offset tile loader: what K = 1024 x N = 64 runs)
    'c5_k520_n64_distinct': lambda: configs.config_c5(K=520, N=64, nt=6, distinct=True),
    'c5_k264_n64_L2': lambda: configs.config_c5(K=264, N=64, nt=6, L=2, distinct=True),
    # an ensemble proper (one drift, control operators mu_k H1: ensemble_objectives, objectives.py:1054-1094) with more
    # objectives than CUs: the matrix-core ensemble kernel (kh_ens.h), four objectives per workgroup
    'c5_k600': lambda: configs.config_c5(K=600, N=8, nt=16),
    'c5_k520_n64': lambda: configs.config_c5(K=520, N=64, nt=6),
    'c5_k300_L2': lambda: configs.config_c5(K=300, N=12, nt=16, L=2, distinct=True),
    'c5_k1100_L3': lambda: configs.config_c5(K=1100, N=6, nt=9, L=3),
    # objectives sharing one operator list, N > 64: the cooperative matrix-core kernels
    'c4_d9': lambda: configs.config_c4(d=9, nt=41, n_logical=2),
    'c4_d10_k9': lambda: configs.config_c4(d=10, nt=21, n_logical=3),
    'shared_n96_L2': lambda: configs.config_shared(K=20, N=96, nt=21, L=2),
    'shared_n300': lambda: configs.config_shared(K=16, N=300, nt=6, L=1),
}


@pytest.mark.parametrize('name', sorted(SMALL))
def test_sweeps_match_oracle(name):
    """Each of the three sweeps, called through the C ABI, vs the oracle's."""
    spec = SMALL[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    eng = _engine(spec)
    pulses = np.array(gp)
    # forward sweep with storage (optimize.py:302-313)
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    assert np.abs(states.cpu().numpy() - ref_states).max() < 1e-12
    assert np.abs(fw_T.cpu().numpy() - ref_T).max() < 1e-12
    tau = eng.tau(spec.target, fw_T).cpu().numpy()
    assert np.abs(tau - ko.tau_vals(prob, ref_T)).max() < 1e-12
    # backward sweep (optimize.py:413-425)
    chi_T = CHI[spec.chi](prob, ref_T, ko.tau_vals(prob, ref_T))
    norms = np.linalg.norm(chi_T, axis=1)
    chi_T = chi_T / norms[:, None]
    chi = eng.backward(chi_T, pulses)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    assert np.abs(chi.cpu().numpy() - ref_chi).max() < (1e-11 if name.startswith('c4_d') else 1e-12)
    # forward sweep with sequential update (optimize.py:444-508)
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    # the stiff N=25 Liouvillian amplifies round-off ~10x (the oracle's own Pade vs
    # SciPy's differ by 1.2e-12 there, tests/test_oracle_golden.py)
    tol = 1e-11 if name.startswith('c4_d') else 1e-12
    assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < tol * scale
    assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < tol
    assert np.abs(g_a.cpu().numpy() - ref_ga).max() < tol * max(1.0, np.abs(ref_ga).max())
    # the sweep cut at the cross-objective sum (multi-GPU form) with a 1-rank "all-reduce"
    opt2, psi2, ga2 = eng.forward_update_sharded(chi, norms, spec.init, pulses, np.array(S), np.array(lam),
                                                 lambda x: x)
    # (the per-interval path may run a different kernel family than the single launch)
    assert np.abs(opt2.cpu().numpy() - np.array(ref_opt)).max() < tol * scale
    assert np.abs(psi2.cpu().numpy() - ref_psi).max() < tol
    assert np.abs(ga2.cpu().numpy() - ref_ga).max() < tol * max(1.0, np.abs(ref_ga).max())
    assert np.abs((opt2 - opt).cpu().numpy()).max() < 1e-12 * scale
    assert eng.kernel.startswith(('tile64', 'mini', 'ens64')) == (spec.N <= 64)
    small = spec.N <= 16 and spec.K <= 8 and spec.L == 1
    quad = small and spec.N <= 4 and spec.K <= 4
    assert (eng.kernel == 'mini4/wave') == quad and (eng.kernel == 'mini16/wave') == (small and not quad)
    assert (eng.kernel == 'tile64/256') == (name == 'c5_k300')
    assert (eng.kernel == 'tile64/stream') == (name in ('c5_k600_distinct', 'c5_k300_L2', 'c5_k1100_L3',
                                                         'c5_k520_n64_distinct', 'c5_k264_n64_L2'))
    assert (eng.kernel == 'ens64/mfma') == (name in ('c5_k600', 'c5_k520_n64', 'c5_k300_ens'))
    assert (eng.kernel == 'coop16/mfma') == (name.startswith('c4_d') and spec.N > 64 or name.startswith('shared'))
    assert (eng.kernel == 'tile128/512') == (name in ('c5_n80', 'c5_n100', 'c5_n128'))
    eng.close()


@pytest.mark.parametrize('name', ['c4_d9', 'c4_d10_k9', 'shared_n300'])
def test_coop_update_sums_on_the_adjoint_side_vs_one_more_round(name, monkeypatch):
    """Cooperative kernels, one control, first order: the update sums as <H_1^+ chi | phi> -- H_1^+ chi for the whole
    co-state store by one block-sparse matrix-core pass in front of the sweep (kh_coop_adjoint_side; a diagonal
    commutator control in the transmon cases, a dense Hermitian one with a ragged last row block in 'shared_n300') --
    against the form with one more cross-workgroup round per interval (KH_COOP_NO_ADJ=1: what second order and two
    controls use).  Same pulses to rounding, and the adjoint-side sweep issues one product per interval less."""
    spec = SMALL[name]()
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 1.0 / (2 * spec.K))
    out = {}
    for flag in ('0', '1'):
        monkeypatch.setenv('KH_COOP_NO_ADJ', flag)
        eng = _engine(spec)
        assert eng.kernel == 'coop16/mfma'
        chi = eng.backward(chi_T, pulses)
        opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
        eng.check()
        out[flag] = (opt.cpu().numpy(), psi_T.cpu().numpy(), g_a.cpu().numpy(), eng.stats()['matvecs'])
        eng.close()
    scale = max(1.0, np.abs(out['1'][0]).max())
    assert np.abs(out['0'][0] - out['1'][0]).max() < 1e-13 * scale
    assert np.abs(out['0'][1] - out['1'][1]).max() < 1e-13
    assert np.abs(out['0'][2] - out['1'][2]).max() < 1e-13 * max(1.0, np.abs(out['1'][2]).max())
    intervals = len(spec.tlist) - 1
    assert out['1'][3] - out['0'][3] == pytest.approx(spec.K * intervals)  # one round per interval less


@pytest.mark.parametrize('name', ['c5_n16', 'c5_n64', 'c5_n64_L2', 'c5_n33'])
@pytest.mark.parametrize('kernel', ['generic', 'tile512', 'tile256'])
def test_kernel_families_agree(name, kernel, monkeypatch):
    """generic and both register-tile variants give the same sweeps (<= 1e-13)."""
    spec = SMALL[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    monkeypatch.setenv('KH_KERNEL', kernel)
    eng = _engine(spec)
    if kernel == 'generic':
        assert eng.kernel == 'generic'
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.37)
    chi = eng.backward(chi_T, pulses)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    assert np.abs(chi.cpu().numpy() - ref_chi).max() < 1e-12
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < 1e-12 * max(1.0, np.abs(np.array(ref_opt)).max())
    assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-12
    eng.close()


@pytest.mark.parametrize('name', ['c4_d9', 'c4_d10_k9', 'c5_n80', 'c5_n128'])
@pytest.mark.parametrize('kernel', ['tilen', 'generic'])
def test_register_generator_kernels_for_n_up_to_128(name, kernel, monkeypatch):
    """64 < N <= 128 with the generator in registers (kh_tilen.h; KH_KERNEL=tilen forces it also where the objectives
    share their operators and the cooperative kernels would run) and the generic kernels it replaces there: the three
    sweeps vs the oracle, Hilbert and Liouville space."""
    spec = SMALL[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    monkeypatch.setenv('KH_KERNEL', kernel)
    eng = _engine(spec)
    assert eng.kernel == ('tile128/512' if kernel == 'tilen' else 'generic')
    pulses = np.array(gp)
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    tol = 1e-11 if name.startswith('c4_d') else 1e-12
    assert np.abs(states.cpu().numpy() - ref_states).max() < tol
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.02 if name.startswith('c4_d') else 0.37)
    chi = eng.backward(chi_T, pulses)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    assert np.abs(chi.cpu().numpy() - ref_chi).max() < tol
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < tol * scale
    assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < tol
    assert np.abs(g_a.cpu().numpy() - ref_ga).max() < tol * max(1.0, np.abs(ref_ga).max())
    eng.close()
    if kernel == 'tilen':
        # (round 6) with the control operators not in registers the update sums above were taken on the adjoint side
        # (kh_gen_adjoint_side); the forward-side form of the same sweep
        monkeypatch.setenv('KH_GEN_ADJ', '0')
        eng = _engine(spec)
        opt0, psi0, _ = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
        eng.check()
        assert np.abs(opt0.cpu().numpy() - np.array(ref_opt)).max() < tol * scale
        assert np.abs(psi0.cpu().numpy() - ref_psi).max() < tol
        eng.close()


@pytest.mark.parametrize('L', [2, 3, 4])
def test_full_gpu_ensemble_with_several_controls_vs_oracle_and_generic(L, monkeypatch):
    """256 objectives (one workgroup per CU) with L = 2, 3, 4 controls: the register-tile update sweep gathers the L
    sums over all 256 slots with L waves side by side -- against the oracle on a short time grid (N = 24 keeps the
    oracle's 256 x 20 x 2 dense expm affordable) and against the generic kernels, which gather with one wave."""
    spec = configs.config_c5(K=256, N=24, nt=21, L=L, distinct=True)
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 1.0 / (2 * spec.K))
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    out = {}
    for kernel in ('tile', 'generic'):
        if kernel == 'generic':
            monkeypatch.setenv('KH_KERNEL', 'generic')
        eng = _engine(spec)
        assert eng.kernel == ('generic' if kernel == 'generic' else 'tile64/512')
        chi = eng.backward(chi_T, pulses)
        assert np.abs(chi.cpu().numpy() - ref_chi).max() < 1e-12
        opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
        eng.check()
        out[kernel] = opt.cpu().numpy()
        assert np.abs(out[kernel] - np.array(ref_opt)).max() < 1e-12 * scale
        assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-12
        assert np.abs(g_a.cpu().numpy() - ref_ga).max() < 1e-12 * max(1.0, np.abs(ref_ga).max())
        # bitwise repeatable (fixed summation order in every gathering wave)
        opt2, _, _ = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
        eng.check()
        assert np.array_equal(opt2.cpu().numpy(), out[kernel])
        eng.close()
    assert np.abs(out['tile'] - out['generic']).max() < 1e-13 * scale


TILEX_CASES = {
    # five to eight controls, N <= 64 (kh_tile64x.h): which operators are resident / streamed changes with L
    'L5_n64': lambda: configs.config_c5(K=4, N=64, nt=21, L=5),
    'L6_n20': lambda: configs.config_c5(K=5, N=20, nt=31, L=6, distinct=True),
    'L7_n33': lambda: configs.config_c5(K=3, N=33, nt=17, L=7, distinct=True),
    'L8_n64': lambda: configs.config_c5(K=4, N=64, nt=21, L=8, distinct=True),
    'L5_k260': lambda: configs.config_c5(K=260, N=6, nt=6, L=5),  # more objectives than CUs: plain sweeps in turns only
}


@pytest.mark.parametrize('name', sorted(TILEX_CASES))
def test_five_to_eight_controls_register_tiles(name, monkeypatch):
    """N <= 64 with 5 ... 8 controls (reference optimize.py:393-418, 444-508 loop over any number of pulses): the
    register-tile kernels with the operators beyond the CU's room streamed per interval (kh_tile64x.h) -- plain sweeps in
    both directions, the update sweep with its sums on the adjoint side, against the oracle; objectives without one of
    their controls (a register-resident one, an LDS-resident one, a streamed one: the engine's zero tile and a hole in
    the adjoint-side store); the second-order update and the per-interval form fall to the generic kernels on the same
    engine; ``KH_TX=0`` is the generic family throughout."""
    import torch

    from krotov_amd import _lib

    spec = TILEX_CASES[name]()
    if name == 'L6_n20':
        spec.Hc[2][5] = None   # streamed
        spec.Hc[0][3] = None   # in LDS
    if name == 'L7_n33':
        spec.Hc[1][1] = None   # in registers
        spec.Hc[2][6] = None   # streamed, fetched ahead
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses, Sa, lama = np.array(gp), np.array(S), np.array(lam)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.37 * min(1.0, 8.0 / spec.K))
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    _lib.forget_launched_kernels()
    eng = _engine(spec)
    assert eng.kernel == 'tile64x/512'
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    assert np.abs(states.cpu().numpy() - ref_states).max() < 1e-12
    assert np.abs(fw_T.cpu().numpy() - ref_T).max() < 1e-12
    chi = eng.backward(chi_T, pulses)
    assert np.abs(chi.cpu().numpy() - ref_chi).max() < 1e-12
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, Sa, lama)
    eng.check()
    assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < 1e-12 * scale
    assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-12
    assert np.abs(g_a.cpu().numpy() - ref_ga).max() < 1e-12 * max(1.0, np.abs(ref_ga).max())
    again = eng.forward_update(chi, norms, spec.init, pulses, Sa, lama)
    assert torch.equal(again[0], opt) and torch.equal(again[1], psi_T)  # (bitwise repeatable)
    launched = _lib.kernel_instantiations(launched_only=True)
    assert 'kh_tx_sweep_store<%d>' % spec.L in launched
    assert ('kh_tx_forward_update<%d>' % spec.L in launched) == (name != 'L5_k260')
    # one launch per interval (what a sharded sweep over RCCL runs): the generic kernels on the same engine
    opt2, psi2, _ = eng.forward_update_sharded(chi, norms, spec.init, pulses, Sa, lama, lambda t: None, graph_chunk=0)
    eng.check()
    assert np.abs(opt2.cpu().numpy() - np.array(ref_opt)).max() < 1e-12 * scale
    assert np.abs(psi2.cpu().numpy() - ref_psi).max() < 1e-12
    if name in ('L5_n64', 'L7_n33', 'L8_n64'):
        # second order (optimize.py:434-443, 468-469): the update sweep of the generic family, stores of this one
        rng = np.random.default_rng(5)
        sigma_vals = -(1.0 + rng.random(len(spec.tlist) - 1))
        prev = ref_states
        so_opt, so_psi, so_ga, so_store = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam, sigma_vals=sigma_vals,
                                                                  fw_prev=prev, store=True)
        store = torch.full((spec.K, len(spec.tlist), spec.N), float('nan'), dtype=torch.complex128, device=eng.device)
        eng.set_second_order(prev, store, sigma_vals)
        opt3, psi3, _ = eng.forward_update(chi, norms, spec.init, pulses, Sa, lama)
        eng.check()
        assert np.abs(opt3.cpu().numpy() - np.array(so_opt)).max() < 1e-12 * max(1.0, np.abs(np.array(so_opt)).max())
        assert np.abs(store.cpu().numpy() - so_store).max() < 1e-12
        eng.set_second_order()
    eng.close()
    # the switch
    monkeypatch.setenv('KH_TX', '0')
    gen = _engine(spec)
    assert gen.kernel == 'generic'
    chi_g = gen.backward(chi_T, pulses)
    assert float((chi_g - chi).abs().max()) < 1e-12
    opt_g = gen.forward_update(chi_g, norms, spec.init, pulses, Sa, lama)[0]
    gen.check()
    assert float((opt_g - opt).abs().max()) < 1e-12 * scale
    gen.close()


GEN_ADJ_CASES = {
    'L6_n20': lambda: configs.config_c5(K=5, N=20, nt=31, L=6, distinct=True),
    'L8_n64': lambda: configs.config_c5(K=4, N=64, nt=21, L=8),
    'L5_n100': lambda: configs.config_c5(K=3, N=100, nt=13, L=5, distinct=True),   # (N not a multiple of 16)
    'L2_n160': lambda: configs.config_c5(K=2, N=160, nt=7, L=2, distinct=True),    # (generator in the scratch matrix)
    'c4_d6': lambda: configs.config_c4(d=6, nt=41, n_logical=2),                    # Liouville space: mu = i dL/d eps
}


@pytest.mark.parametrize('name', sorted(GEN_ADJ_CASES))
def test_generic_update_sums_on_the_adjoint_side(name, monkeypatch):
    """Generic kernels, first order, dense operators (what problems with 5...8 controls and per-objective operators
    beyond N = 128 run): the update sums are taken as <H_l^+ chi_k(t_n) | phi_k(t_n)> with the left factors formed for the
    whole co-state store in front of the sweep (kh_gen_adjoint_side, fp64 matrix cores) instead of L streamed
    matrix-vector products per objective and interval (reference optimize.py:454-470).  Single launch and one launch per
    interval, against the oracle and against the forward-side form (``KH_GEN_ADJ=0``); one objective without its last
    control (a null operator: the store has a hole there and the sweep skips the sum)."""
    spec = GEN_ADJ_CASES[name]()
    if name == 'L6_n20':
        spec.Hc[2][5] = None
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses, Sa, lama = np.array(gp), np.array(S), np.array(lam)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.37)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    tol = 1e-11 if spec.is_super else 1e-12
    monkeypatch.setenv('KH_KERNEL', 'generic')
    out = {}
    for adj in ('1', '0'):
        monkeypatch.setenv('KH_GEN_ADJ', adj)
        eng = _engine(spec)
        assert eng.kernel == 'generic'
        chi = eng.backward(chi_T, pulses)
        for form in ('single', 'stepwise'):
            if form == 'single':
                opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, Sa, lama)
            else:
                opt, psi_T, g_a = eng.forward_update_sharded(chi, norms, spec.init, pulses, Sa, lama, lambda t: None,
                                                             graph_chunk=0)
            eng.check()
            out[adj, form] = opt.cpu().numpy()
            assert np.abs(out[adj, form] - np.array(ref_opt)).max() < tol * scale
            assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < tol
            assert np.abs(g_a.cpu().numpy() - ref_ga).max() < tol * max(1.0, np.abs(ref_ga).max())
        eng.close()
    assert np.array_equal(out['1', 'single'], out['1', 'stepwise'])
    assert np.abs(out['1', 'single'] - out['0', 'single']).max() < 1e-13 * scale


@pytest.mark.parametrize('name', ['c1', 'c2l', 'c3', 'c5_n64', 'c5_n33'])
def test_q2_update_forward_side_partial_sums(name, monkeypatch):
    """The q2 update sweep normally takes <chi|H phi> on the adjoint side when the control operators are
    +/- their own adjoints (Hermitian H_l: sign +1; commutator super-operators, c2l: sign -1).  KH_NO_ADJ=1
    keeps the forward-side kernel (the one non-Hermitian controls get): same results."""
    spec = SMALL[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.37)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    results = []
    monkeypatch.setenv('KH_KERNEL', 'q2')  # (the small cases would otherwise run the one-wave kernels)
    for no_adj in ('0', '1'):
        monkeypatch.setenv('KH_NO_ADJ', no_adj)
        eng = _engine(spec)
        assert eng.kernel == 'tile64q2/512'
        opt, psi_T, g_a = eng.forward_update(ref_chi, norms, spec.init, pulses, np.array(S), np.array(lam))
        eng.check()
        assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < 1e-12 * scale
        assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-12
        assert np.abs(g_a.cpu().numpy() - ref_ga).max() < 1e-12 * max(1.0, np.abs(ref_ga).max())
        results.append(opt.cpu().numpy())
        eng.close()
    assert np.abs(results[0] - results[1]).max() < 1e-13 * scale


@pytest.mark.parametrize('name', ['c1', 'c3', 'c5_n64', 'c5_n33'])
def test_q2_real_spectrum_series_vs_taylor(name, monkeypatch):
    """Hermitian generators (real spectrum) get the truncated-Chebyshev coefficients in the q2 kernels (two
    degrees fewer at the same tolerance); KH_TAYLOR=1 keeps plain Taylor coefficients.  Both match the oracle
    and each other; the shorter series issues fewer products."""
    spec = SMALL[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.37)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    out, issued = [], []
    monkeypatch.setenv('KH_KERNEL', 'q2')  # (the small cases would otherwise run the one-wave kernels)
    for taylor in ('0', '1'):
        monkeypatch.setenv('KH_TAYLOR', taylor)
        eng = _engine(spec)
        assert eng.kernel == 'tile64q2/512'
        chi = eng.backward(chi_T, pulses)
        assert np.abs(chi.cpu().numpy() - ref_chi).max() < 1e-12
        opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
        eng.check()
        assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < 1e-12 * scale
        assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-12
        out.append(opt.cpu().numpy())
        issued.append(eng.stats()['matvecs'])
        eng.close()
    assert np.abs(out[0] - out[1]).max() < 1e-13 * scale
    assert issued[0] <= issued[1]


@pytest.mark.parametrize('name', ['c2l', 'c4_d5', 'c4_d9', 'c4_d10_k9'])
def test_near_imaginary_spectrum_series_vs_taylor(name, monkeypatch):
    """Weakly damped Liouvillians: f A is anti-Hermitian up to a small Hermitian part of the drift, which the engine
    measures; the Chebyshev-form series then applies with a margin (kh_common.h; register-tile, one-wave and -- up
    to theta = 4 -- cooperative kernels).  KH_TAYLOR=1 keeps Taylor.  Both match the oracle and each other; the
    shorter series issues fewer products where the degree table has room for it."""
    spec = SMALL[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    # (||H_1|| ~ 1e2 and lambda_a = 1 in the transmon cases: keep the updated pulses O(1), as in
    # test_second_order_update_sweep, so that the problem stays well conditioned)
    norms = np.full(spec.K, 0.37 * (0.02 if name.startswith('c4_d') else 1.0))
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    tol = 1e-11 if name.startswith('c4_d') else 1e-12
    out, issued = [], []
    for taylor in ('0', '1'):
        monkeypatch.setenv('KH_TAYLOR', taylor)
        eng = _engine(spec)
        chi = eng.backward(chi_T, pulses)
        assert np.abs(chi.cpu().numpy() - ref_chi).max() < tol
        opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
        eng.check()
        assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < tol * scale
        assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < tol
        out.append(opt.cpu().numpy())
        issued.append(eng.stats()['matvecs'])
        eng.close()
    assert np.abs(out[0] - out[1]).max() < 10 * tol * scale
    assert issued[0] <= issued[1]
    if name in ('c4_d9', 'c4_d10_k9'):  # (cooperative kernels: the form reaches to theta = 4)
        assert issued[0] < issued[1]


def test_objective_propagate_on_device():
    """Objective.propagate with the GPU propagator = ONE forward sweep with storage; same states and expectation
    values as the host loop over a NumPy propagator (Hilbert space and a Liouvillian acting on a density matrix)."""
    import krotov_amd
    from helpers import numpy_plugins
    prop, _, _ = numpy_plugins()
    rng = np.random.default_rng(5)
    N = 6
    G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    H0 = (G + G.conj().T) / 4
    G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    H1 = (G + G.conj().T) / 8
    eps = lambda t, args: 0.7 * np.sin(3 * t) + 0.2  # noqa: E731
    psi0 = np.zeros(N, dtype=complex)
    psi0[0] = 1.0
    tlist = np.linspace(0, 4, 201)
    obj = krotov_amd.Objective(initial_state=psi0, target=psi0, H=[H0, [H1, eps]])
    host = obj.propagate(tlist, propagator=prop)
    dev = obj.propagate(tlist, propagator=krotov_amd.propagators.expm)
    assert dev.solver == 'expm' and len(dev.states) == len(tlist)
    assert max(np.abs(np.asarray(a) - b).max() for a, b in zip(dev.states, host.states)) < 1e-12
    P0 = np.zeros((N, N), dtype=complex)
    P0[0, 0] = 1.0
    dev_e = obj.propagate(tlist, propagator=krotov_amd.propagators.expm, e_ops=[P0, H0])
    host_e = obj.propagate(tlist, propagator=prop, e_ops=[P0, H0])
    assert len(dev_e.states) == 0
    assert np.abs(dev_e.expect[0] - host_e.expect[0]).max() < 1e-12
    assert np.abs(dev_e.expect[1] - host_e.expect[1]).max() < 1e-12
    # Liouville space: the unitary Liouvillian of the same system on rho = |psi><psi| reproduces the populations
    L0 = krotov_amd.objectives.liouvillian(H0, [])
    L1 = krotov_amd.objectives.liouvillian(H1, [])
    rho0 = np.outer(psi0, psi0.conj())
    obj_l = krotov_amd.Objective(initial_state=rho0, target=rho0, H=[L0, [L1, eps]])
    dev_l = obj_l.propagate(tlist, propagator=krotov_amd.propagators.HipExpm(liouville=True), e_ops=[P0])
    assert np.abs(dev_l.expect[0] - host_e.expect[0]).max() < 1e-11


ENS_CASES = {
    # name: (spec, KH_ENS_NCG, second order)
    'k40_n64_cg1': (lambda: configs.config_c5(K=40, N=64, nt=9), '1', False),
    'k37_n33_cg2': (lambda: configs.config_c5(K=37, N=33, nt=9), '2', False),   # ragged: the last workgroup owns one objective
    'k70_n64_cg4': (lambda: configs.config_c5(K=70, N=64, nt=7), '4', False),
    'k100_n16_cg8': (lambda: configs.config_c5(K=100, N=16, nt=7), '8', False),
    'k40_n64_cg1_so': (lambda: configs.config_c5(K=40, N=64, nt=9), '1', True),
    'k37_n33_cg2_so': (lambda: configs.config_c5(K=37, N=33, nt=9), '2', True),
    'k70_n64_cg4_so': (lambda: configs.config_c5(K=70, N=64, nt=7), '4', True),
    'k100_n16_cg8_so': (lambda: configs.config_c5(K=100, N=16, nt=7), '8', True),
    # Liouville space (mu = i dL/d eps, factor 1, non-Hermitian generator): three objectives under one operator list
    'c2l_cg1': (lambda: configs.config_c2_liouville(nt=60), '1', False),
    'c2l_cg2_so': (lambda: configs.config_c2_liouville(nt=60), '2', True),
    # norms large enough for several sub-steps per interval
    'k12_n20_substeps': (lambda: _c5_large_drift(), '2', False),
}


def _c5_large_drift():
    spec = configs.config_c5(K=12, N=20, nt=9)
    big = 6.0 * spec.H0[0]  # ||H0|| dt = 2.4: three sub-steps per interval
    spec.H0 = [big] * spec.K
    return spec


@pytest.mark.parametrize('name', sorted(ENS_CASES))
def test_ensemble_kernel_vs_oracle(name, monkeypatch):
    """kh_ens_forward_update<NCG, SO> (objectives sharing a drift and a control operator up to a real scale: the update
    sweep on the matrix cores, 2 NCG objectives per workgroup; optimize.py:444-508) vs the oracle, every column-group
    count, first and second order, Hilbert and Liouville space, ragged last workgroup, sub-stepped intervals; and the
    family the engine would have taken without it gives the same pulses."""
    import torch

    make, ncg, so = ENS_CASES[name]
    spec = make()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    monkeypatch.setenv('KH_ENS', '1')
    monkeypatch.setenv('KH_ENS_NCG', ncg)
    eng = _engine(spec)
    assert eng.kernel == 'ens64/mfma'
    pulses = np.array(gp)
    rng = np.random.default_rng(11)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = (0.2 + rng.random(spec.K)) * min(1.0, 8.0 / spec.K)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    chi = eng.backward(chi_T, pulses)
    kw = {}
    if so:
        older = [p * (1.0 + 0.2 * rng.standard_normal(p.shape)) for p in gp]
        _, prev = ko.forward_propagation(prob, older, store=True)
        sigma_vals = -(1.0 + rng.random(len(spec.tlist) - 1)) * min(1.0, 8.0 / spec.K)
        kw = dict(sigma_vals=sigma_vals, fw_prev=prev, store=True)
        store = torch.full((spec.K, len(spec.tlist), spec.N), float('nan'), dtype=torch.complex128, device=eng.device)
        eng.set_second_order(prev, store, sigma_vals)
    ref = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam, **kw)
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    scale = max(1.0, np.abs(np.array(ref[0])).max())
    assert np.abs(opt.cpu().numpy() - np.array(ref[0])).max() < 1e-12 * scale
    assert np.abs(psi_T.cpu().numpy() - ref[1]).max() < 1e-12
    assert np.abs(g_a.cpu().numpy() - ref[2]).max() < 1e-12 * max(1.0, np.abs(ref[2]).max())
    if so:
        assert np.abs(store.cpu().numpy() - ref[3]).max() < 1e-12
    if name.endswith('substeps'):
        assert eng.stats()['matvecs'] > 14 * spec.K * (len(spec.tlist) - 1)  # several sub-steps per interval
    eng_matvecs = eng.stats()['matvecs']
    eng.close()
    if not so and ncg == '2':
        # first order with four objectives per workgroup ran the A^2-chain form (kh_ens2_forward_update: [P0; P1; P2]
        # passes, update sums on the adjoint side); the term-by-term form of the same sweep (KH_ENS2=0)
        monkeypatch.setenv('KH_ENS2', '0')
        eng1 = _engine(spec)
        assert eng1.kernel == 'ens64/mfma'
        opt1, psi1, g1 = eng1.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
        eng1.check()
        assert np.abs(opt1.cpu().numpy() - np.array(ref[0])).max() < 1e-12 * scale
        assert np.abs(psi1.cpu().numpy() - ref[1]).max() < 1e-12
        assert np.abs(g1.cpu().numpy() - ref[2]).max() < 1e-12 * max(1.0, np.abs(ref[2]).max())
        assert eng1.stats()['matvecs'] > eng_matvecs  # (24 against 20 products per objective and step at degree 12)
        eng1.close()
        monkeypatch.delenv('KH_ENS2')
    # the same sweep without the ensemble kernel
    monkeypatch.setenv('KH_ENS', '0')
    eng0 = _engine(spec)
    assert eng0.kernel != 'ens64/mfma'
    if so:
        store0 = torch.empty_like(store)
        eng0.set_second_order(prev, store0, sigma_vals)
    opt0 = eng0.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))[0]
    eng0.check()
    assert np.abs((opt0 - opt).cpu().numpy()).max() < 1e-12 * scale
    eng0.close()


def test_ensemble_detection(monkeypatch):
    """The ensemble kernel is taken only for operator lists (H0, s_k H1): a perturbed control operator or a second
    drift leaves the engine with the streaming kernel, a drift that is an equal COPY still counts as shared."""
    spec = configs.config_c5(K=520, N=8, nt=5)
    assert _engine(spec).kernel == 'ens64/mfma'
    spec.H0 = [h.copy() for h in spec.H0]  # equal content, distinct arrays
    assert _engine(spec).kernel == 'ens64/mfma'
    bad = configs.config_c5(K=520, N=8, nt=5)
    bad.Hc[77] = [bad.Hc[77][0].copy()]
    bad.Hc[77][0][3, 4] *= 1.0 + 1e-12
    assert _engine(bad).kernel == 'tile64/stream'
    bad = configs.config_c5(K=520, N=8, nt=5)
    bad.H0[519] = bad.H0[519] + 1e-9 * np.eye(8)
    assert _engine(bad).kernel == 'tile64/stream'
    monkeypatch.setenv('KH_ENS', '0')
    assert _engine(spec).kernel == 'tile64/stream'


SECOND_ORDER_CASES = [
    ('c3', None), ('c5_n16', None), ('c3', 'mini'), ('c5_n64', None), ('c5_n64', 'tile512'), ('c5_n64', 'generic'), ('c5_n33', 'tile256'),
    ('c5_n64_L2', None), ('c5_n12_L3', None), ('c5_n80', None), ('c5_n80', 'generic'), ('c5_n100', None), ('c4_d9', 'tilen'), ('c2l', None),
    ('lindblad', 'sparse'), ('c5_n12_L3', 'sparse'), ('c5_k600', None), ('c5_k300_L2', None), ('c5_k600_distinct', None),
    ('c5_k264_n64_L2', None),
    ('c4_d9', None), ('shared_n96_L2', None), ('c3', 'coop'), ('shared_n96_L2', 'coop16cols'), ('shared_n96_L2', 'coop2cols'), ('c4_d9', 'coop2cols'),
]


@pytest.mark.parametrize('name,kernel', SECOND_ORDER_CASES)
def test_second_order_update_sweep(name, kernel, monkeypatch):
    """kh_set_second_order + the update sweep (reference optimize.py:434-443, 451-452,
    468-469, 492-500) in every kernel family vs the oracle: pulses, g_a, final and
    stored states, with phi_prev from a different pulse so that Delta phi != 0."""
    import torch

    spec = configs.config_sparse_lindblad() if name == 'lindblad' else SMALL[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    if kernel in ('coop16cols', 'coop2cols'):  # the cooperative kernels with 16 / 2 (instead of 4) objectives per workgroup
        monkeypatch.setenv('KH_COOP_COLS', kernel[4:-4])
    elif kernel is not None and kernel != 'sparse':
        monkeypatch.setenv('KH_KERNEL', kernel)
    if kernel == 'sparse':  # operators in CSR form: the matrix-in-registers kernels (kh_ell.h)
        from krotov_amd.engine import HipKrotovEngine

        eng = HipKrotovEngine(configs.sparse_ops(spec), np.diff(spec.tlist), is_super=spec.is_super)
        assert eng.kernel == 'ell/csr'
    else:
        eng = _engine(spec)
    pulses = np.array(gp)
    rng = np.random.default_rng(5)
    older = [p * (1.0 + 0.2 * rng.standard_normal(p.shape)) for p in gp]  # the "previous iteration"
    _, prev = ko.forward_propagation(prob, older, store=True)
    sigma_vals = -(1.0 + rng.random(len(spec.tlist) - 1))
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = 0.2 + rng.random(spec.K)
    if name.startswith(('c4_d', 'shared')):
        # (||H_1|| ~ 1e2..1e3 and lambda_a = 1, 2 there: keep the updated pulses O(1) so that the
        # problem stays well conditioned)
        norms *= 0.02
        sigma_vals *= 1e-3
    if name.startswith('c5_k'):  # (hundreds of objectives add up: same reason)
        norms *= 8.0 / spec.K
        sigma_vals *= 8.0 / spec.K
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    chi = eng.backward(chi_T, pulses)
    ref_opt, ref_psi, ref_ga, ref_store = ko.forward_update_sweep(
        prob, ref_chi, norms, gp, S, lam, sigma_vals=sigma_vals, fw_prev=prev, store=True)
    first_opt = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)[0]
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    assert np.abs(np.array(first_opt) - np.array(ref_opt)).max() > 1e-6 * scale  # the sigma term matters here
    store = torch.full((spec.K, len(spec.tlist), spec.N), float('nan'), dtype=torch.complex128, device=eng.device)
    eng.set_second_order(prev, store, sigma_vals)
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    tol = 1e-11 if name.startswith('c4_d') else 1e-12
    assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < tol * scale
    assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < tol
    assert np.abs(g_a.cpu().numpy() - ref_ga).max() < tol * max(1.0, np.abs(ref_ga).max())
    assert np.abs(store.cpu().numpy() - ref_store).max() < tol
    # per-interval (multi-GPU) form
    store.fill_(float('nan'))
    opt2, psi2, _ = eng.forward_update_sharded(chi, norms, spec.init, pulses, np.array(S), np.array(lam),
                                               lambda x: x)
    assert np.abs(opt2.cpu().numpy() - np.array(ref_opt)).max() < tol * scale
    assert np.abs(psi2.cpu().numpy() - ref_psi).max() < tol
    assert np.abs(store.cpu().numpy() - ref_store).max() < tol
    # and back to first order
    eng.set_second_order()
    opt1 = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))[0]
    assert np.abs(opt1.cpu().numpy() - np.array(first_opt)).max() < tol * scale
    from krotov_amd._lib import KrotovHipError

    with pytest.raises(KrotovHipError):
        eng.set_second_order(store, store, sigma_vals)
    eng.close()


def test_second_order_optimize_pulses_vs_reference_loop():
    """optimize_pulses(sigma=...) on the GPU vs the reference's second-order loop
    (tests/golden/ref_so_c3.npz) and the oracle; sigma.refresh sees the trajectories."""
    from helpers import SigmaA, product_sigma

    g = golden('ref_so_c3')
    spec = configs.config_c3(nt=201)
    spec.lambda_a = 20.0
    sig = product_sigma(0.0, 2.0)
    probe = {}

    def hook(**kw):
        if kw['iteration'] == 2:
            probe['fw'] = np.array(kw['forward_states'][1][57])
            probe['fw0'] = np.array(kw['forward_states0'][1][57])
            probe['len'] = (len(kw['forward_states']), len(kw['forward_states'][0]))

    res = _optimize_on_device(spec, int(g['iter_stop']), sigma=sig, info_hook=hook)
    got = np.array([np.array(p) for p in res.all_pulses])
    assert np.abs(got - g['all_pulses']).max() < 1e-9
    assert np.abs(np.array(res.tau_vals) - g['tau_vals']).max() < 1e-9
    assert np.abs(np.array(sig.history) - g['A_history']).max() < 1e-8
    assert sig.calls == [(spec.K, len(spec.tlist), True)] * 2
    osig = SigmaA(0.0, 2.0)
    ref = oracle_optimize(spec, int(g['iter_stop']), sigma=osig)
    assert np.abs(got - ref['all_pulses']).max() < 1e-12 * max(1.0, np.abs(ref['all_pulses']).max())
    assert np.abs(np.array(res.tau_vals) - ref['tau_vals']).max() < 1e-12
    # the trajectories handed to the hooks are those of iterations 2 and 1
    prob = spec_to_oracle(spec)
    assert probe['len'] == (spec.K, len(spec.tlist))
    for key, pulses in (('fw', got[2]), ('fw0', got[1])):
        want = ko.forward_propagation(prob, [pulses[0]], store=True)[1][1, 57]
        assert np.abs(probe[key].reshape(-1) - want).max() < 1e-12


def _tiled(spec, times):
    """The same objectives `times` times over (operators shared): more objectives than the GPU has CUs."""
    return configs.ProblemSpec(
        name=spec.name + '_x%d' % times, H0=list(spec.H0) * times, Hc=list(spec.Hc) * times, is_super=spec.is_super,
        init=np.tile(spec.init, (times, 1)), target=np.tile(spec.target, (times, 1)), tlist=spec.tlist,
        controls=spec.controls, update_shape=spec.update_shape, lambda_a=spec.lambda_a, chi=spec.chi)


def _banded(N, bands, nt, K=2):
    """Hermitian banded drift (`bands` diagonals) and a banded control on N levels: a sparse Hilbert-space problem."""
    rng = np.random.default_rng(11)
    half = bands // 2

    def band(width, scale):
        A = np.zeros((N, N), dtype=np.complex128)
        for d in range(width + 1):
            v = rng.standard_normal(N - d) + (1j * rng.standard_normal(N - d) if d else 0)
            A += np.diag(v, d) + (np.diag(v.conj(), -d) if d else 0)
        return scale * A / np.linalg.norm(A, 2)

    H0, H1 = band(half, 3.0), band(half - 1, 1.0)
    init = np.zeros((K, N), dtype=np.complex128)
    init[np.arange(K), np.arange(K)] = 1.0
    target = np.roll(init, 1, axis=1)
    T = 0.3
    return configs.ProblemSpec(
        name='banded_n%d' % N, H0=[H0] * K, Hc=[[H1]] * K, is_super=False, init=init, target=target,
        tlist=np.linspace(0, T, nt), controls=[lambda t, args: 0.7 * np.sin(np.pi * t / T) ** 2 + 0.1],
        update_shape=lambda t: 1.0, lambda_a=2.0, chi='re')


SPARSE_CASES = {
    # name: (spec, kernel family the engine picks by itself)
    'lindblad': (lambda: configs.config_sparse_lindblad(), 'ell/csr'),            # N = 144, ~7 entries per row
    'lindblad_n625': (lambda: configs.config_sparse_lindblad(d=25, nt=9, K=2), 'ell/csr'),   # two rows per lane (N > 512)
    'lindblad_n900': (lambda: configs.config_sparse_lindblad(d=30, nt=4, K=1), 'ell/csr'),   # 1024-thread form (N > 768, E <= 8)
    'banded_n800': (lambda: _banded(800, 11, nt=4), 'ell/csr'),   # two rows per lane of 512 threads (N > 768, 8 < E <= 16)
    'lindblad_k300': (lambda: _tiled(configs.config_sparse_lindblad(d=5, nt=13, K=5), 60), 'generic/csr'),  # more objectives than CUs
    'c5_n33': (lambda: SMALL['c5_n33'](), 'generic/csr'),                         # 33 entries per row: too wide for registers
    'c5_n12_L3': (lambda: SMALL['c5_n12_L3'](), 'ell/csr'),                       # three controls, distinct drifts, full rows
    'c5_n16': (lambda: SMALL['c5_n16'](), 'ell/csr'),                             # Hermitian: the real-spectrum series
}


@pytest.mark.parametrize('force_generic', [False, True])
@pytest.mark.parametrize('name', sorted(SPARSE_CASES))
def test_sparse_operator_sweeps(name, force_generic, monkeypatch):
    """kh_engine_create_csr: operators in CSR form (the regime of the
    reference's DensityMatrixODEPropagator, propagators.py:162-327) -- every sweep vs the oracle
    on sparse Lindbladians (~7 entries per row; one or two rows per lane) and on fully populated rows, through the
    matrix-in-registers kernels (kh_ell.h) and through the generic CSR kernels (KH_KERNEL=generic)."""
    from krotov_amd.engine import HipKrotovEngine

    builder, family = SPARSE_CASES[name]
    if force_generic:
        # (cases the engine runs on the generic kernels by itself: the switch must leave them there, same numbers)
        monkeypatch.setenv('KH_KERNEL', 'generic')
        family = 'generic/csr'
    spec = builder()
    ops = configs.sparse_ops(spec)
    if name == 'lindblad':
        assert ops[0][0].nnz < 0.06 * spec.N**2 and ops[0][0] is ops[1][0]
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    eng = HipKrotovEngine(ops, np.diff(spec.tlist), is_super=spec.is_super)
    assert eng.kernel == family
    pulses = np.array(gp)
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    assert np.abs(states.cpu().numpy() - ref_states).max() < 1e-12
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.4)
    chi = eng.backward(chi_T, pulses)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    assert np.abs(chi.cpu().numpy() - ref_chi).max() < 1e-12
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < 1e-12 * scale
    assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-12
    assert np.abs(g_a.cpu().numpy() - ref_ga).max() < 1e-12 * max(1.0, np.abs(ref_ga).max())
    opt2, psi2, _ = eng.forward_update_sharded(chi, norms, spec.init, pulses, np.array(S), np.array(lam), lambda x: x)
    assert np.abs(opt2.cpu().numpy() - np.array(ref_opt)).max() < 1e-12 * scale
    eng.close()


def test_sparse_liouvillian_of_dimension_4096():
    """The reference's ``DensityMatrixODEPropagator`` has no size limit (propagators.py:162-327); the register form of
    the sparse kernels ends at N = 2048 and the generic kernels' LDS vectors at N = 2540.  A d = 64 ladder (N = 4096, 5.9
    entries per row, two density matrices) must run -- the streamed padded-row kernels -- and give the sweeps of the
    oracle's restated zvode step at tight tolerances (1e-12 / 1e-14: the integrator's own error is ~1e-10 here) to
    1e-8; trace preservation to 1e-12 independently of any reference."""
    from krotov_amd.engine import HipKrotovEngine

    spec = configs.config_sparse_lindblad(d=64, nt=5, K=2)
    ops = configs.sparse_ops(spec)
    assert spec.N == 4096
    eng = HipKrotovEngine(ops, np.diff(spec.tlist), is_super=True)
    assert eng.kernel == 'ellstream/csr'
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    prob = ko.OracleProblem(ops, spec.init, spec.target, spec.tlist, is_super=True,
                            ode=dict(rtol=1e-12, atol=1e-14, nsteps=200000))
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    got = states.cpu().numpy()
    assert np.abs(got - ref_states).max() < 1e-8
    d = 64
    tr = got.reshape(spec.K, len(spec.tlist), d, d).trace(axis1=2, axis2=3)
    assert np.abs(tr - tr[:, :1]).max() < 1e-12
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.4)
    # (the backward sweep propagates with the adjoint Liouvillians: the oracle's ODE step takes them as given)
    adj = [[None if o is None else o.conj().T.tocsr() for o in row] for row in ops]
    prob_bw = ko.OracleProblem(adj, spec.init, spec.target, spec.tlist, is_super=True, ode=prob.ode)
    ref_chi = np.empty_like(ref_states)
    ref_chi[:, -1] = chi_T
    for n in range(len(spec.tlist) - 2, -1, -1):
        for k in range(spec.K):
            ref_chi[k, n] = ko.step_ode(prob_bw.ops[k], [p[n] for p in gp], spec.tlist[n + 1] - spec.tlist[n], ref_chi[k, n + 1], prob.ode)
    chi = eng.backward(chi_T, pulses)
    assert np.abs(chi.cpu().numpy() - ref_chi).max() < 1e-8
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < 1e-8 * scale
    assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-8
    eng.close()


def test_density_matrix_ode_propagator_drop_in():
    """optimize_pulses(propagator=DensityMatrixODEPropagator()) with scipy.sparse Liouvillians:
    sparse device path vs the oracle (and vs the dense device path)."""
    import scipy.sparse as sp

    spec = configs.config_sparse_lindblad(d=8, nt=41, K=3)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    made = {}
    for obj in objectives:  # the same nested lists, operators as scipy.sparse matrices
        for i, term in enumerate(obj.H):
            op = term[0] if isinstance(term, list) else term
            made.setdefault(id(op), (sp.csr_matrix(op), op))
            if isinstance(term, list):
                term[0] = made[id(op)][0]
            else:
                obj.H[i] = made[id(op)][0]
    kw = dict(chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2, store_all_pulses=True)
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist,
                                     propagator=krotov_amd.propagators.DensityMatrixODEPropagator(), **kw)
    from krotov_amd.engine import LAST_ENGINE

    assert LAST_ENGINE().kernel == 'ell/csr'
    ref = oracle_optimize(spec, 2)
    got = np.array([np.array(p) for p in res.all_pulses])
    assert np.abs(got - ref['all_pulses']).max() < 1e-12 * max(1.0, np.abs(ref['all_pulses']).max())
    assert np.abs(np.array(res.tau_vals) - ref['tau_vals']).max() < 1e-12
    dense = _optimize_on_device(spec, 2)
    assert np.abs(got - np.array([np.array(p) for p in dense.all_pulses])).max() < 1e-12
    assert np.asarray(res.states[0]).shape == np.asarray(objectives[0].initial_state).shape


def test_infohook_chaining_on_device():
    """reference tests/test_infohooks.py:15-72 with propagator=expm on the GPU: hooks that change
    lambda_a between iterations, chained return values, known answer 0.001978333994757067."""
    from helpers import check_infohook_chaining

    check_infohook_chaining(propagator=krotov_amd.propagators.expm)


@pytest.mark.parametrize('name', ['re', 'ss', 'sm', 'hs'])
def test_boundary_costates_on_device(name):
    """kh_chi_boundary vs the host form of krotov.functionals.chis_* (reference
    functionals.py:177-437) + the normalisation of optimize.py:407-410."""
    from krotov_amd import functionals

    spec = configs.config_c5(K=7, N=33, nt=5)
    rng = np.random.default_rng(11)
    eng = _engine(spec)
    fw = rng.standard_normal((spec.K, spec.N)) + 1j * rng.standard_normal((spec.K, spec.N))
    fw /= np.linalg.norm(fw, axis=1)[:, None]
    weights = 0.5 + rng.random(spec.K)
    tau = np.array([np.vdot(spec.target[k], fw[k]) for k in range(spec.K)])
    fn = getattr(functionals, 'chis_' + name)
    want = functionals.chi_stacked(fn, spec.target, weights, fw, tau)
    norms = np.linalg.norm(want, axis=1)
    c, d = functionals.chi_coefficients(fn, weights, tau, spec.K)
    chi, got_norms = eng.chi_boundary(spec.target, fw, c, d)
    assert np.abs(got_norms.cpu().numpy() - norms).max() < 1e-15
    assert np.abs(chi.cpu().numpy() - want / norms[:, None]).max() < 1e-15
    eng.close()


GOLDEN_CASES = {
    'ref_c1_tls': lambda: configs.config_c1(),
    'ref_c2_hilbert': lambda: configs.config_c2_hilbert(),
    'ref_c2_liouville': lambda: configs.config_c2_liouville(),
    'ref_c3_iswap': lambda: configs.config_c3(),
    'ref_c4_small': lambda: configs.config_c4(d=5, nt=201, n_logical=2),
    'ref_c5_small': lambda: configs.config_c5(K=6, N=16, nt=201, L=1),
    'ref_c5_small_L3': lambda: configs.config_c5(K=5, N=12, nt=151, L=3, distinct=True),
    'ref_c5_n64': lambda: configs.config_c5(K=8, N=64, nt=401, L=1),
    # chis_hs from the reference's own loop (functionals.py:389-437): chi_k(T) = w/2K (rho_tgt - rho(T))
    'ref_c4_small_hs': lambda: _with_chi(configs.config_c4(d=5, nt=201, n_logical=2), 'hs'),
    # one and two intervals (tests/helpers.py: SHORT_GRID_CASES)
    'ref_c5_nt2': lambda: helpers.short_grid_spec('ref_c5_nt2', configs),
    'ref_c5_nt3': lambda: helpers.short_grid_spec('ref_c5_nt3', configs),
    'ref_c3_nt2': lambda: helpers.short_grid_spec('ref_c3_nt2', configs),
}


def _with_chi(spec, chi):
    spec.chi = chi
    return spec


def _optimize_on_device(spec, iters, **kw):
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    prop = krotov_amd.propagators.HipExpm(liouville=True) if spec.is_super else krotov_amd.propagators.expm
    return krotov_amd.optimize_pulses(
        objectives, pulse_options, spec.tlist, propagator=prop,
        chi_constructor=getattr(krotov_amd.functionals, 'chis_' + spec.chi),
        iter_stop=iters, store_all_pulses=True, **kw)


def test_more_controls_than_the_kernels_take(caplog):
    """The reference takes any number of controls (optimize.py:33-55).  The register-resident kernel families are
    compiled for 8, the generic kernels for 32 (round 6: their per-control values live in LDS): 9, 17 and 32 controls stay
    on the device sweeps -- single launch with the sums gathered in groups of eight --; 33 must not raise either:
    ``optimize_pulses`` runs the host loop around single-interval propagations on the GPU.  All arrive at the oracle's
    pulses."""
    import logging

    from krotov_amd.engine import LAST_ENGINE

    for L, on_device in ((33, False), (32, True), (17, True), (9, True), (8, True)):
        spec = configs.config_c5(K=3 if L > 9 else 2, N=6, nt=7, L=L, distinct=True)
        caplog.clear()
        caplog.set_level(logging.WARNING, logger='krotov')
        res = _optimize_on_device(spec, 2)
        ref = oracle_optimize(spec, 2)
        got = np.array([np.array(p) for p in res.all_pulses])
        assert got.shape[1] == L
        assert np.abs(got - ref['all_pulses']).max() < 1e-12 * max(1.0, np.abs(ref['all_pulses']).max())
        assert np.abs(np.array(res.tau_vals) - ref['tau_vals']).max() < 1e-12
        assert ('host loop around single-step' in caplog.text) == (not on_device)
        if on_device:
            # (five to eight controls at N <= 64: the register-tile kernels with streamed operators, kh_tile64x.h)
            assert LAST_ENGINE().kernel == ('tile64x/512' if L <= 8 else 'generic') and LAST_ENGINE().L == L


def test_seventeen_controls_every_form_of_the_generic_update():
    """More than eight controls at engine level (generic kernels): single launch over 20 workgroups (in-kernel exchange in
    groups of eight controls), one launch per interval, adjoint-side and forward-side sums, second order -- the oracle's
    pulses, final states and g_a integrals in every form."""
    spec = configs.config_c5(K=20, N=10, nt=9, L=17, distinct=True)
    spec.Hc[3][16] = None
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses, Sa, lama = np.array(gp), np.array(S), np.array(lam)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.linspace(0.2, 0.5, spec.K)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    for adj in ('1', '0'):
        os.environ['KH_GEN_ADJ'] = adj
        try:
            eng = _engine(spec)
            assert eng.kernel == 'generic'
            chi = eng.backward(chi_T, pulses)
            assert np.abs(chi.cpu().numpy() - ref_chi).max() < 1e-12
            for form in ('single', 'stepwise'):
                if form == 'single':
                    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, Sa, lama)
                else:
                    opt, psi_T, g_a = eng.forward_update_sharded(chi, norms, spec.init, pulses, Sa, lama, lambda t: None,
                                                                 graph_chunk=0)
                eng.check()
                assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < 1e-12 * scale
                assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-12
                assert np.abs(g_a.cpu().numpy() - ref_ga).max() < 1e-12 * max(1.0, np.abs(ref_ga).max())
            eng.close()
        finally:
            os.environ.pop('KH_GEN_ADJ', None)
    # second order (forward-side sums with the folded bra)
    fw_T, fw_prev = None, None
    eng = _engine(spec)
    fw_T, fw_prev = eng.forward(pulses, spec.init, store=True)
    sig = np.full(len(spec.tlist) - 1, -3.0)
    import torch

    fw_store = torch.empty_like(fw_prev)
    eng.set_second_order(fw_prev, fw_store, sig)
    chi = eng.backward(chi_T, pulses)
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, Sa, lama)
    eng.check()
    so_opt, so_psi, so_ga, so_states = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam, sigma_vals=sig,
                                                               fw_prev=fw_prev.cpu().numpy(), store=True)
    assert np.abs(opt.cpu().numpy() - np.array(so_opt)).max() < 1e-12 * max(1.0, np.abs(np.array(so_opt)).max())
    assert np.abs(fw_store.cpu().numpy() - so_states).max() < 1e-12
    eng.close()


@pytest.mark.parametrize('cols', ['2', '4', '16'])
@pytest.mark.parametrize('name', ['ref_c2_liouville', 'ref_c3_iswap', 'ref_c4_small'])
def test_cooperative_kernels_vs_reference_loop_goldens(name, cols, monkeypatch):
    """The shared-operator matrix-core kernels (forced onto the small gate problems whose
    objectives share one operator list; 2, 4 and 16 objectives per workgroup) vs the
    reference's own loop."""
    monkeypatch.setenv('KH_KERNEL', 'coop')
    monkeypatch.setenv('KH_COOP_COLS', cols)
    g = golden(name)
    res = _optimize_on_device(GOLDEN_CASES[name](), int(g['iter_stop']))
    from krotov_amd.engine import LAST_ENGINE

    assert LAST_ENGINE().kernel == 'coop16/mfma'
    got = np.array([np.array(p) for p in res.all_pulses])
    assert np.abs(got - g['all_pulses']).max() < 1e-9
    assert np.abs(np.array(res.tau_vals) - g['tau_vals']).max() < 1e-9


@pytest.mark.parametrize('name', sorted(GOLDEN_CASES))
def test_optimize_pulses_vs_reference_loop_goldens(name):
    """optimize_pulses(propagator=expm) on the GPU vs the outputs of the
    reference's own optimize_pulses on the same inputs (committed fixtures)."""
    g = golden(name)
    spec = GOLDEN_CASES[name]()
    res = _optimize_on_device(spec, int(g['iter_stop']))
    got = np.array([np.array(p) for p in res.all_pulses])
    tol = 1e-10 if name == 'ref_c4_small_hs' else (2e-11 if name == 'ref_c4_small' else 2e-12)
    scale = max(1.0, np.abs(g['all_pulses']).max())
    assert np.abs(got - g['all_pulses']).max() < tol * scale
    assert np.abs(np.array(res.tau_vals) - g['tau_vals']).max() < tol
    fw_T = np.array([np.asarray(s).ravel(order='F') for s in res.states])
    assert np.abs(fw_T - g['fw_T']).max() < tol
    assert np.abs(np.array(res.optimized_controls) - g['optimized_controls']).max() < tol * scale


FULL5_CASES = {
    # fixture: (spec, kernel the engine must pick, tolerance)
    'ref_c5_full5': (lambda: configs.config_c5(), 'tile64q2/512', 1e-10),
    'ref_c4_full5': (lambda: configs.config_c4(), 'coop16/mfma', 1e-9),
}


@pytest.mark.parametrize('name', sorted(FULL5_CASES))
def test_full_size_five_iterations_vs_reference_loop(name):
    """SURVEY.md 8d's acceptance at FULL size: BASELINE config 5 (256 x N = 64 x 4000 intervals) and config 4 (16 density
    matrices, 400-dim Liouvillian, 1000 intervals) through ``optimize_pulses`` on the GPU for as many iterations as the
    fixture holds (five; tests/golden/make_reference_goldens.py c5full5 / c4full5: the reference's own loop, 2.7 / 3.7
    CPU-hours) -- the pulses after EVERY iteration, tau of every objective after every iteration, the final states.  A
    lost fixture fails the test."""
    import krotov_amd.engine as engine_mod

    make, kernel, tol = FULL5_CASES[name]
    g = golden(name)
    iters = int(g['iter_stop'])
    assert iters == 5
    spec = make()
    res = _optimize_on_device(spec, iters)
    assert engine_mod.LAST_ENGINE().kernel == kernel
    got = np.array([np.array(p) for p in res.all_pulses])
    assert got.shape == g['all_pulses'].shape
    scale = max(1.0, np.abs(g['all_pulses']).max())
    for i in range(iters + 1):  # (per iteration: a drift that grows with the iteration count shows where it starts)
        assert np.abs(got[i] - g['all_pulses'][i]).max() < tol * scale, 'pulses after iteration %d' % i
        assert np.abs(np.array(res.tau_vals[i]) - g['tau_vals'][i]).max() < tol, 'tau after iteration %d' % i
    fw_T = np.array([np.asarray(s).ravel(order='F') for s in res.states])
    assert np.abs(fw_T - g['fw_T']).max() < tol


@pytest.mark.parametrize('name,ncg', [('ref_c5_n64', '1'), ('ref_c5_n64', '2'), ('ref_c5_small', '4')])
def test_ensemble_kernel_vs_reference_loop_goldens(name, ncg, monkeypatch):
    """The matrix-core ensemble kernel (kh_ens.h; forced onto the small robustness ensembles with KH_ENS=1) through
    ``optimize_pulses`` vs the outputs of the reference's own loop on the same inputs (2e-12 vs
    ``ref_c5_n64``)."""
    import krotov_amd.engine as engine_mod

    monkeypatch.setenv('KH_ENS', '1')
    monkeypatch.setenv('KH_ENS_NCG', ncg)
    g = golden(name)
    spec = GOLDEN_CASES[name]()
    res = _optimize_on_device(spec, int(g['iter_stop']))
    assert engine_mod.LAST_ENGINE().kernel == 'ens64/mfma'
    got = np.array([np.array(p) for p in res.all_pulses])
    scale = max(1.0, np.abs(g['all_pulses']).max())
    assert np.abs(got - g['all_pulses']).max() < 2e-12 * scale
    assert np.abs(np.array(res.tau_vals) - g['tau_vals']).max() < 2e-12
    fw_T = np.array([np.asarray(s).ravel(order='F') for s in res.states])
    assert np.abs(fw_T - g['fw_T']).max() < 2e-12


def test_tls_dump_18_iterations_on_device():
    """reference tests/test_result_serialization/oct_result.dump: every pulse of
    all 18 iterations (4.5k sequential steps each way per iteration) to 1e-9."""
    g = golden('dump_tls_ss')
    res = _optimize_on_device(configs.config_c1(), len(g['iters']) - 1)
    got = np.array([np.array(p) for p in res.all_pulses])
    assert np.abs(got[0] - g['all_pulses'][0]).max() == 0.0
    assert np.abs(got - g['all_pulses']).max() < 1e-9
    assert np.abs(np.array(res.tau_vals)[:, 0] - g['tau_vals'][:, 0]).max() < 1e-9
    assert np.abs(got - g['all_pulses']).max() < 1e-11  # measured ~1e-13


def test_continue_from_reference_dump_on_device():
    """An optimisation the reference ran and dumped (QuTiP objects inside; read by Result.load without QuTiP) is
    continued on the GPU: iterations 19 and 20 as if all 20 had run here."""
    import os
    spec = configs.config_c1()
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    path = os.path.join(os.path.dirname(__file__), 'golden', 'reference_tls_oct_result.dump')
    loaded = krotov_amd.result.Result.load(path, objectives=objectives)
    kw = dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_ss,
              store_all_pulses=True, iter_stop=20)
    cont = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, continue_from=loaded, **kw)
    scratch = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, **kw)
    assert list(cont.iters) == list(range(21))
    assert np.abs(np.array(cont.all_pulses[19:]) - np.array(scratch.all_pulses[19:])).max() < 1e-9
    assert np.abs(np.array(cont.tau_vals[19:]) - np.array(scratch.tau_vals[19:])).max() < 1e-9


def test_transmon17_dump_on_device():
    """reference docs/notebooks/transmonxgate_opt_result.dump, iterations 5 -> 8."""
    g = golden('dump_transmon17')
    H0, H1, psi0, psi1 = g['H0'], g['H1'], g['psi0'], g['psi1']
    ctrl = g['controls_it5'][0].copy()
    H = [H0, [H1, ctrl]]
    objs = [krotov_amd.Objective(initial_state=psi0, target=psi1, H=H),
            krotov_amd.Objective(initial_state=psi1, target=psi0, H=H)]
    S = lambda t: krotov_amd.shapes.flattop(t, 0.0, 10.0, 0.5, func='sinsq')  # noqa: E731
    res = krotov_amd.optimize_pulses(
        objs, {id(ctrl): dict(lambda_a=1.0, update_shape=S)}, g['tlist'],
        propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_re, iter_stop=3)
    tau = np.array(res.tau_vals)
    sgn = np.sign((tau[0] * np.conj(g['tau_vals'][5])).real)
    assert np.abs(sgn * tau[0] - g['tau_vals'][5]).max() < 1e-8
    # (tau is fixed by the committed states: a flipped sign would be a different problem, not a phase convention)
    assert np.all(sgn > 0)
    assert np.abs(tau - g['tau_vals'][5:9]).max() < 1e-8


def test_ensemble_dump_on_device():
    """reference docs/notebooks/ensemble_opt_result.dump: K=5, N=3, L=4, it. 12 -> 16."""
    g = golden('dump_ensemble')
    ctrls = [c.copy() for c in g['controls_it12']]
    T = g['tlist'][-1]
    S = lambda t: krotov_amd.shapes.flattop(t, 0.0, T, 0.3, func='sinsq')  # noqa: E731
    objs = []
    psi0 = np.array([1, 0, 0], dtype=complex)
    for mu in g['mu']:
        H = [g['H0']] + [[mu * g['Hc'][l], ctrls[l]] for l in range(4)]
        objs.append(krotov_amd.Objective(initial_state=psi0, target=g['target'], H=H))
    opts = {id(c): dict(lambda_a=float(g['lambda_a']), update_shape=S) for c in ctrls}
    res = krotov_amd.optimize_pulses(objs, opts, g['tlist'], propagator=krotov_amd.propagators.expm,
                                     chi_constructor=krotov_amd.functionals.chis_re, iter_stop=4)
    assert np.abs(np.array(res.tau_vals) - g['tau_vals'][12:17]).max() < 1e-9


def _lambda_dump_on_device(g, controls, lambda_a, iters):
    """The Lambda system of the reference's notebooks 02 / 03 (one objective, N = 3, four controls) from a dump
    fixture's controls, `iters` iterations on the GPU."""
    ctrls = [np.array(c, dtype=np.float64) for c in controls]
    T = g['tlist'][-1]
    S = lambda t: krotov_amd.shapes.flattop(t, 0.0, T, 0.3, func='sinsq')  # noqa: E731
    H = [g['H0']] + [[g['Hc'][l], ctrls[l]] for l in range(4)]
    obj = krotov_amd.Objective(initial_state=np.array([1, 0, 0], dtype=complex), target=g['target'], H=H)
    opts = {id(c): dict(lambda_a=lambda_a, update_shape=S) for c in ctrls}
    return krotov_amd.optimize_pulses([obj], opts, g['tlist'], propagator=krotov_amd.propagators.expm,
                                      chi_constructor=krotov_amd.functionals.chis_re, iter_stop=iters)


def test_nonherm_dump_on_device():
    """reference docs/notebooks/non_herm_opt_result.dump, iterations 40 -> 45: H0 has an anti-Hermitian part (decay of
    the intermediate level), so this is the fixture that pins the backward step exp(+i H^dagger dt) -- on
    the device through the adjoint operators the engine stages, and through the Taylor series (no real spectrum)."""
    g = golden('dump_nonherm')
    res = _lambda_dump_on_device(g, g['controls_it40'], float(g['lambda_a']), 5)
    assert np.abs(np.array(res.tau_vals) - g['tau_vals'][40:46]).max() < 1e-9
    from krotov_amd.engine import LAST_ENGINE

    assert LAST_ENGINE().kernel.startswith('tile64')


@pytest.mark.parametrize('kernel', [None, 'generic'])
def test_nonherm_dump_kernel_families(kernel, monkeypatch):
    """... and the same through the generic kernels (the register-tile family runs by default)."""
    if kernel is not None:
        monkeypatch.setenv('KH_KERNEL', kernel)
    g = golden('dump_nonherm')
    res = _lambda_dump_on_device(g, g['controls_it40'], float(g['lambda_a']), 2)
    assert np.abs(np.array(res.tau_vals) - g['tau_vals'][40:43]).max() < 1e-9


def test_lambda_rwa_dump_on_device():
    """reference docs/notebooks/lambda_rwa_opt_result.dump: all 12 iterations from the true guess (N = 3, L = 4)."""
    g = golden('dump_lambda_rwa')
    res = _lambda_dump_on_device(g, g['guess_controls'], 0.5, 12)
    assert np.abs(np.array(res.tau_vals) - g['tau_vals']).max() < 1e-9
    # and where the reference ended up: its optimized controls (on the time grid)
    assert np.abs(np.array(res.optimized_controls) - g['optimized_controls']).max() < 1e-8


def _three_states_problem():
    """The reference's notebook 06 from tests/golden/dump_3states.npz: two coupled 5-level transmons in Liouville space
    (625-dim sparse Liouvillian, 4.8-6.4 entries per row), sqrt(iSWAP) by the three-states method with weights, two
    controls (Re / Im of the drive), 2000 grid points; controls at iteration 3 of the reference's run."""
    import scipy.sparse as sp

    g = golden('dump_3states')
    N = int(g['N'])
    L = [sp.csr_matrix((g['L%d_data' % i], g['L%d_indices' % i], g['L%d_indptr' % i]), shape=(N, N)) for i in range(3)]
    ctrls = [np.array(c, dtype=np.float64) for c in g['controls_it3']]
    T = g['tlist'][-1]
    S = lambda t: krotov_amd.shapes.flattop(t, 0.0, T, float(g['t_rise']))  # noqa: E731  (notebook cell 50)
    objs = []
    for k in range(3):
        obj = krotov_amd.Objective(initial_state=g['rho0'][k], target=g['rho_tgt'][k], H=[L[0], [L[1], ctrls[0]], [L[2], ctrls[1]]])
        obj.weight = float(g['weights'][k])
        objs.append(obj)
    opts = {id(c): dict(lambda_a=float(g['lambda_a']), update_shape=S) for c in ctrls}
    return g, objs, opts


def test_three_states_dump_sparse_propagator_on_device():
    """reference docs/notebooks/3states_opt_result.dump -- the reference's ONE result for its
    DensityMatrixODEPropagator (propagators.py:162-327) -- iterations 3 -> 6 on the CSR path of the engine
    (kh_engine_create_csr).  Two comparisons:
    * with the dump itself.  The reference integrates with zvode at rtol 1e-6 / atol 1e-8 and is itself only good to
      ~1e-4 after 2 000 steps (its tau of iteration 3 is 7.6e-5 off the converged value, 1.5e-4 at iteration 6), while
      the engine takes the exact exponential action: agreement to 5e-4, the solver's accuracy;
    * with the SAME propagator at tightened tolerances (rtol 1e-11 / atol 1e-13; `tau_tight_it3/4` of the fixture, from
      the oracle's restatement of the zvode step, which reproduces the dump at the default tolerances to 2e-12,
      tests/test_oracle_golden.py): 1e-8 -- the difference to the dump is the reference's integration error, not the
      engine's."""
    g, objs, opts = _three_states_problem()
    res = krotov_amd.optimize_pulses(
        objs, opts, g['tlist'], propagator=krotov_amd.propagators.DensityMatrixODEPropagator(reentrant=True),
        chi_constructor=krotov_amd.functionals.chis_re,
        info_hook=krotov_amd.info_hooks.print_table(J_T=krotov_amd.functionals.J_T_re, out=open(os.devnull, 'w')),
        iter_stop=3)
    from krotov_amd.engine import LAST_ENGINE

    assert LAST_ENGINE().kernel == 'ell/csr'
    tau = np.array(res.tau_vals)
    d_dump = np.abs(tau - g['tau_vals'][3:7]).max()
    d_J = np.abs(np.array(res.info_vals) - g['info_vals'][3:7]).max()
    d_tight = max(np.abs(tau[0] - g['tau_tight_it3']).max(), np.abs(tau[1] - g['tau_tight_it4']).max())
    print("3states: max |d tau| vs dump %.2e, |d J_T| %.2e; vs the tight-tolerance propagator %.2e" % (d_dump, d_J, d_tight))
    assert d_dump < 5e-4 and d_J < 5e-4
    assert d_tight < 1e-8
    # the optimisation moves by more than the comparison's tolerance: iteration 6 is not iteration 3
    assert np.abs(g['tau_vals'][6] - g['tau_vals'][3]).max() > 1.5e-3


def test_runs_are_bitwise_repeatable():
    spec = configs.config_c5(K=24, N=64, nt=101)
    a = _optimize_on_device(spec, 2)
    b = _optimize_on_device(spec, 2)
    assert np.array_equal(np.array(a.all_pulses), np.array(b.all_pulses))
    assert np.array_equal(np.array(a.tau_vals), np.array(b.tau_vals))


def test_edge_cases(monkeypatch):
    from krotov_amd.engine import HipKrotovEngine

    rng = np.random.default_rng(5)
    # non-uniform dt, control absent from one objective, more objectives than CUs: 300 -> two 256-thread
    # workgroups per CU (register tiles), 600 -> the streaming register-tile kernel (kh_tile64s.h), or (KH_NO_STREAM=1) the
    # register-tile kernel with one launch per interval, or (KH_NO_STEPWISE=1) the generic kernels' persistent loop
    # (the plain sweeps of such engines run kh_q2_sweep_store, objectives in turns; the second K = 300 case keeps the
    # update sweep's own family for them: KH_Q2_STORE=0)
    for K, kernel, q2_store in ((300, 'tile64/256', True), (300, 'tile64/256', False), (600, 'tile64/stream', True),
                                (600, 'tile64/512 per interval', True), (600, 'generic', True)):
        if kernel == 'generic':
            monkeypatch.setenv('KH_NO_STEPWISE', '1')
        if kernel == 'tile64/512 per interval':
            monkeypatch.setenv('KH_NO_STREAM', '1')
        else:
            monkeypatch.delenv('KH_NO_STREAM', raising=False)
        if q2_store:
            monkeypatch.delenv('KH_Q2_STORE', raising=False)
        else:
            monkeypatch.setenv('KH_Q2_STORE', '0')
        N, nt = 6, 21
        tl = np.cumsum(np.concatenate([[0.0], rng.uniform(0.01, 0.05, nt - 1)]))
        H0 = [configs.herm(rng, N, 3.0) for _ in range(K)]
        H1 = configs.herm(rng, N, 1.0)
        ops = [[H0[k], (None if k == 7 else H1)] for k in range(K)]
        init = rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))
        init /= np.linalg.norm(init, axis=1)[:, None]
        target = np.roll(init, 1, axis=0)
        prob = ko.OracleProblem(ops, init, target, tl)
        gp = [0.3 * np.sin(np.arange(nt - 1))]
        S = [np.ones(nt - 1)]
        eng = HipKrotovEngine(ops, np.diff(tl))
        assert eng.kernel == kernel
        chi_T = target / np.linalg.norm(target, axis=1)[:, None]
        norms = np.full(K, 1.0 / (2 * K))
        chi = eng.backward(chi_T, np.array(gp))
        ref_chi = ko.backward_sweep(prob, chi_T, gp)
        assert np.abs(chi.cpu().numpy() - ref_chi).max() < 1e-12
        opt, psi_T, g_a = eng.forward_update(chi, norms, init, np.array(gp), np.array(S), np.array([2.0]))
        eng.check()
        ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, [2.0])
        assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < 1e-12
        assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-12
        eng.close()
    monkeypatch.delenv('KH_NO_STEPWISE')
    monkeypatch.delenv('KH_Q2_STORE', raising=False)
    # N = 1 and a large step norm (several Taylor sub-steps)
    ops1 = [[np.array([[2.5 + 0j]]), np.array([[40.0 + 0j]])]]
    eng = HipKrotovEngine(ops1, [0.5, 0.25])
    out = eng.forward(np.array([[0.3, -0.2]]), np.array([[1.0 + 0j]])).cpu().numpy()
    want = np.exp(-1j * (2.5 + 40 * 0.3) * 0.5) * np.exp(-1j * (2.5 - 40 * 0.2) * 0.25)
    assert abs(out[0, 0] - want) < 1e-13
    eng.close()
    # the single-step drop-in of krotov.propagators.expm, forwards / backwards / Liouville
    H = [H0[0], [H1, 0.7]]
    v = init[0]
    got = krotov_amd.propagators.expm(H, v.reshape(-1, 1), 0.03)
    assert got.shape == (N, 1)
    assert np.abs(got.ravel() - ko.step([H0[0], H1], [0.7], 0.03, v)).max() < 1e-13
    got = krotov_amd.propagators.expm(H, v, 0.03, backwards=True)
    assert np.abs(got - ko.step([H0[0], H1], [0.7], 0.03, v, backwards=True)).max() < 1e-13
    rho = np.outer(v, v.conj())
    Ls = [configs.liouvillian_dense(H0[0]), [configs.liouvillian_dense(H1), 0.7]]
    got = krotov_amd.propagators.expm(Ls, rho, 0.03)
    U = ko.expm_pade13(-1j * (H0[0] + 0.7 * H1) * 0.03)
    assert got.shape == (N, N) and np.abs(got - U @ rho @ U.conj().T).max() < 1e-13
    with pytest.raises(NotImplementedError):
        krotov_amd.propagators.expm(H, v, 0.03, c_ops=[H1])


def test_unitary_liouville_cross_check():
    """Liouville-space expm has no reference golden: propagating
    rho = |psi><psi| with L = -i[H, .] must equal the Hilbert-space result."""
    spec_h = configs.config_c3(nt=201)
    eng_h = _engine(spec_h)
    gp, _, _ = oracle_controls(spec_h)
    psi_T = eng_h.forward(np.array(gp), spec_h.init).cpu().numpy()
    L0 = configs.liouvillian_dense(spec_h.H0[0])
    L1 = configs.liouvillian_dense(spec_h.Hc[0][0])
    from krotov_amd.engine import HipKrotovEngine

    eng_l = HipKrotovEngine([[L0, L1]] * 4, np.diff(spec_h.tlist), is_super=True)
    rho0 = np.array([np.outer(p, p.conj()).ravel(order='F') for p in spec_h.init])
    rho_T = eng_l.forward(np.array(gp), rho0).cpu().numpy()
    want = np.array([np.outer(p, p.conj()).ravel(order='F') for p in psi_T])
    assert np.abs(rho_T - want).max() < 1e-12


def test_full_size_c5_properties():
    """BASELINE config 5 at full size (K=256, N=64, 4000 intervals): properties
    that need no oracle run -- norm conservation, and <chi(t_n)|phi(t_n)> constant
    in n when both sweeps use the same pulses (U^dagger U = 1 step by step)."""
    import torch

    spec = configs.config_c5()
    eng = _engine(spec)
    assert eng.kernel.startswith('tile64')
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    nrm = torch.linalg.vector_norm(states, dim=2)
    assert float((nrm - 1).abs().max()) < 1e-11
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    chi = eng.backward(chi_T, pulses)
    ov = (chi.conj() * states).sum(dim=2)  # (K, nt)
    assert float((ov - ov[:, -1:]).abs().max()) < 1e-10
    # tau from the kernel equals the stored overlap at t = T
    tau = eng.tau(spec.target, fw_T)
    assert float((tau - ov[:, -1]).abs().max()) < 1e-13
    del states, ov
    # one update sweep: finite, shape-limited, and exactly reproducible
    norms = np.full(spec.K, 1.0 / (2 * spec.K))
    a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    b = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    opt = a[0].cpu().numpy()
    assert np.all(np.isfinite(opt)) and opt[0, 0] == pulses[0, 0] and opt[0, -1] == pulses[0, -1]
    assert float((torch.linalg.vector_norm(a[1], dim=1) - 1).abs().max()) < 1e-11
    # one iteration of the reference's own optimize_pulses loop at full size (tests/golden/README.md): a lost
    # fixture fails the test, it does not skip the comparison
    g = golden('ref_c5_full')
    assert np.abs(opt - g['all_pulses'][1]).max() < 1e-10
    tau1 = eng.tau(spec.target, a[1]).cpu().numpy()
    assert np.abs(tau1 - g['tau_vals'][1]).max() < 1e-10
    eng.close()


FULL_SIZE_LEGS = {
    # what bench.py publishes next to the headline, at the sizes it publishes them
    'L4': (dict(L=4), 'tile64/512'),
    'distinct': (dict(distinct=True), 'tile64q2/512'),
    'N96': (dict(N=96), 'tile128/512'),
    'K1024': (dict(K=1024), 'ens64/mfma'),
    'K1024_distinct': (dict(K=1024, distinct=True), 'tile64/stream'),
}


@pytest.mark.parametrize('leg', sorted(FULL_SIZE_LEGS))
def test_full_size_published_legs_properties(leg, monkeypatch):
    """The side legs of the bench line at FULL size (4000 intervals): no oracle finishes there, so
    size-independent properties -- norms conserved along the stored trajectory, <chi(t_n)|phi(t_n)> constant in n,
    tau = the stored overlap at T, the update sweep bitwise repeatable and shape-limited -- and the first 200 intervals
    of the update sweep against the GENERIC kernels on the same co-states (the sequential update of interval n depends
    on intervals <= n only, so a prefix is a complete problem of its own)."""
    import torch

    kw, want_kernel = FULL_SIZE_LEGS[leg]
    spec = configs.config_c5(**kw)
    eng = _engine(spec)
    assert eng.kernel == want_kernel
    gp, S, lam = oracle_controls(spec)
    pulses, S, lam = np.array(gp), np.array(S), np.array(lam)
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    assert float((torch.linalg.vector_norm(states, dim=2) - 1).abs().max()) < 1e-11
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    chi = eng.backward(chi_T, pulses)
    ov = (chi.conj() * states).sum(dim=2)  # (K, nt)
    assert float((ov - ov[:, -1:]).abs().max()) < 1e-10
    assert float((eng.tau(spec.target, fw_T) - ov[:, -1]).abs().max()) < 1e-13
    del states, ov
    norms = np.full(spec.K, 1.0 / (2 * spec.K))
    a = eng.forward_update(chi, norms, spec.init, pulses, S, lam)
    eng.check()
    b = eng.forward_update(chi, norms, spec.init, pulses, S, lam)
    eng.check()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    opt = a[0].cpu().numpy()
    assert np.all(np.isfinite(opt)) and np.array_equal(opt[:, 0], pulses[:, 0]) and np.array_equal(opt[:, -1], pulses[:, -1])
    assert np.abs(opt - pulses).max() > 1e-6  # (the sweep did update)
    assert float((torch.linalg.vector_norm(a[1], dim=1) - 1).abs().max()) < 1e-11
    # the 200-interval prefix on the generic kernels: same operators, same co-states, same guess
    n_pre = 200
    chi_pre = chi[:, :n_pre + 1].contiguous()
    eng.close()
    del chi, a, b
    monkeypatch.setenv('KH_KERNEL', 'generic')
    from krotov_amd.engine import HipKrotovEngine

    ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    gen = HipKrotovEngine(ops, np.diff(spec.tlist)[:n_pre], is_super=False)
    assert gen.kernel == 'generic'
    g_opt, _, _ = gen.forward_update(chi_pre, norms, spec.init, pulses[:, :n_pre].copy(), S[:, :n_pre].copy(), lam)
    gen.check()
    scale = max(1.0, np.abs(opt).max())
    assert np.abs(g_opt.cpu().numpy() - opt[:, :n_pre]).max() < 1e-12 * scale
    gen.close()


def _two_rank_spec(case):
    """'c5': per-objective operators, register-tile kernels; 'c4': objectives sharing one
    operator list with N > 64 (BASELINE config 4's shape, small): cooperative matrix-core
    kernels, 4 density matrices per rank; 'c4so': the same with the second-order update."""
    if case == 'c5':
        spec = configs.config_c5(K=6, N=64, nt=61, L=1)
        spec.chi = 'sm'
        return spec
    if case == 'c5nt3':  # two intervals (the peer-window epochs advance once per interval), constant update shape and a
        spec = configs.config_c5(K=6, N=64, nt=3, L=1)  # guess that is non-zero on the grid: the update is no no-op
        spec.chi = 'sm'
        spec.update_shape = lambda t: 1.0
        spec.controls = [lambda t, args: 0.5 * (0.4 + 0.6 * t * 2000.0)]
        return spec
    if case == 'c3':  # small problem: the one-wave-per-objective kernels, 2 + 2 objectives
        return configs.config_c3(nt=301)
    if case == 'k1100':  # 550 objectives per rank: not co-resident, so no in-kernel exchange -- the peer windows
        spec = configs.config_c5(K=1100, N=6, nt=13, L=1, distinct=True)  # are refused and every interval is a launch + all-reduce
        spec.chi = 'sm'
        return spec
    if case == 'k1100ens':  # the same as an ensemble proper (one drift, scaled control operators): 550 objectives per rank
        spec = configs.config_c5(K=1100, N=6, nt=13, L=1)  # on the matrix-core ensemble kernel, sums through the peer windows
        spec.chi = 'sm'
        return spec
    if case == 'c4k25':  # 13 + 12 objectives per rank: two objectives per cooperative workgroup (7 + 6 column groups)
        return configs.config_c4(d=9, nt=31, n_logical=5)
    if case in ('c5w8', 'c5w5'):  # BASELINE config 5's 8-GPU partition: 8 x 32 objectives of N = 64 -- 256 workgroups, one
        # per CU; as 52 + 4 x 51 on five ranks, the most that share one device (MAX_RANKS_SHARING_A_GPU)
        spec = configs.config_c5(K=256, N=64, nt=25, L=1)
        spec.chi = 'sm'
        return spec
    if case == 'c5w4':  # ... and its 4-GPU partition cut down to 4 x 9 (uneven shards: 36 = 9 + 9 + 9 + 9; L = 1)
        spec = configs.config_c5(K=38, N=64, nt=41, L=1)  # 38 -> 10 + 10 + 9 + 9
        return spec
    if case in ('c4w4', 'c4w8', 'c4w5'):  # BASELINE config 4's partition: 16 density matrices as 4 x 4 / 8 x 2 / 4 + 4 x 3 (N = 81 here)
        return configs.config_c4(d=9, nt=41, n_logical=4)
    if case == 'sparse':  # sparse Liouvillians through DensityMatrixODEPropagator: the matrix-in-registers kernels, 2 + 2
        return configs.config_sparse_lindblad(d=9, nt=41, K=4)
    if case == 'n80':  # per-objective operators, N = 80, two controls: the register-generator kernels, 3 + 3 objectives
        return configs.config_c5(K=6, N=80, nt=31, L=2)
    if case == 'L6':  # six controls at N = 48: register tiles with a streamed operator (kh_tile64x.h), 3 + 2 objectives
        return configs.config_c5(K=5, N=48, nt=25, L=6, distinct=True)
    if case == 'c4full':  # BASELINE config 4 at full size (debugging the 8-rank bench leg; not in a test list)
        return configs.config_c4()
    if case == 'c5w4L2':  # two controls (one-term-per-phase kernels), 4 x 5
        return configs.config_c5(K=20, N=64, nt=31, L=2, distinct=True)
    return configs.config_c4(d=9, nt=41, n_logical=3)  # N = 81, K = 9 -> 5 + 4 objectives


def _rank_placement(rank, world):
    """(device index, backend, one_device_per_rank) of a test rank: with at least ``world`` GPUs in the box every rank
    gets its own device and the host collectives are RCCL (``nccl``) -- the sums then cross xGMI through real peer
    windows --; with fewer (the one-GPU box these tests were written on) the ranks share devices round-robin and gloo
    moves the tensors through the host (RCCL refuses two ranks on one device).  The same rule as bench.py."""
    import torch

    n_dev = max(1, torch.cuda.device_count())
    own = n_dev >= world
    return rank % n_dev, os.environ.get('KH_DIST_BACKEND', 'nccl' if own else 'gloo'), own


# Ranks that share one device each hold it from a process of their own, and the test process holds it too.  The suite
# keeps to at most six processes on a GPU at once (shared GPU nodes stop a run beyond that): up to five ranks share a
# device (world 5 covers the one-device protocol beyond four ranks), more ranks need a device each.
MAX_PROCESSES_ON_A_GPU = 6
MAX_RANKS_SHARING_A_GPU = MAX_PROCESSES_ON_A_GPU - 1


def _skip_unless_devices_for(world):
    """Skip (before any work) a test of ``world`` ranks that would put more than MAX_RANKS_SHARING_A_GPU of them on one
    device: it then needs a GPU per rank."""
    import torch

    n_dev = torch.cuda.device_count()
    if world > MAX_RANKS_SHARING_A_GPU and n_dev < world:
        pytest.skip("needs %d GPUs (one per rank), found %d: %d ranks sharing one GPU would be %d processes on it, more "
                    "than the %d the suite keeps to" % (world, n_dev, world, world + 1, MAX_PROCESSES_ON_A_GPU))


def _two_rank_worker(rank, world, port, queue, case='c5'):
    """One of ``world`` ranks (see _rank_placement: one GPU each where the box has them, else sharing the single GPU with
    gloo moving the CUDA tensors through the host): the real multi-rank device path -- peer windows inside the
    persistent kernels, or kh_update_begin/step/end with an all-reduce per interval; tau / state all-gathers."""
    import os
    import sys

    import torch
    import torch.distributed as dist

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    from test_hip_parity import _rank_placement

    dev, backend, own_device = _rank_placement(rank, world)
    torch.cuda.set_device(dev)
    if not own_device:
        os.environ.setdefault('KH_COOP_XCD', '0')  # (ranks sharing a device must not claim the same XCDs: DESIGN.md 4)
    if backend == 'nccl':
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', dev))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        import krotov_amd as ka
        from krotov_amd import configs as cfg

        from test_hip_parity import _two_rank_spec

        spec = _two_rank_spec(case)
        objectives, pulse_options = cfg.spec_to_objectives(spec, ka)
        prop = ka.propagators.HipExpm(liouville=True) if spec.is_super else ka.propagators.expm
        if case == 'sparse':
            import scipy.sparse as sp

            made = {}
            for obj in objectives:  # the same nested lists, operators as scipy.sparse matrices
                for i, term in enumerate(obj.H):
                    op = term[0] if isinstance(term, list) else term
                    made.setdefault(id(op), (sp.csr_matrix(op), op))
                    if isinstance(term, list):
                        term[0] = made[id(op)][0]
                    else:
                        obj.H[i] = made[id(op)][0]
            prop = ka.propagators.DensityMatrixODEPropagator()
        extra = {}
        if case == 'c4so':
            from helpers import product_sigma

            extra['sigma'] = product_sigma(0.0, 2e-3)  # (||L_1|| ~ 1e2: keeps the pulses O(1))
        res = ka.optimize_pulses(
            objectives, pulse_options, spec.tlist, propagator=prop,
            chi_constructor=getattr(ka.functionals, 'chis_' + spec.chi), iter_stop=2, store_all_pulses=True,
            process_group=dist.group.WORLD, **extra)
        import krotov_amd.engine as engine_mod

        eng = engine_mod.LAST_ENGINE()
        used_p2p = bool(getattr(eng, '_p2p_used', False))
        if used_p2p and getattr(eng, '_p2p_fell_back', False):
            used_p2p = 'fallback'  # (peer windows first, then -- after a failed sweep -- the per-interval transport)
        try:
            p2p = eng.p2p_stats() if used_p2p else None
        except Exception as exc:
            p2p = {'error': repr(exc)[:200]}
        diag = {'device': dev, 'backend': dist.get_backend(), 'own_device': own_device, 'world': dist.get_world_size(),
                'p2p': p2p, 'why': getattr(eng, 'p2p_why', None)}
        queue.put((rank, np.array(res.all_pulses), np.array(res.tau_vals), used_p2p, eng.kernel, diag))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('case', ['c5', 'c5nt3', 'c3', 'c4', 'c4so', 'c4k25', 'k1100', 'k1100ens', 'n80', 'L6', 'sparse'])
def test_two_ranks_sharded_on_one_gpu(case):
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    queue = ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, queue, case)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted([queue.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    spec = _two_rank_spec(case)
    if case == 'c4so':
        from helpers import SigmaA

        ref = oracle_optimize(spec, 2, sigma=SigmaA(0.0, 2e-3))
    else:
        ref = oracle_optimize(spec, 2)
    tol = 1e-12 if case in ('c5', 'c5nt3', 'c3', 'k1100', 'k1100ens', 'n80', 'L6', 'sparse') else 1e-11  # (stiff Liouvillian, as in test_sweeps_match_oracle)
    for _, pulses, tau, used_p2p, kernel, _diag in out:
        assert np.abs(pulses - ref['all_pulses']).max() < tol * max(1.0, np.abs(ref['all_pulses']).max())
        assert np.abs(tau - ref['tau_vals']).max() < tol
        assert kernel == {'c5': 'tile64q2/512', 'c5nt3': 'tile64q2/512', 'c3': 'mini4/wave', 'k1100': 'tile64/stream', 'k1100ens': 'ens64/mfma',
                          'n80': 'tile128/512', 'L6': 'tile64x/512', 'sparse': 'ell/csr'}.get(case, 'coop16/mfma')
    assert np.array_equal(out[0][1], out[1][1])
    if case == 'c5nt3':  # (both intervals move in the first iteration)
        assert np.abs(ref['all_pulses'][1] - ref['all_pulses'][0]).min() > 1e-6
    # the path this test is here for: the sums crossed the ranks inside the persistent kernels, through the
    # peer-mapped windows -- not through the per-interval fallback
    if case == 'k1100':
        assert not any(o[3] for o in out)
        _check_placement(out, 2, windows=False)
    elif os.environ.get('KH_P2P', '1') != '0':
        assert all(o[3] for o in out), "peer-window exchange was not used: %r" % ([(o[3], o[5]['why']) for o in out],)
        _check_placement(out, 2, windows=True)


def _run_ranks(world, case, env=None, timeout=600):
    """`world` ranks sharing the one GPU (spawned processes, gloo for the host collectives); returns their records
    (rank, all_pulses, tau_vals, used_p2p, kernel, diag) in rank order."""
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})  # (spawned children inherit the environment)
    try:
        ctx = mp.get_context('spawn')
        queue = ctx.Queue()
        procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, queue, case)) for r in range(world)]
        for p in procs:
            p.start()
        out = sorted([queue.get(timeout=timeout) for _ in range(world)], key=lambda t: t[0])
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def _check_placement(out, world, windows):
    """What a box with one GPU per rank must show (nothing to assert where the ranks share a device): every rank on its
    own device, RCCL underneath ``torch.distributed`` with ``world`` ranks, and -- when the sums went through the peer
    windows -- ``kh_p2p_stats`` reporting ``world`` ranks and a non-zero wait between publishing this GPU's sum and
    holding every GPU's (the cross-GPU hop: over xGMI here)."""
    import torch

    diags = [o[5] for o in out]
    assert all(d['world'] == world for d in diags)
    if torch.cuda.device_count() < world:
        assert not any(d['own_device'] for d in diags)
        return False
    assert sorted(d['device'] for d in diags) == list(range(world)), diags
    assert all(d['own_device'] and d['backend'] == 'nccl' for d in diags), diags
    if windows:
        for d in diags:
            assert d['p2p'] is not None and 'error' not in d['p2p'], d
            assert d['p2p']['ranks'] == world and d['p2p']['cross_gpu_wait_us'] > 0.0, d
    return True


@pytest.mark.parametrize('case,world', [('c5w8', 8), ('c5w4', 4), ('c4w4', 4), ('c4w8', 8), ('c5w4L2', 4), ('c5w5', 5),
                                        ('c4w5', 5)])
def test_ranks_sharded_on_one_gpu_world_4_and_8(case, world):
    """BASELINE's partitions at world = 4 and 8: config 5 as 8 x 32 objectives of N = 64 -- its
    256 workgroups are co-resident on the one MI355X, so the whole cross-rank protocol (IPC windows opened by 7 peers,
    system-scope publication by each rank's leader, every workgroup polling its own window, epochs across sweeps) runs
    for real, minus the xGMI link --, config 4's 16 density matrices as 4 x 4 and 8 x 2.  All ranks must arrive at
    bit-identical pulses, within 1e-12 of the oracle, and through the peer windows.  World 8 needs a GPU per rank
    (MAX_RANKS_SHARING_A_GPU); on one device the same partitions run as five ranks (c5w5: 52 + 4 x 51 objectives,
    c4w5: 4 + 4 x 3 density matrices)."""
    _skip_unless_devices_for(world)
    out = _run_ranks(world, case)
    spec = _two_rank_spec(case)
    ref = oracle_optimize(spec, 2)
    tol = 1e-12 if case.startswith('c5') else 1e-11
    want_kernel = {'c5w8': 'tile64q2/512', 'c5w5': 'tile64q2/512', 'c5w4': 'tile64q2/512',
                   'c5w4L2': 'tile64/512'}.get(case, 'coop16/mfma')
    assert len(out) == world
    for _, pulses, tau, used_p2p, kernel, _diag in out:
        assert np.abs(pulses - ref['all_pulses']).max() < tol * max(1.0, np.abs(ref['all_pulses']).max())
        assert np.abs(tau - ref['tau_vals']).max() < tol
        assert kernel == want_kernel
        assert np.array_equal(pulses, out[0][1]) and np.array_equal(tau, out[0][2])
    if os.environ.get('KH_P2P', '1') != '0':
        assert all(o[3] for o in out), "peer-window exchange was not used: %r" % ([(o[3], o[5]['why']) for o in out],)
        _check_placement(out, world, windows=True)


@pytest.mark.parametrize('case,world,fail_rank', [('c5w4', 4, 2), ('c4w4', 4, 0)])
def test_exchange_timeout_mid_sweep_falls_back_on_all_ranks(case, world, fail_rank):
    """Fault injection: KH_P2P_FAIL_AT=<interval> makes the leader workgroup of rank
    KH_P2P_FAIL_RANK withhold its GPU's sum at that interval of the SECOND update sweep -- every rank's kernel then
    runs into the bound of its wait, kh_check reports KH_ERR_TIMEOUT on all of them, the ranks agree (all-reduce of
    the flag), drop the peer windows for good and redo the sweep with one all-reduce per interval
    (krotov_amd/optimize.py, _HipBackend.iterate).  The numbers must be the oracle's, on every rank."""
    out = _run_ranks(world, case, env={'KH_P2P_FAIL_AT': '7', 'KH_P2P_FAIL_RANK': str(fail_rank), 'KH_P2P_FAIL_SWEEP': '2',
                                        'KH_TIMEOUT_MS': '300'})
    spec = _two_rank_spec(case)
    ref = oracle_optimize(spec, 2)
    tol = 1e-12 if case.startswith('c5') else 1e-11
    for _, pulses, tau, used_p2p, kernel, _diag in out:
        assert np.abs(pulses - ref['all_pulses']).max() < tol * max(1.0, np.abs(ref['all_pulses']).max())
        assert np.abs(tau - ref['tau_vals']).max() < tol
        assert np.array_equal(pulses, out[0][1])
    # the first sweep went through the windows, the second one fell back: the engine records both
    assert all(o[3] == 'fallback' for o in out), [o[3] for o in out]
    _check_placement(out, world, windows=False)


@pytest.mark.parametrize('case,world', [('c5', 2), ('c5w4', 4)])
def test_ranks_with_one_all_reduce_per_interval(case, world):
    """The north star's transport with more than one rank (``KH_P2P=0``): kh_update_begin / step_dev / end with one
    all-reduce of the L sums per time interval -- RCCL with ``world`` ranks and HIP-graph replay of the interval loop
    where the box has a GPU per rank, gloo through the host where the ranks share the one GPU.  Same numbers either
    way: the oracle's, bit-identical on all ranks."""
    out = _run_ranks(world, case, env={'KH_P2P': '0'})
    spec = _two_rank_spec(case)
    ref = oracle_optimize(spec, 2)
    for _, pulses, tau, used_p2p, kernel, diag in out:
        assert np.abs(pulses - ref['all_pulses']).max() < 1e-12 * max(1.0, np.abs(ref['all_pulses']).max())
        assert np.abs(tau - ref['tau_vals']).max() < 1e-12
        assert np.array_equal(pulses, out[0][1]) and np.array_equal(tau, out[0][2])
        assert not used_p2p and diag['why'] == 'KH_P2P=0'
    _check_placement(out, world, windows=False)


def test_full_size_c4_liouville_properties(monkeypatch):
    """BASELINE config 4 as concretised in SURVEY.md 8d: transmon in Liouville space,
    400-dim vec(rho), 16 density-matrix objectives sharing one operator list, 1000
    intervals (cooperative matrix-core kernels).  No reference golden exists for
    Liouville-space expm: checked by properties -- trace preservation,
    <chi|rho> conservation between the adjoint (backward) and forward sweeps --, against
    the per-objective generic kernels at full size, and against the oracle on a short
    prefix of the time grid."""
    import torch

    spec = configs.config_c4()
    assert spec.N == 400 and spec.K == 16
    eng = _engine(spec)
    assert eng.kernel == 'coop16/mfma'
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    d = 20
    tr = states.reshape(spec.K, len(spec.tlist), d, d).diagonal(dim1=2, dim2=3).sum(-1)  # tr rho_k(t_n)
    tr0 = torch.as_tensor(np.array([np.trace(v.reshape(d, d, order='F')) for v in spec.init]), device=tr.device)
    assert float((tr - tr0[:, None]).abs().max()) < 1e-11
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    chi = eng.backward(chi_T, pulses)
    ov = (chi.conj() * states).sum(dim=2)
    assert float((ov - ov[:, -1:]).abs().max()) < 1e-10
    opt, psi_T, g_a = eng.forward_update(chi, np.full(spec.K, 1.0 / (2 * spec.K)), spec.init, pulses,
                                         np.array(S), np.array(lam))
    eng.check()
    assert np.all(np.isfinite(opt.cpu().numpy()))
    # one iteration of the reference's own optimize_pulses loop at full size (tests/golden/ref_c4_full.npz: 16 x 1000
    # x 3 dense 400 x 400 expm, 53 CPU-minutes; tests/golden/README.md): the guess pulses, the updated pulses and
    # tau before and after -- a lost fixture fails the test, it does not skip the comparison.  This is the check of
    # the degree-20 near-imaginary-spectrum series at theta = 2.6 against the reference's Pade expm.
    g = golden('ref_c4_full')
    assert np.abs(pulses - g['all_pulses'][0]).max() == 0.0
    assert np.abs(opt.cpu().numpy() - g['all_pulses'][1]).max() < 1e-9 * max(1.0, np.abs(g['all_pulses'][1]).max())
    tau0 = eng.tau(spec.target, fw_T).cpu().numpy()
    tau1 = eng.tau(spec.target, psi_T).cpu().numpy()
    assert np.abs(tau0 - g['tau_vals'][0]).max() < 1e-9
    assert np.abs(tau1 - g['tau_vals'][1]).max() < 1e-9
    assert np.abs(psi_T.cpu().numpy() - g['fw_T']).max() < 1e-9
    eng.close()
    # the same full-size sweeps through the generic (one workgroup per objective) kernels
    monkeypatch.setenv('KH_KERNEL', 'generic')
    gen = _engine(spec)
    assert gen.kernel == 'generic'
    fw_gen = gen.forward(pulses, spec.init)
    assert float((fw_gen - fw_T).abs().max()) < 1e-10
    opt_gen, psi_gen, _ = gen.forward_update(chi, np.full(spec.K, 1.0 / (2 * spec.K)), spec.init, pulses,
                                             np.array(S), np.array(lam))
    gen.check()
    assert float((opt_gen - opt).abs().max()) < 1e-10 * max(1.0, float(opt.abs().max()))
    assert float((psi_gen - psi_T).abs().max()) < 1e-10
    gen.close()
    monkeypatch.delenv('KH_KERNEL')
    # oracle on the first 6 intervals, 2 objectives
    short = configs.config_c4(nt=1001)
    short.tlist = short.tlist[:7]
    sub = configs.ProblemSpec(name='c4_prefix', H0=short.H0[:2], Hc=short.Hc[:2], is_super=True,
                              init=short.init[[1, 5]], target=short.target[[1, 5]], tlist=short.tlist,
                              controls=short.controls, update_shape=short.update_shape, lambda_a=1.0, chi='re')
    prob = spec_to_oracle(sub)
    eng2 = _engine(sub)
    p6 = pulses[:, :6]
    got = eng2.forward(p6, sub.init).cpu().numpy()
    want = ko.forward_propagation(prob, [p6[0]])
    assert np.abs(got - want).max() < 1e-11
    eng2.close()


@pytest.mark.parametrize('kernel', ['q2', 'tile512', 'generic', 'mini', 'one-wave'])
def test_nonuniform_grid_and_large_step_norms(kernel, monkeypatch):
    """Non-uniform dt and ||H dt|| up to ~4 (several Taylor sub-steps per interval,
    degrees changing along the grid), non-Hermitian drift: every kernel family
    ('one-wave': N = 4, the whole problem in one wave, objectives of different norms)."""
    from krotov_amd.engine import HipKrotovEngine

    if kernel != 'one-wave':
        monkeypatch.setenv('KH_KERNEL', kernel)
    rng = np.random.default_rng(11)
    K, N, nt = 3, (4 if kernel == 'one-wave' else 10), 25
    tl = np.cumsum(np.concatenate([[0.0], rng.uniform(0.02, 0.4, nt - 1)]))
    ops = []
    for k in range(K):
        H0 = configs.herm(rng, N, 9.0) - 0.05j * np.diag(rng.uniform(0, 1, N))  # non-Hermitian (decay)
        H1 = configs.herm(rng, N, 2.0)
        ops.append([H0, H1])
    init = rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))
    init /= np.linalg.norm(init, axis=1)[:, None]
    target = np.roll(init, 1, axis=1)
    prob = ko.OracleProblem(ops, init, target, tl)
    gp = [0.8 * np.cos(np.arange(nt - 1) * 0.7)]
    S = [np.linspace(0.2, 1.0, nt - 1)]
    eng = HipKrotovEngine(ops, np.diff(tl))
    assert eng.kernel == {'q2': 'tile64q2/512', 'tile512': 'tile64/512', 'mini': 'mini16/wave',
                          'one-wave': 'mini4/wave'}.get(kernel, kernel)
    fw_T, states = eng.forward(np.array(gp), init, store=True)
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    assert np.abs(states.cpu().numpy() - ref_states).max() < 1e-11
    chi_T = target / np.linalg.norm(target, axis=1)[:, None]
    norms = np.array([0.3, 0.5, 0.2])
    chi = eng.backward(chi_T, np.array(gp))
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    assert np.abs(chi.cpu().numpy() - ref_chi).max() < 1e-11
    opt, psi_T, g_a = eng.forward_update(chi, norms, init, np.array(gp), np.array(S), np.array([3.0]))
    eng.check()
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, [3.0])
    assert np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() < 1e-11
    assert np.abs(psi_T.cpu().numpy() - ref_psi).max() < 1e-11
    assert np.abs(g_a.cpu().numpy() - ref_ga).max() < 1e-11
    assert eng.stats()['matvecs'] > 0
    eng.close()


def _rccl_one_rank_worker(port, queue):
    """One rank, nccl (= RCCL) backend, peer windows off: the per-interval form of the update sweep with a real
    RCCL all-reduce between the launches and HIP-graph replay of the interval loop."""
    import os
    import sys

    import torch
    import torch.distributed as dist

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), KH_P2P='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        import krotov_amd as ka
        from krotov_amd import configs as cfg

        spec = cfg.config_c5(K=6, N=64, nt=301, L=1)  # (301 intervals: several replays of the 64-interval graph)
        objectives, pulse_options = cfg.spec_to_objectives(spec, ka)
        res = ka.optimize_pulses(
            objectives, pulse_options, spec.tlist, propagator=ka.propagators.expm,
            chi_constructor=ka.functionals.chis_re, iter_stop=2, store_all_pulses=True,
            process_group=dist.group.WORLD)
        queue.put((np.array(res.all_pulses), np.array(res.tau_vals)))
    finally:
        dist.destroy_process_group()


def test_rccl_all_reduce_per_interval_one_rank():
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    queue = ctx.Queue()
    proc = ctx.Process(target=_rccl_one_rank_worker, args=(port, queue))
    proc.start()
    pulses, tau = queue.get(timeout=300)
    proc.join(timeout=60)
    assert proc.exitcode == 0
    ref = oracle_optimize(configs.config_c5(K=6, N=64, nt=301, L=1), 2)
    assert np.abs(pulses - ref['all_pulses']).max() < 1e-12 * max(1.0, np.abs(ref['all_pulses']).max())
    assert np.abs(tau - ref['tau_vals']).max() < 1e-12


def test_control_in_several_terms_on_device():
    """One control driving several terms of H (reference tests/test_mu.py:52-129: sigma_+ and sigma_- under the
    same control, so that dH/d eps = sigma_x): the device path sums the operators of a control once
    (krotov_amd/optimize.py, ``summed``) and must agree with the same problem written with the summed operator,
    and with the oracle."""
    rng = np.random.default_rng(11)
    N, K, nt = 6, 3, 121
    tlist = np.linspace(0.0, 3.0, nt)

    def herm(scale):
        G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        return scale * (G + G.conj().T) / 2

    H0 = [herm(1.0) for _ in range(K)]
    lower = np.diag(np.sqrt(np.arange(1, N)), 1).astype(complex)  # sigma_- / annihilation-like
    ctrl = 0.3 * np.sin(np.pi * tlist / tlist[-1])
    psi0 = np.zeros(N, dtype=complex)
    psi0[0] = 1.0
    psi1 = np.zeros(N, dtype=complex)
    psi1[1] = 1.0
    split = [krotov_amd.Objective(initial_state=psi0, target=psi1, H=[H0[k], [lower, ctrl], [lower.conj().T, ctrl]])
             for k in range(K)]
    joined = [krotov_amd.Objective(initial_state=psi0, target=psi1, H=[H0[k], [lower + lower.conj().T, ctrl]])
              for k in range(K)]
    S = lambda t: krotov_amd.shapes.flattop(t, 0.0, tlist[-1], 0.3, func='sinsq')  # noqa: E731
    out = []
    for objs in (split, joined):
        res = krotov_amd.optimize_pulses(
            objs, {id(ctrl): dict(lambda_a=2.0, update_shape=S)}, tlist, propagator=krotov_amd.propagators.expm,
            chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2, store_all_pulses=True)
        out.append((np.array(res.all_pulses), np.array(res.tau_vals)))
    assert np.abs(out[0][0] - out[1][0]).max() < 1e-13 and np.abs(out[0][1] - out[1][1]).max() < 1e-13
    # oracle on the summed operator
    ops = [[H0[k], lower + lower.conj().T] for k in range(K)]
    prob = ko.OracleProblem(ops, np.array([psi0] * K), np.array([psi1] * K), tlist)
    _, gp, Sarr = ko.initialize_controls([ctrl], [S], tlist)
    ref = ko.optimize(prob, gp, Sarr, [2.0], ko.chis_re, 2, norm=lambda p, c: float(np.linalg.norm(c)))
    assert np.abs(out[0][0] - np.array(ref['all_pulses'])).max() < 1e-12
    assert np.abs(out[0][1] - np.array(ref['tau_vals'])).max() < 1e-12


def test_dump_result_and_continue_on_device(tmp_path):
    """check_convergence = dump_result on the device path (result.states is still a device-backed view when the
    hook runs), then Result.load + continue_from."""
    spec = configs.config_c5(K=4, N=64, nt=61)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    path = str(tmp_path / 'oct.dump')
    kw = dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_re,
              store_all_pulses=True)
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, iter_stop=2,
                                     check_convergence=krotov_amd.convergence.dump_result(path, every=1), **kw)
    loaded = krotov_amd.result.Result.load(path, objectives=objectives)
    assert list(loaded.iters) == [0, 1, 2]
    assert np.abs(np.array([np.asarray(x) for x in loaded.states]) - np.array([np.asarray(x) for x in res.states])).max() == 0.0
    cont = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, iter_stop=4, continue_from=loaded, **kw)
    scratch = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, iter_stop=4, **kw)
    assert list(cont.iters) == list(range(5))
    assert np.abs(np.array(cont.all_pulses[3:]) - np.array(scratch.all_pulses[3:])).max() < 1e-12
    assert np.abs(np.array(cont.tau_vals[3:]) - np.array(scratch.tau_vals[3:])).max() < 1e-12
    # the same result written in the REFERENCE's dump format (krotov.result.Result, NumPy mode; the device-backed states
    # are fetched for it) and read back: identical fields, and the continuation from it ends where the other one does
    ref_path = str(tmp_path / 'oct_reference_format.dump')
    res.dump(ref_path, reference=True)
    again = krotov_amd.result.Result.load(ref_path, objectives=objectives)
    assert list(again.iters) == [0, 1, 2] and again.message == res.message
    assert np.array_equal(np.array(again.optimized_controls), np.array(res.optimized_controls))
    assert np.abs(np.array([np.asarray(x) for x in again.states]) - np.array([np.asarray(x) for x in res.states])).max() == 0.0
    cont2 = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, iter_stop=4, continue_from=again, **kw)
    assert np.array_equal(np.array(cont2.all_pulses[3:]), np.array(cont.all_pulses[3:]))


@pytest.mark.no_oracle
def test_two_update_sweeps_on_two_streams():
    """Two engines, each filling the GPU with one workgroup per objective, launched back to back on two streams: the
    single-launch update sweeps need all their workgroups resident at once, so the launches must not interleave
    (cooperative launch) -- both must come back complete and equal to their solo runs."""
    import torch

    specs = [configs.config_c5(K=256, N=64, nt=201, seed=s) for s in (0, 1)]
    engs, args, solo = [], [], []
    for spec in specs:
        eng = _engine(spec)
        gp, S, lam = oracle_controls(spec)
        pulses = np.array(gp)
        chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
        chi = eng.backward(chi_T, pulses)
        a = (chi, np.full(spec.K, 1.0 / (2 * spec.K)), spec.init, pulses, np.array(S), np.array(lam))
        a = tuple(x if torch.is_tensor(x) else eng.dev(x, torch.complex128 if np.iscomplexobj(x) else torch.float64)
                  for x in a)
        out = eng.forward_update(*a)
        eng.check()
        engs.append(eng)
        args.append(a)
        solo.append([o.clone() for o in out])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    both = []
    for _ in range(3):
        both = []
        for eng, a, st in zip(engs, args, streams):
            with torch.cuda.stream(st):
                both.append(eng.forward_update(*a))
        torch.cuda.synchronize()
        for eng, out, ref in zip(engs, both, solo):
            eng.check()
            assert all(torch.equal(o, r) for o, r in zip(out, ref))
    for eng in engs:
        eng.close()


@pytest.mark.no_oracle
def test_update_sweep_next_to_a_busy_stream(monkeypatch):
    """Half of the CUs are held by another stream of the process when the single-launch update sweep (one workgroup
    per CU, all of them needed at once) is launched.  Neither a plain nor a cooperative launch waits for the other
    stream on ROCm 7.2 (measured: both start on the free half), so the sweep's in-kernel waits run into their bound
    (5 ms here, 60 ms of occupation): the C ABI must report KH_ERR_TIMEOUT -- no hang, no silently wrong pulses --
    and the per-interval form of the sweep, which ``optimize_pulses`` falls back to, must give the solo result."""
    import torch

    from krotov_amd import _lib

    monkeypatch.setenv('KH_TIMEOUT_MS', '5')
    # one objective per CU of THIS device (256 on an MI355X; fewer on a partition or under a CU mask), half of them held
    num_cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    spec = configs.config_c5(K=min(256, num_cus), N=64, nt=201)
    eng = _engine(spec)
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    chi = eng.backward(chi_T, pulses)
    a = (chi, np.full(spec.K, 1.0 / (2 * spec.K)), spec.init, pulses, np.array(S), np.array(lam))
    solo = eng.forward_update(*a)
    eng.check()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    timed_out = 0
    for attempt in range(3):
        with torch.cuda.stream(side):
            _lib.check(eng._lib.kh_debug_occupy(eng._handle, max(1, num_cus // 2), 60.0, eng._stream()))
        out = eng.forward_update(*a)  # (default stream: nothing orders it behind the side stream)
        torch.cuda.synchronize()
        try:
            eng.check()
            assert all(torch.equal(o, r) for o, r in zip(out, solo))  # (it fitted after all)
        except _lib.KrotovHipError as exc:
            assert 'timed out' in str(exc) and exc.code == _lib.KH_ERR_TIMEOUT
            timed_out += 1
            break
    # the path this test exists for must really have run: with half of the CUs held for 60 ms and a 5 ms bound, a
    # sweep that needs all 256 workgroups at once cannot get through three times in a row
    if timed_out == 0:
        # (a scheduler that waits for the other stream, a device with spare CUs: nothing is wrong with the library, the
        # situation this test is about just cannot be provoked here)
        pytest.skip("the busy stream never made the in-kernel exchange time out on this device")
    scale = max(1.0, float(solo[0].abs().max()))
    # what optimize_pulses does first: the same sweep on half the workgroups, each walking through
    # two objectives per interval, WHILE the other stream still holds its half of the CUs -- about twice the time of
    # the undisturbed sweep, not the ten times of one launch per interval
    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return out, t0.elapsed_time(t1)

    ms_solo = min(timed(lambda: eng.forward_update(*a))[1] for _ in range(3))
    eng.check()
    grid = eng.set_update_workgroups(max(1, num_cus // 2))
    assert grid == max(1, min(spec.K, num_cus // 2))
    with torch.cuda.stream(side):
        _lib.check(eng._lib.kh_debug_occupy(eng._handle, max(1, num_cus // 2), 60.0, eng._stream()))
    halved, ms_halved = timed(lambda: eng.forward_update(*a))
    eng.check()
    assert eng.stats()['workgroups'] == grid
    assert float((halved[0] - solo[0]).abs().max()) < 1e-12 * scale
    assert float((halved[1] - solo[1]).abs().max()) < 1e-12
    print("update sweep: %.2f ms undisturbed, %.2f ms on %d workgroups next to the busy stream" % (ms_solo, ms_halved, grid))
    # (measured 2.6-2.8x on three boxes, profiles/r05/busy_stream.txt; one launch per interval is ~10x: the bound leaves
    # room for the timer's and the other stream's jitter without letting that regression through)
    assert ms_halved <= 3.5 * ms_solo
    assert eng.set_update_workgroups(0) == spec.K
    # ... and the last resort: one launch per interval
    again = eng.forward_update_sharded(*a, lambda x: None, graph_chunk=0)
    eng.check()
    assert float((again[0] - solo[0]).abs().max()) < 1e-12 * scale
    assert float((again[1] - solo[1]).abs().max()) < 1e-12
    eng.close()


@pytest.mark.no_oracle
def test_optimize_pulses_survives_a_busy_stream(monkeypatch, caplog):
    """The same disturbance under ``optimize_pulses``: the iteration whose update sweep times out is redone interval
    by interval and the run ends with the pulses of an undisturbed one."""
    import torch

    import krotov_amd.engine as engine_mod
    from krotov_amd import _lib

    monkeypatch.setenv('KH_TIMEOUT_MS', '5')
    spec = configs.config_c5(K=256, N=64, nt=201)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    kw = dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_re, iter_stop=3,
              store_all_pulses=True)
    calm = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, **kw)
    side = torch.cuda.Stream()

    def disturb(**args):
        if args['iteration'] == 1:  # right before the sweeps of iteration 2
            eng = engine_mod.LAST_ENGINE()
            with torch.cuda.stream(side):
                _lib.check(eng._lib.kh_debug_occupy(eng._handle, 128, 60.0, eng._stream()))
        return None

    import logging

    caplog.set_level(logging.WARNING, logger='krotov')
    busy = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, info_hook=disturb, **kw)
    torch.cuda.synchronize()
    assert np.abs(np.array(busy.all_pulses) - np.array(calm.all_pulses)).max() < 1e-12
    assert np.abs(np.array(busy.tau_vals) - np.array(calm.tau_vals)).max() < 1e-12
    # the disturbed sweep was redone on half the workgroups (not interval by interval)
    text = caplog.text
    if 'single-launch update sweep failed' in text:
        assert 'repeating it on 128 workgroups' in text and 'one launch per interval' not in text, text


@pytest.mark.parametrize('name', ['c5_n100', 'c5_n80', 'c4_d9', 'c5_n33', 'c5_n12_L3', 'c5_k600'])
def test_kernels_do_not_read_uninitialised_lds(name, monkeypatch):
    """Dynamic LDS holds what the previous kernel on the CU left there.  ``kh_debug_occupy`` leaves all-ones (NaN)
    in 128 KiB of every CU; the sweeps launched right behind it must still be the oracle's (the term vectors
    of kh_tilen.h beyond row N met zero matrix elements, and 0 * NaN poisons every row)."""
    import torch

    from krotov_amd import _lib

    if name == 'c4_d9':
        monkeypatch.setenv('KH_KERNEL', 'tilen')
    spec = SMALL[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.5 / spec.K)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    eng = _engine(spec)
    num_cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count

    def poison():
        _lib.check(eng._lib.kh_debug_occupy(eng._handle, 2 * num_cus, 0.05, eng._stream()))

    poison()
    chi = eng.backward(chi_T, pulses)
    poison()
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    tol = 1e-11 if spec.is_super else 1e-12
    assert np.abs(chi.cpu().numpy() - ref_chi).max() < tol
    assert np.abs(opt.cpu().numpy() - np.array(ref[0])).max() < tol * max(1.0, np.abs(np.array(ref[0])).max())
    assert np.abs(psi_T.cpu().numpy() - ref[1]).max() < tol
    eng.close()


@pytest.mark.parametrize('name,grid,want', [('c5_n64', 3, 3), ('c5_n64_L2', 1, 1), ('c5_n33', 2, 2), ('c5_k300', 100, 100),
                                            ('c5_k520_n64', 40, 33), ('c5_k600', 75, 75), ('c5_n12_L3', 2, 2)])
def test_update_sweep_on_fewer_workgroups(name, grid, want):
    """``kh_set_update_workgroups`` (what follows a KH_ERR_TIMEOUT): the register-tile families run their single-launch
    update sweep as kh_stream_forward_update on the given number of workgroups, ensembles as kh_ens_forward_update with
    more objectives per workgroup -- against the oracle; families without such a form say KH_ERR_UNSUPPORTED."""
    from krotov_amd import _lib

    spec = SMALL[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.5 / spec.K)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    eng = _engine(spec)
    full = eng.set_update_workgroups(0)
    assert eng.set_update_workgroups(grid) == want and want < full
    chi = eng.backward(chi_T, pulses)
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    assert np.abs(opt.cpu().numpy() - np.array(ref[0])).max() < 1e-12 * max(1.0, np.abs(np.array(ref[0])).max())
    assert np.abs(psi_T.cpu().numpy() - ref[1]).max() < 1e-12
    assert np.abs(g_a.cpu().numpy() - ref[2]).max() < 1e-12 * max(1.0, np.abs(ref[2]).max())
    assert eng.stats()['workgroups'] == want
    too_few = (spec.K + 15) // 16 - 1  # (the kernels take at most 16 objectives per workgroup)
    if too_few >= 1:
        with pytest.raises(_lib.KrotovHipError) as info:
            eng.set_update_workgroups(too_few)
        assert info.value.code == _lib.KH_ERR_UNSUPPORTED
    assert eng.set_update_workgroups(0) == full
    eng.close()
    other = _engine(SMALL['c4_d9']())  # cooperative kernels: no form with fewer workgroups
    with pytest.raises(_lib.KrotovHipError) as info:
        other.set_update_workgroups(2)
    assert info.value.code == _lib.KH_ERR_UNSUPPORTED
    other.close()


@pytest.mark.parametrize('name', ['c5_n100', 'c5_n80', 'c5_n64', 'c5_n64_L2'])
def test_advanced_tiles_with_a_pulse_spanning_orders_of_magnitude(name):
    """The register-resident kernels ADVANCE their generator from interval to interval (A += (eps - eps') H_l, restarted
    from the drift every 64 intervals) instead of re-forming it: rounding of the advances is of the order of the LARGEST
    pulse value seen since the restart and does not shrink when the pulse does.  A guess pulse that sweeps
    three orders of magnitude within one restart period must still give the oracle's sweeps to the usual 1e-12
    (measured: 1e-15 -- the advances' rounding is relative to the generator's own magnitude at that time and is
    wiped out at every restart)."""
    spec = SMALL[name]()
    nt = len(spec.tlist)
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    # 30 -> 0.03 -> 30 over the grid, on top of the guess: theta per step up to ~3 (sub-steps) down to ~1e-3
    env = 30.0 * 10.0 ** (-1.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(nt - 1) / (nt - 1))))
    gp = [env * (0.3 + np.abs(g)) for g in gp]
    pulses = np.array(gp)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.1 / spec.K)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    eng = _engine(spec)
    chi = eng.backward(chi_T, pulses)
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    scale = max(1.0, np.abs(np.array(ref[0])).max())
    errs = (np.abs(chi.cpu().numpy() - ref_chi).max(), np.abs(opt.cpu().numpy() - np.array(ref[0])).max() / scale,
            np.abs(psi_T.cpu().numpy() - ref[1]).max())
    print("%s (%s): |d chi| %.1e  |d pulse| / scale %.1e  |d psi(T)| %.1e" % (name, eng.kernel, *errs))
    assert max(errs) < 1e-12
    eng.close()


MM_CASES = {
    'c5_n64': lambda: configs.config_c5(K=8, N=64, nt=61),
    'c5_n33': lambda: configs.config_c5(K=5, N=33, nt=41),
    'c5_k24_long': lambda: configs.config_c5(K=24, N=64, nt=301, distinct=True),  # several restarts of the tiles
    'c5_n20_small_norm': lambda: _scaled(configs.config_c5(K=12, N=20, nt=41), 2e-3),   # degree 4: P = 2, Pf = 1
    'c5_n20_tiny_norm': lambda: _scaled(configs.config_c5(K=12, N=20, nt=41), 1e-7),    # degree 2: P = 1
    'c5_n48_large_norm': lambda: _scaled(configs.config_c5(K=9, N=48, nt=41), 3.0),     # sub-steps (theta > 1)
}


def _scaled(spec, factor):
    """The same problem with every operator multiplied by ``factor`` (other series degrees / sub-step counts)."""
    spec.H0 = [factor * h for h in spec.H0]
    spec.Hc = [[factor * h for h in row] for row in spec.Hc]
    return spec


@pytest.mark.parametrize('name', sorted(MM_CASES))
def test_update_kernel_series_regimes(name):
    """The single-launch update sweep of the register-tile kernels across the regimes of the series -- tiny norms
    (degree 2: one product), small norms, sub-steps (theta > theta_max), several restarts of the advanced tiles,
    ragged N -- against the oracle."""
    spec = MM_CASES[name]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    ref_T = ko.forward_propagation(prob, gp, store=False)
    chi_T = CHI[spec.chi](prob, ref_T, ko.tau_vals(prob, ref_T))
    norms = np.linalg.norm(chi_T, axis=1)
    chi_T = chi_T / norms[:, None]
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    eng = _engine(spec)
    chi = eng.backward(chi_T, pulses)
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    out = (opt.cpu().numpy(), psi_T.cpu().numpy(), g_a.cpu().numpy())
    eng.close()
    scale = max(1.0, np.abs(np.array(ref_opt)).max())
    assert np.abs(out[0] - np.array(ref_opt)).max() < 1e-12 * scale
    assert np.abs(out[1] - ref_psi).max() < 1e-12
    assert np.abs(out[2] - ref_ga).max() < 1e-12 * max(1.0, np.abs(ref_ga).max())


def test_bench_dump_outputs_match_the_oracle(tmp_path):
    """``python bench.py --dump-outputs DIR`` end to end on the device path (the final states fetched from the device on
    first access, the tau values from the device): one warm-up and one timed Krotov iteration of a small config-5
    ensemble; the three files must hold the oracle's two iterations on the same seeded inputs."""
    import json
    import subprocess
    import sys

    from krotov_amd.conversions import pulse_onto_tlist

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / 'dump'
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '1', '--warmup', '1', '--K', '8',
           '--nt', '101', '--no-cpu-baseline', '--no-config4', '--no-variants', '--no-sparse', '--dump-outputs', str(out)]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    rec = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith('{')][-1])
    assert rec['steps'] == 1 and rec['warmup'] == 1 and rec['ms_per_step'] > 0
    assert sorted(os.listdir(str(out))) == ['optimized_controls.npy', 'states.npy', 'tau_vals.npy']
    got = {n: np.load(str(out / (n + '.npy'))) for n in ('optimized_controls', 'tau_vals', 'states')}
    assert all(a.dtype == np.float64 for a in got.values())
    ref = oracle_optimize(configs.config_c5(K=8, N=64, nt=101, L=1), 2)
    want_controls = np.array([pulse_onto_tlist(p) for p in ref['all_pulses'][-1]])
    assert got['optimized_controls'].shape == want_controls.shape == (1, 101)
    assert np.abs(got['optimized_controls'] - want_controls).max() < 1e-11 * max(1.0, np.abs(want_controls).max())
    assert got['tau_vals'].shape == (8, 2) and got['states'].shape == (8, 64, 2)
    assert np.abs(got['tau_vals'][:, 0] + 1j * got['tau_vals'][:, 1] - ref['tau_vals'][-1]).max() < 1e-11
    assert np.abs(got['states'][..., 0] + 1j * got['states'][..., 1] - ref['fw_T']).max() < 1e-11
    assert abs(rec['final_J_T_re'] - (1 - np.mean(got['tau_vals'][:, 0]))) < 1e-12


@pytest.mark.no_oracle
def test_bench_plain_run_measures_the_headline_alone():
    """``python bench.py --gpus 1`` without ``--full`` on the headline's shape (256 objectives, N = 64, one control; a
    shortened grid): the line carries the headline and its own kernel figures, and none of the side measurements that
    only ``--full`` runs."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--nt', '101']
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, proc.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 1 and rec['steps'] == 2 and rec['warmup'] == 1 and rec['value'] > 0 and rec['ms_per_step'] > 0
    assert rec['unit'] == 'props/s' and rec['higher_is_better'] is True and rec['dtype'] == 'f64'
    assert rec['config']['objectives'] == 256 and rec['config']['kernel'] == 'tile64q2/512'
    assert rec['kernels']['update_sweep_ms'] > 0 and rec['roofline']['frac'] > 0
    side = {'cpu_baseline', 'speedup_vs_cpu_baseline', 'config4', 'L4', 'distinct', 'L8', 'N96', 'K1024',
            'K1024_distinct', 'sparse', 'strong', 'weak', 'rccl'}
    assert not side & set(rec), sorted(side & set(rec))
    assert not rec.get('degraded', False)


@pytest.mark.no_oracle
def test_bench_self_launches_two_ranks(tmp_path):
    """``python bench.py --gpus 2 --full`` with no launcher and no WORLD_SIZE in the environment -- the form the driver's
    scaling run uses -- must start its ranks itself, print ONE JSON line from rank 0 and exit 0.  Here both ranks
    share the one GPU (host collectives over gloo, picked automatically; the in-kernel peer windows as on a node).
    The line must carry the headline (weak scaling), the strong-scaling measurement, the RCCL-per-interval leg and
    the number of ranks torch.distributed saw."""
    import json
    import subprocess
    import sys

    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.pop('KH_DIST_BACKEND', None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (--K 128: the two ranks' workgroups must be resident on the ONE GPU at the same time -- 2 x 128 fill it)
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--full',
           '--no-cpu-baseline', '--nt', '201', '--K', '128']
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, proc.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 2 and rec['n_ranks_seen'] == 2 and rec['steps'] == 2
    assert rec['scaling'] == 'weak' and rec['config']['objectives'] == 256
    assert rec['strong']['objectives'] == 128 and rec['strong']['value'] > 0
    assert 'peer-mapped windows' in rec['config']['parallelism']
    assert 'all-reduce per time step' in rec['rccl']['parallelism'] and rec['rccl']['value'] > 0
    # BASELINE config 4 (quoted on 2 and 4 GPUs): its 16 density matrices over the two ranks, cooperative kernels
    assert 'error' not in rec['config4'], rec['config4']
    assert rec['config4']['kernel'].startswith('coop') and rec['config4']['value'] > 0
    assert rec['value'] > 0 and rec['roofline']['frac'] > 0
    # the weak headline names its total, and the figure of the job BASELINE names (--K objectives IN TOTAL) sits beside it
    assert rec['config']['objectives_total'] == 256 and rec['config']['objectives_per_gpu'] == 128
    assert rec['value_baseline_config5'] == rec['strong']['value'] and rec['baseline_config5_objectives_total'] == 128
    _check_rank_diagnostics(rec, 2)


@pytest.mark.no_oracle
def test_bench_two_gpus_strong_scaling_where_the_box_has_them():
    """``python bench.py --gpus 2 --scaling strong --full`` on a box with at least two GPUs: BASELINE config 5 to the letter (256
    objectives in total, 128 per GPU) with one rank per device -- RCCL underneath, the sums through peer windows over
    xGMI.  Skipped on the one-GPU box these tests were written on (the same command line with ranks sharing the device
    is test_bench_self_launches_two_ranks)."""
    import json
    import subprocess
    import sys

    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs, found %d: nothing crosses xGMI" % torch.cuda.device_count())
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.pop('KH_DIST_BACKEND', None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--scaling', 'strong', '--steps', '2', '--warmup', '1',
           '--full', '--no-cpu-baseline', '--nt', '401']
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    rec = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith('{')][0])
    assert rec['n_gpus'] == 2 and rec['n_ranks_seen'] == 2 and rec['scaling'] == 'strong'
    assert rec['config']['objectives_total'] == 256 and rec['config']['objectives_per_gpu'] == 128
    assert rec['value_baseline_config5'] == rec['value'] and rec['weak']['objectives_total'] == 512
    assert sorted(r['device'] for r in rec['ranks']) == [0, 1]
    assert all(r['transport'] == 'peer windows' and r['p2p']['cross_gpu_wait_us'] > 0.0 for r in rec['ranks']), rec['ranks']
    assert 'RCCL all-reduce per time step' in rec['rccl']['parallelism'] and not rec.get('degraded', False)


def _check_rank_diagnostics(rec, world):
    """the line of a sharded run explains itself -- per rank the transport really used (and why, if
    not the peer windows), the set-up self-test's round trip, the per-interval wait inside the GPU and across the
    GPUs; the all-reduce's own cost in the 'rccl' leg; the prediction of DESIGN.md 4 next to the measurement."""
    for part in (rec, rec['strong']):
        ranks = part['ranks']
        assert [r['rank'] for r in ranks] == list(range(world))
        for r in ranks:
            assert r['transport'] == 'peer windows' and r['why'] is None, r
            # (ranks sharing ONE device wait for a queue switch per round: tens of ms here, ~1 us across real GPUs)
            assert r['p2p']['selftest_round_us'] > 0.0 and r['p2p']['ranks'] == world, r
            assert r['p2p']['local_wait_us'] > 0.0 and r['p2p']['cross_gpu_wait_us'] > 0.0, r
            assert r['update_sweep_ms'] > 0 and r['kernel'] == 'tile64q2/512'
    for r in rec['rccl']['ranks']:
        assert r['transport'] == 'all-reduce per interval' and r['why'] == 'KH_P2P=0' and r['allreduce_us'] > 0.0, r
    assert not rec.get('degraded', False) and 'degraded_why' not in rec


@pytest.mark.no_oracle
def test_bench_gpus_8_dry_run_on_one_gpu(tmp_path):
    """``python bench.py --gpus 8 --full`` -- the driver's SCALE command at its largest N -- as a dry run: 8 ranks sharing the one
    GPU, 32 objectives each (config 5's 8-GPU partition: 256 workgroups in total, all co-resident), a shortened grid.
    The weak (headline), strong and rccl legs must be there, nothing degraded, the peer windows used, far inside the
    driver's 1 800 s.  (The config-4 leg is exercised with two ranks in test_bench_self_launches_two_ranks and at world 8
    by test_ranks_sharded_on_one_gpu_world_4_and_8[c4w8]: at full size with EIGHT processes on ONE device it works but
    takes minutes -- 155 s for two iterations, measured with scripts/debug_ranks.py c4full 8 -- because a device runs the
    kernels of at most four hardware queues at once and ranks that wait for each other inside their kernels then wait
    for a queue switch in every interval; with one rank per GPU that cannot happen.)  Needs a GPU per rank
    (MAX_RANKS_SHARING_A_GPU)."""
    import json
    import subprocess
    import sys
    import time

    _skip_unless_devices_for(8)
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.pop('KH_DIST_BACKEND', None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '8', '--steps', '2', '--warmup', '1', '--full',
           '--no-cpu-baseline', '--nt', '101', '--K', '32', '--no-config4']
    t0 = time.time()
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200)
    wall = time.time() - t0
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, proc.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 8 and rec['n_ranks_seen'] == 8
    assert rec['scaling'] == 'weak' and rec['config']['objectives'] == 256
    assert rec['strong']['objectives'] == 32 and rec['strong']['value'] > 0
    assert 'peer-mapped windows' in rec['config']['parallelism']
    assert 'all-reduce per time step' in rec['rccl']['parallelism'] and rec['rccl']['value'] > 0
    assert not rec.get('degraded', False)
    assert rec['roofline']['bound'] == 'fp64-valu' and rec['roofline']['executed_frac'] > 0
    assert wall < 900, wall
    _check_rank_diagnostics(rec, 8)
    print("bench.py --gpus 8 dry run: %.0f s wall; weak %.1f ms, strong %.1f ms, rccl %.1f ms per iteration" % (
        wall, rec['ms_per_step'], rec['strong']['ms_per_step'], rec['rccl']['ms_per_step']))


def test_fuzz_parity_fixed_seed():
    """A fixed-seed slice of tests/fuzz_parity.py: 40 randomly drawn small problems around the kernel families' dispatch
    boundaries, the three sweeps of each against the oracle (the script itself runs for as long as one lets it)."""
    import fuzz_parity

    done, failures = fuzz_parity.fuzz(seed=20260930, cases=40, verbose=False)
    assert done == 40 and not failures, '\n'.join(failures)


def test_fuzz_parity_absent_controls_fixed_seed():
    """A fixed-seed slice of ``tests/fuzz_parity.py --drop-any``: 40 drawn problems (as many as the test above: the
    oracle's share, which dominates, is 4 s here against 8 s there), 18 of them with a control that an objective does not
    have -- 4 with one control: K = 513 and 520 ensemble members without it (objective 0, the last one), N = 81 on the
    register-generator kernels, K = 9 at N = 4; two problems of one objective (K = 1) among the rest."""
    import fuzz_parity

    stats = {}
    done, failures = fuzz_parity.fuzz(seed=20261018, cases=40, verbose=True, drop_any=True, stats=stats)
    print(stats)
    assert done == 40 and not failures, '\n'.join(failures)
    assert stats == {'absent': 18, 'absent_L1': 4}
    assert 3 * stats['absent'] >= done and stats['absent_L1'] >= 1

