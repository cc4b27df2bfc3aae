"""Sparse problems beyond N = 4096 -- and rows wider than 32 entries beyond N = 2540 --: the padded-row family's third
form, ``"ellglobal/csr"`` (krotov_amd/csrc/kh_ellg.h: every vector in global memory, a run-time loop over the rows).
The reference's ``DensityMatrixODEPropagator`` (propagators.py:162-327) and its sparse ``expm`` path have no size limit.

1. forced (``KH_KERNEL=ellglobal``) at small N against the oracle, at the project's bounds: 1e-12 in
   Hilbert space, 1e-11 in Liouville space -- the constructions the streamed form's cases of test_instantiations.py use;
2. unforced beyond the old limits (engine creation raised there before): a d = 65 Lindbladian against the oracle's
   restated zvode step, a banded Hermitian problem of dimension 5003 and a 13-qubit spin chain against
   ``scipy.sparse.linalg.expm_multiply`` and against properties that need no reference;
3. through ``optimize_pulses(..., propagator=DensityMatrixODEPropagator())``;
4. host only: registry, row layout, the N limit, the spin-chain builder, and the witness for the bound of 2.
"""
import ctypes

import numpy as np
import pytest

from helpers import oracle_controls, spec_to_oracle
from krotov_amd import _lib, configs
from oracle import krotov_oracle as ko

SWEEP = 'kh_ellg_sweep_store<512>'
UPDATE = 'kh_ellg_forward_update<512, false>'
UPDATE_SO = 'kh_ellg_forward_update<512, true>'


def _banded(N, bands, nt, K=2):
    from test_hip_parity import _banded as make

    return make(N, bands, nt, K=K)


def _tiled(spec, times):
    from test_hip_parity import _tiled as make

    return make(spec, times)


# ---------------------------------------------------------------------------
# 1. forced at small N against the oracle
# ---------------------------------------------------------------------------
FORCED = {
    # name: (spec, second order, expected instantiations, update grid or None)
    # two passes of the row loop with a ragged tail (600 = 512 + 88), rows wider than the register forms take
    'banded_n600_e21': (lambda: _banded(600, 21, nt=4, K=1), False, (SWEEP, UPDATE), None),
    'lindblad_d12': (lambda: configs.config_sparse_lindblad(d=12, nt=21, K=3), False, (SWEEP, UPDATE), None),
    'c5_n12_L3': (lambda: configs.config_c5(K=5, N=12, nt=31, L=3, distinct=True), False, (SWEEP, UPDATE), None),
    'c5_n12_L3_so': (lambda: configs.config_c5(K=5, N=12, nt=31, L=3, distinct=True), True, (UPDATE_SO,), None),
    # rows wider than 32: only this form of the family accepts them (when forced; unforced the generic kernels keep them)
    'banded_n48_e37': (lambda: _banded(48, 37, nt=9), False, (SWEEP, UPDATE), None),
    # K = 300 > #CUs: several objectives per workgroup
    'lindblad_k300': (lambda: _tiled(configs.config_sparse_lindblad(d=5, nt=13, K=5), 60), False, (SWEEP, UPDATE), None),
    # K = 5 on two workgroups: three and two objectives per workgroup
    'c5_n12_L3_two_workgroups': (lambda: configs.config_c5(K=5, N=12, nt=31, L=3, distinct=True), False, (UPDATE,), 2),
    'c5_n12_L3_two_workgroups_so': (lambda: configs.config_c5(K=5, N=12, nt=31, L=3, distinct=True), True, (UPDATE_SO,), 2),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(FORCED))
def test_forced_global_form_vs_oracle(name, monkeypatch):
    """Forward with storage, backward, the single-launch update sweep (pulses, psi(T), g_a) and, second order, the
    stored trajectory against the oracle (optimize.py:444-508, :849-886); the library's registry confirms which
    instantiations ran.  ``kh_set_update_workgroups``: any grid from ceil(K / 16) on -- one less is refused (K = 300:
    19 accepted, 18 refused; for K = 5 that grid would be 0, the value that restores the engine's own grid)."""
    import torch

    from krotov_amd.engine import HipKrotovEngine

    build, so, expect, grid = FORCED[name]
    monkeypatch.setenv('KH_KERNEL', 'ellglobal')
    spec = build()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    eng = HipKrotovEngine(configs.sparse_ops(spec), np.diff(spec.tlist), is_super=spec.is_super)
    assert eng.kernel == 'ellglobal/csr'
    if spec.K == 300:
        assert eng.set_update_workgroups(19) == 19
        with pytest.raises(_lib.KrotovHipError) as refused:
            eng.set_update_workgroups(18)
        assert refused.value.code == _lib.KH_ERR_UNSUPPORTED
        full = eng.set_update_workgroups(0)
        assert full == min(300, torch.cuda.get_device_properties(eng.device).multi_processor_count)
    if grid is not None:
        assert eng.set_update_workgroups(grid) == grid
    _lib.forget_launched_kernels()
    tol = 1e-11 if spec.is_super else 1e-12
    rng = np.random.default_rng(17)
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    assert np.abs(states.cpu().numpy() - ref_states).max() < tol
    assert np.abs(fw_T.cpu().numpy() - ref_T).max() < tol
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = (0.2 + rng.random(spec.K)) * min(1.0, 8.0 / spec.K)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    chi = eng.backward(chi_T, pulses)
    assert np.abs(chi.cpu().numpy() - ref_chi).max() < tol
    kw = {}
    if so:
        older = [p * (1.0 + 0.2 * rng.standard_normal(p.shape)) for p in gp]  # the "previous iteration"
        _, prev = ko.forward_propagation(prob, older, store=True)
        sigma_vals = -(1.0 + rng.random(len(spec.tlist) - 1)) * min(1.0, 8.0 / spec.K)
        kw = dict(sigma_vals=sigma_vals, fw_prev=prev, store=True)
        store = torch.full((spec.K, len(spec.tlist), spec.N), float('nan'), dtype=torch.complex128, device=eng.device)
        eng.set_second_order(prev, store, sigma_vals)
    ref = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam, **kw)
    opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, np.array(S), np.array(lam))
    eng.check()
    launched = _lib.kernel_instantiations(launched_only=True)
    scale = max(1.0, np.abs(np.array(ref[0])).max())
    print('%s: forward %.1e backward %.1e pulses %.1e psi(T) %.1e g_a %.1e%s' % (
        name, np.abs(states.cpu().numpy() - ref_states).max(), np.abs(chi.cpu().numpy() - ref_chi).max(),
        np.abs(opt.cpu().numpy() - np.array(ref[0])).max() / scale, np.abs(psi_T.cpu().numpy() - ref[1]).max(),
        np.abs(g_a.cpu().numpy() - ref[2]).max() / max(1.0, np.abs(ref[2]).max()),
        ' trajectory %.1e' % np.abs(store.cpu().numpy() - ref[3]).max() if so else ''))
    assert np.abs(opt.cpu().numpy() - np.array(ref[0])).max() < tol * scale
    assert np.abs(psi_T.cpu().numpy() - ref[1]).max() < tol
    assert np.abs(g_a.cpu().numpy() - ref[2]).max() < tol * max(1.0, np.abs(ref[2]).max())
    if so:
        assert np.abs(store.cpu().numpy() - ref[3]).max() < tol
    if grid is not None:
        assert eng.stats()['workgroups'] == grid
    for want in expect:
        assert want in launched, (want, launched)
    eng.close()


# ---------------------------------------------------------------------------
# 2. beyond the old limits, unforced
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_sparse_liouvillian_of_dimension_4225():
    """A d = 65 ladder (N = 4225: beyond the streamed form's two LDS vectors) with the yardsticks of
    ``test_sparse_liouvillian_of_dimension_4096``: the three sweeps against the oracle's restated zvode step at rtol
    1e-12 / atol 1e-14 to 1e-8, trace preservation to 1e-12.  Engine creation raised KH_ERR_UNSUPPORTED here before."""
    from krotov_amd.engine import HipKrotovEngine

    d = 65
    spec = configs.config_sparse_lindblad(d=d, nt=4, K=2)
    ops = configs.sparse_ops(spec)
    assert spec.N == 4225
    eng = HipKrotovEngine(ops, np.diff(spec.tlist), is_super=True)
    assert eng.kernel == 'ellglobal/csr'
    gp, S, lam = oracle_controls(spec)
    pulses = np.array(gp)
    prob = ko.OracleProblem(ops, spec.init, spec.target, spec.tlist, is_super=True,
                            ode=dict(rtol=1e-12, atol=1e-14, nsteps=200000))
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    got = states.cpu().numpy()
    assert np.abs(got - ref_states).max() < 1e-8
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
    launched = _lib.kernel_instantiations(launched_only=True)
    assert SWEEP in launched and UPDATE in launched
    eng.close()


def _gershgorin(m):
    """max_r sum_c |m_rc|: a bound on the spectral norm of a Hermitian matrix that forms nothing dense"""
    return float(abs(m).sum(axis=1).max())


def _banded_sparse(N, seed=5):
    """A Hermitian banded drift with 9 diagonals and two Hermitian controls (3 and 5 diagonals) on N levels, built with
    ``scipy.sparse.diags`` and scaled by their Gershgorin sums (3, 1 and 1).  Returns (operators, their norm bounds)."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)

    def herm_band(half, bound):
        diags, offsets = [rng.standard_normal(N)], [0]
        for d in range(1, half + 1):
            v = rng.standard_normal(N - d) + 1j * rng.standard_normal(N - d)
            diags += [v, v.conj()]
            offsets += [d, -d]
        m = sp.diags(diags, offsets, shape=(N, N), format='csr', dtype=np.complex128)
        return sp.csr_matrix(m * (bound / _gershgorin(m)))

    ops = [herm_band(4, 3.0), herm_band(1, 1.0), herm_band(2, 1.0)]
    return ops, [_gershgorin(m) for m in ops]


def _ket_case(name):
    """(operators [H0, H_1, ...], norm bounds, tlist, guess pulses (L, nt-1), shapes (L, nt-1), lambdas)"""
    if name == 'banded_n5003':
        ops, bounds = _banded_sparse(5003)  # (5003: no multiple of 64 or of 512)
        tlist = np.linspace(0.0, 0.3, 4)
    else:
        spec = configs.config_spin_chain(13, nt=4, K=2)
        ops = configs.sparse_ops(spec)[0]
        bounds = [_gershgorin(m) for m in ops]
        tlist = spec.tlist
    L, nt = len(ops) - 1, len(tlist)
    mid = 0.5 * (tlist[1:] + tlist[:-1]) / tlist[-1]
    pulses = np.array([0.3 * np.sin((l + 1) * np.pi * mid) ** 2 + 0.1 * (l + 1) for l in range(L)])
    shapes = np.array([0.5 + 0.5 * np.sin(np.pi * mid) ** 2 for _ in range(L)])
    lambdas = np.array([2.0 + l for l in range(L)])
    assert pulses.shape == (L, nt - 1)
    return ops, bounds, tlist, pulses, shapes, lambdas


def _expm_multiply_sweep(ops, tlist, pulses, first, backward):
    """The stored states of a plain sweep, step by step with scipy's expm_multiply: forward exp(-i H(eps_n) dt),
    backward exp(+i H(eps_n)^+ dt) from the last grid point (propagators.py:94-117 with the adjoint objectives)."""
    from scipy.sparse.linalg import expm_multiply

    K, nt = first.shape[0], len(tlist)
    out = np.empty((K, nt, first.shape[1]), dtype=np.complex128)
    out[:, -1 if backward else 0] = first
    for step in range(nt - 1):
        n = nt - 2 - step if backward else step
        H = ops[0] + sum(pulses[l, n] * ops[1 + l] for l in range(len(ops) - 1))
        A = (1j * H.conj().T if backward else -1j * H) * (tlist[n + 1] - tlist[n])
        src, dst = (n + 1, n) if backward else (n, n + 1)
        for k in range(K):
            out[k, dst] = expm_multiply(A.tocsc(), out[k, src])
    return out


EXPM_MULTIPLY_BOUND = 1e-12  # the project's Hilbert-space bound; test_expm_multiply_witness: the reference itself is within 1e-13


def test_expm_multiply_witness():
    """Host only.  What the large-N tests compare with -- ``scipy.sparse.linalg.expm_multiply`` -- agrees with the
    oracle's dense ``step`` to 1e-13 on the same banded construction at N = 600 (forward and backward, the pulses of
    the large case): the 1e-12 asserted at N = 5003 and N = 8192 is the project's bound, not the reference's error.
    Measured here: 7.1e-17."""
    ops, _ = _banded_sparse(600)
    tlist = np.linspace(0.0, 0.3, 4)
    _, _, _, pulses, _, _ = _ket_case('banded_n5003')
    rng = np.random.default_rng(3)
    psi = rng.standard_normal((2, 600)) + 1j * rng.standard_normal((2, 600))
    psi /= np.linalg.norm(psi, axis=1)[:, None]
    dense = [m.toarray() for m in ops]
    worst = 0.0
    for backward in (False, True):
        got = _expm_multiply_sweep(ops, tlist, pulses, psi, backward)
        ops_k = [m.conj().T for m in dense] if backward else dense
        for step in range(len(tlist) - 1):
            n = len(tlist) - 2 - step if backward else step
            src, dst = (n + 1, n) if backward else (n, n + 1)
            for k in range(2):
                want = ko.step(ops_k, pulses[:, n], tlist[n + 1] - tlist[n], got[k, src], backwards=backward)
                worst = max(worst, np.abs(got[k, dst] - want).max())
    print('expm_multiply against the dense step: %.2e' % worst)
    assert worst <= 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['banded_n5003', 'spin_chain_n13'])
def test_large_ket_problem(name):
    """Hermitian sparse ket problems beyond N = 4096, K = 2 (two workgroups: the in-kernel exchange is real), norms from
    Gershgorin sums so that nothing dense is ever formed:
      * forward and backward stored states against expm_multiply, step by step, to 1e-12 (see the witness);
      * norm conservation to 1e-12;
      * psi(T) of the update sweep = the plain forward sweep under the pulses the update returned, to 1e-12;
      * the first interval's updated value = guess + S/lambda sum_k ||chi_k|| Im <chi_k(0)| H_l phi_k(0)>, on the host;
      * two runs are bitwise equal."""
    import torch

    from krotov_amd.engine import HipKrotovEngine

    ops, bounds, tlist, pulses, shapes, lambdas = _ket_case(name)
    K, N, L = 2, ops[0].shape[0], len(ops) - 1
    assert N > 4096
    rng = np.random.default_rng(29)
    init = rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))
    init /= np.linalg.norm(init, axis=1)[:, None]
    chi_T = rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))
    chi_T /= np.linalg.norm(chi_T, axis=1)[:, None]
    eng = HipKrotovEngine([ops] * K, np.diff(tlist), op_norms=np.tile(bounds, K))
    assert eng.kernel == 'ellglobal/csr'
    fw_T, states = eng.forward(pulses, init, store=True)
    got = states.cpu().numpy()
    ref = _expm_multiply_sweep(ops, tlist, pulses, init, backward=False)
    err_fw = np.abs(got - ref).max()
    chi = eng.backward(chi_T, pulses)
    got_chi = chi.cpu().numpy()
    ref_chi = _expm_multiply_sweep(ops, tlist, pulses, chi_T, backward=True)
    err_bw = np.abs(got_chi - ref_chi).max()
    err_norm = max(np.abs(np.linalg.norm(got, axis=2) - 1.0).max(), np.abs(np.linalg.norm(got_chi, axis=2) - 1.0).max())
    print('%s: forward %.2e, backward %.2e against expm_multiply; norms %.2e' % (name, err_fw, err_bw, err_norm))
    assert err_fw < EXPM_MULTIPLY_BOUND and err_bw < EXPM_MULTIPLY_BOUND
    assert np.abs(fw_T.cpu().numpy() - ref[:, -1]).max() < EXPM_MULTIPLY_BOUND
    assert err_norm < 1e-12
    norms = np.array([0.4, 0.7])
    opt, psi_T, g_a = eng.forward_update(chi, norms, init, pulses, shapes, lambdas)
    eng.check()
    again = eng.forward_update(chi, norms, init, pulses, shapes, lambdas)
    eng.check()
    for a, b in zip((opt, psi_T, g_a), again):
        assert torch.equal(a, b)
    assert torch.equal(eng.backward(chi_T, pulses), chi)
    plain_T = eng.forward(opt, init)
    err_T = np.abs(psi_T.cpu().numpy() - plain_T.cpu().numpy()).max()
    opt_h = opt.cpu().numpy()
    want0 = np.array([pulses[l, 0] + shapes[l, 0] / lambdas[l] *
                      sum(norms[k] * np.vdot(got_chi[k, 0], ops[1 + l] @ init[k]).imag for k in range(K)) for l in range(L)])
    err_0 = np.abs(opt_h[:, 0] - want0).max()
    print('%s: psi(T) of the update against the plain sweep %.2e; first interval %.2e' % (name, err_T, err_0))
    assert err_T < 1e-12
    assert err_0 < 1e-12 * max(1.0, np.abs(want0).max())
    assert np.abs(opt_h - pulses).max() > 1e-6  # (the update moved the pulses: the checks above are not vacuous)
    launched = _lib.kernel_instantiations(launched_only=True)
    assert SWEEP in launched and UPDATE in launched
    eng.close()


# ---------------------------------------------------------------------------
# 3. through the public call
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_optimize_pulses_on_a_liouvillian_of_dimension_4225():
    """``optimize_pulses(..., propagator=DensityMatrixODEPropagator())`` with scipy.sparse Liouvillians of dimension
    4225 (raised KH_ERR_UNSUPPORTED before): the engine takes the global form and J_T,re = 1 - Re(mean tau) does not
    increase over two iterations (Krotov's monotonic convergence)."""
    import scipy.sparse as sp

    import krotov_amd
    from krotov_amd.engine import LAST_ENGINE

    spec = configs.config_sparse_lindblad(d=65, nt=21, K=2)
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
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist,
                                     propagator=krotov_amd.propagators.DensityMatrixODEPropagator(),
                                     chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2)
    assert LAST_ENGINE().kernel == 'ellglobal/csr'
    J_T = [1.0 - np.mean(np.asarray(tau)).real for tau in res.tau_vals]
    print('J_T per iteration:', J_T)
    assert len(J_T) == 3
    assert J_T[1] <= J_T[0] and J_T[2] <= J_T[1]
    assert J_T[2] < J_T[0]


# ---------------------------------------------------------------------------
# 4. host only
# ---------------------------------------------------------------------------
def test_registry_lists_the_global_form():
    names = _lib.kernel_instantiations()
    for want in (SWEEP, UPDATE, UPDATE_SO):
        assert want in names, want
    assert sum(n.startswith('kh_ellg_') for n in names) == 3
    assert b'ellglobal/csr' in _lib.load().kh_version()


def _layout_global(ops, N):
    """kh_ell_layout_global on scipy.sparse operators -> (rc, E, Ec, off [E][S], vals [n][E][S]), S = N rounded up to 64"""
    lib = _lib.load()
    arr = (_lib.kh_csr * len(ops))()
    keep = []
    for o, m in enumerate(ops):
        indptr, indices = np.ascontiguousarray(m.indptr, dtype=np.int32), np.ascontiguousarray(m.indices, dtype=np.int32)
        data = np.ascontiguousarray(m.data, dtype=np.complex128)
        keep.append((indptr, indices, data))
        arr[o].nnz = len(data)
        arr[o].indptr, arr[o].indices, arr[o].data = indptr.ctypes.data, indices.ctypes.data, data.ctypes.data
    E, Ec = ctypes.c_int32(), ctypes.c_int32()
    rc = lib.kh_ell_layout_global(N, len(ops), arr, ctypes.byref(E), ctypes.byref(Ec), None, None, 0)
    if rc != 0:
        return rc, None, None, None, None
    S = (N + 63) // 64 * 64
    off = np.zeros((E.value, S), dtype=np.int32)
    vals = np.zeros((len(ops), E.value, S), dtype=np.complex128)
    assert lib.kh_ell_layout_global(N, len(ops), arr, ctypes.byref(E), ctypes.byref(Ec), off.ctypes.data, vals.ctypes.data, E.value) == 0
    return 0, E.value, Ec.value, off, vals


def test_row_layout_of_the_global_form():
    """``kh_ell_layout_global`` (host code, no GPU): the streamed form's arrays with rows of any width.  A 40-entry row
    next to rows of 9, control-touched entries first: sum_e vals[o][e][r] x[off[e][r] / 16] = (A_o x)[r], E and Ec
    multiples of four, padded rows point at themselves; the register form's layout refuses the same operators."""
    import scipy.sparse as sp

    N = 100
    rng = np.random.default_rng(2)
    A0 = sp.lil_matrix(_banded_sparse(N)[0][0])
    A0[7, :40] = rng.standard_normal(40) + 1j * rng.standard_normal(40)
    A0 = sp.csr_matrix(A0)
    A1 = sp.csr_matrix(_banded_sparse(N)[0][1])
    rc, E, Ec, off, vals = _layout_global([A0, A1], N)
    assert rc == 0 and E == 40 and Ec == 4 and off.shape == (40, 128)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    assert off.min() >= 0 and off.max() < 16 * N and np.all(off % 16 == 0)
    for o, A in enumerate((A0, A1)):
        y = (vals[o, :, :N] * x[off[:, :N] // 16]).sum(axis=0)
        assert np.abs(y - A @ x).max() < 1e-13
    assert np.all(vals[1, Ec:] == 0.0)  # the control lives in the first Ec slots of every row
    assert np.all(off[:, N:] == 0) and np.all(vals[:, :, N:] == 0.0)
    from test_capi_symbols import _ell_layout

    assert _ell_layout([A0, A1], N)[0] == _lib.KH_ERR_UNSUPPORTED


def test_dimension_beyond_two_to_the_twenty_is_refused():
    import scipy.sparse as sp

    N = 2 ** 20 + 1
    rc = _layout_global([sp.identity(N, dtype=np.complex128, format='csr')], N)[0]
    assert rc == _lib.KH_ERR_UNSUPPORTED
    assert b'2^20' in _lib.load().kh_last_error() or b'1048576' in _lib.load().kh_last_error()


def test_spin_chain_equals_its_dense_kronecker_construction():
    """``configs.config_spin_chain(4, ...)``: J sum Z_i Z_{i+1} + h sum X_i and sum Z_i, bit for bit."""
    spec = configs.config_spin_chain(4, nt=5, K=2)
    X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    Z = np.diag([1.0, -1.0]).astype(np.complex128)
    eye = np.eye(2, dtype=np.complex128)

    def site(op, i, op2=None):
        out = np.eye(1, dtype=np.complex128)
        for j in range(4):
            out = np.kron(out, op if j == i else (op2 if op2 is not None and j == i + 1 else eye))
        return out

    H0 = sum(1.0 * site(Z, i, Z) for i in range(3)) + sum(0.5 * site(X, i) for i in range(4))
    H1 = sum(site(Z, i) for i in range(4))
    assert hasattr(spec.H0[0], 'tocsr') and spec.N == 16 and spec.K == 2 and spec.L == 1
    assert np.array_equal(spec.H0[0].toarray(), H0) and np.array_equal(spec.Hc[0][0].toarray(), H1)
    assert spec.H0[0] is spec.H0[1] and spec.Hc[0][0] is spec.Hc[1][0]
    ops = configs.sparse_ops(spec)
    assert ops[0][0] is ops[1][0] and np.array_equal(ops[0][0].toarray(), H0)
    assert np.array_equal(spec.init[1], np.eye(16)[1]) and np.array_equal(spec.target[1], np.eye(16)[14])
