"""One sparse objective on several workgroups: the padded-row family's fourth form, ``"ellsplit/csr"``
(krotov_amd/csrc/kh_ellg.h, SPLIT: the global form with S workgroups per objective, a barrier among them per term).

1. forced (``KH_KERNEL=ellsplit``, ``KH_ELL_SPLIT=S``) at small N against the oracle, at the project's bounds:
   1e-12 in Hilbert space, 1e-11 in Liouville space -- the cases tests/test_sparse_large.py holds at those bounds on the
   global form.  Small N is where a missing acquire shows: the term planes are at most 10 KB and are read again at the
   same addresses every second term, so the reading CU's vector cache is warm by construction;
2. properties that need no reference: the plain sweeps do not depend on S (bitwise), repeatability, the product count,
   one case at N = 8192, what is refused, ``optimize_pulses`` with ``DensityMatrixODEPropagator(row_split=2)``;
3. host only: the row partition, the registry, the time-out ladder of ``optimize_pulses`` on the engine double.
No GPU test makes a barrier time out: that path runs on the host only.
"""
import ctypes
import functools
import logging

import numpy as np
import pytest

from helpers import oracle_controls, spec_to_oracle
from krotov_amd import _lib, configs
from oracle import krotov_oracle as ko

SWEEP = 'kh_ellgs_sweep_store<512>'
UPDATE = 'kh_ellgs_forward_update<512, false>'
UPDATE_SO = 'kh_ellgs_forward_update<512, true>'
GLOBAL = ('kh_ellg_sweep_store<512>', 'kh_ellg_forward_update<512, false>')


def _banded(N, bands, nt, K=2):
    from test_hip_parity import _banded as make

    return make(N, bands, nt, K=K)


BUILD = {
    'banded_n600_e21': lambda: _banded(600, 21, nt=4, K=1),
    'banded_n48_e37': lambda: _banded(48, 37, nt=9),
    'lindblad_d12': lambda: configs.config_sparse_lindblad(d=12, nt=21, K=3),
    'c5_n12_L3': lambda: configs.config_c5(K=5, N=12, nt=31, L=3, distinct=True),
}

FORCED = [
    # (case, S, groups cap or None, second order, expected instantiations)
    ('banded_n600_e21', 2, None, False, (SWEEP, UPDATE)),  # 10 chunks: 5 + 5, the ragged tail in part 1
    ('banded_n600_e21', 3, None, False, (SWEEP, UPDATE)),  # 4 + 3 + 3
    ('banded_n600_e21', 4, None, False, (SWEEP, UPDATE)),  # 3 + 3 + 2 + 2
    ('banded_n48_e37', 2, None, False, (SWEEP, UPDATE)),   # one chunk: part 1 owns no row and arrives at every barrier
    ('lindblad_d12', 4, None, False, (SWEEP, UPDATE)),     # three groups side by side
    ('c5_n12_L3', 2, 2, False, (SWEEP, UPDATE)),           # two groups: three and two objectives in turns
    ('c5_n12_L3', 2, 2, True, (UPDATE_SO,)),
]


@functools.lru_cache(maxsize=None)
def _reference(case, so):
    """The oracle's three sweeps of a case, computed once and shared (never modified)."""
    spec = BUILD[case]()
    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    rng = np.random.default_rng(17)
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = (0.2 + rng.random(spec.K)) * min(1.0, 8.0 / spec.K)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    kw, prev, sigma_vals = {}, None, None
    if so:
        older = [p * (1.0 + 0.2 * rng.standard_normal(p.shape)) for p in gp]  # the "previous iteration"
        _, prev = ko.forward_propagation(prob, older, store=True)
        sigma_vals = -(1.0 + rng.random(len(spec.tlist) - 1)) * min(1.0, 8.0 / spec.K)
        kw = dict(sigma_vals=sigma_vals, fw_prev=prev, store=True)
    ref = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam, **kw)
    return dict(spec=spec, gp=gp, S=S, lam=lam, ref_T=ref_T, ref_states=ref_states, chi_T=chi_T, norms=norms,
                ref_chi=ref_chi, prev=prev, sigma_vals=sigma_vals, ref=ref)


def _engine(spec, **kw):
    from krotov_amd.engine import HipKrotovEngine

    return HipKrotovEngine(configs.sparse_ops(spec), np.diff(spec.tlist), is_super=spec.is_super, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('case,S,groups,so', [c[:4] for c in FORCED],
                         ids=['%s-S%d%s%s' % (c[0], c[1], '-g%d' % c[2] if c[2] else '', '-so' if c[3] else '') for c in FORCED])
def test_forced_split_form_vs_oracle(case, S, groups, so, monkeypatch):
    """Forward with storage, backward, the single-launch update sweep (pulses, psi(T), g_a) and, second order, the
    stored trajectory against the oracle, at the bounds of ``test_forced_global_form_vs_oracle``; the library's registry
    confirms which instantiations ran."""
    import torch

    expect = [c[4] for c in FORCED if c[:4] == (case, S, groups, so)][0]
    monkeypatch.setenv('KH_KERNEL', 'ellsplit')
    monkeypatch.setenv('KH_ELL_SPLIT', str(S))
    if groups:
        monkeypatch.setenv('KH_ELL_GROUPS', str(groups))
    r = _reference(case, so)
    spec, gp, ref = r['spec'], r['gp'], r['ref']
    pulses = np.array(gp)
    eng = _engine(spec)
    assert eng.kernel == 'ellsplit/csr' and eng.row_split == S
    _lib.forget_launched_kernels()
    tol = 1e-11 if spec.is_super else 1e-12
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    eng.check()
    chi = eng.backward(r['chi_T'], pulses)
    eng.check()
    if so:
        store = torch.full((spec.K, len(spec.tlist), spec.N), float('nan'), dtype=torch.complex128, device=eng.device)
        eng.set_second_order(r['prev'], store, r['sigma_vals'])
    opt, psi_T, g_a = eng.forward_update(chi, r['norms'], spec.init, pulses, np.array(r['S']), np.array(r['lam']))
    eng.check()
    launched = _lib.kernel_instantiations(launched_only=True)
    scale = max(1.0, np.abs(np.array(ref[0])).max())
    print('%s S=%d: forward %.1e backward %.1e pulses %.1e psi(T) %.1e g_a %.1e%s' % (
        case, S, np.abs(states.cpu().numpy() - r['ref_states']).max(), np.abs(chi.cpu().numpy() - r['ref_chi']).max(),
        np.abs(opt.cpu().numpy() - np.array(ref[0])).max() / scale, np.abs(psi_T.cpu().numpy() - ref[1]).max(),
        np.abs(g_a.cpu().numpy() - ref[2]).max() / max(1.0, np.abs(ref[2]).max()),
        ' trajectory %.1e' % np.abs(store.cpu().numpy() - ref[3]).max() if so else ''))
    assert np.abs(states.cpu().numpy() - r['ref_states']).max() < tol
    assert np.abs(fw_T.cpu().numpy() - r['ref_T']).max() < tol
    assert np.abs(chi.cpu().numpy() - r['ref_chi']).max() < tol
    assert np.abs(opt.cpu().numpy() - np.array(ref[0])).max() < tol * scale
    assert np.abs(psi_T.cpu().numpy() - ref[1]).max() < tol
    assert np.abs(g_a.cpu().numpy() - ref[2]).max() < tol * max(1.0, np.abs(ref[2]).max())
    if so:
        assert np.abs(store.cpu().numpy() - ref[3]).max() < tol
    want_grid = S * (groups or spec.K)
    assert eng.stats()['workgroups'] == want_grid
    for want in expect:
        assert want in launched, (want, launched)
    assert not any(n.startswith('kh_ellg_') for n in launched), launched
    eng.close()


# ---------------------------------------------------------------------------
# 2. properties that need no reference
# ---------------------------------------------------------------------------
def _plain_sweeps(eng, spec, pulses, chi_T):
    fw_T, states = eng.forward(pulses, spec.init, store=True)
    eng.check()
    chi = eng.backward(chi_T, pulses)
    eng.check()
    return states, chi


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_plain_sweeps_do_not_depend_on_the_split(monkeypatch):
    """``banded_n600_e21``: the stored forward and backward trajectories for S = 2 and S = 4 are bitwise equal (the same
    instantiation, the same per-row code: any difference is a stale or an early read); against S = 1 (the plain
    instantiations: other code generation) they deviate by at most 1e-13.  The product count does not depend on S either."""
    import torch

    monkeypatch.setenv('KH_KERNEL', 'ellsplit')
    r = _reference('banded_n600_e21', False)
    spec, pulses = r['spec'], np.array(r['gp'])
    eng = _engine(spec, row_split=2)
    assert eng.kernel == 'ellsplit/csr'
    fw2, bw2 = _plain_sweeps(eng, spec, pulses, r['chi_T'])
    assert eng.set_row_split(4) == 4
    fw4, bw4 = _plain_sweeps(eng, spec, pulses, r['chi_T'])
    assert torch.equal(fw2, fw4) and torch.equal(bw2, bw4)
    assert eng.set_row_split(3) == 3
    eng.backward(r['chi_T'], pulses)
    count3 = eng.stats()['matvecs']
    assert eng.set_row_split(1) == 1 and eng.kernel == 'ellglobal/csr'
    _lib.forget_launched_kernels()
    fw1, bw1 = _plain_sweeps(eng, spec, pulses, r['chi_T'])
    count1 = eng.stats()['matvecs']
    opt, psi_T, g_a = eng.forward_update(bw1, r['norms'], spec.init, pulses, np.array(r['S']), np.array(r['lam']))
    eng.check()
    launched = _lib.kernel_instantiations(launched_only=True)
    for want in GLOBAL:  # row_split = 1 restores the global form's own instantiations
        assert want in launched, (want, launched)
    assert not any(n.startswith('kh_ellgs_') for n in launched), launched
    dev_fw, dev_bw = (fw1 - fw2).abs().max().item(), (bw1 - bw2).abs().max().item()
    print('S = 2 against S = 1: forward %.1e backward %.1e; products %g / %g' % (dev_fw, dev_bw, count1, count3))
    assert dev_fw <= 1e-13 and dev_bw <= 1e-13
    assert count1 == count3 and count1 > 0
    eng.close()


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_update_sweep_is_repeatable(monkeypatch):
    """Two runs of the update sweep at the same S: bitwise equal pulses, psi(T) and g_a (K = 3 objectives on 3 x 4
    workgroups: the sums cross twelve workgroups in a fixed order)."""
    import torch

    monkeypatch.setenv('KH_KERNEL', 'ellsplit')
    r = _reference('lindblad_d12', False)
    spec, pulses = r['spec'], np.array(r['gp'])
    eng = _engine(spec, row_split=4)
    chi = eng.backward(r['chi_T'], pulses)
    args = (chi, r['norms'], spec.init, pulses, np.array(r['S']), np.array(r['lam']))
    first = eng.forward_update(*args)
    eng.check()
    again = eng.forward_update(*args)
    eng.check()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    with pytest.raises(_lib.KrotovHipError) as refused:  # a split engine keeps its own grid
        eng.set_update_workgroups(2)
    assert refused.value.code == _lib.KH_ERR_UNSUPPORTED
    assert eng.set_update_workgroups(0) == 12
    eng.close()


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_spin_chain_n13_on_eight_workgroups_per_objective():
    """Unforced, N = 8192, K = 2: the forward trajectories with ``row_split=8`` are bitwise those of ``row_split=2``,
    within 1e-13 of ``row_split=None`` (``"ellglobal/csr"``), and norms are conserved to 1e-12."""
    import torch

    from krotov_amd.engine import HipKrotovEngine

    spec = configs.config_spin_chain(13, nt=4, K=2)
    ops = configs.sparse_ops(spec)
    bounds = [float(abs(m).sum(axis=1).max()) for m in ops[0]]
    mid = 0.5 * (spec.tlist[1:] + spec.tlist[:-1]) / spec.tlist[-1]
    pulses = np.array([0.3 * np.sin(np.pi * mid) ** 2 + 0.1])
    rng = np.random.default_rng(29)
    init = rng.standard_normal((2, spec.N)) + 1j * rng.standard_normal((2, spec.N))
    init /= np.linalg.norm(init, axis=1)[:, None]
    eng = HipKrotovEngine(ops, np.diff(spec.tlist), op_norms=np.tile(bounds, 2))
    assert eng.kernel == 'ellglobal/csr' and eng.row_split == 1
    _, plain = eng.forward(pulses, init, store=True)
    eng.check()
    assert eng.set_row_split(8) == 8 and eng.kernel == 'ellsplit/csr'
    _, s8 = eng.forward(pulses, init, store=True)
    eng.check()
    assert eng.stats()['workgroups'] == 16
    eng.set_row_split(2)
    _, s2 = eng.forward(pulses, init, store=True)
    eng.check()
    assert torch.equal(s8, s2)
    dev = (s8 - plain).abs().max().item()
    err_norm = np.abs(np.linalg.norm(s8.cpu().numpy(), axis=2) - 1.0).max()
    print('N = 8192: row_split 8 against None %.1e; norms %.1e' % (dev, err_norm))
    assert dev <= 1e-13
    assert err_norm < 1e-12
    eng.close()


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_row_split_is_refused_where_no_global_form_runs():
    """A dense engine and an ``ell/csr`` engine answer KH_ERR_UNSUPPORTED, whatever the factor."""
    from krotov_amd.engine import HipKrotovEngine

    dense = configs.config_c5(K=2, N=12, nt=5, L=1, distinct=True)
    objectives_ops = [[dense.H0[k]] + [dense.Hc[k][l] for l in range(dense.L)] for k in range(dense.K)]
    sparse = configs.config_sparse_lindblad(d=5, nt=5, K=2)
    for eng, kernel in ((HipKrotovEngine(objectives_ops, np.diff(dense.tlist)), None), (_engine(sparse), 'ell/csr')):
        assert eng.kernel == kernel or (kernel is None and not eng.kernel.endswith('/csr'))
        for S in (1, 2):
            with pytest.raises(_lib.KrotovHipError) as refused:
                eng.set_row_split(S)
            assert refused.value.code == _lib.KH_ERR_UNSUPPORTED
        eng.close()
    with pytest.raises(_lib.KrotovHipError) as refused:
        _engine(sparse, row_split=2)
    assert refused.value.code == _lib.KH_ERR_UNSUPPORTED


@pytest.mark.gpu
@pytest.mark.no_oracle
def test_optimize_pulses_with_a_row_split(monkeypatch):
    """``optimize_pulses(..., propagator=DensityMatrixODEPropagator(row_split=2))`` on ``lindblad_d12`` under
    ``KH_KERNEL=ellsplit``, two iterations: the pulses are within 1e-11 of the same call with ``row_split=None``."""
    import scipy.sparse as sp

    import krotov_amd
    from krotov_amd.engine import LAST_ENGINE

    monkeypatch.setenv('KH_KERNEL', 'ellsplit')

    def run(row_split, kernel):
        spec = BUILD['lindblad_d12']()
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
                                         propagator=krotov_amd.propagators.DensityMatrixODEPropagator(row_split=row_split),
                                         chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2)
        assert LAST_ENGINE().kernel == kernel
        return np.array(res.optimized_controls)

    split = run(2, 'ellsplit/csr')
    plain = run(None, 'ellglobal/csr')
    dev = np.abs(split - plain).max()
    print('pulses after two iterations, row_split 2 against None: %.1e' % dev)
    assert dev < 1e-11 * max(1.0, np.abs(plain).max())
    assert np.abs(plain).max() > 0.0


# ---------------------------------------------------------------------------
# 3. host only
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('N,S', [(100, 4), (600, 3), (600, 4), (48, 2), (8192, 64), (2 ** 20, 64)])
def test_row_partition(N, S):
    """``kh_ellsplit_rows``: contiguous, disjoint ranges that cover [0, N), whole 64-row chunks except the global tail,
    chunk counts that differ by at most one with the larger ones first, empty parts only at the end."""
    lib = _lib.load()
    first, count = ctypes.c_int32(), ctypes.c_int32()
    parts = []
    for part in range(S):
        assert lib.kh_ellsplit_rows(N, S, part, ctypes.byref(first), ctypes.byref(count)) == 0
        parts.append((first.value, count.value))
    assert parts[0][0] == 0
    for (f0, c0), (f1, _) in zip(parts, parts[1:]):
        assert f1 == f0 + c0  # contiguous and disjoint
    assert parts[-1][0] + parts[-1][1] == N  # ... and they cover [0, N)
    for f, c in parts:
        assert c >= 0 and (f % 64 == 0 or c == 0)
        assert c % 64 == 0 or f + c == N  # only the global tail is ragged
    counts = [c for _, c in parts]
    empty = [c == 0 for c in counts]
    assert empty == sorted(empty)  # empty parts come last
    chunks = [(c + 63) // 64 for c in counts]
    assert max(chunks) - min(chunks) <= 1 and chunks == sorted(chunks, reverse=True)
    assert sum(chunks) == (N + 63) // 64
    if (N, S) == (100, 4):
        assert parts == [(0, 64), (64, 36), (100, 0), (100, 0)]
    assert lib.kh_ellsplit_rows(N, S, S, ctypes.byref(first), ctypes.byref(count)) == _lib.KH_ERR_INVALID


def test_registry_lists_the_split_form():
    names = _lib.kernel_instantiations()
    for want in (SWEEP, UPDATE, UPDATE_SO):
        assert want in names, want
    assert sum(n.startswith('kh_ellgs_') for n in names) == 3
    assert b'ellsplit/csr' in _lib.load().kh_version()
    assert 'kh_set_row_split' in _lib.SYMBOLS


def test_auto_row_split():
    """'auto': the largest power of two <= min(CUs // K, chunks // 8, 64), and 1 up to N = 4096 (placeholders until the
    measurement of scripts/perf_ellsplit.py is recorded: see the docstring of ``auto_row_split``)."""
    from krotov_amd.engine import auto_row_split

    assert auto_row_split(256, 1, 4096) == 1
    assert auto_row_split(256, 1, 8192) == 16      # 128 chunks / 8
    assert auto_row_split(256, 3, 131072) == 64    # 85 CUs per objective, 256 chunks / 8: capped at 64
    assert auto_row_split(256, 8, 131072) == 32
    assert auto_row_split(256, 300, 131072) == 1


def test_timed_out_split_engine_goes_back_to_one_workgroup_per_objective(monkeypatch, caplog):
    """``optimize_pulses`` on an engine whose first backward sweep reports KH_ERR_TIMEOUT while ``row_split == 2``: the
    engine is set to ``row_split=1``, the sweep is redone, the optimisation ends with the oracle's numbers and the reason
    is logged once, at INFO.  Driven on the CPU with the oracle-backed engine double."""
    import krotov_amd
    import krotov_amd.engine as engine_mod
    from helpers import oracle_optimize
    from oracle_engine_double import OracleEngineDouble

    script = {'timeouts': 0, 'calls': [], 'created': []}

    class Split(OracleEngineDouble):
        def __init__(self, ops, dt, is_super=False, row_split=None, **kw):
            super().__init__(ops, dt, is_super=is_super, **kw)
            self.row_split = 1 if row_split is None else row_split
            script['created'].append(row_split)

        def set_row_split(self, S):
            script['calls'].append(S)
            self.row_split = S
            return S

        def backward(self, *a, **kw):
            if self.row_split == 2:
                script['timeouts'] += 1
                raise _lib.KrotovHipError("in-kernel exchange timed out", _lib.KH_ERR_TIMEOUT)
            return super().backward(*a, **kw)

    monkeypatch.setattr(engine_mod, 'HipKrotovEngine', Split)
    caplog.set_level(logging.INFO, logger='krotov')
    spec = configs.config_c5(K=3, N=4, nt=9, L=1, distinct=True)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    ref = oracle_optimize(spec, 3)
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist,
                                     propagator=krotov_amd.propagators.HipExpm(sparse=True, row_split=2),
                                     chi_constructor=krotov_amd.functionals.chis_re, iter_stop=3, store_all_pulses=True)
    assert np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() < 1e-12
    assert script['created'] == [2] and script['calls'] == [1] and script['timeouts'] == 1
    assert caplog.text.count('the backward sweep timed out') == 1
    assert 'one workgroup per objective' in caplog.text
    info = [rec for rec in caplog.records if 'row split 2' in rec.getMessage()]
    assert len(info) == 1 and info[0].levelno == logging.INFO
