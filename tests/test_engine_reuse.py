"""Every kernel family on ONE engine that is reused with changed inputs.

``optimize_pulses`` keeps one engine for all iterations, overwrites the same co-state store, pulse, norm and trajectory
tensors in place, switches the engine between forms after a timeout (reduced grid, row split 1, one launch per
interval) and swaps the second-order trajectories every iteration -- while the engine carries state from call to call:
``d_phi``, ``d_slots``, ``d_wg_partial``, ``d_step_partial``, the adjoint-side stores (``d_gen_adj`` with
``gen_adj_ready``, ``d_coop_adj``), the cooperative ring, the sparse scratch planes and split counters, ``guess_dev``,
the second-order pointers, ``reduced_G``, ``row_split``, the replica mask, ``last_update_grid``; and
``HipKrotovEngine._sh`` with its captured HIP graph.  The other parity tests build a fresh engine per input set, so a
family that kept any of this from the previous call would pass them all.

Here every case gets two input sets on the same operators and time grid -- A: what ``build_problem`` of
tests/test_absent_controls.py makes; B: every input changed (``_set_b``) -- and ONE set of device tensors per engine:
the sets are switched with ``copy_``, every ``data_ptr()`` the engine sees stays what it was, and every output tensor is
filled with NaN before the sweep that has to write it.  The sequence (``run_sequence``):

1. A: forward with storage, backward, update sweep            -> the oracle; kept as ``out1``
2. B in the same tensors, the same three sweeps               -> the oracle; kept as ``out2``
3. A again (backward re-run: the store is rewritten in place) -> ``out1`` bit for bit
4. B one launch per interval, then A in one launch            -> the oracle; ``out1`` bit for bit
5. second order on A; B's trajectory and sigma copied into the same tensors (no new ``set_second_order``); off again
                                                              -> the oracle (with the written trajectory); ``out2`` bit for bit
6. B on a reduced grid, then A on the full one                -> the oracle; ``out1`` bit for bit (a refusal leaves no trace)
7. ellglobal: B with the rows split, then A without           -> the oracle; ``out1`` bit for bit

After every step the launch registry must hold exactly the update-kernel instantiation the step is meant to run.
Tolerances are the project's own: 1e-12 in Hilbert space, 1e-11 in Liouville space; pulses and g_a relative to
max(1, max|.|).  ``test_oracle_tells_a_stale_input`` (host only) shows for every case that a sweep of B with ONE input
left over from A moves the pulses or the final states by more than 1e-6: no stale input could pass.

Reference: optimize.py:392-581 (the driver's loop), :444-508 (update sweep), :849-886 (backward sweep)."""
import copy
import functools
import types
import zlib

import numpy as np
import pytest

import helpers
from krotov_amd import configs
from krotov_amd.engine import HipKrotovEngine
from oracle import krotov_oracle as ko
from test_absent_controls import TOL_HILBERT, TOL_LIOUVILLE, _check, _engine_ops, build_problem, compute_sweeps

WITNESS = 1e-6  # the project's witness threshold (tests/test_absent_controls.py): six orders above the tolerance


# ---------------------------------------------------------------------------
# the two input sets
# ---------------------------------------------------------------------------
def _set_a(p):
    """Input set A: what ``build_problem`` made, as arrays."""
    return types.SimpleNamespace(prob=p.prob, gp=np.array(p.gp), S=np.array(p.S), lam=np.array(p.lam, dtype=np.float64),
                                 norms=np.array(p.norms), chi_T=np.array(p.chi_T), older=np.array(p.older),
                                 sigma_vals=np.array(p.sigma_vals), tol=p.tol)


def _rows(rng, mask):
    """Random normalised complex rows, zero where ``mask`` is (behind N_k of a mixed problem)."""
    v = (rng.standard_normal(mask.shape) + 1j * rng.standard_normal(mask.shape)) * mask
    return v / np.linalg.norm(v, axis=1)[:, None]


def _set_b(a, seed, dims=None):
    """Input set B on A's operators and time grid; every input changes."""
    rng = np.random.default_rng(seed)
    K, N = a.prob.init.shape
    mask = np.arange(N)[None, :] < np.array(dims if dims is not None else [N] * K)[:, None]
    gp = np.array([0.7 * q[::-1] + 0.1 * np.cos(np.linspace(0, 3, len(q))) for q in a.gp])
    prob = copy.copy(a.prob)
    prob.init = _rows(rng, mask)
    return types.SimpleNamespace(
        prob=prob, gp=gp, S=np.array([0.5 * s[::-1] + 0.25 for s in a.S]),
        lam=np.array([1.7 * lam * (1.0 + 0.3 * l) for l, lam in enumerate(a.lam)]),
        norms=0.6 * a.norms[::-1] + 0.05 * rng.random(K), chi_T=_rows(rng, mask),
        older=gp * (1.0 + 0.2 * rng.standard_normal(gp.shape)), sigma_vals=0.6 * a.sigma_vals[::-1], tol=a.tol)


def _seed(key):
    return [zlib.crc32(key.encode()), 0xb]


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
PROBLEMS, CASES = {}, {}


def problem_of(key, build, fmt='dense'):
    PROBLEMS[key] = types.SimpleNamespace(build=build, fmt=fmt)


def case(name, kernel, plain, upd, step, so=None, reduced=None, env=None, prob=None, split=None):
    """``plain``: the instantiations of the forward and backward sweeps; ``upd`` / ``step`` / ``so``: the ONE update-kernel
    instantiation the single first-order launch / the launches per interval / the second-order launch must run (``so=None``:
    no second-order run); ``reduced``: (workgroups asked for, workgroups got, instantiation) of the reduced grid, ``None``
    where the family refuses one; ``split``: the instantiations of the sweeps with the rows split (step 7)."""
    CASES[name] = types.SimpleNamespace(kernel=kernel, plain=tuple(plain), upd=upd, step=step, so=so, reduced=reduced,
                                        env=dict(env or {}), prob=prob or name, split=split)
    assert CASES[name].prob in PROBLEMS, name


def _c5(K, N, nt=9, L=1, distinct=False):
    return lambda: configs.config_c5(K=K, N=N, nt=nt, L=L, distinct=distinct)


_GEN, _TILE1 = 'kh_gen_forward_update<false>', 'kh_tile_forward_update<1, %d, false, false>'

# ---- one wave per objective (kh_mini.h); one launch per interval: the one-term-per-phase tile kernel
problem_of('mini4', _c5(3, 3))
problem_of('mini16', _c5(5, 7))
case('mini4', 'mini4/wave', ['kh_quad_sweep_store'], 'kh_quad_forward_update<false>', _TILE1 % 1, so='kh_quad_forward_update<true>')
case('mini16', 'mini16/wave', ['kh_mini_sweep_store'], 'kh_mini_forward_update<false>', _TILE1 % 1, so='kh_mini_forward_update<true>')

# ---- two terms per phase (kh_tile64q2.h): <second order, sums on the adjoint side, single GPU>; reduced grid: the streaming
# kernel <controls, second order, N == 64> on half the objectives' workgroups
problem_of('q2_n17', _c5(5, 17, distinct=True))
problem_of('q2_n64', _c5(3, 64, distinct=True))
case('q2_n17', 'tile64q2/512', ['kh_q2_sweep_store'], 'kh_q2_forward_update<false, true, true>', _TILE1 % 1,
     so='kh_q2_forward_update<true, false, true>', reduced=(3, 3, 'kh_stream_forward_update<1, false, false>'))
case('q2_n64', 'tile64q2/512', ['kh_q2_sweep_store'], 'kh_q2_forward_update<false, true, true>', _TILE1 % 1,
     so='kh_q2_forward_update<true, false, true>', reduced=(2, 2, 'kh_stream_forward_update<1, false, true>'))
case('q2_n17_fwd_side', 'tile64q2/512', ['kh_q2_sweep_store'], 'kh_q2_forward_update<false, false, true>', _TILE1 % 1,
     reduced=(3, 3, 'kh_stream_forward_update<1, false, false>'), env={'KH_NO_ADJ': '1'}, prob='q2_n17')

# ---- one term per phase (kh_tile64.h): <rows per thread, controls, second order, single GPU>
for _l in (2, 3, 4):
    problem_of('tile512_L%d' % _l, _c5(4, 17, L=_l, distinct=True))
    case('tile512_L%d' % _l, 'tile64/512', ['kh_tile_sweep_store<1, %d>' % _l], 'kh_tile_forward_update<1, %d, false, true>' % _l,
         _TILE1 % _l, so='kh_tile_forward_update<1, %d, true, true>' % _l,
         reduced=(2, 2, 'kh_stream_forward_update<%d, false, false>' % _l))
# two workgroups per compute unit (the shape of test_update_sweep_on_fewer_workgroups' c5_k300: 100 workgroups)
problem_of('tile256', _c5(300, 16, nt=6, distinct=True))
case('tile256', 'tile64/256', ['kh_q2_sweep_store'], 'kh_tile_forward_update<2, 1, false, true>', 'kh_tile_forward_update<2, 1, false, false>',
     so='kh_tile_forward_update<2, 1, true, true>', reduced=(100, 100, 'kh_stream_forward_update<1, false, false>'))

# ---- more objectives than co-resident workgroups (kh_tile64s.h): 135 x 2 and 130 x 2 objectives; reduced: 68 x 4, 65 x 4
problem_of('stream_L4_n8', _c5(270, 8, nt=6, L=4))
problem_of('stream_L3_n64', _c5(260, 64, nt=4, L=3, distinct=True))
case('stream_L4_n8', 'tile64/stream', ['kh_tile_sweep_store<1, 4>'], 'kh_stream_forward_update<4, false, false>', _TILE1 % 4,
     so='kh_stream_forward_update<4, true, false>', reduced=(68, 68, 'kh_stream_forward_update<4, false, false>'))
case('stream_L3_n64', 'tile64/stream', ['kh_tile_sweep_store<1, 3>'], 'kh_stream_forward_update<3, false, true>', _TILE1 % 3,
     so='kh_stream_forward_update<3, true, true>', reduced=(65, 65, 'kh_stream_forward_update<3, false, true>'))

# ---- ensembles (kh_ens.h): <column groups, second order>; kh_ens2_forward_update<2>: the A^2 chain with the sums on the
# adjoint side, first order and two column groups only -- which is also what 300 objectives get on 75 workgroups, while
# 520 objectives on 65 take four column groups; second order of the ens2 engine: kh_ens_forward_update<2, true>
problem_of('ens', _c5(300, 16, nt=6))
problem_of('ens2', _c5(520, 8, nt=12))  # (the k520_n8 row of tests/test_series_regimes.py)
case('ens', 'ens64/mfma', ['kh_q2_sweep_store'], 'kh_ens_forward_update<1, false>', 'kh_tile_forward_update<2, 1, false, false>',
     so='kh_ens_forward_update<1, true>', reduced=(75, 75, 'kh_ens2_forward_update<2>'))
case('ens2', 'ens64/mfma', ['kh_q2_sweep_store'], 'kh_ens2_forward_update<2>', _TILE1 % 1,
     so='kh_ens_forward_update<2, true>', reduced=(65, 65, 'kh_ens_forward_update<4, false>'))

# ---- five to eight controls (kh_tile64x.h): no second-order and no per-interval kernel of its own -- the generic one
problem_of('tx_L6', _c5(3, 20, L=6, distinct=True))
case('tx_L6', 'tile64x/512', ['kh_tx_sweep_store<6>'], 'kh_tx_forward_update<6>', _GEN, so=_GEN)

# ---- the generator in registers, 64 < N <= 128 (kh_tilen.h): <elements per lane, [second order,] H1 in registers>; several
# controls: the adjoint-side store
problem_of('tn_n70', _c5(3, 70))
problem_of('tn_n90_L2', _c5(3, 90, L=2))
case('tn_n70', 'tile128/512', ['kh_tn_sweep_store<20, true>'], 'kh_tn_forward_update<20, false, true>', _GEN,
     so='kh_tn_forward_update<20, true, true>')
case('tn_n90_L2', 'tile128/512', ['kh_tn_sweep_store<24, false>'], 'kh_tn_forward_update<24, false, false>', _GEN,
     so='kh_tn_forward_update<24, true, false>')

# ---- generic kernels (kh_generic.h), the update sums on the adjoint side (d_gen_adj) and on the forward side
problem_of('generic', _c5(4, 33, distinct=True))
case('generic', 'generic', ['kh_gen_sweep_store<false>'], _GEN, _GEN, so=_GEN, env={'KH_KERNEL': 'generic'})
case('generic_fwd_side', 'generic', ['kh_gen_sweep_store<false>'], _GEN, _GEN, env={'KH_KERNEL': 'generic', 'KH_GEN_ADJ': '0'},
     prob='generic')

# ---- cooperative matrix-core kernels (kh_coop.h): <slots, objectives per workgroup, second order, sums on the adjoint side,
# A^2 chain, cross-GPU stage>; one launch per interval: the generic kernel
for _name, _K, _L in (('coop_L1', 4, 1), ('coop_L1_c16', 20, 1), ('coop_L2', 4, 2)):
    problem_of(_name, lambda K=_K, L=_L: configs.config_shared(K=K, N=96, nt=4, L=L))
case('coop_L1', 'coop16/mfma', ['kh_coop_sweep_store<8, 4, true>'], 'kh_coop_forward_update<8, 4, false, true, true, false>', _GEN,
     so='kh_coop_forward_update<8, 4, true, false, true, true>')
case('coop_L1_c16', 'coop16/mfma', ['kh_coop_sweep_store<8, 16, true>'], 'kh_coop_forward_update<8, 16, false, true, true, false>', _GEN,
     so='kh_coop_forward_update<8, 16, true, false, true, true>', env={'KH_COOP_COLS': '16'})
case('coop_L2', 'coop16/mfma', ['kh_coop_sweep_store<8, 4, false>'], 'kh_coop_forward_update<8, 4, false, false, false, true>', _GEN,
     so='kh_coop_forward_update<8, 4, true, false, false, true>')

# ---- sparse operators (kh_ell.h, kh_ellg.h in both forms, the generic CSR kernels): the d = 5 Lindbladian; one launch per
# interval: the generic CSR kernel
problem_of('ell', lambda: configs.config_sparse_lindblad(d=5, nt=9, K=3), fmt='csr')
case('ell', 'ell/csr', ['kh_ell_sweep_store<512, 1, 8, false>'], 'kh_ell_forward_update<512, 1, 8, false, false>', _GEN,
     so='kh_ell_forward_update<512, 1, 8, true, false>')
case('ellstream', 'ellstream/csr', ['kh_ell_sweep_store<512, 8, 4, true>'], 'kh_ell_forward_update<512, 8, 4, false, true>', _GEN,
     so='kh_ell_forward_update<512, 8, 4, true, true>', env={'KH_KERNEL': 'ellstream'}, prob='ell')
case('ellglobal', 'ellglobal/csr', ['kh_ellg_sweep_store<512>'], 'kh_ellg_forward_update<512, false>', _GEN,
     so='kh_ellg_forward_update<512, true>', reduced=(2, 2, 'kh_ellg_forward_update<512, false>'), env={'KH_KERNEL': 'ellglobal'},
     prob='ell', split=('kh_ellgs_sweep_store<512>', 'kh_ellgs_forward_update<512, false>'))
case('generic_csr', 'generic/csr', ['kh_gen_sweep_store<false>'], _GEN, _GEN, env={'KH_KERNEL': 'generic'}, prob='ell')

# ---- objectives of different dimension and kind (kh_engine_create_mixed), against the restatement of
# tests/test_mixed_objectives.py (``oracle_adapter``, through ``build_problem``)
problem_of('mixed', lambda: configs.config_mixed('dims', nt=11), fmt='mixed')
case('mixed', 'generic/mixed', ['kh_gen_sweep_store<true>'], 'kh_gen_forward_update<true>', 'kh_gen_forward_update<true>',
     so='kh_gen_forward_update<true>')

# ---- the captured HIP graph of the per-interval form (section "graph" below): 11 intervals, blocks of 4
GRAPH_CHUNK = 4
problem_of('q2_n17_nt12', _c5(5, 17, nt=12, distinct=True))
problem_of('generic_nt12', _c5(4, 33, nt=12, distinct=True))
problem_of('mixed_nt12', lambda: configs.config_mixed('dims', nt=12), fmt='mixed')
GRAPH_CASES = {
    'q2_n17': types.SimpleNamespace(prob='q2_n17_nt12', kernel='tile64q2/512', step=_TILE1 % 1, env={}),
    'generic': types.SimpleNamespace(prob='generic_nt12', kernel='generic', step=_GEN, env={'KH_KERNEL': 'generic'}),
    'mixed': types.SimpleNamespace(prob='mixed_nt12', kernel='generic/mixed', step='kh_gen_forward_update<true>', env={}),
}


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(problem of ``build_problem``, set A, set B) of a problem of the table (built once; never modified)."""
    pr = PROBLEMS[key]
    spec = pr.build()
    p = build_problem(pr, spec)
    a = _set_a(p)
    return p, a, _set_b(a, _seed(key), getattr(spec, 'dims', None))


def _second_order(key):
    return any(c.so is not None for c in CASES.values() if c.prob == key)


@functools.lru_cache(maxsize=None)
def oracle(key):
    """The oracle's sweeps of both sets (``compute_sweeps``: under ``MemoExpm``), computed once and shared by the GPU tests
    and the witness (never modified)."""
    _, a, b = inputs(key)
    return compute_sweeps(a, _second_order(key)), compute_sweeps(b, _second_order(key))


# ---------------------------------------------------------------------------
# host only: the table, and the witness that no stale input could pass
# ---------------------------------------------------------------------------
_INPUTS = ('gp', 'S', 'lam', 'norms', 'chi_T', 'older', 'sigma_vals')


def test_case_table_is_what_it_says():
    """Every case builds; A and B share the operators and the time grid; no input of B is A's; the shapes are small."""
    from krotov_amd import _lib

    names = set(_lib.kernel_instantiations())
    for name, c in CASES.items():
        p, a, b = inputs(c.prob)
        assert b.prob.ops is a.prob.ops and b.prob.tlist is a.prob.tlist and b.prob.target is a.prob.target, name
        assert b.prob.init.shape == a.prob.init.shape and not np.array_equal(b.prob.init, a.prob.init), name
        for what in _INPUTS:
            x, y = getattr(a, what), getattr(b, what)
            assert x.shape == y.shape and np.abs(x - y).max() > 1e-3 * np.abs(x).max(), (name, what)
        assert np.all(b.S[:, 0] != 0.0) and np.all(b.S[:, -1] != 0.0), name  # (non-zero at both ends)
        assert np.allclose(np.linalg.norm(b.prob.init, axis=1), 1.0) and np.allclose(np.linalg.norm(b.chi_T, axis=1), 1.0)
        if PROBLEMS[c.prob].fmt == 'mixed':  # (zeros behind N_k, as the engine writes them)
            assert len(set(p.spec.dims)) > 1
            assert all(np.all(b.prob.init[k, n:] == 0) and np.all(b.chi_T[k, n:] == 0) for k, n in enumerate(p.spec.dims)), name
        assert 3 <= len(p.spec.tlist) - 1 <= 10 or name == 'ens2', name
        for want in c.plain + (c.upd, c.step) + ((c.so,) if c.so else ()) + ((c.reduced[2],) if c.reduced else ()) + (c.split or ()):
            assert want in names, (name, want)
    for g in GRAPH_CASES.values():
        nt = len(inputs(g.prob)[0].spec.tlist)
        assert nt - 1 > 2 * GRAPH_CHUNK and g.step in names  # (forward_update_sharded replays a graph from there on)
    assert len({c.prob for c in CASES.values()}) + len(GRAPH_CASES) == len(PROBLEMS)


def _moved(x, y):
    return max(float(np.abs(np.array(x[0]) - np.array(y[0])).max()), float(np.abs(x[1] - y[1]).max()))


@pytest.mark.parametrize('key', sorted(PROBLEMS))
def test_oracle_tells_a_stale_input(key):
    """What an engine holding ONE input of A while it runs B would compute -- B's update sweep with A's init, co-state
    store, norms, guess, shapes or lambda; second order: with A's previous trajectory or sigma -- moves the pulses or the
    final states by more than 1e-6, six orders above the tolerance; and A and B themselves differ by more than that in every
    compared quantity."""
    _, a, b = inputs(key)
    ref_a, ref_b = oracle(key)
    both = dict(states=(ref_a.states, ref_b.states), fw_T=(ref_a.fw_T, ref_b.fw_T), chi=(ref_a.chi, ref_b.chi),
                opt=(ref_a.update[0], ref_b.update[0]), psi_T=(ref_a.update[1], ref_b.update[1]),
                g_a=(ref_a.update[2], ref_b.update[2]))
    if ref_a.so is not None:
        both.update(so_opt=(ref_a.so[0], ref_b.so[0]), so_psi_T=(ref_a.so[1], ref_b.so[1]), so_g_a=(ref_a.so[2], ref_b.so[2]),
                    so_store=(ref_a.so[3], ref_b.so[3]))
    apart = {what: float(np.abs(np.array(x) - np.array(y)).max()) for what, (x, y) in both.items()}
    print('%s A against B: %s' % (key, ', '.join('%s %.2e' % kv for kv in apart.items())))
    for what, d in apart.items():
        assert d > WITNESS, (key, what, d)

    def sweep(prob=b.prob, chi=ref_b.chi, norms=b.norms, gp=b.gp, S=b.S, lam=b.lam, **so):
        return ko.forward_update_sweep(prob, chi, norms, gp, S, lam, **so)

    with helpers.MemoExpm():
        stale = dict(init=sweep(prob=a.prob), chi_store=sweep(chi=ref_a.chi), norms=sweep(norms=a.norms), guess=sweep(gp=a.gp),
                     shapes=sweep(S=a.S), lam=sweep(lam=a.lam))
        moved = {what: _moved(got, ref_b.update) for what, got in stale.items()}
        if ref_b.so is not None:
            moved['prev'] = _moved(sweep(sigma_vals=b.sigma_vals, fw_prev=ref_a.prev), ref_b.so)
            moved['sigma_vals'] = _moved(sweep(sigma_vals=a.sigma_vals, fw_prev=ref_b.prev), ref_b.so)
    print('%s B with one input of A: %s' % (key, ', '.join('%s %.2e' % kv for kv in moved.items())))
    for what, d in moved.items():
        assert d > WITNESS, (key, what, d)


# ---------------------------------------------------------------------------
# GPU: one set of device tensors per engine
# ---------------------------------------------------------------------------
class Device:
    """The tensors an engine sees during a whole test, allocated once: inputs (``put`` copies a set into them), the
    co-state store, the second-order pair and every sweep's ``out=``.  Replica engines: ``B`` replicas."""

    def __init__(self, eng, B=0):
        import torch

        self.eng, self.torch = eng, torch
        K, N, L, nt = eng.K, eng.N, eng.L, eng.nt
        c128, f64 = torch.complex128, torch.float64
        pulse, ctl, sig = ((B, L, nt - 1), (B, L), (B, nt - 1)) if B else ((L, nt - 1), (L,), (nt - 1,))

        def new(shape, dtype):
            return torch.zeros(shape, dtype=dtype, device=eng.device)

        self.t = dict(gp=new(pulse, f64), S=new(pulse, f64), lam=new(ctl, f64), norms=new((K,), f64), init=new((K, N), c128),
                      chi_T=new((K, N), c128), chi=new((K, nt, N), c128), prev=new((K, nt, N), c128), store=new((K, nt, N), c128),
                      sigma=new(sig, f64), opt=new(pulse, f64), psi_T=new((K, N), c128), g_a=new(ctl, f64),
                      fw_T=new((K, N), c128), states=new((K, nt, N), c128))
        self.ptrs = self._ptrs()
        self.second_order = False

    def _ptrs(self):
        return {name: x.data_ptr() for name, x in self.t.items()}

    def unchanged(self):
        """Every tensor is where it was (asserted at the end of every test)."""
        assert self._ptrs() == self.ptrs
        return True

    def _copy(self, name, host):
        self.t[name].copy_(self.torch.from_numpy(np.ascontiguousarray(host)))

    def put(self, s):
        for name in ('gp', 'S', 'lam', 'norms', 'chi_T'):
            self._copy(name, getattr(s, name))
        self._copy('init', s.prob.init)

    def put_second_order(self, prev, sigma_vals):
        self._copy('prev', prev)
        self._copy('sigma', sigma_vals)

    def nan(self, *names):
        for name in names:
            x = self.t[name]
            x.fill_(complex(float('nan'), float('nan')) if x.is_complex() else float('nan'))

    def host(self, *names):
        return tuple(self.t[name].cpu().numpy() for name in names)

    def forward(self, fill=True):
        t = self.t
        if fill:
            self.nan('fw_T', 'states')
        got = self.eng.forward(t['gp'], t['init'], store=True, out=(t['fw_T'], t['states']))
        assert got[0] is t['fw_T'] and got[1] is t['states']
        self.eng.check()
        return self.host('fw_T', 'states')

    def backward(self, fill=True):
        t = self.t
        if fill:
            self.nan('chi')
        assert self.eng.backward(t['chi_T'], t['gp'], out=t['chi']) is t['chi']
        self.eng.check()
        return self.host('chi')[0]

    def args(self, chi=None):
        t = self.t
        return (t['chi'] if chi is None else chi, t['norms'], t['init'], t['gp'], t['S'], t['lam'])

    def update(self, fill=True):
        """The single-launch update sweep into the ``out=`` triple; host copies (opt, psi_T, g_a[, store])."""
        t = self.t
        if fill:
            self.nan('opt', 'psi_T', 'g_a', *(('store',) if self.second_order else ()))
        got = self.eng.forward_update(*self.args(), out=(t['opt'], t['psi_T'], t['g_a']))
        assert all(x is t[name] for x, name in zip(got, ('opt', 'psi_T', 'g_a')))
        self.eng.check()
        return self.host('opt', 'psi_T', 'g_a', *(('store',) if self.second_order else ()))

    def sharded(self, graph_chunk, chi=None):
        got = self.eng.forward_update_sharded(*self.args(chi), lambda x: x, graph_chunk=graph_chunk)
        self.eng.check()
        return tuple(x.cpu().numpy() for x in got)


def _update_errs(got, ref):
    """Against the oracle's (opt, psi_T, g_a[, store]); pulses and g_a relative to max(1, max|.|)."""
    opt, ga = np.array(ref[0]), np.array(ref[2])
    errs = dict(opt=np.abs(got[0] - opt).max() / max(1.0, np.abs(opt).max()), psi_T=np.abs(got[1] - ref[1]).max(),
                g_a=np.abs(got[2] - ga).max() / max(1.0, np.abs(ga).max()))
    if len(ref) > 3:
        errs['fw_store'] = np.abs(got[3] - ref[3]).max()
    return errs


def _bitwise(got, want, name, what):
    """``got`` equals ``want`` bit for bit (the largest difference is printed first)."""
    apart = [float(np.abs(x - y).max()) if not np.array_equal(x, y) else 0.0 for x, y in zip(got, want)]
    print('%s %s: bit for bit %s (max difference %s)' % (name, what, all(np.array_equal(x, y) for x, y in zip(got, want)),
                                                          ', '.join('%.2e' % d for d in apart)))
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x, y), (name, what, i, apart[i])


def _ran(name, what, update, also=()):
    """The registry holds exactly ``update`` as update-kernel instantiations (and ``also``) since it was last emptied;
    empties it for the next step."""
    from krotov_amd import _lib

    launched = list(_lib.kernel_instantiations(launched_only=True))
    print('%s %s launched: %s' % (name, what, ', '.join(launched)))
    assert sorted(n for n in launched if 'forward_update' in n) == sorted(set(update)), (name, what, update, launched)
    for want in also:
        assert want in launched, (name, what, want, launched)
    _lib.forget_launched_kernels()


def _refuses(call):
    from krotov_amd import _lib

    with pytest.raises(_lib.KrotovHipError) as err:
        call()
    assert err.value.code == _lib.KH_ERR_UNSUPPORTED


def _plain_and_update(dev, s, ref, name, what, c):
    """Step 1 / 2: the three sweeps of set ``s`` in the engine's tensors against the oracle; returns the update's result."""
    dev.put(s)
    fw_T, states = dev.forward()
    chi = dev.backward()
    got = dev.update()
    errs = dict(states=np.abs(states - ref.states).max(), fw_T=np.abs(fw_T - ref.fw_T).max(), chi=np.abs(chi - ref.chi).max())
    errs.update(_update_errs(got, ref.update))
    _check(errs, s.tol, name, what)
    _ran(name, what, [c.upd], c.plain)
    return got


def _switch_to(dev, s, ref, name, what):
    """Set ``s`` into the tensors and its co-state store rewritten in place (against the oracle)."""
    dev.put(s)
    _check(dict(chi=np.abs(dev.backward() - ref.chi).max()), s.tol, name, what + ', backward')


def run_sequence(name, c, monkeypatch, device_cls=Device, engine_cls=HipKrotovEngine):
    from krotov_amd import _lib


    for key, value in c.env.items():
        monkeypatch.setenv(key, value)
    p, a, b = inputs(c.prob)
    ref_a, ref_b = oracle(c.prob)
    spec, fmt = p.spec, PROBLEMS[c.prob].fmt
    eng = engine_cls(_engine_ops(spec, fmt), np.diff(spec.tlist), is_super=spec.kinds if fmt == 'mixed' else spec.is_super)
    try:
        assert eng.kernel == c.kernel
        dev = device_cls(eng)
        _lib.forget_launched_kernels()
        # 1., 2.: A, then B in the same tensors
        out1 = _plain_and_update(dev, a, ref_a, name, '1. A', c)
        out2 = _plain_and_update(dev, b, ref_b, name, '2. B', c)
        # 3.: A again
        _switch_to(dev, a, ref_a, name, '3. A again')
        _bitwise(dev.update(), out1, name, '3. A again')
        _ran(name, '3. A again', [c.upd], c.plain)
        # 4.: B one launch per interval, A in one launch
        _switch_to(dev, b, ref_b, name, '4. B per interval')
        got = dev.sharded(0)
        _check(_update_errs(got, ref_b.update), b.tol, name, '4. B per interval')
        _ran(name, '4. B per interval', [c.step], c.plain)
        _switch_to(dev, a, ref_a, name, '4. A in one launch')
        _bitwise(dev.update(), out1, name, '4. A in one launch')
        _ran(name, '4. A in one launch', [c.upd])
        # 5.: second order on A; B's trajectory and sigma into the same tensors; off again
        if c.so is not None:
            t = dev.t
            dev.put_second_order(ref_a.prev, a.sigma_vals)
            eng.set_second_order(t['prev'], t['store'], t['sigma'])
            dev.second_order = True
            _check(_update_errs(dev.update(), ref_a.so), a.tol, name, '5. second order, A')
            _switch_to(dev, b, ref_b, name, '5. second order, B')
            dev.put_second_order(ref_b.prev, b.sigma_vals)
            _check(_update_errs(dev.update(), ref_b.so), b.tol, name, '5. second order, B')
            _ran(name, '5. second order', [c.so])
            eng.set_second_order()
            dev.second_order = False
            _bitwise(dev.update(), out2, name, '5. first order again, B')
            _ran(name, '5. first order again, B', [c.upd])
        else:
            _switch_to(dev, b, ref_b, name, '6. B')
        # 6.: B on a reduced grid, A on the full one (the tensors hold B here)
        _lib.forget_launched_kernels()
        full = eng.set_update_workgroups(0)
        if c.reduced is not None:
            ask, want, kernel = c.reduced
            assert eng.set_update_workgroups(ask) == want and want < full
            _check(_update_errs(dev.update(), ref_b.update), b.tol, name, '6. B on %d of %d workgroups' % (want, full))
            assert eng.stats()['workgroups'] == want
            _ran(name, '6. B on a reduced grid', [kernel])
            assert eng.set_update_workgroups(0) == full
        else:
            _refuses(lambda: eng.set_update_workgroups(2))
        _switch_to(dev, a, ref_a, name, '6. A on the full grid')
        _bitwise(dev.update(), out1, name, '6. A on the full grid')
        _ran(name, '6. A on the full grid', [c.upd])
        # 7.: B with every objective's rows on two workgroups, A on one
        if c.split is not None:
            assert eng.set_row_split(2) == 2 and eng.kernel == 'ellsplit/csr'
            _switch_to(dev, b, ref_b, name, '7. B, rows split')
            _check(_update_errs(dev.update(), ref_b.update), b.tol, name, '7. B, rows split')
            _ran(name, '7. B, rows split', [c.split[1]], [c.split[0]])
            assert eng.set_row_split(1) == 1 and eng.kernel == c.kernel
            _switch_to(dev, a, ref_a, name, '7. A, rows whole')
            _bitwise(dev.update(), out1, name, '7. A, rows whole')
            _ran(name, '7. A, rows whole', [c.upd], c.plain)
        else:
            _refuses(lambda: eng.set_row_split(2))
        assert dev.unchanged() and dev.t['chi'].data_ptr() == dev.ptrs['chi']
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_engine_reused_with_changed_inputs(name, monkeypatch):
    run_sequence(name, CASES[name], monkeypatch)


# ---------------------------------------------------------------------------
# GPU: the captured HIP graph of the per-interval form
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(GRAPH_CASES))
def test_captured_graph_reused_with_changed_inputs(name, monkeypatch, device_cls=Device, engine_cls=HipKrotovEngine):
    """``forward_update_sharded`` replays a graph captured for (co-state store address, block length): B in the same
    tensors hits the cache, a store at another address re-captures, a plain-loop sweep in between disturbs nothing."""
    from krotov_amd import _lib

    g = GRAPH_CASES[name]
    for key, value in g.env.items():
        monkeypatch.setenv(key, value)
    p, a, b = inputs(g.prob)
    ref_a, ref_b = oracle(g.prob)
    spec, fmt = p.spec, PROBLEMS[g.prob].fmt
    eng = engine_cls(_engine_ops(spec, fmt), np.diff(spec.tlist), is_super=spec.kinds if fmt == 'mixed' else spec.is_super)
    try:
        assert eng.kernel == g.kernel and eng.nt - 1 > 2 * GRAPH_CHUNK
        dev = device_cls(eng)
        _lib.forget_launched_kernels()

        def replay(s, ref, what, chi=None):
            if chi is None:
                _switch_to(dev, s, ref, name, what)
            got = dev.sharded(GRAPH_CHUNK, chi)
            _check(_update_errs(got, ref.update), s.tol, name, what)
            _ran(name, what, [g.step])
            return got

        first = replay(a, ref_a, 'A, capture')
        graph, key = eng._sh['graph'], eng._sh['graph_key']
        assert graph is not None and key == (dev.ptrs['chi'], GRAPH_CHUNK)
        replay(b, ref_b, 'B, replay')
        assert eng._sh['graph'] is graph and eng._sh['graph_key'] == key
        _bitwise(replay(a, ref_a, 'A, replay'), first, name, 'A, replay')
        assert eng._sh['graph'] is graph
        # a sweep of the plain loop in between
        _switch_to(dev, b, ref_b, name, 'B, plain loop')
        _check(_update_errs(dev.sharded(0), ref_b.update), b.tol, name, 'B, plain loop')
        _ran(name, 'B, plain loop', [g.step])
        _bitwise(replay(a, ref_a, 'A, replay after the plain loop'), first, name, 'A, replay after the plain loop')
        assert eng._sh['graph'] is graph and eng._sh['graph_key'] == key
        # the co-state store at another address
        clone = dev.t['chi'].clone()
        assert clone.data_ptr() != dev.ptrs['chi']
        replay(a, ref_a, 'A, store at another address', chi=clone)
        assert eng._sh['graph'] is not graph and eng._sh['graph_key'] == (clone.data_ptr(), GRAPH_CHUNK)
        assert dev.unchanged()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# GPU: Lindblad form (kh_lind.h)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lindblad_inputs():
    """(case, A, B, oracle of A, oracle of B) of ``test_lindblad_form._random(5, 3, 2, 2, 13, seed)``; A: the inputs of
    tests/test_lindblad_form.py's sweep test."""
    import test_lindblad_form as tlf

    case_ = tlf._random(5, 3, 2, 2, 13, 21)
    prob = case_.oracle()
    rng = np.random.default_rng(5)
    M = len(case_.dt)
    a = types.SimpleNamespace(prob=prob, gp=np.array(tlf._pulses(case_)), S=np.array([np.linspace(0.2, 1.0, M)] * case_.L),
                              lam=np.array([0.7 + 0.3 * l for l in range(case_.L)]), norms=0.5 * (1.0 + rng.random(case_.K)) / case_.K,
                              chi_T=prob.target / np.linalg.norm(prob.target, axis=1)[:, None], older=np.zeros((case_.L, M)),
                              sigma_vals=-np.ones(M), tol=TOL_LIOUVILLE)
    b = _set_b(a, _seed('lindblad_form'))
    return case_, a, b, compute_sweeps(a, False), compute_sweeps(b, False)


def test_lindblad_inputs_differ():
    _, a, b, ref_a, ref_b = lindblad_inputs()
    for what in ('gp', 'S', 'lam', 'norms', 'chi_T'):
        assert np.abs(getattr(a, what) - getattr(b, what)).max() > 1e-3, what
    assert _moved(ref_a.update, ref_b.update) > WITNESS and np.abs(ref_a.chi - ref_b.chi).max() > WITNESS


@pytest.mark.gpu
def test_lindblad_engine_reused_with_changed_inputs(device_cls=Device, engine_cls=HipKrotovEngine):
    import torch

    from krotov_amd import _lib

    case_, a, b, ref_a, ref_b = lindblad_inputs()
    name = 'lindblad_form'
    c = types.SimpleNamespace(plain=('kh_lind_sweep_store<1>',), upd='kh_lind_forward_update<1>')
    eng = engine_cls(case_.H, case_.dt, c_ops=case_.C)
    try:
        assert eng.kernel == 'lindblad/matrix'
        dev = device_cls(eng)
        _lib.forget_launched_kernels()
        out1 = _plain_and_update(dev, a, ref_a, name, '1. A', c)
        _plain_and_update(dev, b, ref_b, name, '2. B', c)
        _switch_to(dev, a, ref_a, name, '3. A again')
        _bitwise(dev.update(), out1, name, '3. A again')
        _ran(name, '3. A again', [c.upd], c.plain)
        # 4., 5. (and the reduced grid): refused, and no trace of the refusals
        _refuses(lambda: dev.sharded(0))
        _refuses(lambda: eng.set_second_order(dev.t['prev'], dev.t['store'], dev.t['sigma']))
        _refuses(lambda: eng.set_update_workgroups(2))
        torch.cuda.synchronize()
        _bitwise(dev.update(), out1, name, 'A after the refusals')
        _ran(name, 'A after the refusals', [c.upd])
        assert dev.unchanged()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# GPU: replica engines (kh_replica.h)
# ---------------------------------------------------------------------------
REPLICAS = 'L2'  # tests/test_replicas.py: batch('L2'), the first three replicas (two objectives, N = 7, two controls)


@functools.lru_cache(maxsize=None)
def replica_inputs():
    """Per replica (A, B, oracle of A, oracle of B) with the second-order sweeps; A: the replica's own inputs."""
    import test_replicas as tr
    import test_replicas_second_order as trs

    reps = list(tr.batch(REPLICAS)[:3])
    sig = trs.sigma_rows(reps)
    out = []
    for i, r in enumerate(reps):
        rng = np.random.default_rng(17 + i)
        gp = np.array(r.pulses)
        a = types.SimpleNamespace(prob=helpers.spec_to_oracle(r), gp=gp, S=np.array(r.shapes), lam=np.array(r.lambdas, dtype=np.float64),
                                  norms=np.array(r.chi_norms), chi_T=r.target / np.linalg.norm(r.target, axis=1)[:, None],
                                  older=gp * (1.0 + 0.2 * rng.standard_normal(gp.shape)), sigma_vals=sig[i], tol=TOL_HILBERT)
        b = _set_b(a, _seed('replica %d' % i))
        out.append((a, b, compute_sweeps(a, True), compute_sweeps(b, True)))
    return reps, out


def test_replica_inputs_differ():
    for a, b, ref_a, ref_b in replica_inputs()[1]:
        for what in _INPUTS:
            assert np.abs(getattr(a, what) - getattr(b, what)).max() > 1e-3 * np.abs(getattr(a, what)).max(), what
        assert _moved(ref_a.update, ref_b.update) > WITNESS and _moved(ref_a.so, ref_b.so) > WITNESS
        assert _moved(ref_a.so, ref_a.update) > WITNESS  # (the sigma term is really on)


@pytest.mark.gpu
def test_replica_engine_reused_with_changed_inputs_and_mask(device_cls=Device, engine_cls=HipKrotovEngine):
    """All replicas on A; replica 1 off and B in the same tensors: the others are the oracle's B, replica 1's slices of
    every output still hold A's values bit for bit; all on A again: the first run bit for bit.  The same with one sigma
    row per replica (``set_second_order_replicas``), B's rows copied into the same tensor; and off again."""
    import test_replicas as tr
    from krotov_amd import _lib

    reps, sets = replica_inputs()
    nB, Kr, L = len(reps), reps[0].K, reps[0].L
    name = 'replicas'
    arrays = tr._inputs(reps)
    eng = engine_cls(arrays['ops'], arrays['dt'], is_super=reps[0].is_super, replicas=nB)
    plain, upd, so = 'kh_rep_sweep_store<%d>' % L, 'kh_rep_forward_update<%d>' % L, 'kh_rep_forward_update_so<%d>' % L
    outputs = ('fw_T', 'states', 'chi', 'opt', 'psi_T', 'g_a')

    def batch_of(which):
        """The batch's arrays with replica i taking set ``which[i]`` ('a' / 'b')."""
        pick = [sets[i][0 if w == 'a' else 1] for i, w in enumerate(which)]
        refs = [sets[i][2 if w == 'a' else 3] for i, w in enumerate(which)]
        s = types.SimpleNamespace(
            prob=types.SimpleNamespace(init=np.concatenate([x.prob.init for x in pick])), gp=np.array([x.gp for x in pick]),
            S=np.array([x.S for x in pick]), lam=np.array([x.lam for x in pick]), norms=np.concatenate([x.norms for x in pick]),
            chi_T=np.concatenate([x.chi_T for x in pick]), prev=np.concatenate([r.prev for r in refs]),
            sigma_vals=np.array([x.sigma_vals for x in pick]))
        return s, refs

    def rows(x, i, per):
        return x[i * per:(i + 1) * per]

    def of_replica(host, i):
        """Replica i's slices of the host copies of ``outputs`` (+ 'store')."""
        return tuple(rows(x, i, 1)[0] if key in ('opt', 'g_a') else rows(x, i, Kr) for key, x in host.items())

    def sweeps(dev, fill, second_order=False):
        dev.forward(fill)
        dev.backward(fill)
        dev.update(fill)
        names = outputs + (('store',) if second_order else ())
        return dict(zip(names, dev.host(*names)))

    def compare(host, refs, active, what, second_order=False):
        for i in active:
            ref, tol = refs[i], sets[i][0].tol
            errs = dict(fw_T=np.abs(rows(host['fw_T'], i, Kr) - ref.fw_T).max(), states=np.abs(rows(host['states'], i, Kr) - ref.states).max(),
                        chi=np.abs(rows(host['chi'], i, Kr) - ref.chi).max())
            got = (host['opt'][i], rows(host['psi_T'], i, Kr), host['g_a'][i]) + ((rows(host['store'], i, Kr),) if second_order else ())
            errs.update(_update_errs(got, ref.so if second_order else ref.update))
            _check(errs, tol, name, '%s, replica %d' % (what, i))

    try:
        assert eng.kernel == 'replica16/wave'
        dev = device_cls(eng, B=nB)
        _lib.forget_launched_kernels()
        all_a, refs_a = batch_of('aaa')
        all_b, refs_b = batch_of('bbb')
        # first order
        dev.put(all_a)
        first = sweeps(dev, True)
        compare(first, refs_a, range(nB), 'A')
        _ran(name, 'A', [upd], [plain])
        eng.set_active_replicas([1, 0, 1])
        dev.put(all_b)
        masked = sweeps(dev, False)  # (no NaN: replica 1's slices must keep A's values)
        compare(masked, refs_b, (0, 2), 'B, replica 1 off')
        _bitwise(of_replica(masked, 1), of_replica(first, 1), name, 'replica 1 off: its slices')
        _ran(name, 'B, replica 1 off', [upd], [plain])
        eng.set_active_replicas(None)
        dev.put(all_a)
        again = sweeps(dev, True)
        _bitwise(tuple(again.values()), tuple(first.values()), name, 'A again, all on')
        _ran(name, 'A again', [upd], [plain])
        # second order: one sigma row per replica
        t = dev.t
        dev.put_second_order(all_a.prev, all_a.sigma_vals)
        eng.set_second_order_replicas(t['prev'], t['store'], t['sigma'])
        dev.second_order = True
        so_first = sweeps(dev, True, True)
        compare(so_first, refs_a, range(nB), 'second order, A', True)
        _ran(name, 'second order, A', [so], [plain])
        eng.set_active_replicas([1, 0, 1])
        dev.put(all_b)
        dev.put_second_order(all_b.prev, all_b.sigma_vals)  # (the same tensors; no new set_second_order_replicas)
        so_masked = sweeps(dev, False, True)
        compare(so_masked, refs_b, (0, 2), 'second order, B, replica 1 off', True)
        _bitwise(of_replica(so_masked, 1), of_replica(so_first, 1), name, 'second order, replica 1 off: its slices')
        _ran(name, 'second order, B, replica 1 off', [so], [plain])
        eng.set_active_replicas(None)
        dev.put(all_a)
        dev.put_second_order(all_a.prev, all_a.sigma_vals)
        so_again = sweeps(dev, True, True)
        _bitwise(tuple(so_again.values()), tuple(so_first.values()), name, 'second order, A again, all on')
        eng.set_second_order_replicas()
        dev.second_order = False
        _lib.forget_launched_kernels()
        back = sweeps(dev, True)
        _bitwise(tuple(back.values()), tuple(first.values()), name, 'first order again, A')
        _ran(name, 'first order again, A', [upd], [plain])
        # no per-interval form: the C ABI refuses before it touches anything
        rc = eng._lib.kh_update_begin(eng._handle, t['chi'].data_ptr(), t['norms'].data_ptr(), t['init'].data_ptr(), t['gp'].data_ptr(),
                                      t['opt'].data_ptr(), t['g_a'].data_ptr(), t['g_a'].data_ptr(), eng._stream())
        assert rc == _lib.KH_ERR_UNSUPPORTED
        assert dev.unchanged()
    finally:
        eng.close()
