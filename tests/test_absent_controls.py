"""Every kernel family with a control that some objectives do not have.

A ``None`` entry of the operator table (``NULL`` in ``kh_problem.ops``, ``kh_csr.data == NULL``) says "this control does
not occur in this objective": local controls, or an objective driven by some of the pulses only -- the reference's ``mu``
returns zero there (mu.py:126-127).  Engine creation and every kernel family branch on it (``KhFacts::has_h1`` /
``all_h1``, the tile loaders' ``op != nullptr`` clauses, ``stage_squares``, ``kh_coop_resolve_tables``,
``build_ell_host``), and each case below takes one of those branches against the oracle, which serves ``None`` itself
(``OracleProblem``): forward sweep with storage, backward sweep, the first-order update sweep in one launch and in the
per-interval form, and the second-order sweep with its written trajectory where the family has one.  Tolerances are the
project's own: 1e-12 in Hilbert space, 1e-11 in Liouville space; pulses and g_a relative to max(1, max|.|).

Unless a case says otherwise objective 0 (``has_h1`` looks at it) and the last objective (ragged tails) lack control 0
and the objectives in between keep it; drifts are per objective (``distinct=True``) so that no shared-operator shortcut
applies.  ``test_oracle_tells_absent_from_present`` (host only) shows for every case that filling the missing entries
with another objective's operator moves every compared quantity by more than 1e-6: a kernel that ignored the ``NULL``
could not pass.  Where a control is absent from ALL objectives its sums are sums of exact zeros: the returned pulse is
the guess bit for bit, its g_a is exactly 0.0 and, with one control, the update sweep's final states are those of the
plain forward sweep (``exact=``).

Reference: mu.py:74-140, optimize.py:444-508 (update sweep), :849-886 (backward sweep)."""
import copy
import functools
import types

import numpy as np
import pytest

import helpers
from helpers import oracle_controls, spec_to_oracle
from krotov_amd import configs
from oracle import krotov_oracle as ko

TOL_HILBERT, TOL_LIOUVILLE = 1e-12, 1e-11


# ---------------------------------------------------------------------------
# problems with absent controls
# ---------------------------------------------------------------------------
def _drop(spec, entries):
    """``Hc[k][l] = None`` for every (k, l) of ``entries``; ``spec.removed`` keeps the operators that left."""
    spec.removed = getattr(spec, 'removed', {})
    for k, l in entries:
        spec.Hc[k] = list(spec.Hc[k])  # (the rows may be one shared list)
        spec.removed[k, l] = spec.Hc[k][l]
        spec.Hc[k][l] = None
    return spec


def _drop_ends(spec, l=0):
    """The pattern of most cases: objective 0 and the last objective lack control ``l``."""
    return _drop(spec, [(0, l), (spec.K - 1, l)])


def _drop_everywhere(spec, l):
    """No objective has control ``l``; objectives that shared one operator list still share one."""
    spec.removed = {(k, l): spec.Hc[k][l] for k in range(spec.K)}
    if all(row is spec.Hc[0] for row in spec.Hc):
        row = list(spec.Hc[0])
        row[l] = None
        spec.Hc = [row] * spec.K
    else:
        spec.Hc = [[None if j == l else op for j, op in enumerate(row)] for row in spec.Hc]
    return spec


def _filled(spec):
    """The same problem with the control present: a missing entry gets objective 0's operator, or the next objective's
    that has one (what a kernel reading the wrong table entry would use); the operator that was removed where no
    objective of that dimension has the control."""
    new = copy.copy(spec)
    new.Hc = [list(row) for row in spec.Hc]
    for (k, l), own in spec.removed.items():
        donors = [0] + list(range(k + 1, spec.K)) + list(range(1, k))
        new.Hc[k][l] = next((spec.Hc[d][l] for d in donors
                             if spec.Hc[d][l] is not None and spec.Hc[d][l].shape == own.shape), own)
    return new


def _c5(K, N, L=1, nt=9, distinct=True):
    return configs.config_c5(K=K, N=N, nt=nt, L=L, distinct=distinct)


def _tile(N, L):
    """K = 4: control 0 absent from objective 0 (with four controls it is one of the two operators the update kernel
    parks in LDS; with three only the drift is parked) and, from two controls on, the last control from objective 1."""
    return _drop(_c5(4, N, L), [(0, 0)] + ([(1, L - 1)] if L >= 2 else []))


def _shared(L):
    spec = configs.config_shared(K=4, N=96, nt=4, L=L)
    if L == 2:
        # config_shared's second guess, 0.5 sin(2 pi t / T), is 0.0, 6e-17 and -1e-16 on this grid of three intervals: a
        # control with such a pulse leaves no trace in the plain sweeps whether its operator is there or not (the
        # witness below caught it: the co-state stores agreed to 6e-17).  The same amplitude a quarter period on
        T = spec.tlist[-1]
        spec.controls[1] = lambda t, args: 0.5 * np.cos(2.0 * np.pi * t / T)
    return spec


def _lindblad5():
    """The d = 5 Lindbladian (N = 25, CSR): the objectives share one operator list, objective 1 gets a row of its own
    without the control."""
    return _drop(configs.config_sparse_lindblad(d=5, nt=9, K=3), [(1, 0)])


def _banded(N, bands, nt, K):
    from test_hip_parity import _banded as make

    return make(N, bands, nt, K=K)


def _c5_csr():
    return _drop(_c5(5, 12, L=3), [(1, 0), (3, 2)])


def _mixed():
    """config_mixed('dims'): the 5-level ket (objective 1) lacks the control."""
    return _drop(configs.config_mixed('dims', nt=11), [(1, 0)])


CASES = {}


def case(name, build, kernel, expect, so=None, fmt='dense', env=None, forbid=(), exact=None, row_split=None, state_roundings=0):
    """``expect`` / ``so``: the instantiations the plain and first-order sweeps / the second-order sweep must launch
    (``so=None``: no second-order run); ``forbid``: prefixes that must not have run; ``exact``: the control that no
    objective has; ``state_roundings``: 0 where the update sweep's final states must be the forward sweep's bit for bit,
    else the roundings per interval by which the two kernels may differ (see the case)."""
    CASES[name] = types.SimpleNamespace(build=build, kernel=kernel, expect=tuple(expect), so=None if so is None else tuple(so),
                                        fmt=fmt, env=dict(env or {}), forbid=tuple(forbid), exact=exact, row_split=row_split,
                                        state_roundings=state_roundings)


# ---- one wave per objective (kh_mini.h)
case('mini4', lambda: _drop_ends(_c5(3, 3)), 'mini4/wave', ['kh_quad_sweep_store', 'kh_quad_forward_update<false>'],
     so=['kh_quad_forward_update<true>'])
case('mini16', lambda: _drop_ends(_c5(5, 7)), 'mini16/wave', ['kh_mini_sweep_store', 'kh_mini_forward_update<false>'],
     so=['kh_mini_forward_update<true>'])
case('mini16_nowhere', lambda: _drop_everywhere(_c5(5, 7), 0), 'mini16/wave', ['kh_mini_sweep_store', 'kh_mini_forward_update<false>'],
     exact=0)

# ---- two terms per phase (kh_tile64q2.h): <second order, sums on the adjoint side, single GPU>; P1 = P2 = NULL where H1 is
for _n, _K in ((17, 5), (64, 3)):
    _q2 = lambda N=_n, K=_K: _drop_ends(_c5(K, N))  # noqa: E731
    case('q2_n%d' % _n, _q2, 'tile64q2/512', ['kh_q2_sweep_store', 'kh_q2_forward_update<false, true, true>'],
         so=['kh_q2_forward_update<true, false, true>'])
    case('q2_n%d_fwd_side' % _n, _q2, 'tile64q2/512', ['kh_q2_sweep_store', 'kh_q2_forward_update<false, false, true>'],
         env={'KH_NO_ADJ': '1'})
    case('q2_n%d_p2p_form' % _n, _q2, 'tile64q2/512', ['kh_q2_sweep_store', 'kh_q2_forward_update<false, true, false>'],
         so=['kh_q2_forward_update<true, false, false>'], env={'KH_Q2_SINGLE': '0'})
case('q2_n17_nowhere', lambda: _drop_everywhere(_c5(5, 17), 0), 'tile64q2/512',
     ['kh_q2_sweep_store', 'kh_q2_forward_update<false, true, true>'], exact=0)

# ---- one term per phase (kh_tile64.h): <rows per thread, controls, second order, single GPU>
for _n in (17, 64):
    case('tile512_L1_n%d' % _n, lambda N=_n: _tile(N, 1), 'tile64/512',
         ['kh_tile_sweep_store<1, 1>', 'kh_tile_forward_update<1, 1, false, true>'],
         so=['kh_tile_forward_update<1, 1, true, true>'], env={'KH_KERNEL': 'tile512'})
    for _l in (2, 3, 4):
        case('tile512_L%d_n%d' % (_l, _n), lambda N=_n, L=_l: _tile(N, L), 'tile64/512',
             ['kh_tile_sweep_store<1, %d>' % _l, 'kh_tile_forward_update<1, %d, false, true>' % _l],
             so=['kh_tile_forward_update<1, %d, true, true>' % _l])
case('tile256', lambda: _drop_ends(_c5(4, 16)), 'tile64/256', ['kh_tile_sweep_store<2, 1>', 'kh_tile_forward_update<2, 1, false, true>'],
     env={'KH_KERNEL': 'tile256'})

# ---- the generator in registers, 64 < N <= 128 (kh_tilen.h): <elements per lane, [second order,] H1 in registers>; one
# absent entry demotes "H1 in registers" (KhFacts::all_h1)
_H1REG = ('kh_tn_sweep_store<20, true>', 'kh_tn_forward_update<20, false, true>', 'kh_tn_forward_update<20, true, true>')
_tn70 = lambda: _drop_ends(_c5(3, 70))  # noqa: E731
_tn90 = lambda: _drop(_c5(3, 90, L=2), [(0, 0), (2, 0), (1, 1)])  # noqa: E731
case('tn_n70', _tn70, 'tile128/512', ['kh_tn_sweep_store<20, false>', 'kh_tn_forward_update<20, false, false>'],
     so=['kh_tn_forward_update<20, true, false>'], forbid=_H1REG)
case('tn_n70_fwd_side', _tn70, 'tile128/512', ['kh_tn_sweep_store<20, false>', 'kh_tn_forward_update<20, false, false>'],
     env={'KH_GEN_ADJ': '0'}, forbid=_H1REG)
case('tn_n90_L2', _tn90, 'tile128/512', ['kh_tn_sweep_store<24, false>', 'kh_tn_forward_update<24, false, false>'],
     so=['kh_tn_forward_update<24, true, false>'])
case('tn_n90_L2_fwd_side', _tn90, 'tile128/512', ['kh_tn_sweep_store<24, false>', 'kh_tn_forward_update<24, false, false>'],
     env={'KH_GEN_ADJ': '0'})

# ---- generic kernels (kh_generic.h): sums on the adjoint side (kh_gen_adjoint_side skips the absent operator) and on the
# forward side
_gen = lambda: _drop_ends(_c5(4, 33))  # noqa: E731
case('generic', _gen, 'generic', ['kh_gen_sweep_store<false>', 'kh_gen_forward_update<false>'], so=['kh_gen_forward_update<false>'],
     env={'KH_KERNEL': 'generic'})
case('generic_fwd_side', _gen, 'generic', ['kh_gen_sweep_store<false>', 'kh_gen_forward_update<false>'],
     env={'KH_KERNEL': 'generic', 'KH_GEN_ADJ': '0'})

# ---- cooperative matrix-core kernels (kh_coop.h): <slots, objectives per workgroup, second order, sums on the adjoint
# side, A^2 chain, cross-GPU stage>.  The operators are shared, so a control is absent from ALL objectives: (a) control 1
# of two (a NULL entry of the shared list), (b) the only control (the A^2 chain with P1 = P2 = NULL; has_h1 is false, so
# the adjoint-side form is off)
for _cols in (2, 4, 16):
    _t = 'kh_coop_forward_update<8, %d, ' % _cols
    case('coop_c%d_L2' % _cols, lambda: _drop_everywhere(_shared(2), 1), 'coop16/mfma',
         [_t + 'false, false, false, true>', 'kh_coop_sweep_store<8, %d, false>' % _cols], so=[_t + 'true, false, false, true>'],
         env={'KH_COOP_COLS': str(_cols)}, exact=1)
# (b) state_roundings: the update sweep's final states are NOT the forward sweep's bit for bit here -- measured 3.1e-17, one
# unit in the last place of elements of size 0.13, with pulse and g_a exact.  The two sweeps run the same operators (the
# NULL tables add nothing to A and A^2 in either) through the same series, but through two functions: the update kernel
# through kh_coop_expm_action_sq, the plain sweep through kh_coop_expm_action_sq_ahead (the fragment updates moved out
# of the interval's chain).  Their owner arithmetic is the same text -- state += c2 * w, sacc = fma(hn, t2, sacc),
# state += f * w -- written as a product followed by an addition, which the compiler may contract into one fused
# multiply-add (one rounding instead of two) and decides per function.  The other families call ONE series function from
# both kernels and keep bit-equality.  Bound: two roundings for each of at most 64 terms of an interval, 2^-53 each on
# states of norm 1, intervals adding up.
case('coop_L1_nowhere', lambda: _drop_everywhere(_shared(1), 0), 'coop16/mfma',
     ['kh_coop_forward_update<8, 4, false, false, true, true>', 'kh_coop_sweep_store<8, 4, true>'],
     forbid=('kh_coop_forward_update<8, 4, false, true, ',), exact=0, state_roundings=2 * 64)

# ---- ensemble detection (kh_ens.h): one member without the control, or objective 0 (has_h1), and it is no ensemble
for _name, _k in (('ens_middle', 150), ('ens_first', 0)):
    case(_name, lambda k=_k: _drop(_c5(300, 16, nt=6, distinct=False), [(k, 0)]), 'tile64/256',
         ['kh_q2_sweep_store', 'kh_tile_forward_update<2, 1, false, true>'], forbid=('kh_ens',))

# ---- sparse operators (kh_ell.h, kh_ellg.h in both forms, the generic CSR kernels)
case('ell_lindblad', _lindblad5, 'ell/csr', ['kh_ell_sweep_store<512, 1, 8, false>', 'kh_ell_forward_update<512, 1, 8, false, false>'],
     so=['kh_ell_forward_update<512, 1, 8, true, false>'], fmt='csr')
case('ell_banded', lambda: _drop_ends(_banded(40, 11, 9, 3)), 'ell/csr',
     ['kh_ell_sweep_store<512, 1, 12, false>', 'kh_ell_forward_update<512, 1, 12, false, false>'],
     so=['kh_ell_forward_update<512, 1, 12, true, false>'], fmt='csr')
case('ell_lindblad_nowhere', lambda: _drop_everywhere(configs.config_sparse_lindblad(d=5, nt=9, K=3), 0), 'ell/csr',
     ['kh_ell_sweep_store<512, 1, 8, false>', 'kh_ell_forward_update<512, 1, 8, false, false>'], fmt='csr', exact=0)
for _name, _build in (('lindblad', _lindblad5), ('c5_L3', _c5_csr)):
    case('ellstream_' + _name, _build, 'ellstream/csr', ['kh_ell_sweep_store<512, 8, 4, true>', 'kh_ell_forward_update<512, 8, 4, false, true>'],
         so=['kh_ell_forward_update<512, 8, 4, true, true>'], fmt='csr', env={'KH_KERNEL': 'ellstream'})
    case('ellglobal_' + _name, _build, 'ellglobal/csr', ['kh_ellg_sweep_store<512>', 'kh_ellg_forward_update<512, false>'],
         so=['kh_ellg_forward_update<512, true>'], fmt='csr', env={'KH_KERNEL': 'ellglobal'})
    case('ellsplit_' + _name, _build, 'ellsplit/csr', ['kh_ellgs_sweep_store<512>', 'kh_ellgs_forward_update<512, false>'],
         so=['kh_ellgs_forward_update<512, true>'], fmt='csr', env={'KH_KERNEL': 'ellglobal'}, row_split=2)
    case('generic_csr_' + _name, _build, 'generic/csr', ['kh_gen_sweep_store<false>', 'kh_gen_forward_update<false>'],
         fmt='csr', env={'KH_KERNEL': 'generic'})

# ---- objectives of different dimension and kind (kh_engine_create_mixed): against the restatement of
# tests/test_mixed_objectives.py
case('mixed', _mixed, 'generic/mixed', ['kh_gen_sweep_store<true>', 'kh_gen_forward_update<true>'], so=['kh_gen_forward_update<true>'],
     fmt='mixed')

REPLICA = 'replica_L1'  # tests/test_replicas.py: batch('L1_absent'), replica 1


def _mixed_oracle(spec):
    """The restatement of tests/test_mixed_objectives.py (zero-padded to the stride, Liouvillians L as i L); it pads
    arrays, so the absent control goes in as the zero operator, which the oracle treats exactly as ``None``."""
    from test_mixed_objectives import oracle_adapter

    zero = copy.copy(spec)
    zero.Hc = [[np.zeros_like(spec.H0[k]) if op is None else op for op in row] for k, row in enumerate(spec.Hc)]
    return oracle_adapter(zero)


def build_problem(c, spec):
    """Everything the sweeps of a case ``c`` on ``spec`` take (shared with tests/test_nonselfadjoint_controls.py)."""
    prob = _mixed_oracle(spec) if c.fmt == 'mixed' else spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    rng = np.random.default_rng(17)
    # (||H_l|| ~ 1e2 .. 1e3 with lambda_a = 2 under the shared-operator problems, and hundreds of objectives add up: keep
    # the updated pulses O(1), as tests/test_instantiations.py does)
    shared = spec.name.startswith('shared')
    norms = (0.2 + rng.random(spec.K)) * min(1.0, 8.0 / spec.K) * (0.02 if shared else 1.0)
    older = [p * (1.0 + 0.2 * rng.standard_normal(p.shape)) for p in gp]  # the "previous iteration" of second order
    sigma_vals = -(1.0 + rng.random(len(spec.tlist) - 1)) * min(1.0, 8.0 / spec.K) * (1e-3 if shared else 1.0)
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    return types.SimpleNamespace(spec=spec, prob=prob, gp=gp, S=S, lam=lam, norms=norms, older=older, sigma_vals=sigma_vals,
                                 chi_T=chi_T, tol=TOL_LIOUVILLE if prob.is_super else TOL_HILBERT)


def compute_sweeps(p, second_order, use_scipy=False):
    """The oracle's sweeps of a problem of :func:`build_problem`."""
    out = types.SimpleNamespace(prev=None, so=None)
    with helpers.MemoExpm():
        out.fw_T, out.states = ko.forward_propagation(p.prob, p.gp, store=True, use_scipy=use_scipy)
        out.chi = ko.backward_sweep(p.prob, p.chi_T, p.gp, use_scipy=use_scipy)
        out.update = ko.forward_update_sweep(p.prob, out.chi, p.norms, p.gp, p.S, p.lam, use_scipy=use_scipy)
        if second_order:
            _, out.prev = ko.forward_propagation(p.prob, p.older, store=True, use_scipy=use_scipy)
            out.so = ko.forward_update_sweep(p.prob, out.chi, p.norms, p.gp, p.S, p.lam, use_scipy=use_scipy,
                                             sigma_vals=p.sigma_vals, fw_prev=out.prev, store=True)
    return out


@functools.lru_cache(maxsize=None)
def problem(name, present=False):
    """Everything a case's sweeps take (built once; never modified)."""
    c = CASES[name]
    spec = c.build()
    if present:
        spec = _filled(spec)
    return build_problem(c, spec)


@functools.lru_cache(maxsize=None)
def oracle_sweeps(name, present=False):
    """The oracle's sweeps of a case, computed once and shared by the GPU test and the witness (never modified)."""
    return compute_sweeps(problem(name, present), CASES[name].so is not None and not present)


# ---------------------------------------------------------------------------
# host only: the oracle tells "absent" from "present" in every case
# ---------------------------------------------------------------------------
def _replica_sweeps(present):
    import test_replicas as tr

    if not present:
        _, chi, (opt, psi_T, _) = tr.oracle_sweeps('L1_absent', 1)
        return opt, psi_T, chi
    r = copy.copy(tr.batch('L1_absent')[1])
    r.Hc = [list(row) for row in r.Hc]
    assert r.Hc[0][0] is None
    r.Hc[0][0] = r.Hc[1][0]
    prob = spec_to_oracle(r)
    chi = ko.backward_sweep(prob, r.target / np.linalg.norm(r.target, axis=1)[:, None], r.pulses)
    opt, psi_T, _ = ko.forward_update_sweep(prob, chi, r.chi_norms, r.pulses, r.shapes, r.lambdas)
    return opt, psi_T, chi


@pytest.mark.parametrize('name', sorted(CASES) + [REPLICA])
def test_oracle_tells_absent_from_present(name):
    """The updated pulses, the final states and the co-state store of the problem with the control absent and of the same
    problem with the missing entries filled (objective 0's operator, or the next objective's; the removed operator where
    the control is absent everywhere) differ by more than 1e-6 each -- eleven orders of magnitude above the tolerance of
    the GPU comparison, so a kernel that read another objective's operator in place of the missing one would fail it."""
    if name == REPLICA:
        absent, filled = _replica_sweeps(False), _replica_sweeps(True)
    else:
        a, f = oracle_sweeps(name), oracle_sweeps(name, True)
        absent, filled = (a.update[0], a.update[1], a.chi), (f.update[0], f.update[1], f.chi)
    moved = {what: float(np.abs(np.array(x) - np.array(y)).max())
             for what, x, y in zip(('opt', 'psi_T', 'chi'), absent, filled)}
    print('%s: %s' % (name, ', '.join('%s %.2e' % kv for kv in moved.items())))
    for what, d in moved.items():
        assert d > 1e-6, (name, what, d)
    if name != REPLICA and CASES[name].exact is not None:  # the oracle's own exactness: the pulse nobody feels stays the guess
        l = CASES[name].exact
        assert np.array_equal(absent[0][l], problem(name).gp[l]) and oracle_sweeps(name).update[2][l] == 0.0


def test_case_table_is_what_it_says():
    """Every case has an absent entry; the default pattern takes the control from objective 0 and from the last one and
    leaves it to an objective in between; shared operator lists stay shared."""
    for name, c in CASES.items():
        spec = problem(name).spec
        gone = [(k, l) for k in range(spec.K) for l in range(spec.L) if spec.Hc[k][l] is None]
        assert gone and sorted(gone) == sorted(spec.removed), name
        assert all(spec.H0[k] is not None for k in range(spec.K))
        if c.exact is not None:
            assert [k for k, l in gone if l == c.exact] == list(range(spec.K)), name
    for name in ('mini4', 'mini16', 'q2_n17', 'q2_n64', 'tile256', 'tn_n70', 'generic', 'ell_banded'):
        spec = problem(name).spec
        assert spec.K >= 3 and spec.L == 1
        assert [k for k in range(spec.K) if spec.Hc[k][0] is None] == [0, spec.K - 1], name
    for name in ('coop_c4_L2', 'coop_L1_nowhere', 'ell_lindblad_nowhere'):
        spec = problem(name).spec
        assert all(row is spec.Hc[0] for row in spec.Hc) and all(h is spec.H0[0] for h in spec.H0), name
    ops = configs.sparse_ops(problem('ell_lindblad').spec)
    assert ops[1][1] is None and ops[0][1] is ops[2][1] and ops[0][0] is ops[1][0]


def test_objectives_leave_the_absent_term_out():
    """``configs.spec_to_objectives`` leaves the term out of ``H`` (no zero matrix), so ``optimize._operator_rows`` is what
    produces the ``None``."""
    import krotov_amd
    from krotov_amd.conversions import extract_controls_mapping

    spec = _e2e_spec(5)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    assert [len(obj.H) for obj in objectives] == [3, 2, 3] and len(pulse_options) == 2
    controls = krotov_amd.conversions.extract_controls(objectives)
    mapping = extract_controls_mapping(objectives, controls)
    from krotov_amd.optimize import _operator_rows
    from krotov_amd._ingest import to_dense

    rows, _ = _operator_rows(objectives, mapping, len(controls), to_dense)
    l1 = controls.index(spec.controls[1])
    assert [row[1 + l1] is None for row in rows] == [False, True, False]
    assert all(row[1 + (1 - l1)] is not None for row in rows)


def test_drop_any_draws_from_its_own_generator():
    """``fuzz_parity.py --drop-any`` decides with a generator of its own: the default stream draws the same problems with
    and without it (the cases of the two older fixed-seed fuzz tests stay what they are), and it reaches what the default
    stream never does -- one control, objective 0 and the last one."""
    import fuzz_parity

    seed = 20261018
    plain, dropping = np.random.default_rng(seed), np.random.default_rng(seed)
    rng_drop = np.random.default_rng([seed, 0xd709])
    where = set()
    for _ in range(40):
        a, tag_a, fmt_a = fuzz_parity.draw(plain)
        b, tag_b, fmt_b = fuzz_parity.draw(dropping, rng_drop=rng_drop)
        assert (a.name, a.K, a.N, a.L, len(a.tlist), fmt_a) == (b.name, b.K, b.N, b.L, len(b.tlist), fmt_b)
        assert tag_b.replace(' shared', '').startswith(tag_a.replace(' shared', ''))
        assert all(x is y for x, y in zip(a.H0, b.H0)) or np.array_equal(a.H0[-1], b.H0[-1])
        for k, row in enumerate(b.Hc):
            for l, op in enumerate(row):
                if op is None and a.Hc[k][l] is not None:
                    where.add(('first' if k == 0 else 'last' if k == b.K - 1 else 'middle', b.L == 1))
    assert {w for w, _ in where} == {'first', 'middle', 'last'} and any(one for _, one in where)
    assert plain.random() == dropping.random()


# ---------------------------------------------------------------------------
# GPU: every family against the oracle
# ---------------------------------------------------------------------------
def _engine_ops(spec, fmt):
    if fmt == 'csr':
        return configs.sparse_ops(spec)
    return [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]


def _check(errs, tol, name, what):
    print('%s %s (tolerance %.0e): %s' % (name, what, tol, ', '.join('%s %.2e' % kv for kv in errs.items())))
    for key, err in errs.items():
        assert err < tol, (name, what, key, err)


def check_case(name, c, p, ref, monkeypatch):
    """The sweeps of case ``c`` (a row of a ``case`` table) on the GPU against the oracle's ``ref`` of problem ``p``: forward
    with storage, backward, the update sweep in one launch and per interval, second order where ``c.so`` says so; the
    kernel family and the launched instantiations.  Returns what the single-launch sweeps gave (host arrays), the
    products the update sweep issued (``matvecs_update``) and the launched instantiations."""
    import torch

    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    for key, value in c.env.items():
        monkeypatch.setenv(key, value)
    spec, init, tol = p.spec, p.prob.init, p.tol
    pulses, Sa, lama = np.array(p.gp), np.array(p.S), np.array(p.lam)
    ref_opt, ref_psi, ref_ga = np.array(ref.update[0]), ref.update[1], ref.update[2]
    scale, ga_scale = max(1.0, np.abs(ref_opt).max()), max(1.0, np.abs(ref_ga).max())
    eng = HipKrotovEngine(_engine_ops(spec, c.fmt), np.diff(spec.tlist), is_super=spec.kinds if c.fmt == 'mixed' else spec.is_super)
    try:
        if c.row_split:
            assert eng.set_row_split(c.row_split) == c.row_split
        assert eng.kernel == c.kernel
        _lib.forget_launched_kernels()
        fw_T, states = (x.cpu().numpy() for x in eng.forward(pulses, init, store=True))
        eng.check()
        chi = eng.backward(p.chi_T, pulses)
        eng.check()
        opt, psi_T, g_a = (x.cpu().numpy() for x in eng.forward_update(chi, p.norms, init, pulses, Sa, lama))
        eng.check()
        launched = list(_lib.kernel_instantiations(launched_only=True))
        got = types.SimpleNamespace(chi=chi.cpu().numpy(), opt=opt, psi_T=psi_T, g_a=g_a, matvecs_update=eng.stats()['matvecs'])
        _check(dict(states=np.abs(states - ref.states).max(), fw_T=np.abs(fw_T - ref.fw_T).max(),
                    chi=np.abs(chi.cpu().numpy() - ref.chi).max(), opt=np.abs(opt - ref_opt).max() / scale,
                    psi_T=np.abs(psi_T - ref_psi).max(), g_a=np.abs(g_a - ref_ga).max() / ga_scale), tol, name, 'single launch')
        # the sweep cut at the cross-objective sum (the multi-GPU form) with a one-rank "all-reduce"
        opt2, psi2, ga2 = (x.cpu().numpy() for x in eng.forward_update_sharded(chi, p.norms, init, pulses, Sa, lama, lambda x: x))
        eng.check()
        _check(dict(opt=np.abs(opt2 - ref_opt).max() / scale, psi_T=np.abs(psi2 - ref_psi).max(),
                    g_a=np.abs(ga2 - ref_ga).max() / ga_scale), tol, name, 'per interval')
        if c.so is not None:
            store = torch.full((spec.K, len(spec.tlist), spec.N), float('nan'), dtype=torch.complex128, device=eng.device)
            eng.set_second_order(ref.prev, store, p.sigma_vals)
            opt3, psi3, ga3 = (x.cpu().numpy() for x in eng.forward_update(chi, p.norms, init, pulses, Sa, lama))
            eng.check()
            so_opt = np.array(ref.so[0])
            _check(dict(opt=np.abs(opt3 - so_opt).max() / max(1.0, np.abs(so_opt).max()), psi_T=np.abs(psi3 - ref.so[1]).max(),
                        g_a=np.abs(ga3 - ref.so[2]).max() / max(1.0, np.abs(ref.so[2]).max()),
                        fw_store=np.abs(store.cpu().numpy() - ref.so[3]).max()), tol, name, 'second order')
            eng.set_second_order()
        launched_so = got.launched = list(_lib.kernel_instantiations(launched_only=True))
        print('%s launched: %s' % (name, ', '.join(launched_so)))
        for want in c.expect:
            assert want in launched, (want, launched)
        for want in c.so or ():
            assert want in launched_so, (want, launched_so)
        for prefix in c.forbid:
            assert not any(n.startswith(prefix) for n in launched_so), (prefix, launched_so)
        if c.exact is not None:
            # every term of this control's sum is a product with an exact zero
            l = c.exact
            assert np.array_equal(opt[l], pulses[l]) and np.array_equal(opt2[l], pulses[l])
            assert g_a[l] == 0.0 and ga2[l] == 0.0
            if spec.L == 1:  # ... so the update sweep is the plain forward sweep under the guess
                apart = np.abs(psi_T - fw_T).max()
                print('%s update sweep against forward sweep: %.2e' % (name, apart))
                if c.state_roundings:
                    assert apart <= (len(spec.tlist) - 1) * c.state_roundings * 2.0 ** -53
                else:
                    assert np.array_equal(psi_T, fw_T)
    finally:
        eng.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_absent_control_vs_oracle(name, monkeypatch):
    check_case(name, CASES[name], problem(name), oracle_sweeps(name), monkeypatch)


@pytest.mark.gpu
def test_replica_with_absent_control_vs_oracle():
    """``kh_rep_*<1>``: objective 0 of replica 1 of three lacks the only control (the engine run and the comparison are
    those of tests/test_replicas.py)."""
    import test_replicas as tr
    from krotov_amd import _lib

    reps = tr.batch('L1_absent')
    assert reps[1].Hc[0][0] is None and all(op is not None for b in (0, 2) for row in reps[b].Hc for op in row)
    _lib.load()
    _lib.forget_launched_kernels()
    got = tr.run_engine(reps)
    launched = _lib.kernel_instantiations(launched_only=True)
    for want in ('kh_rep_sweep_store<1>', 'kh_rep_forward_update<1>'):
        assert want in launched, (want, launched)
    tr.compare_with_oracle('L1_absent', got)


# ---------------------------------------------------------------------------
# GPU, end to end: two iterations of optimize_pulses against the oracle's loop
# ---------------------------------------------------------------------------
def _e2e_spec(N, b=0, absent=True):
    """Three objectives, two controls; control 1 occurs in objectives 0 and 2 only (``absent``).  ``b``: a replica's own
    seed and grid."""
    spec = configs.config_c5(K=3, N=N, nt=9, L=2, distinct=True, seed=b, T=(9 - 1) / 4000.0 * (1.0 + 0.25 * b))
    if absent:
        spec.Hc[1] = [spec.Hc[1][0], None]
    return spec


def _e2e_lindblad():
    """The d = 5 Lindbladian with a second control (on the hopping), which objective 1 does not have."""
    spec = configs.config_sparse_lindblad(d=5, nt=9, K=3)
    hop = np.diag(np.sqrt(np.arange(1, 5)), k=1)
    L2 = configs.liouvillian_dense(0.3 * (hop + hop.T))
    T = spec.tlist[-1]
    spec.controls = [spec.controls[0], lambda t, args: 0.4 * np.sin(2 * np.pi * t / T)]
    L1 = spec.Hc[0][0]
    spec.Hc = [[L1, L2], [L1, None], [L1, L2]]
    spec.L = 2
    return spec


def _compare_run(res, spec, tol, what):
    ref = helpers.oracle_optimize(spec, 2)
    d_pulse = np.abs(np.array(res.all_pulses) - ref['all_pulses']).max() / max(1.0, np.abs(ref['all_pulses']).max())
    d_tau = np.abs(np.array(res.tau_vals) - ref['tau_vals']).max()
    print('%s: pulses %.2e tau %.2e (tolerance %.0e)' % (what, d_pulse, d_tau, tol))
    assert d_pulse < tol and d_tau < tol, (what, d_pulse, d_tau)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [5, 17])
def test_optimize_pulses_with_absent_control(N):
    import krotov_amd

    spec = _e2e_spec(N)
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    assert len(objectives[1].H) == 2  # the term is left out: optimize._operator_rows yields the None
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, propagator=krotov_amd.propagators.expm,
                                     chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2, store_all_pulses=True)
    assert krotov_amd.engine.LAST_ENGINE().kernel == 'tile64/512'
    _compare_run(res, spec, TOL_HILBERT, 'expm N=%d' % N)


@pytest.mark.gpu
def test_density_matrix_ode_propagator_with_absent_control():
    import krotov_amd

    spec = _e2e_lindblad()
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    assert len(objectives[1].H) == 2
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist,
                                     propagator=krotov_amd.propagators.DensityMatrixODEPropagator(),
                                     chi_constructor=krotov_amd.functionals.chis_re, iter_stop=2, store_all_pulses=True)
    assert krotov_amd.engine.LAST_ENGINE().kernel == 'ell/csr'
    _compare_run(res, spec, TOL_LIOUVILLE, 'DensityMatrixODEPropagator d=5')


@pytest.mark.gpu
def test_optimize_pulses_batch_with_absent_control():
    import krotov_amd

    specs = [_e2e_spec(5, b, absent=b == 1) for b in range(3)]  # only replica 1 has the objective without control 1
    problems = []
    for spec in specs:
        objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
        problems.append(dict(objectives=objectives, pulse_options=pulse_options, tlist=spec.tlist))
    assert [len(pr['objectives'][1].H) for pr in problems] == [3, 2, 3]
    results = krotov_amd.optimize_pulses_batch(problems, iter_stop=2, store_all_pulses=True, propagator=krotov_amd.propagators.expm,
                                               chi_constructor=krotov_amd.functionals.chis_re)
    assert krotov_amd.engine.LAST_ENGINE().kernel == 'replica16/wave'
    for b, (spec, res) in enumerate(zip(specs, results)):
        _compare_run(res, spec, TOL_HILBERT, 'batch replica %d' % b)
