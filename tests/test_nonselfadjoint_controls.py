"""Every kernel family with a control operator that is neither plus nor minus its own adjoint, and the operator
classifier at its edges.

Everywhere else in the suite H_l^dagger = +-H_l (Hermitian controls, commutator super-operators), so H_l, H_l^dagger,
H_l^T and conj(H_l) may be mixed up without a trace.  The code that uses or branches on a control's adjoint:

* ``kh_adjoint_kernel`` stages ``bw[1 + l]`` = H_l^dagger, the control of the backward generator A^dagger = H0^dagger +
  sum eps_l H_l^dagger (every ``*_sweep_store`` kernel in the backward direction);
* ``stage_squares`` forms the backward P1 = H0^dagger H1^dagger + H1^dagger H0^dagger and P2 = (H1^dagger)^2 of the A^2
  chains (q2, mini, cooperative, replica); ``stage_coop`` the fragment-ordered copies of ``bw``;
* ``_create_sparse`` uploads ``mat.conj().T`` and ``build_ell_host`` builds the ``dir == 1`` pools, whose row width differs
  from the forward one only under a pattern that is not symmetric (``ladder`` below);
* ``kh_gen_adjoint_side`` computes V = H_lk^dagger chi from ``d_ops_bw`` for the generic, ``kh_tn_*``, ``kh_tx_*``,
  ``kh_stream_*`` and ensemble update kernels, ``kh_coop_adjoint_side`` under the block mask that
  ``kh_coop_adj_mask_kernel`` takes from ``bw[1]`` (mask(H^dagger) != mask(H) under ``ladder``);
* ``kh_adjoint_sign_kernel`` / ``kh_herm_defect_kernel`` (dense), ``csr_equal`` / ``csr_part_fro2`` (sparse) and
  ``classify_operators`` decide ``adj_sign`` (q2 takes +-H1 chi for H1^dagger chi: ``kh_q2_forward_update<., true, .>``),
  ``real_spectrum`` and ``imag_defect`` (the shortened Chebyshev-form series instead of Taylor's).

Kinds of control (``_vary``): ``lower`` -- Hermitian plus a strictly lower-triangular complex part of the same norm (dense,
non-normal); ``ladder`` -- super-diagonals at offsets 1 and 20 plus one dense row (not even structurally symmetric);
``liouv`` -- -i[H1, .] + D[C], neither plus nor minus its adjoint in Liouville space; ``anti`` -- i x Hermitian in Hilbert
space (adj_sign = -1 without ``is_super``) and i x commutator in Liouville space (adj_sign = +1 with ``is_super``).  With
several controls only the last one is changed, in the ``_last`` variants only the last objective's: the flags are "all
controls of all objectives".  Drifts stay as they are.

Which case takes which branch: the ``CASES`` table (sections q2 ... mixed) names kernel family and instantiations, as
tests/test_absent_controls.py does and through its machinery (``check_case``): forward sweep with storage, backward
sweep, update sweep in one launch and per interval, second order where the family has it, against the oracle at 1e-12
(Hilbert space) / 1e-11 (Liouville space), pulses and g_a relative to max(1, max|.|).  ``PAIRS`` are the same problem
with the update sums on the adjoint side and on the forward side, which must agree to 1e-13 x scale.
``test_oracle_tells_right_from_wrong`` (host only) shows for every case that (a) a backward generator built from H_l,
(b) one built from H_l^T, (c) update sums with +H_l or -H_l in place of H_l^dagger and (d), under ``ladder``, the block
mask of H_l in place of that of H_l^dagger each move every compared quantity by more than 1e-6.
``test_real_spectrum_series_on_the_disk`` / ``test_series_witness`` (host only): what a wrongly accepted real-spectrum
series costs -- under 100 x the tolerance wherever the sub-steps stay at theta <= 1, so only the product count shows it
there, and 100 x and more on the ``*_hot_anti`` rows of the padded-row and cooperative families.  The edge rows are the
classifier's: each asserts the decision (the q2 instantiation that ran; the products issued against the same run with
``KH_TAYLOR=1``), not only the result.

Reference: optimize.py:444-508 (update sweep), :849-886 (backward sweep); objectives.py:240-258 (adjoint objectives)."""
import copy
import functools
import types

import numpy as np
import pytest

import helpers
import test_absent_controls as tac
from helpers import spec_to_oracle
from helpers import nonselfadjoint_variant as _vary
from krotov_amd import configs
from oracle import krotov_oracle as ko

TOL_HILBERT, TOL_LIOUVILLE = tac.TOL_HILBERT, tac.TOL_LIOUVILLE
TOL_FORMS = 1e-13  # two forms of one sum (tests/test_hip_parity.py, test_q2_update_forward_side_partial_sums)


# ---------------------------------------------------------------------------
# controls that are not self-adjoint
# ---------------------------------------------------------------------------
def _replace(spec, make, ks=None, l=None):
    """``Hc[k][l] = s_k make(Hc[0][l] / s_0)`` for the objectives ``ks`` (default: all) with the ensemble's scales s_k
    (``spec.mu``; else 1): the new control is shared where the old one was.  ``l`` defaults to the LAST control."""
    l = spec.L - 1 if l is None else l
    mu = getattr(spec, 'mu', None)
    scale = (lambda k: mu[k]) if mu is not None else (lambda k: 1.0)
    new = make(spec.Hc[0][l] / scale(0))
    everywhere, shared = ks is None, all(row is spec.Hc[0] for row in spec.Hc)
    ks = list(range(spec.K)) if ks is None else list(ks)
    if shared:
        row = list(spec.Hc[0])
        row[l] = new
        spec.Hc = [row if k in ks else spec.Hc[0] for k in range(spec.K)]
    else:
        spec.Hc = [list(r) for r in spec.Hc]
        for k in ks:
            spec.Hc[k][l] = new if mu is None else scale(k) * new
    spec.changed = sorted(set(getattr(spec, 'changed', [])) | {(k, l) for k in ks})
    assert not everywhere or len(spec.changed) >= spec.K
    return spec


def _nsa(spec, kind, ks=None, l=None, seed=5, row_cols=None):
    rng = np.random.default_rng(seed)
    return _replace(spec, lambda H: _vary(kind, H, rng, row_cols), ks, l)


def _last(spec, kind, **kw):
    """Only the last objective's control is changed."""
    return _nsa(spec, kind, ks=[spec.K - 1], **kw)


def _c5(K, N, L=1, nt=9, distinct=True):
    return configs.config_c5(K=K, N=N, nt=nt, L=L, distinct=distinct)


def _shared(L):
    return tac._shared(L)  # (its second guess pulse is not ~0 on this grid)


def _lindblad5(K=3, nt=9):
    return configs.config_sparse_lindblad(d=5, nt=nt, K=K)


def _liouv(spec, ks=None):
    """The d = 5 Lindbladian's control -i[H1, .] becomes -i[H1, .] + D[C] with C = sqrt(0.03) x the lowering operator:
    ||D[C]|| T = 0.03 x 4 x 4 = 0.5 under the guess of at most 0.8."""
    d = int(round(np.sqrt(spec.N)))
    H1 = np.diag(np.arange(d) / (d - 1.0)).astype(np.complex128)
    C = np.sqrt(0.03) * np.diag(np.sqrt(np.arange(1, d)), k=1)
    return _replace(spec, lambda old: configs.liouvillian_dense(H1, [C]), ks)


def _liouv_selfadjoint(spec):
    """i x the commutator with 0.25 x a random complex Hermitian H: the super-operator 0.25 [H, .] equals its own adjoint,
    bit for bit (adj_sign = +1 with ``is_super``), and not its transpose (the witness found that of the diagonal H1: a
    real symmetric matrix); 0.25: e^(0.8 x 0.25 x 2 x 4) bounds the growth of the states."""
    d = int(round(np.sqrt(spec.N)))
    H = configs.herm(np.random.default_rng(5), d, 0.25)
    return _replace(spec, lambda old: 1j * configs.liouvillian_dense(H))


def _banded(N=40, bands=11, nt=9, K=3):
    return tac._banded(N, bands, nt, K)


def _banded_ladder(ks=None):
    """The dense row has 16 entries: 17 control-touched slots in front of every row's up to 10 drift-only entries make
    the forward rows 28 wide (the 32-slot kernels), the backward ones (a dense COLUMN) stay at 12."""
    return _nsa(_banded(), 'ladder', ks=ks, row_cols=16)


def _hot(spec, fmt, theta, a_rel=4.0):
    """A row for the series witness, where the case says otherwise about theta and the amplitude: the control is i x D
    with D = diag(-1 ... 1) -- anti-Hermitian, adj_sign = -1, and its norm bound is its spectral radius --, under a guess
    of a_rel x the drift's bound that changes sign from interval to interval (what one interval grows the next takes
    back: the states stay O(1)), on a uniform grid with theta = dt (n_0 + |eps| n_1) just under ``theta``."""
    _replace(spec, lambda old: 1j * np.diag(np.linspace(-1.0, 1.0, spec.N)).astype(np.complex128))
    bounds = helpers.series_bounds(helpers.explicit(spec, fmt))[0]
    a = a_rel * bounds[0] / bounds[1]
    dt = 0.999 * theta / (bounds[0] + a * bounds[1])
    spec.tlist = dt * np.arange(len(spec.tlist))
    spec.controls = [lambda t, args: a * (1.0 if int(np.floor(t / dt)) % 2 == 0 else -1.0)]
    spec.lambda_a = 0.1 * spec.lambda_a  # (the witness: under the problem's own lambda_a wrong update sums moved psi_T by 3e-7 only)
    return spec


def _mixed():
    """config_mixed('dims'): the 5-level ket's control becomes ``lower``, the qutrit Liouvillian's gets a dissipator."""
    spec = configs.config_mixed('dims', nt=11)
    spec.Hc = [list(row) for row in spec.Hc]
    spec.Hc[1][0] = _vary('lower', spec.Hc[1][0], np.random.default_rng(5))
    a, x = configs._ladder(3)
    spec.Hc[2][0] = configs.liouvillian_dense(x, [np.sqrt(0.05) * a])
    spec.changed = [(1, 0), (2, 0)]
    return spec


CASES = {}


def case(name, build, kernel, expect, so=None, fmt='dense', env=None, forbid=(), row_split=None, ladder=False, series=None):
    """A row of the table, in the form of ``test_absent_controls.case`` (``check_case`` reads it); ``ladder``: witness (d);
    ``series``: the cap of the real-spectrum table a wrong accept would run (rows of the series witness)."""
    CASES[name] = types.SimpleNamespace(build=build, kernel=kernel, expect=tuple(expect), so=None if so is None else tuple(so),
                                        fmt=fmt, env=dict(env or {}), forbid=tuple(forbid), exact=None, row_split=row_split,
                                        state_roundings=0, ladder=ladder, series=series)


# ---- two terms per phase (kh_tile64q2.h): <second order, sums on the adjoint side, single GPU>.  Detection alone puts the
# sums on the forward side (adj_sign = 0); ``anti``: adjoint side with sign -1 (Hilbert space) / +1 (Liouville space)
_Q2_ADJ = 'kh_q2_forward_update<false, true, '
for _n, _K in ((17, 5), (64, 3)):
    for _tag, _make in (('lower', _nsa), ('lower_last', _last)):
        case('q2_n%d_%s' % (_n, _tag), lambda N=_n, K=_K, make=_make: make(_c5(K, N), 'lower'), 'tile64q2/512',
             ['kh_q2_sweep_store', 'kh_q2_forward_update<false, false, true>'], so=['kh_q2_forward_update<true, false, true>'],
             env={'KH_KERNEL': 'q2'}, forbid=(_Q2_ADJ,))
    case('q2_n%d_anti' % _n, lambda N=_n, K=_K: _nsa(_c5(K, N), 'anti'), 'tile64q2/512',
         ['kh_q2_sweep_store', 'kh_q2_forward_update<false, true, true>'], so=['kh_q2_forward_update<true, false, true>'],
         env={'KH_KERNEL': 'q2'}, forbid=('kh_q2_forward_update<false, false, ',))
case('q2_liouville_selfadjoint', lambda: _liouv_selfadjoint(_lindblad5()), 'tile64q2/512',
     ['kh_q2_sweep_store', 'kh_q2_forward_update<false, true, true>'], env={'KH_KERNEL': 'q2'},
     forbid=('kh_q2_forward_update<false, false, ',))
case('q2_liouville_liouv', lambda: _liouv(_lindblad5()), 'tile64q2/512',
     ['kh_q2_sweep_store', 'kh_q2_forward_update<false, false, true>'], env={'KH_KERNEL': 'q2'}, forbid=(_Q2_ADJ,))

# ---- one wave per objective (kh_mini.h): the backward A^2 chain from the staged adjoints
case('mini4', lambda: _nsa(_c5(3, 3), 'lower'), 'mini4/wave', ['kh_quad_sweep_store', 'kh_quad_forward_update<false>'],
     so=['kh_quad_forward_update<true>'])
case('mini16', lambda: _nsa(_c5(5, 7), 'lower'), 'mini16/wave', ['kh_mini_sweep_store', 'kh_mini_forward_update<false>'],
     so=['kh_mini_forward_update<true>'])
case('mini16_last', lambda: _last(_c5(5, 7), 'lower'), 'mini16/wave', ['kh_mini_sweep_store', 'kh_mini_forward_update<false>'])

# ---- one term per phase (kh_tile64.h): <rows per thread, controls, second order, single GPU>; the LAST control only
for _n in (17, 64):
    for _l in (1, 2, 3, 4):
        case('tile512_L%d_n%d' % (_l, _n), lambda N=_n, L=_l: _nsa(_c5(4, N, L), 'lower'), 'tile64/512',
             ['kh_tile_sweep_store<1, %d>' % _l, 'kh_tile_forward_update<1, %d, false, true>' % _l],
             so=['kh_tile_forward_update<1, %d, true, true>' % _l], env={'KH_KERNEL': 'tile512'} if _l == 1 else None)
case('tile256', lambda: _nsa(_c5(4, 16), 'lower'), 'tile64/256', ['kh_tile_sweep_store<2, 1>', 'kh_tile_forward_update<2, 1, false, true>'],
     env={'KH_KERNEL': 'tile256'})

# ---- the generator in registers, 64 < N <= 128 (kh_tilen.h): <elements per lane, [second order,] H1 in registers>; the
# update sums from the adjoint-side store V = H_l^dagger chi (kh_gen_adjoint_side) or, KH_GEN_ADJ=0, on the forward side
_tn70 = lambda: _nsa(_c5(3, 70), 'lower')  # noqa: E731
_tn90 = lambda: _nsa(_c5(3, 90, L=2), 'lower')  # noqa: E731
for _tag, _env in (('', None), ('_fwd_side', {'KH_GEN_ADJ': '0'})):
    case('tn_n70' + _tag, _tn70, 'tile128/512', ['kh_tn_sweep_store<20, true>', 'kh_tn_forward_update<20, false, true>'],
         so=['kh_tn_forward_update<20, true, true>'] if not _tag else None, env=_env)
    case('tn_n90_L2' + _tag, _tn90, 'tile128/512', ['kh_tn_sweep_store<24, false>', 'kh_tn_forward_update<24, false, false>'],
         so=['kh_tn_forward_update<24, true, false>'] if not _tag else None, env=_env)

# ---- five controls at N <= 64 (kh_tile64x.h) and more objectives than CUs (kh_tile64s.h): both read the adjoint-side store
case('tx_L5', lambda: _nsa(_c5(3, 17, L=5), 'lower'), 'tile64x/512', ['kh_tx_sweep_store<5>', 'kh_tx_forward_update<5>'])
case('stream_L4_n8', lambda: _nsa(configs.config_c5(K=270, N=8, nt=6, L=4), 'lower'), 'tile64/stream',
     ['kh_stream_forward_update<4, false, false>'])

# ---- generic kernels (kh_generic.h), both sides
_gen = lambda: _nsa(_c5(4, 33), 'lower')  # noqa: E731
case('generic', _gen, 'generic', ['kh_gen_sweep_store<false>', 'kh_gen_forward_update<false>'], so=['kh_gen_forward_update<false>'],
     env={'KH_KERNEL': 'generic'})
case('generic_fwd_side', _gen, 'generic', ['kh_gen_sweep_store<false>', 'kh_gen_forward_update<false>'],
     env={'KH_KERNEL': 'generic', 'KH_GEN_ADJ': '0'})

# ---- ensemble (kh_ens.h): the members share one control that is not self-adjoint, up to their real scales
case('ens', lambda: _nsa(_c5(300, 16, nt=6, distinct=False), 'lower'), 'ens64/mfma', ['kh_ens_forward_update<1, false>'])

# ---- cooperative matrix-core kernels (kh_coop.h): <slots, objectives per workgroup, second order, sums on the adjoint
# side, A^2 chain, cross-GPU stage>; mask(H1^dagger) != mask(H1)
for _cols in (2, 4, 16):
    _t = 'kh_coop_forward_update<8, %d, ' % _cols
    _e = {'KH_COOP_COLS': str(_cols)}
    _one = lambda: _nsa(_shared(1), 'ladder')  # noqa: E731
    case('coop_c%d' % _cols, _one, 'coop16/mfma', [_t + 'false, true, true, false>', 'kh_coop_sweep_store<8, %d, true>' % _cols],
         so=[_t + 'true, false, true, true>'], env=_e, ladder=True)
    case('coop_c%d_p2p_form' % _cols, _one, 'coop16/mfma', [_t + 'false, true, true, true>'], env=dict(_e, KH_COOP_SINGLE='0'),
         ladder=True)
    case('coop_c%d_fwd_side' % _cols, _one, 'coop16/mfma', [_t + 'false, false, true, true>'], env=dict(_e, KH_COOP_NO_ADJ='1'),
         forbid=(_t + 'false, true, ',), ladder=True)
case('coop_c4_L2', lambda: _nsa(_shared(2), 'ladder'), 'coop16/mfma',
     ['kh_coop_forward_update<8, 4, false, false, false, true>', 'kh_coop_sweep_store<8, 4, false>'],
     so=['kh_coop_forward_update<8, 4, true, false, false, true>'], env={'KH_COOP_COLS': '4'}, ladder=True)

# ---- sparse operators (kh_ell.h, kh_ellg.h in both forms, the generic CSR kernels): ``ladder`` on the banded problem
# (forward rows 28 wide, backward rows 12: the 32-slot instantiation runs both pools) and ``liouv`` on the d = 5 Lindbladian
case('ell_banded_ladder', _banded_ladder, 'ell/csr',
     ['kh_ell_sweep_store<512, 1, 32, false>', 'kh_ell_forward_update<512, 1, 32, false, false>'],
     so=['kh_ell_forward_update<512, 1, 32, true, false>'], fmt='csr')
case('ell_banded_ladder_last', lambda: _banded_ladder([2]), 'ell/csr',
     ['kh_ell_sweep_store<512, 1, 32, false>', 'kh_ell_forward_update<512, 1, 32, false, false>'], fmt='csr')
case('ell_lindblad_liouv', lambda: _liouv(_lindblad5()), 'ell/csr',
     ['kh_ell_sweep_store<512, 1, 8, false>', 'kh_ell_forward_update<512, 1, 8, false, false>'],
     so=['kh_ell_forward_update<512, 1, 8, true, false>'], fmt='csr')
for _name, _build in (('banded_ladder', _banded_ladder), ('lindblad_liouv', lambda: _liouv(_lindblad5()))):
    case('ellstream_' + _name, _build, 'ellstream/csr', ['kh_ell_sweep_store<512, 8, 4, true>', 'kh_ell_forward_update<512, 8, 4, false, true>'],
         so=['kh_ell_forward_update<512, 8, 4, true, true>'], fmt='csr', env={'KH_KERNEL': 'ellstream'})
    case('ellglobal_' + _name, _build, 'ellglobal/csr', ['kh_ellg_sweep_store<512>', 'kh_ellg_forward_update<512, false>'],
         so=['kh_ellg_forward_update<512, true>'], fmt='csr', env={'KH_KERNEL': 'ellglobal'})
    case('ellsplit_' + _name, _build, 'ellsplit/csr', ['kh_ellgs_sweep_store<512>', 'kh_ellgs_forward_update<512, false>'],
         so=['kh_ellgs_forward_update<512, true>'], fmt='csr', env={'KH_KERNEL': 'ellglobal'}, row_split=2)
    case('generic_csr_' + _name, _build, 'generic/csr', ['kh_gen_sweep_store<false>', 'kh_gen_forward_update<false>'],
         fmt='csr', env={'KH_KERNEL': 'generic'})

# ---- rows of the series witness: the families whose accepted series runs beyond theta = 2 (padded rows: up to 6,
# cooperative A^2 chain: up to 4), at a theta just under a threshold theta_b(m) of their table, the generator dominated by
# the anti-Hermitian control.  A wrongly accepted real-spectrum series is then 100 x the tolerance and more off per step
# (test_series_witness); the engine must reject it by detection (Taylor's series: test_classifier_sparse_controls)
case('ell_hot_anti', lambda: _hot(_banded(nt=7), 'csr', 4.5743), 'ell/csr',
     ['kh_ell_sweep_store<512, 1, 12, false>', 'kh_ell_forward_update<512, 1, 12, false, false>'], fmt='csr', series=6.0)
case('coop_hot_anti', lambda: _hot(_shared(1), 'dense', 2.9243), 'coop16/mfma',
     ['kh_coop_forward_update<8, 4, false, true, true, false>', 'kh_coop_sweep_store<8, 4, true>'], env={'KH_COOP_COLS': '4'},
     series=4.0)

# ---- objectives of different dimension and kind
case('mixed', _mixed, 'generic/mixed', ['kh_gen_sweep_store<true>', 'kh_gen_forward_update<true>'], so=['kh_gen_forward_update<true>'],
     fmt='mixed')

# the same problem with the update sums on the adjoint side and on the forward side
PAIRS = [('tn_n70', 'tn_n70_fwd_side'), ('tn_n90_L2', 'tn_n90_L2_fwd_side'), ('generic', 'generic_fwd_side')] + \
        [('coop_c%d' % c, 'coop_c%d_fwd_side' % c) for c in (2, 4, 16)]


@functools.lru_cache(maxsize=None)
def problem(name):
    """Everything a case's sweeps take (built once; never modified)."""
    return tac.build_problem(CASES[name], CASES[name].build())


@functools.lru_cache(maxsize=None)
def oracle_sweeps(name, use_scipy=False):
    return tac.compute_sweeps(problem(name), CASES[name].so is not None, use_scipy=use_scipy)


# ---- two problems outside the table's form: Lindblad form (H + c_ops, explicit interval values) and a replica batch
@functools.lru_cache(maxsize=None)
def lindblad_case():
    """Matrix form, d = 6, one collapse operator, two objectives; the control's Hamiltonian part is ``lower``."""
    import test_lindblad_form as tlf

    c = tlf._random(6, 2, 1, 1, 8, 3)
    H1 = _vary('lower', c.H[0][1], np.random.default_rng(5))
    c.H = [[row[0], H1] for row in c.H]
    rng = np.random.default_rng(5)
    p = types.SimpleNamespace(spec=c, prob=c.oracle(), gp=tlf._pulses(c), S=[np.linspace(0.2, 1.0, len(c.dt))], lam=[0.7],
                              norms=0.5 * (1.0 + rng.random(c.K)) / c.K, tol=TOL_LIOUVILLE)
    p.chi_T = p.prob.target / np.linalg.norm(p.prob.target, axis=1)[:, None]
    return p


@functools.lru_cache(maxsize=None)
def replica_batch():
    """Three L = 1 problems (those of ``test_replicas.batch('L1_small')``); only the LAST replica's control -- of all its
    objectives -- is ``lower``."""
    import test_replicas as tr

    reps = [copy.copy(r) for r in tr.batch('L1_small')[:3]]
    _nsa(reps[2], 'lower')
    return reps


def _replica_problem(r):
    p = types.SimpleNamespace(spec=r, prob=spec_to_oracle(r), gp=r.pulses, S=r.shapes, lam=r.lambdas, norms=r.chi_norms, tol=TOL_HILBERT)
    p.chi_T = r.target / np.linalg.norm(r.target, axis=1)[:, None]
    return p


def _extra_problem(name):
    return lindblad_case() if name == 'lindblad_form' else _replica_problem(replica_batch()[2])


@functools.lru_cache(maxsize=None)
def _extra_sweeps(name, use_scipy=False):
    return tac.compute_sweeps(_extra_problem(name), False, use_scipy=use_scipy)


EXTRA = ('lindblad_form', 'replica_L1')


def _p_and_ref(name, use_scipy=False):
    if name in EXTRA:
        return _extra_problem(name), _extra_sweeps(name, use_scipy), False
    return problem(name), oracle_sweeps(name, use_scipy), CASES[name].ladder


# ---------------------------------------------------------------------------
# host only: what the cases are; the oracle tells right from wrong and agrees with itself
# ---------------------------------------------------------------------------
def _equal_adjoint(op, sign):
    return np.array_equal(op, sign * op.conj().T)


def test_case_table_is_what_it_says():
    """The changed controls are neither plus nor minus their adjoint (``anti``: minus in Hilbert space, plus in Liouville
    space, exactly), the others and every drift are what the builders of krotov_amd/configs.py made; with several controls
    only the last is changed, in the ``_last`` cases only the last objective's; shared lists stay shared."""
    for name, c in CASES.items():
        spec = problem(name).spec
        if c.fmt == 'mixed':
            continue
        supers = spec.is_super
        for k in range(spec.K):
            for l in range(spec.L):
                op, was_changed = spec.Hc[k][l], (k, l) in spec.changed
                plus, minus = _equal_adjoint(op, 1.0), _equal_adjoint(op, -1.0)
                if name.endswith(('_anti', '_selfadjoint')):
                    assert was_changed and (plus, minus) == ((True, False) if supers else (False, True)), (name, k, l)
                elif was_changed:
                    assert not plus and not minus and l == spec.L - 1, (name, k, l)
                    part = 0.5 * (op + (1.0 if supers else -1.0) * op.conj().T)  # what makes the generator non-normal
                    eps = max(np.abs(p).max() for p in problem(name).gp)
                    assert np.linalg.norm(part, 2) * eps * spec.tlist[-1] <= 1.0, (name, k, l)
                else:
                    assert (minus if supers else plus), (name, k, l)
        if '_last' in name:
            assert sorted({k for k, _ in spec.changed}) == [spec.K - 1], name
        else:
            assert sorted({k for k, _ in spec.changed}) == list(range(spec.K)), name
        assert 6 <= len(spec.tlist) - 1 <= 11 or name.startswith(('coop', 'ens', 'stream')), name
    for name in ('coop_c4', 'coop_c4_L2', 'ell_lindblad_liouv', 'ell_banded_ladder'):
        spec = problem(name).spec
        assert all(row is spec.Hc[0] for row in spec.Hc) and all(h is spec.H0[0] for h in spec.H0), name
    spec = problem('ell_banded_ladder_last').spec
    assert spec.Hc[0] is spec.Hc[1] and spec.Hc[2] is not spec.Hc[0]
    # the block masks of the ladder and of its adjoint differ (what kh_coop_adj_mask_kernel must get right)
    H1 = problem('coop_c4').spec.Hc[0][0]
    assert not np.array_equal(_block_mask(H1), _block_mask(H1.conj().T))
    # the matrix-form case: the control's Hamiltonian part is not Hermitian, the drift's is
    c = lindblad_case().spec
    assert not _equal_adjoint(c.H[0][1], 1.0) and _equal_adjoint(c.H[0][0], 1.0) and c.d == 6 and len(c.C[0]) == 1
    reps = replica_batch()
    assert [any(not _equal_adjoint(op, 1.0) for row in r.Hc for op in row) for r in reps] == [False, False, True]


def _block_mask(H, b=16):
    """(N / 16, N / 16) booleans: the 16 x 16 block holds a non-zero."""
    G = (H.shape[0] + b - 1) // b
    P = np.zeros((G * b, G * b), dtype=bool)
    P[:H.shape[0], :H.shape[1]] = H != 0
    return P.reshape(G, b, G, b).any(axis=(1, 3))


def _with_adjoints(prob, control):
    """``prob`` whose adjoint objectives take ``control(H_l)`` for H_l^dagger (the drift's adjoint stays right)."""
    wrong = copy.copy(prob)
    wrong.adjoint_ops = lambda: [[row[0].conj().T] + [None if o is None else control(o) for o in row[1:]] for row in prob.ops]
    return wrong


class _Mu:
    """``ko._mu_apply`` with ``control(H_l)`` for H_l: the update sum <chi| mu |phi> = <mu^dagger chi|phi> of a kernel that
    took a wrong operator for H_l^dagger on the adjoint side (mu carries the factor i in Liouville space, as in the oracle)."""

    def __init__(self, control):
        self.control = control

    def __enter__(self):
        self.orig = ko._mu_apply

        def mu(problem, k, l, state):
            op = problem.ops[k][1 + l]
            if op is None:
                return 0 * state
            return (1j if problem.is_super else 1.0) * (self.control(op) @ state)

        ko._mu_apply = mu

    def __exit__(self, *exc):
        ko._mu_apply = self.orig
        return False


def _wrong_variants(p, ref, ladder):
    """{variant: {quantity: distance from the right result}}"""
    def update(prob, chi):
        with helpers.MemoExpm():
            return ko.forward_update_sweep(prob, chi, p.norms, p.gp, p.S, p.lam)

    def dist(x, y):
        d = float(np.abs(np.array(x) - np.array(y)).max())
        return d if np.isfinite(d) else float('inf')  # (the hot rows: a wrong backward generator grows until the update overflows)

    out = {}
    controls = [o for row in p.prob.ops for o in row[1:] if o is not None]
    # (a), (b): the backward generator from H_l / from H_l^T; the update sweep then runs on that co-state store ((a) is
    # no mistake where every control IS its own adjoint: the self-adjoint super-operator)
    for tag, control in (('a: H_l', lambda o: o), ('b: H_l^T', lambda o: o.T)):
        if all(np.array_equal(control(o), o.conj().T) for o in controls):
            continue
        with helpers.MemoExpm():
            chi = ko.backward_sweep(_with_adjoints(p.prob, control), p.chi_T, p.gp)
        opt, psi_T, _ = update(p.prob, chi)
        out[tag] = dict(chi=dist(chi, ref.chi), opt=dist(opt, ref.update[0]), psi_T=dist(psi_T, ref.update[1]))
    # (c): <s H_l chi|phi> for <H_l^dagger chi|phi> -- unless s H_l IS the adjoint of every control (the ``anti`` cases)
    for s in (1.0, -1.0):
        if all(_equal_adjoint(o, s) for o in controls):
            continue
        with _Mu(lambda o, s=s: s * o.conj().T):  # (s H_l)^dagger in the ket
            opt, psi_T, _ = update(p.prob, ref.chi)
        out['c: %+d H_l' % s] = dict(opt=dist(opt, ref.update[0]), psi_T=dist(psi_T, ref.update[1]))
    # (d): V = (H_l^dagger under the block mask of H_l) chi, i.e. <chi| (H_l under the mask of H_l^dagger) |phi>
    if ladder:
        with _Mu(lambda o: np.where(np.kron(_block_mask(o.conj().T), np.ones((16, 16), dtype=bool))[:o.shape[0], :o.shape[1]], o, 0.0)):
            opt, psi_T, _ = update(p.prob, ref.chi)
        out['d: mask of H_l'] = dict(opt=dist(opt, ref.update[0]), psi_T=dist(psi_T, ref.update[1]))
    return out


@pytest.mark.parametrize('name', sorted(CASES) + list(EXTRA))
def test_oracle_tells_right_from_wrong(name):
    """(a) the backward generator built with H_l, (b) with H_l^T, (c) the update sums with +H_l chi or -H_l chi for
    H_l^dagger chi, (d) under ``ladder`` the block mask of H_l for that of H_l^dagger: each moves the co-state store (a, b),
    the updated pulses and the final states by more than 1e-6, five orders of magnitude and more above the tolerance of
    the GPU comparison.  The variants restate the mistakes on top of the oracle's own sweeps; the oracle is unchanged."""
    p, ref, ladder = _p_and_ref(name)
    with np.errstate(over='ignore', invalid='ignore'):  # (see ``dist``)
        moved = _wrong_variants(p, ref, ladder)
    smallest = min(d for per in moved.values() for d in per.values())
    for tag, per in moved.items():
        print('%s (%s): %s' % (name, tag, ', '.join('%s %.2e' % kv for kv in per.items())))
    print('%s: smallest witness distance %.2e' % (name, smallest))
    assert len(moved) >= (2 if name == 'q2_liouville_selfadjoint' else 3)
    for tag, per in moved.items():
        for what, d in per.items():
            assert d > 1e-6, (name, tag, what, d)


@pytest.mark.parametrize('name', sorted(CASES) + list(EXTRA))
def test_oracle_agrees_with_itself(name):
    """The oracle's two exponentials (its own Pade form, SciPy's) agree to 1e-13 on every sweep of every case: the
    non-normal generators do not cost the reference its accuracy."""
    p, own, _ = _p_and_ref(name)
    other = _p_and_ref(name, use_scipy=True)[1]
    opt_scale = max(1.0, np.abs(np.array(own.update[0])).max())
    apart = dict(states=np.abs(own.states - other.states).max(), chi=np.abs(own.chi - other.chi).max(),
                 opt=np.abs(np.array(own.update[0]) - np.array(other.update[0])).max() / opt_scale,
                 psi_T=np.abs(own.update[1] - other.update[1]).max(), fw_T=np.abs(own.fw_T - other.fw_T).max(),
                 g_a=np.abs(own.update[2] - other.update[2]).max() / max(1.0, np.abs(own.update[2]).max()))
    if own.so is not None:  # the second-order sweep with its stored trajectory
        so_scale = max(1.0, np.abs(np.array(own.so[0])).max())
        apart.update(so_opt=np.abs(np.array(own.so[0]) - np.array(other.so[0])).max() / so_scale,
                     so_psi_T=np.abs(own.so[1] - other.so[1]).max(), so_store=np.abs(own.so[3] - other.so[3]).max(),
                     so_g_a=np.abs(own.so[2] - other.so[2]).max() / max(1.0, np.abs(own.so[2]).max()))
    print('%s: %s' % (name, ', '.join('%s %.2e' % kv for kv in apart.items())))
    assert np.abs(own.states).max() < 10.0  # the states stay O(1): the absolute tolerances mean what they mean elsewhere
    for what, d in apart.items():
        assert d <= 1e-13, (name, what, d)


# ---- the series a wrong accept would run
def _disk_error(c, theta, n=48):
    """max over the disk |z| <= theta of |sum_j c_j z^j - e^z|: the error of the polynomial on any NORMAL generator
    f A dt of norm theta (on the boundary by the maximum principle; sampled there and on the two axes)."""
    z = theta * np.exp(2j * np.pi * np.arange(4 * n) / (4 * n))
    return float(np.abs(helpers.series_polynomial(c, z) - np.exp(z)).max())


def test_real_spectrum_series_on_the_disk():
    """What a wrongly accepted real-spectrum series could cost, from the library's exported tables.  Register families
    sub-step at theta <= 1, so they run degrees up to m = 14 (theta_b(14) = 1.058), each at theta <= theta_b(m): on EVERY
    normal generator of that norm -- the anti-Hermitian extreme included -- the degree-m polynomial is less than 100 x
    1e-12 from the exponential, so no result-level comparison at the project's tolerance could show the wrong accept
    there; the product count does.  The padded-row family runs the form up to theta = 6 and the cooperative A^2 chain up
    to 4: just under their last thresholds the same maximum is beyond 100 x 1e-12 -- the rows ``ell_hot_anti`` and
    ``coop_hot_anti`` sit there."""
    theta_b, c = helpers.series_coefficients(2.0)
    assert np.array_equal(theta_b, helpers.series_degree_tables()['real'])
    worst = 0.0
    for m in range(2, 16, 2):
        assert theta_b[m] < (1.06 if m == 14 else 1.0)
        worst = max(worst, _disk_error(c[m, :m + 1], theta_b[m]))
    assert theta_b[16] > 1.0  # (degree 16 serves theta > 1.058 only: never picked under sub-steps at theta <= 1)
    print('real-spectrum polynomial on the disk |z| <= theta_b(m), m <= 14: at most %.2e from e^z (%.1f x 1e-12)' % (worst, worst / 1e-12))
    assert 1e-12 < worst < 100 * 1e-12
    for cap, m_last in ((4.0, 22), (6.0, 26)):
        theta_b, c = helpers.series_coefficients(cap)
        assert theta_b[m_last] < cap <= theta_b[m_last + 2]
        far = _disk_error(c[m_last, :m_last + 1], theta_b[m_last])
        print('cap %g: degree %d on the disk |z| <= %.3f: %.2e from e^z (%.0f x 1e-12)' % (cap, m_last, theta_b[m_last], far, far / 1e-12))
        assert far >= 100 * 1e-12


SERIES_ROWS = sorted(name for name, c in CASES.items() if c.series)


@pytest.mark.parametrize('name', SERIES_ROWS)
def test_series_witness(name):
    """The real-spectrum polynomial of the degree the engine would pick had it wrongly accepted the form (``series_plan``
    on the family's table and cap), on the case's actual generator f (H0 + eps H1) dt of every interval under the guess:
    its distance from the exponential (spectral norm: the step's error on a unit state) is 100 x the case's tolerance or
    more, with theta just under a threshold theta_b(m) of the table."""
    c, p = CASES[name], problem(name)
    spec = p.spec
    theta_b, coeff = helpers.series_coefficients(c.series)
    theta = helpers.theta_sequence(helpers.explicit(spec, c.fmt))[0]
    nsub, deg = helpers.series_plan(theta, c.series, theta_b)
    f = 1.0 if spec.is_super else -1.0j
    factors = []
    for n, dt in enumerate(np.diff(spec.tlist)):
        m = int(deg[n])
        assert nsub[n] == 1 and 0.99 * theta_b[m] < theta[n] <= theta_b[m], (n, theta[n], theta_b[m])
        Z = f * (spec.H0[0] + p.gp[0][n] * spec.Hc[0][0]) * dt
        err = np.linalg.norm(helpers.series_polynomial(coeff[m, :m + 1], Z) - ko.expm_dense(Z), 2)
        factors.append(err / p.tol)
    print('%s: theta %.4f just under theta_b(%d) = %.4f; smallest series-witness factor %.0f x the tolerance %.0e'
          % (name, theta[0], int(deg[0]), theta_b[int(deg[0])], min(factors), p.tol))
    assert min(factors) >= 100.0, factors


def test_ladder_rows_are_wider_forward_than_backward():
    """``kh_ell_layout`` / ``kh_ell_layout_global`` (host code of the library) on the banded problem with the ``ladder``
    control and on its adjoints: the dense row makes the forward rows 28 slots wide, the dense column it becomes leaves
    the backward rows at 12 (one instantiation, that of the wider direction, serves both pools)."""
    from test_capi_symbols import _ell_layout
    from test_sparse_large import _layout_global
    import scipy.sparse as sp

    spec = problem('ell_banded_ladder').spec
    fw = [sp.csr_matrix(spec.H0[0]), sp.csr_matrix(spec.Hc[0][0])]
    bw = [sp.csr_matrix(m.conj().T) for m in fw]
    E_fw, E_bw = _ell_layout(fw, spec.N)[0], _ell_layout(bw, spec.N)[0]
    Eg_fw, Eg_bw = _layout_global(fw, spec.N)[1], _layout_global(bw, spec.N)[1]
    print('ladder on banded_n40: padded row width forward %d backward %d; global form %d / %d' % (E_fw, E_bw, Eg_fw, Eg_bw))
    assert (E_fw, E_bw) == (28, 12) and (Eg_fw, Eg_bw) == (28, 12)
    # ... and with Hermitian operators they are equal
    plain = _banded()
    ops = [sp.csr_matrix(plain.H0[0]), sp.csr_matrix(plain.Hc[0][0])]
    assert _ell_layout(ops, plain.N)[0] == _ell_layout([sp.csr_matrix(m.conj().T) for m in ops], plain.N)[0] == 12


def test_nonselfadjoint_draws_from_its_own_generator():
    """``fuzz_parity.py --nonselfadjoint`` decides with a generator of its own: the default stream draws the same problems
    with and without it, bit for bit apart from the controls it replaces, and all three kinds occur."""
    import fuzz_parity

    seed = 20261018
    plain, varied = np.random.default_rng(seed), np.random.default_rng(seed)
    rng_nsa = np.random.default_rng([seed, 0x5ad1])
    kinds = set()
    for _ in range(40):
        a, tag_a, fmt_a = fuzz_parity.draw(plain)
        b, tag_b, fmt_b = fuzz_parity.draw(varied, rng_nsa=rng_nsa)
        assert (a.name, a.K, a.N, a.L, len(a.tlist), fmt_a) == (b.name, b.K, b.N, b.L, len(b.tlist), fmt_b)
        assert tag_b.startswith(tag_a.replace(' shared', ''))
        assert all(np.array_equal(x, y) for x, y in zip(a.H0, b.H0))
        changed = getattr(b, 'changed', {})
        kinds |= set(changed.values())
        for k in range(a.K):
            for l in range(a.L):
                x, y = a.Hc[k][l], b.Hc[k][l]
                if (k, l) in changed:
                    assert not np.array_equal(x, y) and not _equal_adjoint(y, 1.0)
                else:
                    assert (x is None and y is None) or np.array_equal(x, y)
    assert kinds == {'lower', 'ladder', 'anti'}
    assert plain.random() == varied.random()


# ---------------------------------------------------------------------------
# GPU: every family against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_nonselfadjoint_control_vs_oracle(name, monkeypatch):
    tac.check_case(name, CASES[name], problem(name), oracle_sweeps(name), monkeypatch)


def _backward_and_update(c, p, monkeypatch, env=None, ref=None, name=''):
    """Backward and update sweep of a case's engine under ``env`` (on top of the case's own); host arrays, the products the
    update sweep issued and the launched instantiations.  ``ref``: compared with the oracle at the case's tolerance."""
    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    with monkeypatch.context() as m:
        for key, value in dict(c.env, **(env or {})).items():
            m.setenv(key, value)
        spec = p.spec
        eng = HipKrotovEngine(tac._engine_ops(spec, c.fmt), np.diff(spec.tlist), is_super=spec.is_super)
        try:
            if c.row_split:
                eng.set_row_split(c.row_split)
            _lib.forget_launched_kernels()
            chi = eng.backward(p.chi_T, np.array(p.gp))
            opt, psi_T, g_a = (x.cpu().numpy() for x in eng.forward_update(chi, p.norms, p.prob.init, np.array(p.gp), np.array(p.S), np.array(p.lam)))
            eng.check()
            got = types.SimpleNamespace(kernel=eng.kernel, chi=chi.cpu().numpy(), opt=opt, psi_T=psi_T, g_a=g_a,
                                        matvecs=eng.stats()['matvecs'], launched=list(_lib.kernel_instantiations(launched_only=True)))
        finally:
            eng.close()
    if ref is not None:
        ref_opt, ref_ga = np.array(ref.update[0]), ref.update[2]
        tac._check(dict(chi=np.abs(got.chi - ref.chi).max(), opt=np.abs(got.opt - ref_opt).max() / max(1.0, np.abs(ref_opt).max()),
                        psi_T=np.abs(got.psi_T - ref.update[1]).max(),
                        g_a=np.abs(got.g_a - ref_ga).max() / max(1.0, np.abs(ref_ga).max())), p.tol, name, 'against the oracle')
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('adj,fwd', PAIRS)
def test_adjoint_side_and_forward_side_sums_agree(adj, fwd, monkeypatch):
    """V = H_l^dagger chi taken once per sweep (``kh_gen_adjoint_side`` / ``kh_coop_adjoint_side``) against <chi|H_l phi>
    on the forward side (KH_GEN_ADJ=0 / KH_COOP_NO_ADJ=1): the same problem, 1e-13 x scale apart at the most."""
    assert CASES[adj].build is CASES[fwd].build
    p = problem(adj)
    a = _backward_and_update(CASES[adj], p, monkeypatch)
    b = _backward_and_update(CASES[fwd], p, monkeypatch)
    scale, ga_scale = max(1.0, np.abs(a.opt).max()), max(1.0, np.abs(a.g_a).max())
    apart = dict(chi=np.abs(a.chi - b.chi).max(), opt=np.abs(a.opt - b.opt).max() / scale, psi_T=np.abs(a.psi_T - b.psi_T).max(),
                 g_a=np.abs(a.g_a - b.g_a).max() / ga_scale)
    print('%s against %s: %s' % (adj, fwd, ', '.join('%s %.2e' % kv for kv in apart.items())))
    for what, d in apart.items():
        assert d <= TOL_FORMS, (adj, fwd, what, d)


@pytest.mark.gpu
def test_lindblad_form_with_nonhermitian_control_vs_oracle():
    """``lindblad/matrix``: H rho - rho H of a control H that is not Hermitian, forward and backward (the oracle runs the
    Liouvillian ``liouvillian_dense`` makes of the same operators).  One family serves every sweep of this engine
    (``kh_lind_*<row blocking>``); it has no per-interval form (``forward_update_sharded`` answers KH_ERR_UNSUPPORTED:
    tests/test_lindblad_form.py) and no second order."""
    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine

    p, ref = lindblad_case(), _extra_sweeps('lindblad_form')
    c = p.spec
    eng = HipKrotovEngine(c.H, c.dt, c_ops=c.C)
    try:
        assert eng.kernel == 'lindblad/matrix'
        _lib.forget_launched_kernels()
        fw_T, states = (x.cpu().numpy() for x in eng.forward(np.array(p.gp), p.prob.init, store=True))
        chi = eng.backward(p.chi_T, np.array(p.gp))
        opt, psi_T, g_a = (x.cpu().numpy() for x in eng.forward_update(chi, p.norms, p.prob.init, np.array(p.gp), np.array(p.S), np.array(p.lam)))
        eng.check()
        launched = list(_lib.kernel_instantiations(launched_only=True))
    finally:
        eng.close()
    print('lindblad_form launched: %s' % ', '.join(launched))
    assert sorted(launched) == ['kh_lind_forward_update<1>', 'kh_lind_sweep_store<1>'], launched
    ref_opt = np.array(ref.update[0])
    tac._check(dict(states=np.abs(states - ref.states).max(), fw_T=np.abs(fw_T - ref.fw_T).max(), chi=np.abs(chi.cpu().numpy() - ref.chi).max(),
                    opt=np.abs(opt - ref_opt).max() / max(1.0, np.abs(ref_opt).max()), psi_T=np.abs(psi_T - ref.update[1]).max(),
                    g_a=np.abs(g_a - ref.update[2]).max() / max(1.0, np.abs(ref.update[2]).max())), p.tol, 'lindblad_form', 'single launch')


def _compare_replicas(reps, got):
    Kr = reps[0].K
    for b, r in enumerate(reps):
        p = _replica_problem(r)
        ref = _extra_sweeps('replica_L1') if r is replica_batch()[2] else tac.compute_sweeps(p, False)
        rows = slice(b * Kr, (b + 1) * Kr)
        ref_opt = np.array(ref.update[0])
        tac._check(dict(forward=np.abs(got[0][rows] - ref.fw_T).max(), chi=np.abs(got[1][rows] - ref.chi).max(),
                        opt=np.abs(got[2][b] - ref_opt).max() / max(1.0, np.abs(ref_opt).max()),
                        psi_T=np.abs(got[3][rows] - ref.update[1]).max(),
                        g_a=np.abs(got[4][b] - ref.update[2]).max() / max(1.0, np.abs(ref.update[2]).max())), p.tol,
                   'replica %d' % b, 'against the oracle')


@pytest.mark.gpu
def test_replica_batch_with_one_nonselfadjoint_control(monkeypatch):
    """``kh_rep_*<1>``: only the last of three replicas has a control that is not Hermitian.  One coefficient set serves
    the engine, so the whole batch runs on Taylor's: as many products as the same batch under KH_TAYLOR=1 -- and more than
    the batch of the three Hermitian problems, which takes the real-spectrum series."""
    import test_replicas as tr
    from krotov_amd import _lib

    reps = replica_batch()
    _lib.load()
    _lib.forget_launched_kernels()
    got = tr.run_engine(reps)
    launched = _lib.kernel_instantiations(launched_only=True)
    print('replica_L1 launched: %s' % ', '.join(launched))
    for want in ('kh_rep_sweep_store<1>', 'kh_rep_forward_update<1>'):
        assert want in launched, (want, launched)
    _compare_replicas(reps, got)
    hermitian = tr.run_engine(tr.batch('L1_small')[:3])[5]['matvecs']
    monkeypatch.setenv('KH_TAYLOR', '1')
    taylor = tr.run_engine(reps)[5]['matvecs']
    print('replica batch: matvecs %d, under KH_TAYLOR=1 %d, the Hermitian batch %d' % (got[5]['matvecs'], taylor, hermitian))
    assert got[5]['matvecs'] == taylor and hermitian < taylor


# ---------------------------------------------------------------------------
# GPU: the classifier at its edges -- every row asserts the decision
# ---------------------------------------------------------------------------
Q2_ADJ, Q2_FWD = 'kh_q2_forward_update<false, true, true>', 'kh_q2_forward_update<false, false, true>'
_q2_row = lambda build: types.SimpleNamespace(build=build, fmt='dense', env={'KH_KERNEL': 'q2'}, row_split=None, so=None)  # noqa: E731


def _decide(row, monkeypatch, name, taylor=True, no_adj=False):
    """The sweeps of an edge problem against the oracle, as the engine decides by itself; ``taylor`` / ``no_adj``: the
    products of the same problem under KH_TAYLOR=1 / KH_NO_ADJ=1 next to it."""
    p = tac.build_problem(row, row.build())
    ref = tac.compute_sweeps(p, False)
    got = _backward_and_update(row, p, monkeypatch, ref=ref, name=name)
    got.taylor = _backward_and_update(row, p, monkeypatch, env={'KH_TAYLOR': '1'}, ref=ref, name=name + ' KH_TAYLOR=1').matvecs if taylor else None
    got.no_adj = _backward_and_update(row, p, monkeypatch, env={'KH_NO_ADJ': '1'}, ref=ref, name=name + ' KH_NO_ADJ=1') if no_adj else None
    print('%s: %s; matvecs %d, under KH_TAYLOR=1 %s; launched %s' % (name, got.kernel, got.matvecs, got.taylor, ', '.join(got.launched)))
    return got


def _one_ulp(spec, what, where):
    """One element of the last objective's control (drift) moves by one unit in its last place: ``where`` = 'first' ->
    Re [0, 1]; 'last' -> Re of the last off-diagonal element [N - 1, N - 2]; 'diag' -> Im of the last diagonal element (0.0
    -> the smallest subnormal).  N = 17: the last elements sit in the tail of the 256-thread strided loop (289 = 256 + 33)."""
    k, N = spec.K - 1, spec.N
    if what == 'control':
        spec.Hc = [list(row) for row in spec.Hc]
        op = spec.Hc[k][0] = np.array(spec.Hc[k][0])
    else:
        spec.H0 = list(spec.H0)
        op = spec.H0[k] = np.array(spec.H0[k])
    i, j = {'first': (0, 1), 'last': (N - 1, N - 2), 'diag': (N - 1, N - 1)}[where]
    if where == 'diag':
        assert op[i, j].imag == 0.0
        op[i, j] = complex(op[i, j].real, np.nextafter(0.0, 1.0))
    else:
        op[i, j] = complex(np.nextafter(op[i, j].real, np.inf), op[i, j].imag)
    assert not _equal_adjoint(op, 1.0) and np.abs(op - op.conj().T).max() < 1e-12
    return spec


@functools.lru_cache(maxsize=None)
def _hermitian_q2(N, K):
    """The unchanged Hermitian problem of the one-bit rows (run once per size, under a patch context of its own)."""
    with pytest.MonkeyPatch.context() as mp:
        return _decide(_q2_row(lambda: _c5(K, N)), mp, 'hermitian_n%d' % N)


@pytest.mark.gpu
@pytest.mark.parametrize('where', ['first', 'last', 'diag'])
@pytest.mark.parametrize('what', ['control', 'drift'])
@pytest.mark.parametrize('N,K', [(17, 5), (64, 3)])
def test_classifier_one_bit_off(N, K, what, where, monkeypatch):
    """A Hermitian q2 problem with one bit of one operator of the last objective changed.  In the control: the sums move
    to the forward side (ADJ = false) and the series is Taylor's.  In the drift: ADJ stays true, and the series is what
    ``classify_operators`` prescribes for a defect of ~0 -- never longer than Taylor's."""
    name = 'one_bit_n%d_%s_%s' % (N, what, where)
    whole = _hermitian_q2(N, K)
    assert Q2_ADJ in whole.launched and Q2_FWD not in whole.launched and whole.matvecs < whole.taylor
    got = _decide(_q2_row(lambda: _one_ulp(_c5(K, N), what, where)), monkeypatch, name)
    if what == 'control':
        assert Q2_FWD in got.launched and Q2_ADJ not in got.launched, got.launched
        assert got.matvecs == got.taylor
    else:
        assert Q2_ADJ in got.launched and Q2_FWD not in got.launched, got.launched
        assert got.matvecs <= got.taylor
    assert got.taylor == whole.taylor


@pytest.mark.gpu
def test_classifier_beyond_the_grid_cap(monkeypatch):
    """K = 300, N = 8, L = 4: 1500 operators for the 1024 workgroups of ``kh_adjoint_sign_kernel``; only operator 1499 (the
    last control of the last objective), which a workgroup reaches in its SECOND pass, is not self-adjoint -- and the
    decision flips from the real-spectrum series to Taylor's."""
    row = lambda build: types.SimpleNamespace(build=build, fmt='dense', env={}, row_split=None, so=None)  # noqa: E731
    base = lambda: configs.config_c5(K=300, N=8, nt=6, L=4)  # noqa: E731
    whole = _decide(row(base), monkeypatch, 'k300_hermitian')
    got = _decide(row(lambda: _last(base(), 'lower')), monkeypatch, 'k300_operator_1499')
    assert got.kernel == whole.kernel and 300 * 5 > 1024
    assert whole.matvecs < whole.taylor and got.matvecs == got.taylor


def _with_defect(spec, delta, dt_all=None):
    """Every drift H0 - i gamma D (D diagonal, positive: decay) with gamma such that delta = max_k ||gamma D||_F x max dt,
    on a grid whose LAST interval is the longest (1.5 x)."""
    dt = np.diff(spec.tlist)
    dt[-1] *= 1.5
    spec.tlist = np.concatenate([[0.0], np.cumsum(dt)])
    D = np.diag(np.linspace(0.2, 1.0, spec.N)).astype(np.complex128)
    gamma = delta / (np.linalg.norm(D) * (dt.max() if dt_all is None else dt_all))
    made = {}
    for k, H in enumerate(spec.H0):
        if id(H) not in made:
            made[id(H)] = (H - 1j * gamma * D, H)
    spec.H0 = [made[id(H)][0] for H in spec.H0]
    part = max(np.linalg.norm(0.5 * (H - H.conj().T)) for H in spec.H0)
    assert abs(part * (dt.max() if dt_all is None else dt_all) - delta) < 1e-12
    return spec


def _slow_banded():
    """The banded problem on a grid 16 times as long (theta ~ 2.3 per interval): at the theta ~ 0.15 of its own grid the
    defect form and Taylor's series have the same degree and the decision would leave no trace in the product count."""
    spec = _banded()
    spec.tlist = 16.0 * spec.tlist
    return spec


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['q2', 'ell', 'replica'])
def test_classifier_defect_threshold(family, monkeypatch):
    """delta = || anti-Hermitian part of the drift ||_F x max dt at 0.049 and at 0.051 around the threshold 0.05 of the
    shortened series, the largest step being the LAST one: below, no more products than Taylor's; above, exactly Taylor's.
    Dense detection kernel, its host twin for sparse operators (``csr_part_fro2``), and a replica engine (the largest step
    over all replicas)."""
    pairs = {}
    for delta in (0.049, 0.051):
        name = 'defect_%s_%.3f' % (family, delta)
        if family == 'replica':
            import test_replicas as tr

            reps = [copy.copy(r) for r in tr.batch('L1_small')[:3]]
            dt_max = max(np.diff(r.tlist)[-1] * 1.5 for r in reps)
            reps = [_with_defect(r, delta, dt_all=dt_max) for r in reps]
            got = tr.run_engine(reps)
            _compare_replicas(reps, got)
            with monkeypatch.context() as m:
                m.setenv('KH_TAYLOR', '1')
                taylor = tr.run_engine(reps)[5]['matvecs']
            pairs[delta] = (got[5]['matvecs'], taylor)
        else:
            if family == 'q2':
                row = _q2_row(lambda d=delta: _with_defect(_c5(3, 17), d))
            else:
                row = types.SimpleNamespace(build=lambda d=delta: _with_defect(_slow_banded(), d), fmt='csr', env={}, row_split=None, so=None)
            got = _decide(row, monkeypatch, name)
            assert got.kernel == ('tile64q2/512' if family == 'q2' else 'ell/csr')
            if family == 'q2':  # (the controls are Hermitian on both sides of the threshold)
                assert Q2_ADJ in got.launched and Q2_FWD not in got.launched
            pairs[delta] = (got.matvecs, got.taylor)
    print('defect threshold, %s: (matvecs, Taylor) below %s above %s' % (family, pairs[0.049], pairs[0.051]))
    assert pairs[0.049][0] <= pairs[0.049][1] and pairs[0.051][0] == pairs[0.051][1]
    assert pairs[0.049][0] < pairs[0.051][0]  # (the decision really changed in between)


@pytest.mark.gpu
def test_classifier_sign_per_objective_only(monkeypatch):
    """Objective 0's control is Hermitian, objective 1's anti-Hermitian: each is +- its adjoint, neither sign holds for
    all, so the sums stay on the forward side (ADJ = false) and the series is Taylor's."""
    def build():
        spec = _c5(2, 17)
        spec.Hc[1] = [1j * spec.Hc[1][0]]
        return spec

    got = _decide(_q2_row(build), monkeypatch, 'sign_per_objective', no_adj=True)
    assert Q2_FWD in got.launched and Q2_ADJ not in got.launched, got.launched
    assert got.matvecs == got.taylor == got.no_adj.matvecs
    for what in ('opt', 'psi_T', 'g_a'):  # (the override is the same decision: the same kernel, the same numbers)
        assert np.array_equal(getattr(got, what), getattr(got.no_adj, what)), what


def _slower_banded(factor=8.0):
    spec = _banded()
    spec.tlist = factor * spec.tlist
    return spec


@pytest.mark.gpu
@pytest.mark.parametrize('control', ['ladder', 'hot_anti'])
def test_classifier_sparse_controls(control, monkeypatch):
    """The host twin ``csr_equal`` on its rejecting side: the banded problem with its Hermitian control runs the
    Chebyshev form (fewer products than under KH_TAYLOR=1; a grid 8 times as long, theta ~ 1.9, where the two series
    differ in degree), with the ``ladder`` control -- neither sign -- exactly Taylor's products; the row of the series
    witness (``anti``: minus its adjoint, which qualifies a Hilbert-space generator for nothing) likewise."""
    row = lambda build: types.SimpleNamespace(build=build, fmt='csr', env={}, row_split=None, so=None)  # noqa: E731
    if control == 'ladder':
        whole = _decide(row(_slower_banded), monkeypatch, 'sparse_hermitian')
        assert whole.kernel == 'ell/csr' and whole.matvecs < whole.taylor
        got = _decide(row(lambda: _nsa(_slower_banded(), 'ladder', row_cols=16)), monkeypatch, 'sparse_ladder')
    else:
        got = _decide(row(CASES['ell_hot_anti'].build), monkeypatch, 'sparse_hot_anti')
    assert got.kernel == 'ell/csr' and got.matvecs == got.taylor


# ---------------------------------------------------------------------------
# GPU: the fuzz sweep with non-self-adjoint controls, fixed seed
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_fuzz_parity_nonselfadjoint_fixed_seed():
    """40 drawn problems of ``fuzz_parity.py --nonselfadjoint`` (a random subset of the controls replaced by ``lower`` /
    ``ladder`` / ``anti`` variants) against the oracle at the tolerances of tests/test_hip_parity.py."""
    import fuzz_parity

    stats = {}
    done, failures = fuzz_parity.fuzz(20261018, cases=40, nonselfadjoint=True, stats=stats)
    assert done == 40 and stats['nonselfadjoint'] >= 15, stats  # (a quarter of the draws are Liouville-space problems: unchanged)
    assert not failures, '\n'.join(failures)
