/*
 * krotov_hip.h -- C ABI of the MI355X Krotov engine (libkrotov_hip.so).
 *
 * The library replaces ONE path of qucontrol/krotov: the per-iteration
 * backward/forward time propagation and sequential pulse-update loop of
 * krotov.optimize_pulses (reference src/krotov/optimize.py:393-510), which the
 * reference dispatches per objective through parallel_map
 * (src/krotov/parallelization.py:233-495) to krotov.propagators.expm
 * (src/krotov/propagators.py:79-122).  The reference has no native FFI for
 * this path (it is pure Python); each entry point below names the Python call
 * site it stands in for.  INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary: every call returns 0 on
 *     success or a negative kh_status; kh_last_error() gives the text.
 *   - complex128 = interleaved (re, im) doubles (numpy/torch layout).
 *   - operators: dense N x N, row-major.  States: length-N vectors; density
 *     matrices are column-stacked vec(rho) and operators Liouvillians
 *     (propagators.py:255-257, 306-307).
 *   - "dev" pointers are device (HBM) addresses owned by the caller (e.g.
 *     torch tensors); "host" pointers are ordinary host memory read during the
 *     call.  stream is a hipStream_t passed as void* (NULL = default stream).
 *     All sweeps are asynchronous on that stream.
 *   - not thread-safe per engine; one engine per device per stream.
 *
 * Memory contract (every "dev" pointer of every entry point; enforced by tests/test_memory_contract.py on guarded,
 * minimally aligned buffers)
 *   Alignment.  A device pointer is aligned to its element type and NO MORE is assumed: 16 bytes for kh_cdouble (the
 *     kernels load and store a complex number as one 16-byte access), 8 bytes for double, 4 bytes for int32_t.  Any
 *     element-aligned address qualifies -- a row of a larger array, a slice that starts in the middle of one; no
 *     kernel widens an access over two doubles or two indices of a caller's array.  A pointer below its element's
 *     alignment is undefined behaviour; the C entry points do not inspect addresses.
 *   Extent.  The library reads and writes only the extent documented for each argument ([K][nt][N], [L][nt-1], ...:
 *     exactly that many elements, densely packed, no padding behind rows), for every N, K, L and nt it accepts -- tiles
 *     are masked, nothing is prefetched past the last interval, element nt-1 of an [L][nt-1] array does not exist, a
 *     workgroup without an objective writes nothing.  CSR: indptr [N+1], indices [nnz], data [nnz]; every index read
 *     from them must be a valid column.  Memory next to an extent may hold anything, NaN included, and may be unmapped.
 *   Inputs are never written: operator arrays, CSR arrays, expectation operators, pulses, shapes, lambda, norms,
 *     sigma, init, targets, bell_dev, invariants_dev, chi_T, fw_prev_dev, u_guess_dev, dfdu_dev, src_store_dev and chi_norms_dev of
 *     kh_backward_store_source, ops_table_dev (and the operators it points to), factors_dev and in_store_dev of
 *     kh_apply_store -- and chi_store_dev in the update sweeps (kh_forward_update, kh_update_*), which only
 *     kh_backward_store / kh_backward_store_source write.  Outputs are the arguments marked OUT
 *     (and states_dev, psi_T_dev, chi_store_dev of the plain sweeps, tau_dev, out_dev, chi_T_dev, chi_norms_dev,
 *     J_dev, partial_dev); fw_store_dev and u_opt_dev are outputs of the update sweeps while set.  A sweep writes its outputs
 *     in full (replica engines: the active replicas' slices only, kh_set_active_replicas) and never reads what they
 *     held before it (kh_update_begin ... kh_update_end count as one sweep: opt_dev and g_a_dev are carried from
 *     call to call).
 *   Overlap.  No output overlaps any other argument of the same call, nor an array the engine holds a pointer to
 *     (operators, fw_prev_dev / fw_store_dev / sigma_dev, u_guess_dev / dfdu_dev / u_opt_dev); inputs may overlap one
 *     another freely (equal operator pointers, init_dev == a row block of a stored trajectory, ...).  One exception,
 *     which the per-interval driver relies on: D_dev of kh_update_step / kh_update_step_dev may be partial_dev itself
 *     (the all-reduce ran in place; the sums are read before the next interval's are written).  Between calls every
 *     buffer is the caller's again: the output of one call is commonly the input of the next (psi_T_dev ->
 *     kh_chi_boundary -> kh_backward_store -> kh_forward_update; fw_store_dev and fw_prev_dev swapped per iteration).
 *   Lifetime.  Operator and CSR arrays must stay valid and unchanged while the engine lives; the arrays of
 *     kh_set_second_order(_replicas) and kh_set_parametrization while they are set (their CONTENT may change between
 *     sweeps); everything else until the stream has passed the call.
 */
#ifndef KROTOV_HIP_H
#define KROTOV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kh_engine kh_engine;

typedef struct kh_cdouble {
    double re, im;
} kh_cdouble;

enum kh_status {
    KH_OK = 0,
    KH_ERR_INVALID = -1,     /* bad argument */
    KH_ERR_HIP = -2,         /* a HIP runtime call failed */
    KH_ERR_UNSUPPORTED = -3, /* size outside what the kernels handle */
    KH_ERR_TIMEOUT = -4,     /* in-kernel exchange gave up (see kh_check) */
    KH_ERR_NOMEM = -5
};

/* Problem description handed to kh_engine_create (all host memory, read once).
 *
 * ops[k*(1+L) + 0]   : drift operator of objective k   (sum of the non-list
 *                      entries of Objective.H)
 * ops[k*(1+L) + 1+l] : operator multiplying control l in objective k (sum over
 *                      every nested-list entry that carries control l,
 *                      mu.py:123-134), or NULL when the control does not occur
 *                      in objective k (mu.py:126-127).
 * Entries are DEVICE pointers; equal pointers mean a shared operator (the
 * engine stages each distinct operator, and its adjoint, once).
 */
typedef struct kh_problem {
    int32_t K;        /* objectives handled by this engine (this GPU's shard) */
    int32_t N;        /* state dimension */
    int32_t L;        /* controls: at most 32 (KH_ERR_UNSUPPORTED beyond); the register-resident kernel families
                         take up to 8 (4, 2 for some), with more the generic kernels run.
                         L = 0 (no controls) is accepted by every constructor except kh_engine_create_replicas
                         (KH_ERR_UNSUPPORTED: 1..4 controls): the plain sweeps run with pulses_dev == NULL, while
                         kh_forward_update, kh_update_begin and kh_set_parametrization answer KH_ERR_INVALID */
    int32_t nt;       /* len(tlist); nt-1 intervals */
    int32_t is_super; /* 0: Hilbert space, eqm factor -i (propagators.py:94);
                         1: Liouville space, factor 1 (propagators.py:96-98),
                            and mu = i * dL/d eps (mu.py:130-134) */
    int32_t reserved;
    const double *dt;              /* host [nt-1] interval lengths (may vary,
                                      optimize.py:450) */
    const kh_cdouble *const *ops;  /* host [K*(1+L)] of dev pointers */
    const double *op_norms;        /* host [K*(1+L)] upper bounds on the
                                      spectral norms, or NULL (engine then uses
                                      Frobenius norms: safe, slower) */
    double tol;       /* truncation tolerance of the exponential action per
                         sub-step; tol <= 0 or NaN -> 2^-53.  Every series
                         table of the engine is built for it (as
                         kh_series_tables does). */
    double theta_max; /* largest ||A dt|| handled by one Taylor sub-step;
                         0 -> 1.0 */
} kh_problem;

/* Last error text of the calling thread ("" if none). */
const char *kh_last_error(void);

/* Library/kernels build info, e.g. "krotov_hip 0.1 gfx950". */
const char *kh_version(void);

/* Create an engine on the current HIP device.  Stages adjoint copies of every
 * distinct operator (the adjoint objectives of optimize.py:263,
 * objectives.py:240-258) and the exchange workspace, and reads the operators
 * once more to pick its algorithms: operators that equal their own adjoint bit
 * for bit (Hilbert space) get a shorter series for exp(-i H dt) than the Taylor
 * series every other generator gets, and control operators that equal +/- their
 * adjoint let the update sweep take <chi|dH/d eps|phi> on the co-state's side.
 * Results agree with the general path to rounding; the operator arrays must not
 * change while the engine lives. */
int kh_engine_create(const kh_problem *problem, kh_engine **out);
void kh_engine_destroy(kh_engine *engine);

/* Sparse operators (large Liouvillians with a few entries per row -- the regime of the
 * reference's DensityMatrixODEPropagator, propagators.py:162-327, which integrates
 * d/dt vec(rho) = L vec(rho) with a sparse L).  Same engine, same entry points below;
 * the exponential action is the same truncated Taylor series with CSR
 * matrix-vector products, so results agree with the dense path to round-off (the
 * reference's zvode integration is only accurate to its rtol = 1e-6).
 *   indptr [N+1], indices [nnz] int32, data [nnz] complex: device pointers;
 *   data == NULL: operator absent.  ops_adj[i] is the conjugate transpose of
 *   ops[i] (the adjoint objectives, objectives.py:240-258), supplied by the caller;
 *   op_norms (upper bounds on the spectral norms, e.g. sqrt(||A||_1 ||A||_inf))
 *   are required. */
typedef struct kh_csr {
    int64_t nnz;
    const int32_t *indptr;
    const int32_t *indices;
    const kh_cdouble *data;
} kh_csr;

typedef struct kh_problem_csr {
    int32_t K, N, L, nt, is_super, reserved;  /* as in kh_problem */
    const double *dt;                          /* host [nt-1] */
    const kh_csr *ops;                         /* host [K*(1+L)] */
    const kh_csr *ops_adj;                     /* host [K*(1+L)] */
    const double *op_norms;                    /* host [K*(1+L)]; required: NULL is KH_ERR_INVALID */
    double tol, theta_max;                     /* as in kh_problem */
} kh_problem_csr;

int kh_engine_create_csr(const kh_problem_csr *problem, kh_engine **out);

/* Objectives of different dimension or kind in ONE engine (the reference treats every objective on its own,
 * optimize.py:254-261, 806-911; they meet only in the sum of the pulse update, :454-470): one launch per sweep, the
 * generic kernels' mixed form (kh_engine_kernel: "generic/mixed").
 *   problem->N        the stride S = max(dims) of every state buffer; problem->is_super is ignored
 *   dims     [K]      host: N_k of objective k
 *   is_super [K]      host: 0 Hilbert space (f = -i, mu factor 1), 1 Liouville space (f = 1, mu factor i)
 *   problem->ops[k*(1+L)+j]  a dense row-major dims[k] x dims[k] operator (NULL where a control is absent)
 * Every entry point takes the buffer shapes documented for it, [K][N] and [K][nt][N], at stride S.  Padding contract:
 * the sweeps read the first N_k entries of objective k's states and may find anything behind them; every state they
 * write (stored trajectories, psi_T, the second-order store) holds exact zeros behind them.  kh_tau and
 * kh_chi_boundary run at stride S: their targets must be zero behind N_k.  Dense operators only; Taylor series and the
 * update sums on the forward side; not sharded (kh_p2p_create_window refuses), kh_set_update_workgroups answers
 * KH_ERR_UNSUPPORTED.  KH_ERR_UNSUPPORTED for S > 2540 (the generic kernels' LDS) and more than 32 controls. */
int kh_engine_create_mixed(const kh_problem *problem, const int32_t *dims, const int32_t *is_super, kh_engine **out);

/* Density matrices under a d x d Hamiltonian and Lindblad operators -- the second way the reference writes an open
 * system (Objective.H = [H0, [H1, eps], ...], Objective.c_ops = [C_1, ...]; docs/10_howto.rst, mu.py:106-117) -- in
 * MATRIX form: d/dt rho = A rho + rho B + sum_j C_j rho C_j^+ with A = -i H(eps) - M/2, B = +i H(eps) - M/2,
 * M = sum_j C_j^+ C_j; the d^2 x d^2 Liouvillian is never built (kh_engine_kernel: "lindblad/matrix").  The engine
 * reports N = d*d and every entry point keeps its documented buffer shapes ([K][N], [K][nt][N], states column-stacked
 * vec(rho)); results equal, to rounding, those of kh_engine_create on liouvillian(H, c_ops) with is_super = 1 (the
 * reference ships no propagator that takes c_ops, and its default mu on such an objective is the bare H_l: the
 * Liouvillian form is its own recommended equivalent, and what this engine reproduces -- update sums
 * tr(chi^+ (H_l rho - rho H_l))).
 *   ops      [K*(1+L)]        host array of dev pointers: d x d row-major Hamiltonian parts (drift, then per control;
 *                             NULL: the control does not occur in the objective)
 *   c_ops    [K*n_c]          host array of dev pointers: d x d row-major Lindblad operators (NULL: absent); may be
 *                             NULL when n_c = 0
 *   op_norms [K*(1+L+n_c)]    host: spectral-norm bounds of (H0, H_1..H_L, C_1..C_nc) per objective, or NULL (Frobenius)
 * Limits: d <= 32, n_c <= 4, L <= 4 (KH_ERR_UNSUPPORTED beyond: build the Liouvillian and use kh_engine_create).
 * First-order update in one launch on one GPU: kh_set_second_order (non-NULL arguments), kh_set_update_workgroups
 * (> 0), kh_p2p_create_window and kh_update_begin / _step / _step_dev / _end answer KH_ERR_UNSUPPORTED.
 * kh_last_stats counts one product per series term. */
typedef struct kh_problem_lindblad {
    int32_t K, d, L, nt, n_c, reserved;
    const double *dt;                  /* host [nt-1] */
    const kh_cdouble *const *ops;      /* host [K*(1+L)] */
    const kh_cdouble *const *c_ops;    /* host [K*n_c] */
    const double *op_norms;            /* host [K*(1+L+n_c)] or NULL */
    double tol, theta_max;             /* as in kh_problem */
} kh_problem_lindblad;
int kh_engine_create_lindblad(const kh_problem_lindblad *problem, kh_engine **out);

/* Many independent small optimisations as ONE batch (kh_engine_kernel: "replica16/wave"): `replicas` = B problems of
 * the same shape -- K_r objectives each, dimension N, L controls, nt grid points, one kind -- that differ in
 * everything else: operators, states, weights, pulses, shapes, lambda_a and the time grid.  problem->K is the total
 * B * K_r (divisible by B); the objectives of replica b are k = b K_r ... (b + 1) K_r - 1.  Every sweep is one launch
 * over the batch; a replica's update sums never leave its workgroup, nothing waits on another workgroup, and a
 * replica's results depend neither on B nor on where in the batch it sits.
 *   dt_replicas  host [B][nt-1] time steps of every replica, or NULL: problem->dt for all of them (problem->dt may be
 *                NULL when dt_replicas is given)
 * Limits: dense operators, N <= 16, K_r <= 8, 1 <= L <= 4, one GPU (KH_ERR_UNSUPPORTED beyond;
 * NULL or non-divisible arguments: KH_ERR_INVALID; both decided before the first HIP call).  The coefficient set of
 * the series (Taylor, real spectrum, defect) is chosen from ALL operators of the batch.
 * kh_forward_store / kh_backward_store / kh_forward_update keep their signatures and their state shapes at K total;
 * their pulse-like arguments are per replica (see there).  kh_tau, kh_chi_boundary and kh_expect are per objective and
 * work unchanged.  The second-order update takes one sigma row per replica: kh_set_second_order_replicas.
 * kh_set_second_order (non-NULL arguments: its sigma_dev is ONE row), kh_set_update_workgroups (> 0), kh_set_row_split,
 * kh_p2p_create_window and kh_update_begin / _step / _step_dev / _end answer KH_ERR_UNSUPPORTED.
 * kh_last_stats counts products per objective, summed. */
int kh_engine_create_replicas(const kh_problem *problem, int32_t replicas, const double *dt_replicas, kh_engine **out);

/* Which replicas the following sweeps of a replica engine work on: active_host [B] (host, copied; non-zero: active),
 * or NULL: all of them.  An inactive replica's workgroups return at once: its slices of EVERY output buffer of every
 * sweep (stored states, final states, optimized pulses, g_a) keep what they held.  KH_ERR_UNSUPPORTED on any other
 * engine. */
int kh_set_active_replicas(kh_engine *engine, const int32_t *active_host);

/* Workgroups of the replica update kernel (64 K_r threads) that one compute unit holds at once, as built
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor) -- of the instantiation the next update sweep launches: the
 * second-order one after kh_set_second_order_replicas.  Batches up to that x the number of compute units run in one
 * turn. */
int kh_replica_occupancy(kh_engine *engine, int32_t *workgroups_per_cu);

/* Which kernel family the engine selected: "lindblad/matrix" (kh_engine_create_lindblad), "tile64q2/512", "tile64/512", "tile64/256", "tile64/stream" (more objectives
 * than stay co-resident: one launch, the operators streamed; KH_NO_STREAM=1: "tile64/512 per interval"), "mini16/wave", "mini4/wave", "replica16/wave" (kh_engine_create_replicas), "coop16/mfma", "tile128/512" (per-objective operators, 64 < N <= 128), "ell/csr"
 * (sparse operators with the matrix in registers), "generic", "generic/csr" or "generic/mixed" (kh_engine_create_mixed). */
const char *kh_engine_kernel(const kh_engine *engine);

/* Forward propagation of K states over the whole grid under fixed pulses.
 * Replaces parallel_map[0](_forward_propagation, ...) (optimize.py:302-313,
 * 806-846).
 *   pulses_dev   [L][nt-1] doubles
 *   init_dev     [K][N]
 *   states_dev   [K][nt][N] all stored states (index 0 = init), or NULL to
 *                store nothing (first-order Krotov discards them, :329)
 *   psi_T_dev    [K][N] final states
 * Replica engines (kh_engine_create_replicas): pulses_dev is [B][L][nt-1], every replica under its own pulses.
 */
int kh_forward_store(kh_engine *engine, const double *pulses_dev,
                     const kh_cdouble *init_dev, kh_cdouble *states_dev,
                     kh_cdouble *psi_T_dev, void *stream);

/* Backward propagation of the (normalised) co-states under the guess pulses,
 * storing chi_k(t_n) for every n.  Replaces parallel_map[1](
 * _backward_propagation, ...) (optimize.py:413-425, 849-886): adjoint
 * operators, conjugated (real) pulse values, backwards=True.
 *   chi_T_dev    [K][N]
 *   chi_store_dev[K][nt][N]; [:, nt-1] = chi_T
 * Replica engines (kh_engine_create_replicas): pulses_dev is [B][L][nt-1].
 */
int kh_backward_store(kh_engine *engine, const kh_cdouble *chi_T_dev,
                      const double *pulses_dev, kh_cdouble *chi_store_dev,
                      void *stream);

/* Backward propagation with a source term: the co-state equation of a functional with a state-dependent running cost
 * g_b(phi(t)), d chi / dt = -i H^+ chi + d g_b / d <phi| (no counterpart in the reference, whose how-to "penalize
 * population in a forbidden subspace" names the inhomogeneous equation as not implemented).  With W_k(t_n) =
 * -d g_b / d <phi_k| (t_n) -- the sign convention of chi_k(T) = -d J_T / d <phi_k| --, trapezoid in the source and the
 * engine's own backward step V_n of kh_backward_store:
 *     chi[nt-1] = chi_T,   chi[n] = V_n (chi[n+1] + h_n W[n+1]) + h_n W[n],   h_n = dt_n / 2 / chi_norms[k]
 * (the sweeps propagate chi / ||chi(T)||, so the source is divided by the same norm; it is added once per interval, not
 * per sub-step of the series, with that interval's dt).
 *   chi_T_dev     [K][N]
 *   src_store_dev [K][nt][N] W_k(t_n); read-only (kh_apply_store forms it from a stored trajectory)
 *   chi_norms_dev [K] the norms taken out of chi_T, or NULL: 1
 *   chi_store_dev [K][nt][N] OUT; [:, nt-1] = chi_T
 * With src_store_dev all zeros the result equals kh_backward_store's where the same kernel family runs both.
 * KH_ERR_UNSUPPORTED on replica, Lindblad-form and mixed engines, and where neither the register-tile form (N <= 64, 1..4
 * controls) nor the generic kernels (N <= 2540) take the engine; KH_ERR_INVALID on a null argument (chi_norms_dev
 * excepted) and when src_store_dev overlaps chi_store_dev. */
int kh_backward_store_source(kh_engine *engine, const kh_cdouble *chi_T_dev, const double *pulses_dev,
                             const kh_cdouble *src_store_dev, const double *chi_norms_dev, kh_cdouble *chi_store_dev,
                             void *stream);

/* out[k][n] = factors[n] * Op_k * in[k][n] for a whole stored trajectory, one batched product on the fp64 matrix cores.
 *   ops_table_dev [K] DEVICE array of device pointers to row-major N x N operators in the engine's state space; equal
 *                 pointers share an operator, NULL writes exact zeros for that objective
 *   factors_dev   [nt] real factor per time point, or NULL: 1
 *   in_store_dev  [K][nt][N] read-only
 *   out_store_dev [K][nt][N] OUT
 * The source of kh_backward_store_source for g_b = (lambda_b / T) s_b(t) sum_k <phi_k|D_k|phi_k> is this call with
 * Op_k = D_k and factors[n] = -(lambda_b / T) s_b(t_n) on the forward states of the previous iteration.
 * Uniform engines only: KH_ERR_UNSUPPORTED on mixed and Lindblad-form engines; KH_ERR_INVALID on a null argument
 * (factors_dev excepted) and when in_store_dev overlaps out_store_dev. */
int kh_apply_store(kh_engine *engine, const kh_cdouble *const *ops_table_dev, const double *factors_dev,
                   const kh_cdouble *in_store_dev, kh_cdouble *out_store_dev, void *stream);

/* Forward sweep with the sequential pulse update, whole grid, one launch.
 * Replaces the time loop optimize.py:444-501 (mu() / overlap() per
 * (step, pulse, objective), the cross-objective sum at :470, the update at
 * :471-477 and parallel_map[2](_forward_propagation_step, ...) at :479-491).
 *   chi_store_dev [K][nt][N] from kh_backward_store
 *   chi_norms_dev [K]       norms taken out of chi before the backward sweep
 *   init_dev      [K][N]
 *   guess_dev     [L][nt-1]
 *   shape_dev     [L][nt-1] update shapes S_l on the intervals
 *   lambda_dev    [L]
 *   opt_dev       [L][nt-1] OUT optimized pulses
 *   psi_T_dev     [K][N]    OUT
 *   g_a_dev       [L]       OUT integrals of g_a (optimize.py:475)
 * The cross-objective sum is evaluated in a fixed order (bitwise repeatable).
 * Replica engines (kh_engine_create_replicas): guess_dev, shape_dev and opt_dev are [B][L][nt-1], lambda_dev and
 * g_a_dev [B][L]; the sum runs over the K_r objectives of each replica, in objective order.
 */
int kh_forward_update(kh_engine *engine, const kh_cdouble *chi_store_dev,
                      const double *chi_norms_dev, const kh_cdouble *init_dev,
                      const double *guess_dev, const double *shape_dev,
                      const double *lambda_dev, double *opt_dev,
                      kh_cdouble *psi_T_dev, double *g_a_dev, void *stream);

/* The single-launch update sweep on at most `max_workgroups` workgroups (0: back to the engine's own choice).  What a
 * caller does after kh_check returned KH_ERR_TIMEOUT -- co-tenants held compute units, the sweep's workgroups were not
 * all resident at once -- before it falls back to one launch per interval: the register-tile families (N <= 64, 1..4
 * controls) then run kh_stream_forward_update (every workgroup walks through several objectives per interval, about
 * 2x the time at half the workgroups instead of 10x), ensembles run the matrix-core kernel with more objectives per
 * workgroup.  KH_ERR_UNSUPPORTED for the other families, for sharded engines and below the smallest grid the kernels
 * take (16 objectives per workgroup).  *chosen (may be NULL): the grid the next sweep will use (with 0: the engine's own).  No counterpart in the
 * reference (its objectives are separate processes: parallelization.py:233-311). */
int kh_set_update_workgroups(kh_engine *engine, int32_t max_workgroups, int32_t *chosen);

/* Second-order Krotov update (optimize.py:434-443, 468-469, 492-500): the
 * following update sweeps add 0.5 sigma_n <phi_k(t_n) - fw_prev[k][n] | mu |
 * phi_k(t_n)> to every summand of the pulse update and store the propagated
 * states.
 *   fw_prev_dev  [K][nt][N] states propagated under the guess pulses
 *                (forward_states0; iteration 0: kh_forward_store's states)
 *   fw_store_dev [K][nt][N] OUT states under the optimized pulses
 *   sigma_dev    [nt-1] sigma(t) at the interval mid-points (optimize.py:452)
 * Pass three NULLs to return to the first-order update. */
int kh_set_second_order(kh_engine *engine, const kh_cdouble *fw_prev_dev,
                        kh_cdouble *fw_store_dev, const double *sigma_dev);

/* The second-order update of a replica engine (kh_engine_create_replicas): as kh_set_second_order, with every replica
 * under its own sigma(t).
 *   fw_prev_dev  [K][nt][N] (K = B K_r) states under the guess pulses (iteration 0: kh_forward_store's states)
 *   fw_store_dev [K][nt][N] OUT states under the optimized pulses; an inactive replica's slices keep what they held
 *   sigma_dev    [B][nt-1] sigma_b(t) at replica b's own interval mid-points
 * Three NULLs return the engine to the first-order update; NULL and non-NULL mixed, or fw_store_dev == fw_prev_dev:
 * KH_ERR_INVALID.  KH_ERR_UNSUPPORTED on any engine that is not a replica engine. */
int kh_set_second_order_replicas(kh_engine *engine, const kh_cdouble *fw_prev_dev, kh_cdouble *fw_store_dev,
                                 const double *sigma_dev);

/* Pulse parametrizations (bounded controls): eps_l(t) = f_l(u_l(t)) with an unconstrained u_l, and Krotov's update
 * applied to u_l.  At interval n, with D_l the update sum of today (second order: with its sigma term),
 *   D'      = dfdu[l][n] * D_l                       dfdu = f_l'(u_guess): the derivative at the GUESS
 *   u_new   = u_guess[l][n] + (S_l[n] / lambda_l) D'
 *   g_a_l  += (S_l[n] / lambda_l) D'^2 dt            the running cost in u
 *   eps_new = f_l(u_new)                             what the interval is propagated with
 * A control of kind KH_PAR_NONE is f = identity: the caller passes u = eps and dfdu = 1 for it. */
enum kh_par_kind {
    KH_PAR_NONE = 0,   /* eps = u */
    KH_PAR_LINEAR = 1, /* eps = a u + b */
    KH_PAR_SQUARE = 2, /* eps = u^2 */
    KH_PAR_TANHSQ = 3, /* eps = a tanh^2 u            a = eps_max */
    KH_PAR_TANH = 4    /* eps = a tanh u + b          a = (eps_max - eps_min) / 2, b = (eps_max + eps_min) / 2 */
};

/* While set, the update sweeps (kh_forward_update, kh_update_begin / _step / _step_dev / _end) read u_guess_dev in
 * place of their guess argument, write u_new to u_opt_dev and eps_new to their opt argument.
 *   kind, a, b   [L] host arrays (copied); kind == NULL: parametrizations off, the other arguments are ignored
 *   u_guess_dev  [L][nt-1] u under the guess pulses
 *   dfdu_dev     [L][nt-1] f_l'(u_guess)
 *   u_opt_dev    [L][nt-1] OUT; must not alias u_guess_dev
 * The device pointers must stay valid while the parametrization is set.  Routes: the whole sweep of a register-tile
 * engine (N <= 64, 1..4 controls, its K > 1 workgroups resident) runs kh_tile_forward_update_par; everything else --
 * the other families, the per-interval calls, a grid reduced with kh_set_update_workgroups (any grid >= 1 while
 * parametrized; dropped again with the parametrization) -- runs kh_gen_forward_update_par on min(K, compute units)
 * workgroups.  The plain sweeps keep the engine's own family.  KH_ERR_UNSUPPORTED for replica and Lindblad-form
 * engines, sharded engines (kh_p2p_create_window), a row split above 1 and N beyond the generic kernels' LDS;
 * KH_ERR_INVALID for an unknown kind. */
int kh_set_parametrization(kh_engine *engine, const int32_t *kind, const double *a, const double *b,
                           const double *u_guess_dev, const double *dfdu_dev, double *u_opt_dev);

/* Non-linear controls: H(eps) = H_0 + sum_j eps_c(j)^p_j H_j.  The engine's L operator slots are J = L TERMS; term j
 * belongs to control c(j), 0 <= c(j) < C <= J, and has an integer power p_j in 1..4.  At interval n, with D_j the
 * update sum of slot j as today (second order: with its sigma term),
 *   w_j     = p_j eps_guess,c(j)[n]^(p_j - 1)          the derivative at the GUESS, formed by the caller: dcde_dev
 *   D_c     = sum_{j in c} w_j[n] D_j
 *   eps_c[n]= eps_guess,c[n] + (S_c[n] / lambda_c) D_c
 *   g_a,c  += (S_c[n] / lambda_c) D_c^2 dt_n
 *   c_j     = eps_c[n]^p_j                             by repeated multiplication; what interval n is propagated with
 *                                                      (theta of the series: sum_j |c_j| ||H_j||, as today)
 * The weights are applied after the exchange: the exchanged and the stepwise sums stay per term.
 * While set, the update sweeps (kh_forward_update, kh_update_begin / _step / _step_dev / _end) take guess, shape, lambda,
 * opt and g_a as arrays of C rows (of eps); partial_dev and D_dev stay J sums.  The plain, backward and source-term
 * sweeps and kh_expect are not touched: they take J rows of term coefficients c_j[n] = eps_c(j)[n]^p_j as before.
 *   C             number of controls
 *   term_control  [J] host array (copied); NULL: non-linear controls off, the other arguments are ignored
 *   term_power    [J] host array (copied)
 *   dcde_dev      [J][nt-1] w_j under the guess pulses; must stay valid while set
 * Routes: as kh_set_parametrization's -- the whole sweep of a register-tile engine (N <= 64, 1..4 terms, its K > 1
 * workgroups resident) runs kh_tile_forward_update_nl; everything else runs kh_gen_forward_update_nl on min(K, compute
 * units) workgroups (up to 32 terms; a grid reduced with kh_set_update_workgroups is dropped again with the setting).
 * KH_ERR_UNSUPPORTED for replica and Lindblad-form engines, sharded engines, a row split above 1 and N beyond the
 * generic kernels' LDS; KH_ERR_INVALID for a power outside 1..4, a control index outside 0..C-1, a control without a
 * term, and while a parametrization is set (kh_set_parametrization answers the same while this is set). */
int kh_set_nonlinear(kh_engine *engine, int32_t C, const int32_t *term_control, const int32_t *term_power,
                     const double *dcde_dev);

/* The same sweep cut at the cross-objective sum, for objectives sharded over
 * several GPUs: the caller all-reduces `partial` (L doubles, Im parts) across
 * ranks between two calls (RCCL over xGMI).
 *
 *   kh_update_begin : phi <- init, opt <- guess, g_a <- 0, and the local
 *                     partial sums of interval 0 -> partial_dev[L]
 *   kh_update_step  : given the all-reduced sums D of interval n: update
 *                     eps[n] (optimize.py:471-477), propagate every local phi
 *                     over interval n (:479-491) and emit the local partial
 *                     sums of interval n+1 -> partial_dev[L] (untouched after
 *                     the last interval)
 *   kh_update_end   : psi_T <- phi
 */
int kh_update_begin(kh_engine *engine, const kh_cdouble *chi_store_dev,
                    const double *chi_norms_dev, const kh_cdouble *init_dev,
                    const double *guess_dev, double *opt_dev, double *g_a_dev,
                    double *partial_dev, void *stream);
int kh_update_step(kh_engine *engine, int32_t n, const double *D_dev,
                   const kh_cdouble *chi_store_dev, const double *chi_norms_dev,
                   const double *shape_dev, const double *lambda_dev,
                   double *opt_dev, double *g_a_dev, double *partial_dev,
                   void *stream);
/* kh_update_step with the interval index kept in device memory (*n_dev is read
 * by the kernels and incremented after each call): consecutive calls are then
 * byte-identical launches, so a block of intervals -- including the caller's
 * RCCL all-reduce between them -- can be captured once in a HIP graph and
 * replayed, which removes the per-interval host launch cost of the sharded
 * sweep.  Calls past the last interval are no-ops. */
int kh_update_step_dev(kh_engine *engine, int32_t *n_dev, const double *D_dev,
                       const kh_cdouble *chi_store_dev, const double *chi_norms_dev,
                       const double *shape_dev, const double *lambda_dev,
                       double *opt_dev, double *g_a_dev, double *partial_dev,
                       void *stream);
int kh_update_end(kh_engine *engine, kh_cdouble *psi_T_dev, void *stream);

/* Device-side exchange across the GPUs of one node (objectives sharded over
 * `world` ranks, one per GPU): with it, kh_forward_update stays ONE persistent
 * launch per rank -- after the in-GPU stage the per-GPU sums of every interval
 * are exchanged through peer-mapped windows (xGMI) with system-scope atomics,
 * summed in rank order (bit-identical on every GPU), instead of one RCCL
 * all-reduce plus kernel launches per interval.
 *
 *   kh_p2p_create_window : allocate this rank's window (fine-grained device
 *                          memory) and return its 64-byte IPC handle
 *   kh_p2p_open_peers    : map all ranks' windows from the all-gathered
 *                          handles ([world][64] bytes, rank order)
 *   kh_p2p_selftest      : collective; runs `rounds` in-kernel exchanges and
 *                          verifies the totals.  Only after it succeeded on
 *                          every rank (the caller checks that) does
 *                          kh_forward_update use the cross-GPU stage.
 *   kh_p2p_disable       : fall back to the per-interval path (kh_update_*)
 * Every rank must call kh_forward_update the same number of times (epochs
 * advance in lock step) and synchronise with the others between sweeps (the
 * per-iteration all-gather of tau does). */
int kh_p2p_create_window(kh_engine *engine, int32_t world, int32_t rank,
                         unsigned char *ipc_handle_out /* [64] */);
int kh_p2p_open_peers(kh_engine *engine, const unsigned char *all_handles);
int kh_p2p_selftest(kh_engine *engine, int32_t rounds, void *stream);
int kh_p2p_disable(kh_engine *engine);

/* Diagnostics of the cross-GPU exchange (no counterpart in the reference), for the first run on a real multi-GPU node:
 *   out[0]  us per interval workgroup 0 of this rank waited for its own GPU's workgroups in the last sharded
 *           single-launch update sweep (in-GPU gather),
 *   out[1]  us per interval between publishing this GPU's sum into the peers' windows and holding every rank's sum
 *           (the cross-GPU hop: xGMI stores + the slowest rank's lag),
 *   out[2]  us per round of the last kh_p2p_selftest (publish -> all ranks' values read back, first round excluded),
 *   out[3]  ranks.
 * Kernels that run their own cross-GPU stage (one-wave, N <= 128 register-generator and sparse families) report 0 in
 * out[0], out[1]. */
int kh_p2p_stats(kh_engine *engine, double out[4]);

/* tau_k = <target_k | psi_k(T)> (optimize.py:316-322, 502-508;
 * second_order.py:69-83).  targets_dev, psi_T_dev [K][N]; tau_dev [K]. */
int kh_tau(kh_engine *engine, const kh_cdouble *targets_dev,
           const kh_cdouble *psi_T_dev, kh_cdouble *tau_dev, void *stream);

/* Expectation values of a stored trajectory, for every objective and grid point at once (what the reference's
 * Objective.propagate(..., e_ops=...) evaluates state by state on the host, objectives.py:338-433; the trajectory
 * stays on the device).  K, nt, N and the kind come from the engine; the kernel family does not matter, only the
 * store's layout: any engine of kh_engine_create, _csr or _lindblad qualifies.
 *   states_dev [K][nt][N]  what kh_forward_store (or kh_backward_store) stored
 *   e_ops      [K*n_e]     HOST array of device pointers, e_ops[k*n_e + e]: dense row-major operator e of objective
 *                          k; equal pointers = a shared operator (as kh_problem.ops); NULL = skipped, its outputs
 *                          are exact zeros.  Copied with hipMemcpyAsync on `stream`: keep it until that copy is done.
 *   out_dev    [n_e][K][nt]
 * Hilbert-space engines (is_super = 0): operators N x N, out[e][k][n] = <psi_k(t_n)| O_ke |psi_k(t_n)> (fp64 MFMA).
 * Liouville-space engines (is_super = 1, kh_engine_create_lindblad): N = d*d, operators d x d,
 * out[e][k][n] = tr(O_ke rho_k(t_n)) for column-stacked vec(rho).
 * One pass over the store serves up to 8 operators; more take ceil(n_e / 8) passes.  Results are bitwise repeatable.
 * KH_ERR_INVALID for a NULL engine, states, table or out and for n_e < 1 (checked before the device is touched);
 * KH_ERR_UNSUPPORTED for engines of kh_engine_create_mixed (per-objective operator shapes: not yet).  Calls on one
 * engine share a table buffer: issue them on one stream. */
int kh_expect(kh_engine *engine, const kh_cdouble *states_dev, const kh_cdouble *const *e_ops, int32_t n_e,
              kh_cdouble *out_dev, void *stream);

/* Boundary co-states of the built-in functionals, normalised for the backward
 * sweep: v_k = c_k target_k + d_k psi_k(T), chi_T[k] = v_k / ||v_k||_2,
 * chi_norms[k] = ||v_k||_2.  Replaces the chi_constructor call and the
 * normalisation of optimize.py:396-410 for krotov.functionals.chis_re /
 * chis_ss / chis_sm / chis_hs (functionals.py:177-197, 225-253, 293-317,
 * 389-437), whose per-objective scalars (c_k, d_k) the host derives from
 * tau and the objective weights: re (w/2K, 0), ss (tau_k w/K, 0),
 * sm (w/K^2 sum_j w_j tau_j, 0), hs (w/2K, -w/2K).  All arrays on the device:
 * targets, psi_T, chi_T [K][N]; c, d [K] complex; chi_norms [K]. */
int kh_chi_boundary(kh_engine *engine, const kh_cdouble *targets_dev,
                    const kh_cdouble *psi_T_dev, const kh_cdouble *c_dev,
                    const kh_cdouble *d_dev, kh_cdouble *chi_T_dev,
                    double *chi_norms_dev, void *stream);

/* Boundary co-states of the two gate functionals in the LOCAL INVARIANTS of a two-qubit gate, normalised for the backward
 * sweep: the perfect-entangler functional and the distance to a target gate up to single-qubit gates (the
 * chi_constructors the reference's notebook 07 and its how-tos take from the weylchamber package, run per iteration on
 * the host; krotov_amd/functionals.py: PerfectEntanglerChi, LocalInvariantsChi).  A gate is 4 consecutive objectives
 * k = 4 g ... 4 g + 3, the propagated Bell states; M = K / 4 gates (an ensemble, or one per replica).  With the Bell
 * states B_i and U[i][k] = <B_i|psi_{4g+k}(T)> (4 x 4):
 *   m = U^T U,  t = tr m,  d = det U,  G = t^2 / (16 d),  H = (t^2 - tr m^2) / (4 d),  g3 = Re H
 *   KH_LI_PE:  F = g3 |G| - Re G                  J_G = g3 conj(G) / (2 |G|) - 1/2 (the first term 0 at |G| = 0),  J_H = |G| / 2
 *   KH_LI_LI:  F = |G - G_O|^2 + (g3 - g3_O)^2    J_G = conj(G - G_O),  J_H = g3 - g3_O
 *   J = (1 - w) F + w (1 - tr(U^+ U) / 4)                                              (w = unitarity_weight in [0, 1])
 *   dG/dU = t U / (4 d) - G U^-T,   dH/dU = (t U - U m) / d - H U^-T
 *   D = dJ / d conj U = (1 - w) conj(J_G dG/dU + J_H dH/dU) - (w / 4) U
 *   v_k = -scale sum_i D[i][k] B_i,   chi_T[4g+k] = v_k / ||v_k||_2,   chi_norms[4g+k] = ||v_k||_2,   J[g] = J
 * (scale: the 1/M of a functional that is the mean over an ensemble of M gates; 1 for independent gates).  J is the raw
 * value: negative inside the polyhedron of perfect entanglers.  A zero v_k gives a zero row and norm 0.  A singular U --
 * |d| <= 1e-10 (||U||_F / 2)^4, or not a number -- gives zero rows, norms 0 and J[g] = NaN.
 *   psi_T_dev       [K][N]
 *   bell_dev        [4][N] shared by all gates, or [K/4][4][N] with bell_per_gate != 0
 *   mode            KH_LI_PE or KH_LI_LI
 *   invariants_dev  KH_LI_LI: (Re G_O, Im G_O, g3_O) as [3] doubles, or [K/4][3] with invariants_per_gate != 0;
 *                   KH_LI_PE: not read, may be NULL
 *   chi_T_dev [K][N], chi_norms_dev [K], J_dev [K/4]  OUT
 * One wavefront per gate, every sum in a fixed order: results are bitwise repeatable and do not depend on where in the
 * batch a gate sits.  Any engine of kh_engine_create, _csr or _replicas in Hilbert space (K, N come from the engine; the
 * kernel family does not matter); a replica engine needs K_r divisible by 4 and honours kh_set_active_replicas: an
 * inactive replica's slices of all three outputs keep what they held.  Decided before any HIP call: KH_ERR_INVALID for a
 * NULL argument, K (K_r) not divisible by 4, an unknown mode, w outside [0, 1]; KH_ERR_UNSUPPORTED for Liouville-space
 * engines (is_super), kh_engine_create_lindblad and kh_engine_create_mixed -- those keep the host constructor. */
enum kh_li_mode { KH_LI_PE = 0, KH_LI_LI = 1 };
int kh_chi_local_invariants(kh_engine *engine, const kh_cdouble *psi_T_dev, const kh_cdouble *bell_dev,
                            int32_t bell_per_gate, int32_t mode, const double *invariants_dev,
                            int32_t invariants_per_gate, double unitarity_weight, double scale,
                            kh_cdouble *chi_T_dev, double *chi_norms_dev, double *J_dev, void *stream);

/* The exact gradient of the time-discretised final-time functional for the pulse values (what a quasi-Newton method
 * such as L-BFGS-B takes over with near convergence; Krotov's own update sum is only its first order in dt):
 *   A_kn = H0_k + sum_l eps_l[n] H_lk,   phi_k(t_{n+1}) = exp(f A_kn dt_n) phi_k(t_n),   f = -i (Hilbert) or 1 (Liouville)
 *   dJ_T/d eps_l[n] = -2 sum_k ||chi_k|| Re < chi^_k(t_{n+1}) | L_exp(f dt_n A_kn)[ f dt_n H_lk ] | phi_k(t_n) >
 * with chi_k(T) = -dJ_T/d<phi_k(T)| propagated backward under the SAME pulses and L_exp(X)[E] the Frechet derivative of
 * the matrix exponential (the top-right block of exp([[X, E], [0, X]])), by a Taylor series of the block matrix one
 * degree above the sweeps' table at theta_max = 1 (krotov_amd/csrc/kh_grad.h).  The sum over k runs in objective order.
 *   fw_store_dev      [K][nt][N]   what kh_forward_store stored under `pulses_dev`
 *   chi_store_dev     [K][nt][N]   what kh_backward_store stored under the same pulses (normalised co-states)
 *   chi_norms_dev     [K]          ||chi_k(T)|| (kh_chi_boundary), or NULL: all 1
 *   pulses_dev        [L][nt-1]
 *   grad_dev          [L][nt-1]    OUT
 *   per_objective_dev [K][L][nt-1] OUT the terms of the sum over k, or NULL: a workspace of the engine (allocated by the
 *                                  first such call)
 * The inputs are only read; of the outputs exactly the documented extents are written, every element once.  A control
 * absent from an objective (NULL operator) contributes exact zeros.  Operators are neither assumed Hermitian nor
 * classified.  No atomics: results are bitwise repeatable and do not depend on the launch's grid.
 * Any dense uniform engine of kh_engine_create with 1 <= L <= 4 and N <= 96, whatever its kernel family.  Decided before
 * any HIP call: KH_ERR_INVALID for a NULL engine, store, pulses or grad and for L = 0; KH_ERR_UNSUPPORTED for N > 96,
 * L > 4 and for engines of kh_engine_create_csr, _mixed, _lindblad, _replicas and sharded ones (kh_p2p_*).
 * kh_pulse_gradient_limits answers the limits for a problem description alone (host only, no GPU needed): KH_OK, or the
 * code kh_pulse_gradient would return for an engine of that K, N, L, nt, with the same kh_last_error text. */
int kh_pulse_gradient(kh_engine *engine, const kh_cdouble *fw_store_dev /* [K][nt][N] */,
                      const kh_cdouble *chi_store_dev /* [K][nt][N] */, const double *chi_norms_dev /* [K] or NULL: 1 */,
                      const double *pulses_dev /* [L][nt-1] */, double *grad_dev /* OUT [L][nt-1] */,
                      double *per_objective_dev /* OUT [K][L][nt-1], or NULL: engine workspace */, void *stream);
int kh_pulse_gradient_limits(const kh_problem *problem);

/* After synchronising the stream: returns KH_ERR_TIMEOUT if an in-kernel
 * exchange gave up since the last call (outputs are then invalid), else 0. */
int kh_check(kh_engine *engine);

/* Statistics of the last sweep launched (for the roofline accounting):
 * stats[0] = Taylor matrix-vector products issued per objective, summed over
 * the grid (host-side estimate from the pulses is not possible for the update
 * sweep, so kernels count them), stats[1] = intervals, stats[2] = workgroups. */
int kh_last_stats(kh_engine *engine, double stats[4]);

/* The coefficient tables the kernels evaluate exp(f A dt) v with (host only, no GPU needed; for inspection
 * and tests).  The series is sum_j c_j (f A dt)^j v with real c_j; for every degree m <= 64:
 *   theta[m]            largest ||A dt|| the degree serves at tolerance `tol` (tol <= 0 or NaN: 2^-53),
 *   ratios[m*65 + 0]    c_0,   ratios[m*65 + 1] = c_1,   ratios[m*65 + j] = c_j / c_{j-1}  (j = 2..m).
 * real_spectrum = 0: Taylor (c_j = 1/j!, any generator; replaces SciPy's Pade expm behind
 * krotov.propagators.expm, propagators.py:100-117).  real_spectrum = 1: what an engine uses when every
 * operator equals its own adjoint and f = -+i: the truncated Chebyshev series of exp(-+i theta x) on [-1, 1]
 * in powers of (-+i theta x), even degrees only, theta <= 2 (Taylor beyond). */
int kh_series_tables(int32_t real_spectrum, double tol, double *theta /* [65] */, double *ratios /* [65*65] */);

/* The same tables of the Chebyshev form as an engine builds them for a generator f A dt that is anti-Hermitian only
 * up to a Hermitian part of norm <= `defect` (a weakly damped Liouvillian, a Hamiltonian with a small anti-Hermitian
 * part; the engine measures the defect of the drift, the controls must be exactly (anti-)self-adjoint), valid up to
 * theta <= `theta_cap` (2 for the register-tile kernels, 4 for the cooperative ones, 6 for the sparse ones; at most 8;
 * Taylor beyond).  The truncation
 * error is bounded on the numerical range, (1 + sqrt 2) 2 sum_{k>m} |J_k(theta)| cosh(k asinh(defect / theta)).
 * defect = 0 and theta_cap = 2 give kh_series_tables(1, ...).  Host only. */
int kh_series_tables_defect(double tol, double theta_cap, double defect, double *theta /* [65] */,
                            double *ratios /* [65*65] */);

/* The exactly-Hermitian Chebyshev-form tables (real_spectrum = 1, theta <= 2) with odd degrees too, as an engine
 * hands them to the workgroup-per-objective two-terms-per-phase kernels (KH_ODD_DEGREES=0: not at all): theta[m] of
 * an odd m is the largest theta the degree-m truncation serves by the same bound at the same `tol`; even entries equal
 * kh_series_tables(1, ...) bit for bit; odd m in the Taylor tail repeat m - 1.  Those kernels evaluate degree m as
 *   T_0 = c_0 v,  T_{2p+2} = r2_p (f h A)^2 T_{2p},  s = h (r1_0 v + sum_{p>=1} r1_p T_{2p}),
 *   result = sum_p T_{2p} + f A s
 * with c0[m] = c_0 and rows[(m*32 + p)*2 + {0, 1}] = {r1_p, r2_p}: P = (m + 1) / 2 terms T_0 .. T_{2P-2} and, for an
 * even m, T_m besides; for an odd m = 2P - 1 the row P - 1 is {r1_{P-1}, 0}.  Host only. */
int kh_series_tables_odd(double tol, double *theta /* [65] */, double *c0 /* [65] */, double *rows /* [65*32*2] */);

/* The padded row form the sparse kernels keep in registers (host only, no GPU needed; for inspection and tests): the
 * union of the patterns of an operator list (drift + controls; data == NULL: absent; HOST arrays here), entries some
 * control touches in the first Ec slots of every row, every row padded to E entries (multiples of four).
 *   off  [E][S]          byte offset (16 x column) of every entry's vector element; padding: the row itself
 *   vals [n_ops][E][S]   values of every operator on the union pattern (0 where it has no entry)
 * with S = kh_ell_rows_of(N) padded rows: the threads x rows per lane of the kernel instantiation that serves N (512,
 * 768, 1024, 1536 or 2048; 0: N > 2048).  off / vals may be NULL (sizes only); E_cap: entry slots the caller's arrays can
 * hold.  KH_ERR_UNSUPPORTED when N > 2048 or a row is wider than 32 entries (16 for N > 512, 8 for N > 1024): such
 * engines run the STREAMED form of the same kernels (kh_engine_kernel: "ellstream/csr"; N <= 4096, rows up to 32 entries:
 * the same arrays with S = N rounded up to 64, read from memory in every term instead of living in registers), and
 * the generic CSR kernels beyond that (N <= 2540: their vectors must fit LDS).  What none of these holds -- N > 4096, or
 * N > 2540 with a row wider than 32 -- runs the form with every vector in global memory ("ellglobal/csr", N <= 2^20):
 * kh_ell_layout_global gives its arrays, the streamed form's (S = N rounded up to 64) with rows of any width;
 * KH_ERR_UNSUPPORTED when N > 2^20. */
int32_t kh_ell_rows_of(int32_t N);
int kh_ell_layout(int32_t N, int32_t n_ops, const kh_csr *ops_host, int32_t *E, int32_t *Ec, int32_t *off,
                  kh_cdouble *vals, int32_t E_cap);
int kh_ell_layout_global(int32_t N, int32_t n_ops, const kh_csr *ops_host, int32_t *E, int32_t *Ec, int32_t *off,
                         kh_cdouble *vals, int32_t E_cap);

/* Spread every objective's rows over `workgroups_per_objective` workgroups (kh_engine_kernel: "ellsplit/csr"; no
 * counterpart in the reference): for sparse problems with a few large objectives, which otherwise use as many compute
 * units as there are objectives.  Only CSR engines in the form with global vectors ("ellglobal/csr") take it; every
 * other engine answers KH_ERR_UNSUPPORTED, as do S < 1, S beyond the device's compute units and a sharded engine.  1
 * restores the kernels of "ellglobal/csr" exactly.  The rows are dealt in 64-row chunks (kh_ellsplit_rows: part `part`
 * of S owns [*first, *first + *count), possibly nothing; host only); both sweeps then need all their workgroups resident
 * at once, every in-kernel wait is bounded (kh_check: KH_ERR_TIMEOUT), and kh_set_update_workgroups accepts only 0. */
int kh_set_row_split(kh_engine *engine, int workgroups_per_objective);
int kh_ellsplit_rows(int32_t N, int32_t S, int32_t part, int32_t *first, int32_t *count);

/* Test hook (no counterpart in the reference): keep `workgroups` CUs busy for `milliseconds` on `stream` with a
 * kernel that does nothing but hold a CU's LDS -- the situation the single-launch update sweep must survive
 * (another stream of the process holding compute units while its workgroups need to be resident all at once).
 * tests/test_hip_parity.py::test_update_sweep_next_to_a_busy_stream.  The kernel leaves all-ones bit patterns (NaN as
 * doubles) in the 128 KiB of LDS it held: test_kernels_do_not_read_uninitialised_lds runs the sweeps right behind it. */
int kh_debug_occupy(kh_engine *engine, int32_t workgroups, double milliseconds, void *stream);

/* Test hook (no counterpart in the reference): the sweep-kernel template instantiations of the library, one name per
 * line ("kh_q2_forward_update<false, true, true>").  which = 1: every instantiation some dispatch can select (host
 * only, no GPU needed); which = 0: those this process has launched so far; which = 2: forget that list (returns 0).  Writes at most cap - 1 characters and a
 * terminating 0 into buf (may be NULL); returns the buffer size the whole list needs.  With the environment variable
 * KH_LAUNCH_LOG=<file> every process also appends an instantiation's name to that file at its first launch:
 * tests/test_zz_kernel_coverage.py fails when an instantiation was never launched by an oracle-comparing test.  The
 * adjoint-side pre-passes in front of an update sweep are listed too ("kh_gen_adjoint_side", "kh_coop_adjoint_side"). */
int kh_debug_launched(int32_t which, char *buf, int32_t cap);

/* Test hook (host only, no GPU needed): the lane roles of the two-terms-per-phase kernels' row-broadcast map, as the
 * kernels compute them, for lane `lane` (0..63) of wave `wave` (0..7) of the 512-thread workgroup.
 *   out[0]  the matrix row whose elements the lane holds        out[1]  the first of its 8 adjacent columns
 *   out[2]  the vector element the lane reads from LDS (lane n of a 16-lane row: column out[1] + (n & 7))
 *   out[3]  the first of the four lanes on which the matrix core leaves the sum over the wave's lanes of that row
 *   out[4]  the row whose sum the lane receives                 out[5]  1: the lane writes it to LDS
 *   out[6]  the column half (0: columns 0..31, 1: 32..63) the wave's sums are partial sums of
 * KH_ERR_INVALID outside those ranges. */
int kh_debug_q2_lane_map(int32_t wave, int32_t lane, int32_t *out /* [7] */);

#ifdef __cplusplus
}
#endif
#endif /* KROTOV_HIP_H */
