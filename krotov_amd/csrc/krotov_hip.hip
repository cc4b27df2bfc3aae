// libkrotov_hip.so -- C ABI of the MI355X Krotov engine (include/krotov_hip.h).
//
// Host side: engine object, operator staging (adjoint copies), kernel-family
// selection and launches.  Device side: kh_tile64.h (N <= 64, operators in
// registers) and kh_generic.h (any N).  gfx950 only.
#include <hip/hip_runtime.h>

#include <cxxabi.h>
#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/krotov_hip.h"
#include "kh_common.h"
#include "kh_generic.h"
#include "kh_tile64.h"
#include "kh_tile64s.h"
#include "kh_tile64x.h"
#include "kh_tile64q2.h"
#include "kh_coop.h"
#include "kh_mini.h"
#include "kh_replica.h"
#include "kh_ell.h"
#include "kh_ellg.h"
#include "kh_tilen.h"
#include "kh_ens.h"
#include "kh_lind.h"
#include "kh_expect.h"
#include "kh_chi_li.h"
#include "kh_grad.h"
// the parallel build (krotov_amd/build.py, -DKH_TU=KH_TU_MAIN): the sweep kernels are instantiated in the family units
// (kh_tu.hip), here they are `extern template`; compiled by itself this file is the whole library in one unit
#include "kh_instances.inc"

static thread_local std::string g_last_error;

static int kh_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// a step that reports a status of its own
#define KH_TRY(step)                        \
    do {                                    \
        const int _rc = (step);             \
        if (_rc != KH_OK) return _rc;       \
    } while (0)

#define KH_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t _e = (call);                                                               \
        if (_e != hipSuccess)                                                                 \
            return kh_fail(KH_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                           __FILE__, __LINE__);                                               \
    } while (0)

enum KernelKind { KIND_GENERIC = 0, KIND_TILE_RPT2 = 1, KIND_TILE_RPT1 = 2, KIND_TILE_Q2 = 3, KIND_COOP = 4, KIND_ELL = 5, KIND_TILEN = 6, KIND_TILEX = 7 /* plain sweeps only: kind_store */, KIND_LIND = 8 /* kh_engine_create_lindblad */, KIND_REPLICA = 9 /* kh_engine_create_replicas */ };

// Switches, read from the environment ONCE, at creation (read_switches; not per launch, not per process: engines with
// different settings coexist)
struct KhSwitches {
    std::string kernel;  // KH_KERNEL (testing): "generic" | "tile256" | "tile512" | "q2" | "mini" | "coop" | "tilen" | "tilex" | "ellstream" | "ellglobal" | "ellsplit"
    bool kernel_set = false;
    bool kernel_is(const char *name) const { return kernel_set && kernel == name; }
    bool taylor, odd_degrees, no_adj, near_imag, ellstream, stepwise, stream, coop_xcd, coop_sq, coop_adj, tn_h1reg, tx, q2_store, ens2, gen_adj;
    double ell_cap;
    int ell_split, ell_groups;  // KH_ELL_SPLIT (0: 'auto'), KH_ELL_GROUPS (0: no cap)
    int stream_G, coop_cols, ens, ens_min_k, ens_ncg;
    int grad_grid;  // KH_GRAD_GRID (0: one workgroup column per objective)
    bool coop_launch, q2_single, tile_single, coop_single, poll_delay_set, timeout_set;
    int poll_delay, adj_poll_delay, coop_poll_delay;  // (s_sleep units of 64 cycles)
    long long timeout_ticks;                          // (100 MHz ticks)
    int p2p_fail_at, p2p_fail_rank, p2p_fail_sweep;
};

// Each switch keeps its own reading: "set and != 0" (on), "set and == 0" (off), a number, or (KH_KERNEL) a name.
static KhSwitches read_switches() {
    auto on = [](const char *name) { const char *d = getenv(name); return d != nullptr && atoi(d) != 0; };
    auto off = [](const char *name) { const char *d = getenv(name); return d != nullptr && atoi(d) == 0; };
    auto num = [](const char *name, int dflt) { const char *d = getenv(name); return d != nullptr ? atoi(d) : dflt; };
    KhSwitches s;
    if (const char *d = getenv("KH_KERNEL")) s.kernel = d, s.kernel_set = true;
    s.taylor = on("KH_TAYLOR");                // plain Taylor coefficients everywhere (A/B)
    s.odd_degrees = !off("KH_ODD_DEGREES");    // =0: the two-terms-per-phase kernels get the even-only table too (A/B)
    s.no_adj = on("KH_NO_ADJ");                // <chi|H phi> on the forward side (A/B; dense operators)
    s.near_imag = !off("KH_NEAR_IMAG");        // =0: Taylor instead of the near-imaginary form's coefficients (A/B)
    s.ell_cap = 0.0;                           // KH_ELL_CAP (> 0): another theta cap of the padded-row kernels' Chebyshev form
    if (const char *d = getenv("KH_ELL_CAP")) s.ell_cap = atof(d);
    s.ell_split = num("KH_ELL_SPLIT", 0);      // workgroups per objective under KH_KERNEL=ellsplit (unset: 'auto')
    s.ell_groups = num("KH_ELL_GROUPS", 0);    // at most this many groups of the split form (testing: objectives in turns)
    s.ellstream = !on("KH_NO_ELLSTREAM");      // no streamed padded-row form
    s.stepwise = !on("KH_NO_STEPWISE");        // no register-tile kernel with one launch per interval
    s.stream = !on("KH_NO_STREAM");            // that launch per interval instead of the streaming kernel (A/B)
    s.stream_G = num("KH_STREAM_G", 0);        // workgroups of the streaming kernel (testing)
    s.coop_cols = num("KH_COOP_COLS", 0);      // objectives per cooperative workgroup, 2 | 4 | 16 (testing)
    s.coop_xcd = !off("KH_COOP_XCD");          // =0: no column group per XCD
    s.coop_sq = !on("KH_COOP_NOSQ");           // no A^2 chain in the cooperative kernels
    s.coop_adj = !on("KH_COOP_NO_ADJ");        // the cooperative update sweep's sums by one more round per interval
    s.tn_h1reg = !off("KH_TN_H1REG");          // =0: the tilen kernels stream the control operator
    s.tx = !off("KH_TX");                      // =0: no tile64x kernels (A/B)
    s.q2_store = !off("KH_Q2_STORE");          // =0: the plain sweeps take the update sweep's own family (A/B)
    s.ens = num("KH_ENS", -1);                 // 0: no ensemble kernel; 1: for any K (testing)
    s.ens_min_k = num("KH_ENS_MINK", 257);     // smallest K that takes it
    s.ens_ncg = num("KH_ENS_NCG", 0);          // its column groups, 1 | 2 | 4 | 8 (testing)
    s.grad_grid = num("KH_GRAD_GRID", 0);      // kh_pulse_gradient: objectives in turns on this many workgroup columns (testing)
    s.ens2 = !off("KH_ENS2");                  // =0: no A^2-chain ensemble kernel (A/B)
    s.gen_adj = !off("KH_GEN_ADJ");            // =0: the generic kernels' update sums stay on the forward side
    s.coop_launch = !off("KH_COOP_LAUNCH");    // =0: plain launches instead of cooperative ones (A/B timing)
    s.q2_single = !off("KH_Q2_SINGLE");        // =0: the instantiations with the cross-GPU stage on one GPU too (A/B)
    s.tile_single = !off("KH_TILE_SINGLE");    // =0: the same for the one-term-per-phase kernels
    s.coop_single = !off("KH_COOP_SINGLE");    // =0: the same for the cooperative kernels' adjoint-side form
    // head start of the update-sum stores, ~0.4 us: measured best (one control); given in the environment, several
    // controls do not apply their own default
    s.poll_delay_set = getenv("KH_POLL_DELAY") != nullptr;
    s.poll_delay = num("KH_POLL_DELAY", 16);
    // the same where a matrix-vector product already sits between store and poll (kh_q2_forward_update, sums on the
    // adjoint side).  0 was best while a round polled with two 8-byte loads per slot; the 16-byte polls are out
    // sooner (the optimum moved by 7 units, ~0.2 us), and a first round that comes back stale costs a second round trip: K = 256, N = 64, update sweep 19.79 ms
    // at 0, 18.62 at 4, 17.82 at 6 and 7, 17.88 at 8, 18.37 at 12 (18.2 - 18.3 before the change; profiles/exchange_layout.txt)
    s.adj_poll_delay = num("KH_ADJ_DELAY", 7);
    // the same for the cooperative kernels' block exchange (a polling pass is four 16-byte loads per lane there: an
    // early, stale pass costs little -- measured 0 best)
    s.coop_poll_delay = num("KH_COOP_DELAY", 0);
    // bound on any in-kernel wait (1 s), e.g. longer under a profiler; given in the environment, the cross-GPU sweeps
    // keep it instead of their 10 s
    s.timeout_ticks = 100000000LL;
    s.timeout_set = false;
    if (const char *d = getenv("KH_TIMEOUT_MS"))
        if (atoll(d) > 0) s.timeout_ticks = atoll(d) * 100000LL, s.timeout_set = true;
    // fault injection for the sharded protocol (tests): rank KH_P2P_FAIL_RANK withholds its GPU's sum at interval
    // KH_P2P_FAIL_AT of its KH_P2P_FAIL_SWEEP-th update sweep through the peer windows (1-based; default 1)
    s.p2p_fail_at = num("KH_P2P_FAIL_AT", -1);
    s.p2p_fail_rank = num("KH_P2P_FAIL_RANK", 0);
    s.p2p_fail_sweep = num("KH_P2P_FAIL_SWEEP", 1);
    return s;
}

// What engine_create learns about the problem before it picks the kernel families (the device-side detection kernels,
// the padded row form, the ensemble detection)
struct KhFacts {
    int K, N, L, num_cus;
    bool csr, shared;            // sparse operators; every objective has the same operator list
    bool has_h1, all_h1;         // objective 0 / every objective has its first control
    bool ell = false, ell_stream = false;  // the padded row form (kh_ell.h) was built, in its streamed form
    bool ell_global = false;     // ... in the form with its vectors in global memory (kh_ellg.h; ell_stream: its pools)
    int ell_E = 0;               // ... widest row over all objectives and both directions
    int ens_ncg = 0;             // column groups of the ensemble kernel where the detection found (H0, s_k H1), else 0
    double adj_sign = 0.0;       // +1 / -1: every control operator equals +/- its adjoint exactly (else 0)
    bool real_spectrum = false;  // every operator Hermitian (bit for bit) and f = -+i
    double imag_defect = -1.0;   // >= 0: bound on the Hermitian part of f A dt when the controls' f H_l are exactly
                                 // anti-Hermitian (|| . ||_F of the drift's part x max dt); < 0: not of that kind
    double theta_max;            // as given (<= 0: the families' own default)
    bool lind = false;           // kh_engine_create_lindblad: d x d operators and Lindblad operators, matrix form (kh_lind.h)
};

// Which kernel families an engine runs, with every instantiation parameter (plan_families).  Two residency checks after
// staging may still demote it (q2 -> generic, ensemble off); the runtime fallbacks change kind_store / coop_xcd / coop_adj.
struct KhPlan {
    KernelKind kind = KIND_GENERIC;        // the update sweep (and its one-launch-per-interval form)
    KernelKind kind_store = KIND_GENERIC;  // the plain sweeps (no cross-objective coupling: any K)
    int max_wgs = 0, grid_update = 0;  // workgroups the in-kernel exchange takes; of the single-launch update sweep
    bool mini = false, quad = false;   // kind q2: the one-wave-per-objective kernels (kh_mini.h), one wave in all
    bool stepwise_only = false, stream = false;  // one launch per interval; unless the streaming kernel takes them (kh_tile64s.h) ...
    int stream_G = 0;                            // ... on this many workgroups
    int coop_G = 0, coop_Y = 0, coop_ks = 0, coop_cols = KH_COOP_COLS;  // kh_coop.h: row blocks, column groups, slots, objectives
    bool coop_xcd = false, coop_sq = false, coop_adj = false, coop_series = false;  // (coop_xcd / coop_adj: off at runtime too)
    bool tilen = false, tn_h1reg = false;  // kh_tilen.h lane-order copies; the control in registers too
    int tn_EP = 0;
    bool tx = false, tx_update = false;    // kh_tile64x.h lane-order copies (plain sweeps); its update sweep too
    bool ell_stream = false;               // kh_ell.h: streamed form, row width
    bool ell_global = false;               // kh_ellg.h: the streamed form's pools, every vector in global memory
    int ell_E = 0;
    bool ens = false, ens2 = true;         // kh_ens.h: the single-launch update sweep, whatever `kind` says; the A^2-chain form
    int ens_ncg = 0, ens_G = 0;
    bool stage_sq = false;                 // P0, P1, P2 of A^2 per objective (q2 kernels, the cooperative A^2 chain, ens2)
    double theta_max = 1.0;
    bool series_rows = false;              // series tables: the Chebyshev form's rows (theta cap, Hermitian defect), else Taylor's
    double series_cap = 2.0, series_defect = 0.0;
    // kh_q2_sweep_store / kh_q2_forward_update launches get the table that also serves odd degrees (sweep_args_q2);
    // every other kernel the engine launches keeps the even-only one
    bool q2_odd = false;

    // kh_forward_update runs kh_update_begin / _step / _end (no single launch)
    bool per_interval() const { return stepwise_only && !stream && !ens; }
    // workgroups of the single-launch update sweep
    int single_grid() const { return ens ? ens_G : (stream ? stream_G : grid_update); }
    // the sums cross workgroups (and GPUs) inside the update kernel; else kh_update_step + an all-reduce per interval
    bool exchanges_in_kernel() const { return !(stepwise_only && !ens); }
    // the ensemble kernel's column groups, and its workgroups *G, on at most max_G workgroups (0: its own grid)
    int ens_cols(int K, int max_G, int *G) const {
        int ncg = ens_ncg;
        *G = ens_G;
        if (max_G > 0)
            while (*G > max_G && ncg < KH_ENS_MAXCG) ncg *= 2, *G = (K + 2 * ncg - 1) / (2 * ncg);
        return ncg;
    }
    // the register-tile families, whose update sweep has a form on fewer workgroups (the streaming kernel)
    bool tile_family() const { return (kind == KIND_TILE_Q2 && !mini) || kind == KIND_TILE_RPT1 || kind == KIND_TILE_RPT2; }
    // ... whose single launch can run the tile kernel's parametrized / non-linear form (q2 kind, mini and quad included:
    // the kernel they already run stepwise): one resident workgroup per objective, more than one objective
    bool tile_form(int K) const {
        const bool tile_kind = kind == KIND_TILE_Q2 || kind == KIND_TILE_RPT1 || kind == KIND_TILE_RPT2;
        return tile_kind && !ens && !stream && !stepwise_only && grid_update == K && K > 1;
    }
};

// The variants of the update sweep an engine is switched to between sweeps.  The form of the pulse update: linear controls,
// pulse parametrizations eps_l = f_l(u_l) (kh_set_parametrization) or non-linear controls eps_c^p H_j (kh_set_nonlinear)
enum { FORM_LINEAR = 0, FORM_PAR = 1, FORM_NL = 2 };
struct KhUpdateForm {
    int tag = FORM_LINEAR;
    // FORM_PAR: the caller's device arrays; the engine's own copies of the host arrays kind [L] and a, b [2][L]
    const double *u_guess = nullptr, *dfdu = nullptr;
    double *u_opt = nullptr;
    int *d_kind = nullptr;
    double *d_ab = nullptr;
    std::vector<int> kind_host;  // what d_kind / d_ab hold
    std::vector<double> ab_host;
    // FORM_NL: the L slots are J terms of C controls; the caller's device array; the engine's own table [2][L]: term ->
    // control, term -> power
    const double *dcde = nullptr;
    int C = 0;
    int *d_tab = nullptr;
    std::vector<int> tab_host;  // what d_tab holds
    bool reduced = false;  // reduced_G was set while a form was (kh_set_update_workgroups): dropped with the form
    bool set() const { return tag != FORM_LINEAR; }
};
// what the refusals call a form: kh_set_parametrization's and kh_set_nonlinear's own (refuse_form), and those of the entry
// points that take no engine with a form set
static const struct KhFormWords {
    const char *noun, *plural, *no_rows, *is_set, *engine;
} kh_form_words[] = {
    {},
    {"pulse parametrization", "pulse parametrizations", "no controls to parametrize", "a pulse parametrization is set (kh_set_parametrization)", "a parametrized engine (kh_set_parametrization)"},
    {"non-linear controls", "non-linear controls", "no terms", "non-linear controls are set (kh_set_nonlinear)", "an engine with non-linear controls (kh_set_nonlinear)"},
};
// second-order update (kh_set_second_order, kh_set_second_order_replicas); all NULL = first order
struct KhSecondOrder {
    const cplx *fw_prev = nullptr;
    cplx *fw_store = nullptr;
    const double *sigma = nullptr;
};

struct kh_engine {
    int K, N, L, nt, is_super;
    // kh_engine_create_mixed: objectives of their own dimension and kind; N is then the stride max N_k of every buffer
    bool mixed = false;
    // kh_engine_create_lindblad: d x d Hamiltonians in d_ops_fw / d_ops_bw, the Lindblad operators and A0, B0 per direction
    bool lind = false;
    KhLindArgs lind_fw{}, lind_bw{};
    // kh_engine_create_replicas: B independent problems of Kr objectives each (K = B Kr; kh_replica.h); d_dt is [B][nt-1]
    int replicas = 0, Kr = 0;
    int *d_active = nullptr;     // [B] kh_set_active_replicas
    bool all_active = true;      // (the kernels then get no mask at all)
    const int *active_mask() const { return all_active ? nullptr : d_active; }
    KhMixedArgs mixed_fw{}, mixed_bw{};  // device arrays: dims [K], f [K] per direction, mu [K] (both share dims, mu)
    double tol;
    int device, num_cus;
    KhSwitches sw;
    KhPlan plan;
    std::vector<void *> owned;        // every device allocation made at creation (kh_engine_destroy frees them)
    // device-side problem data
    const cplx **d_ops_fw = nullptr;  // [K*(1+L)]
    const cplx **d_ops_bw = nullptr;  // [K*(1+L)] adjoints
    double *d_norms = nullptr;        // [K*(1+L)]
    double *d_dt = nullptr;           // [nt-1]
    double *d_deg_theta = nullptr;    // [KH_MAX_DEGREE+1] degree thresholds for tol
    KhCsr *d_csr_fw = nullptr;        // [K*(1+L)] sparse operators (kh_engine_create_csr), else NULL
    KhCsr *d_csr_bw = nullptr;        // [K*(1+L)] their conjugate transposes
    KhEll *d_ell_fw = nullptr, *d_ell_bw = nullptr;  // [K] sparse operators in padded row form (kh_ell.h), or NULL
    int *d_ell_off = nullptr;         // ... their column offsets and values (one pool each)
    cplx *d_ell_vals = nullptr;
    bool gen_fits = true;             // the generic kernels' LDS vectors fit (N <= 2540)
    cplx *d_ell_scratch = nullptr;    // the streamed padded-row form's per-workgroup scratch planes [workgroups][stride]
    long long ell_scratch_stride = 0;
    cplx *d_ellg_ws = nullptr;        // kh_ellg.h: per-group workspaces [ellg_wgs][stride] (term planes, running sum, values)
    long long ellg_ws_stride = 0;
    int ellg_wgs = 0;
    // kh_ellg.h's split form (kh_set_row_split): S workgroups per objective on `groups` groups; 1: its plain form
    int row_split = 1, split_groups = 0;
    unsigned int *d_split_counters = nullptr;  // [groups] barrier counters, a memory line each: one block, zeroed per launch
    size_t split_counters_bytes = 0;
    const cplx **d_coop_fops_fw = nullptr, **d_coop_fops_bw = nullptr;  // [1+L] fragment-ordered operator copies
    const cplx **d_coop_sq_fw = nullptr, **d_coop_sq_bw = nullptr;      // [3] the same for P0, P1, P2 (one control)
    kh_u64 *d_coop_vbuf = nullptr;
    size_t coop_vbuf_bytes = 0;
    unsigned int *d_coop_xcc = nullptr;      // [Y * G] placement check of the cooperative kernels (zeroed per launch)
    unsigned char *d_coop_adj_nz = nullptr;  // [G][G] non-zero 16 x 16 blocks of H_1^+
    cplx *d_coop_adj = nullptr;              // [K][nt][N], allocated by the first update sweep
    const cplx *coop_adj_op = nullptr;       // H_1^+, row-major (the staged adjoint of the shared control operator)
    const cplx **d_sq_fw = nullptr;   // [K*3] P0, P1, P2 of A^2 (q2 kernels), forward operators
    const cplx **d_sq_bw = nullptr;   // [K*3] the same for the adjoint operators
    const cplx **d_tn_fw = nullptr, **d_tn_bw = nullptr;  // [K*(1+L)] lane-order operator copies (kh_tilen.h), or NULL
    const cplx **d_tx_fw = nullptr, **d_tx_bw = nullptr;  // [K*(1+L)] lane-order 64 x 64 operator copies (kh_tile64x.h), or NULL
    const cplx *ens_H0 = nullptr, *ens_H1 = nullptr;
    double *d_ens_scale = nullptr;    // [K]
    double *d_q2_theta = nullptr, *d_q2_c0 = nullptr, *d_q2_rows = nullptr, *d_ratios = nullptr;  // series tables of the register-tile kernels
    double *d_q2o_theta = nullptr, *d_q2o_c0 = nullptr, *d_q2o_rows = nullptr;  // plan.q2_odd: the tables with odd degrees
    // workspaces
    cplx *d_phi = nullptr;            // [K][N]
    kh_u64 *d_slots = nullptr;        // [2][G][L][2]
    size_t slots_bytes = 0;
    unsigned int *d_abort = nullptr;
    unsigned long long *d_wait_ticks = nullptr;  // [4] kh_p2p_stats: in-GPU gather, cross-GPU wait (last sharded sweep); self-test ticks, rounds
    double *d_stats = nullptr;        // [4] (+ 64 trace stamps behind them in a KH_TIMING build)
    double *d_wg_partial = nullptr;   // [G][L]
    double *d_step_partial = nullptr; // [L] the interval's sums of kh_forward_update's per-interval path
    cplx *d_gen_scratch = nullptr;    // [gen_scratch_wgs][N][N] generic kernels: the interval's generator (ensure_gen_scratch)
    int gen_scratch_wgs = 0;
    bool gen_scratch_failed = false;
    // generic kernels, first order, dense operators: the update sums on the adjoint side (kh_gen_adjoint_side):
    // H_lk^+ chi_k(t_n) for the whole co-state store, [L][K][nt][N], formed in front of every update sweep
    cplx *d_gen_adj = nullptr;
    bool gen_adj_failed = false;      // the allocation did not fit: the sums stay on the forward side
    bool gen_adj_ready = false;       // d_gen_adj holds the store of the sweep in progress (stepwise launches reuse it)
    double adj_sign = 0.0;            // KhFacts::adj_sign (0 with KH_NO_ADJ)
    const double *guess_dev = nullptr;  // remembered by kh_update_begin
    KhSecondOrder so;
    bool second_order() const { return so.sigma != nullptr; }
    KhUpdateForm form;
    // cross-GPU exchange (kh_p2p_*): objectives sharded over `p2p_world` ranks
    int p2p_world = 1, p2p_rank = 0;
    kh_u64 *p2p_window = nullptr;            // this rank's window (fine-grained device memory)
    size_t p2p_window_bytes = 0;
    std::vector<void *> p2p_opened;          // peer windows opened through IPC
    kh_u64 **d_p2p_peers = nullptr;          // device array [world] of window pointers
    unsigned int p2p_epoch_base = 0;         // advanced by nt per sweep: epochs never repeat
    bool p2p_ready = false;
    int p2p_sweeps = 0;
    double last_intervals = 0, last_wgs = 0;
    int last_update_grid = 0;  // workgroups of the last single-launch update sweep where the ensemble / streaming kernels ran it
    int reduced_G = 0;  // kh_set_update_workgroups: the single-launch update sweep on at most this many workgroups (0: off)
    std::set<const void *> lds_raised;  // kernels whose dynamic-LDS limit was raised on this engine's device
    const cplx **d_expect_tab = nullptr;  // [K * n_e] kh_expect: the last call's operator table (grown on demand)
    size_t expect_tab_entries = 0;
    double *d_grad_ws = nullptr;  // [K][L][nt-1] kh_pulse_gradient without a caller's per-objective array (first such call)
};

// Kernels with more than 64 KiB of dynamic LDS need the limit raised once per device: remembered per
// engine (an engine is bound to one device), not per process.
static int ensure_dynamic_lds(kh_engine *e, const void *func, size_t bytes) {
    if (bytes <= 48 * 1024 || e->lds_raised.count(func)) return KH_OK;
    KH_HIP(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    e->lds_raised.insert(func);
    return KH_OK;
}

// The update-sweep kernels that exchange partial sums in-kernel spin until EVERY workgroup of the grid has
// published: all of them must be resident at once.  Launching them cooperatively makes the runtime check the grid
// against the occupancy of this very kernel (register / LDS footprint as built) -- instead of assuming one
// workgroup per CU from multiProcessorCount.  It does NOT keep other streams off the device (ROCm 7.2, measured:
// tests/test_hip_parity.py::test_update_sweep_next_to_a_busy_stream): CUs held by somebody else still lead to a
// partial start, which the bounded in-kernel waits turn into KH_ERR_TIMEOUT and the caller into a repeat of the
// sweep with one launch per interval (krotov_amd/optimize.py).
// KH_COOP_LAUNCH=0 keeps plain launches (A/B timing: a cooperative launch costs ~15-20 us of host time).
// ---- which sweep-kernel instantiations exist and which have been launched (kh_debug_launched) ----
// Every launch of a sweep kernel goes through launch_plain<Kernel> / launch_persistent<Kernel>; naming the kernel as a
// template argument instantiates KhKernelTag<Kernel>, whose static member registers the instantiation when the library
// is loaded: the registry is exactly the set of instantiations some dispatch can select.
// (engines may be driven from different host threads -- one engine per thread, INTEGRATION.md 4 --: the flags are atomics,
// the registry itself is only appended to while the library is loaded)
struct KhKernelRecord {
    std::string name;
    std::atomic<bool> launched{false};
    std::atomic<bool> logged{false};  // written to KH_LAUNCH_LOG by this process
    explicit KhKernelRecord(std::string n) : name(std::move(n)) {}
};
static std::deque<KhKernelRecord> &kh_kernel_registry() {
    static std::deque<KhKernelRecord> reg;
    return reg;
}
static int kh_register_kernel(const void *host_stub) {
    // the host-side launch stub's symbol, demangled: "void __device_stub__kh_q2_forward_update<false, true, true>(KhSweepArgs, ...)"
    std::string s = "?";
    Dl_info info;
    if (dladdr(host_stub, &info) != 0 && info.dli_sname != nullptr) {
        int status = 0;
        char *dem = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
        s = (status == 0 && dem != nullptr) ? dem : info.dli_sname;
        free(dem);
        if (s.compare(0, 5, "void ") == 0) s = s.substr(5);
        const size_t stub = s.find("__device_stub__");
        if (stub != std::string::npos) s.erase(stub, 15);
        // cut the parameter list: the '(' that closes the name (template arguments hold no parentheses here)
        const size_t paren = s.find('(');
        if (paren != std::string::npos) s = s.substr(0, paren);
    }
    kh_kernel_registry().emplace_back(s);
    return (int)kh_kernel_registry().size() - 1;
}
template <auto Kernel>
struct KhKernelTag {
    static inline const int index = kh_register_kernel((const void *)Kernel);
};
static void kh_note_launch(int index) {
    KhKernelRecord &rec = kh_kernel_registry()[index];
    rec.launched.store(true, std::memory_order_relaxed);
    if (rec.logged.load(std::memory_order_relaxed)) return;
    // (tests: one line per instantiation and process, appended; the variable is read at every launch so that a test
    // session can switch the log on for its oracle-comparing tests only -- tests/conftest.py)
    if (const char *path = getenv("KH_LAUNCH_LOG")) {
        if (path[0] == 0) return;
        if (FILE *f = fopen(path, "a")) {
            fprintf(f, "%s\n", rec.name.c_str());
            fclose(f);
            rec.logged.store(true, std::memory_order_relaxed);
        }
    }
}
template <class... P>
static std::tuple<P...> kh_param_tuple(void (*)(P...));

template <auto Kernel, class... Args>
static void launch_plain(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    kh_note_launch(KhKernelTag<Kernel>::index);
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
}

template <auto Kernel, class... Args>
static int launch_persistent(const kh_engine *e, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    kh_note_launch(KhKernelTag<Kernel>::index);
    if (grid.x * grid.y * grid.z == 1) {
        hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
        return KH_OK;
    }
    if (!e->sw.coop_launch) {
        // a plain launch has the same residency but nobody checks the grid against it (the cooperative launch below
        // does): ask the occupancy of THIS instantiation as built -- registers, scratch, LDS -- once per shape, so that
        // a grid that cannot be co-resident is refused here (KH_ERR_UNSUPPORTED: the caller takes a smaller grid or one
        // launch per interval) instead of ending in a timeout
        static std::map<std::tuple<const void *, unsigned, size_t, int>, int> per_cu_of;
        static std::mutex per_cu_lock;  // (two engines launching from two host threads share the cache)
        const auto key = std::make_tuple((const void *)Kernel, block.x, lds, e->device);
        int per_cu = -1;
        {
            std::lock_guard<std::mutex> hold(per_cu_lock);
            auto it = per_cu_of.find(key);
            if (it != per_cu_of.end()) per_cu = it->second;
        }
        if (per_cu < 0) {
            per_cu = 0;
            KH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)Kernel, (int)block.x, lds));
            std::lock_guard<std::mutex> hold(per_cu_lock);
            per_cu_of.emplace(key, per_cu);
        }
        if ((long long)per_cu * e->num_cus < (long long)grid.x * grid.y * grid.z)
            return kh_fail(KH_ERR_UNSUPPORTED, "the update sweep's %u workgroups cannot all be resident on this device (%d per CU)",
                           grid.x * grid.y * grid.z, per_cu);
        hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
        return KH_OK;
    }
    decltype(kh_param_tuple(Kernel)) packed(args...);
    constexpr size_t NP = std::tuple_size<decltype(packed)>::value;
    void *ptrs[NP];
    int i = 0;
    std::apply([&](auto &...a) { ((ptrs[i++] = (void *)&a), ...); }, packed);
    const hipError_t err = hipLaunchCooperativeKernel((const void *)Kernel, grid, block, ptrs, (unsigned int)lds, st);
    if (err == hipErrorCooperativeLaunchTooLarge) {
        (void)hipGetLastError();
        return kh_fail(KH_ERR_UNSUPPORTED, "the update sweep's %u workgroups cannot all be resident on this device",
                       grid.x * grid.y * grid.z);
    }
    if (err != hipSuccess) return kh_fail(KH_ERR_HIP, "hipLaunchCooperativeKernel failed: %s", hipGetErrorString(err));
    return KH_OK;
}

// the same after raising the kernel's dynamic-LDS limit (ensure_dynamic_lds)
template <auto Kernel, class... Args>
static int launch_plain_lds(kh_engine *e, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    const int rc = ensure_dynamic_lds(e, (const void *)Kernel, lds);
    if (rc == KH_OK) launch_plain<Kernel>(grid, block, lds, st, args...);
    return rc;
}

template <auto Kernel, class... Args>
static int launch_persistent_lds(kh_engine *e, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    const int rc = ensure_dynamic_lds(e, (const void *)Kernel, lds);
    return rc != KH_OK ? rc : launch_persistent<Kernel>(e, grid, block, lds, st, args...);
}

extern "C" const char *kh_last_error(void) { return g_last_error.c_str(); }

// grid <= (resident workgroups per CU of THIS kernel) x CUs ?  (checked once per kernel at engine creation)
static int check_residency(const kh_engine *e, const void *func, int threads, size_t lds, int grid, const char *what) {
    int per_cu = 0;
    KH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, func, threads, lds));
    if ((long long)per_cu * e->num_cus < grid)
        return kh_fail(KH_ERR_UNSUPPORTED, "%s: %d workgroups needed at once, %d x %d CUs resident", what, grid, per_cu,
                       e->num_cus);
    return KH_OK;
}

extern "C" const char *kh_version(void) { return "krotov_hip 0.6 (gfx950; tile64q2, tile64, tile64/stream, tile64x, ens64/mfma, mini16, mini4, replica16/wave, coop16/mfma, ell/csr, ellstream/csr, ellglobal/csr, ellsplit/csr, tile128, generic, generic/csr, generic/mixed, lindblad/matrix kernels)"; }

extern "C" const char *kh_engine_kernel(const kh_engine *e) {
    if (e == nullptr) return "";
    if (e->mixed) return "generic/mixed";
    const KhPlan &p = e->plan;
    if (p.kind == KIND_LIND) return "lindblad/matrix";
    if (p.kind == KIND_REPLICA) return "replica16/wave";
    if (p.ens) return "ens64/mfma";
    switch (p.kind) {
        case KIND_TILE_RPT2: return "tile64/256";
        case KIND_TILE_RPT1: return p.stepwise_only ? (p.stream ? "tile64/stream" : "tile64/512 per interval") : "tile64/512";
        case KIND_TILE_Q2: return p.mini ? (p.quad ? "mini4/wave" : "mini16/wave") : "tile64q2/512";
        case KIND_COOP: return "coop16/mfma";
        case KIND_ELL: return p.ell_global ? (e->row_split > 1 ? "ellsplit/csr" : "ellglobal/csr") : (p.ell_stream ? "ellstream/csr" : "ell/csr");
        case KIND_TILEN: return "tile128/512";
        default: return e->d_csr_fw != nullptr ? "generic/csr" : (p.tx ? "tile64x/512" : "generic");
    }
}

static KhSweepArgs sweep_args(const kh_engine *e, bool backward) {
    KhSweepArgs p;
    p.K = e->K;
    p.N = e->N;
    p.L = e->L;
    p.nt = e->nt;
    p.ops = backward ? e->d_ops_bw : e->d_ops_fw;
    p.csr = backward ? e->d_csr_bw : e->d_csr_fw;
    p.op_norms = e->d_norms;
    p.dt = e->d_dt;
    // equation-of-motion factor (propagators.py:94-99): -i, conj for backwards; 1 for Liouvillians
    if (e->is_super) {
        p.fre = 1.0;
        p.fim = 0.0;
    } else {
        p.fre = 0.0;
        p.fim = backward ? 1.0 : -1.0;
    }
    p.tol = e->tol;
    p.theta_max = e->plan.theta_max;
    p.inv_theta_max = 1.0 / e->plan.theta_max;
    p.deg_theta = e->d_deg_theta;
    p.q2_theta = e->d_q2_theta;
    p.q2_c0 = e->d_q2_c0;
    p.q2_rows = e->d_q2_rows;
    p.q2_odd = 0;
    p.ratios = e->d_ratios;
    p.stats = e->d_stats;
    p.gen_scratch = e->d_gen_scratch;
    p.gen_scratch_wgs = e->gen_scratch_wgs;
    return p;
}

// The arguments of a kh_q2_sweep_store / kh_q2_forward_update launch: the tables that serve odd degrees where the plan
// has them (exactly Hermitian series).  No other kernel is launched with these.
static KhSweepArgs sweep_args_q2(const kh_engine *e, KhSweepArgs p) {
    if (e->plan.q2_odd) {
        p.q2_theta = e->d_q2o_theta;
        p.q2_c0 = e->d_q2o_c0;
        p.q2_rows = e->d_q2o_rows;
        p.q2_odd = 1;
    }
    return p;
}

// The generic kernels' scratch generators (kh_generic.h: dense operators with N > 96): one N x N matrix per workgroup,
// allocated at the first launch that can use it; at most 4 GiB: a launch that asks for more workgroups than that holds
// gets as many scratch matrices as fit (the kernel forms the generator for blockIdx.x < gen_scratch_wgs and streams the
// operators per term in the others), and only a failed allocation leaves the streamed form for good.
static void ensure_gen_scratch(kh_engine *e, int wgs) {
    if (e->d_csr_fw != nullptr || kh_gen_lds_A(e->N, true) || e->gen_scratch_failed) return;
    const size_t per_wg = sizeof(cplx) * (size_t)e->N * e->N;
    const size_t fit = ((size_t)4 << 30) / per_wg;
    if ((size_t)wgs > fit) wgs = (int)fit;
    if (wgs < 1 || e->gen_scratch_wgs >= wgs) return;
    if (e->d_gen_scratch != nullptr) (void)hipFree(e->d_gen_scratch);
    e->d_gen_scratch = nullptr;
    e->gen_scratch_wgs = 0;
    if (hipMalloc(&e->d_gen_scratch, per_wg * (size_t)wgs) != hipSuccess) {
        (void)hipGetLastError();
        e->d_gen_scratch = nullptr;
        e->gen_scratch_failed = true;
        return;
    }
    e->gen_scratch_wgs = wgs;
}

// What a generic kernel is launched with: its grid *grid -- the plain sweeps' workgroups loop over the objectives, no more
// of them than the device runs at once (each may own a scratch generator); the update sweep's are the plan's -- and the
// sweep's arguments with the scratch generators of that many workgroups
static KhSweepArgs gen_sweep_args(kh_engine *e, const KhSweepArgs &p, bool update, int *grid) {
    *grid = update ? e->plan.grid_update : (e->K < 2 * e->num_cus ? e->K : 2 * e->num_cus);
    ensure_gen_scratch(e, *grid);
    KhSweepArgs pg = p;
    pg.gen_scratch = e->d_gen_scratch;
    pg.gen_scratch_wgs = e->gen_scratch_wgs;
    return pg;
}

// The generic kernels' adjoint-side store [L][K][nt][N]: allocated at the first update sweep that can use it, at most
// a quarter of the device memory that is free then (KH_GEN_ADJ=0: never); a store that does not fit leaves the sums on the
// forward side for good.
static bool ensure_gen_adj(kh_engine *e) {
    if (e->d_gen_adj != nullptr) return true;
    if (e->gen_adj_failed) return false;
    if (!e->sw.gen_adj) {
        e->gen_adj_failed = true;
        return false;
    }
    const size_t bytes = sizeof(cplx) * (size_t)e->L * e->K * e->nt * e->N;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 4 || hipMalloc(&e->d_gen_adj, bytes) != hipSuccess) {
        (void)hipGetLastError();
        e->d_gen_adj = nullptr;
        e->gen_adj_failed = true;
        return false;
    }
    return true;
}

extern "C" void kh_engine_destroy(kh_engine *e) {
    if (e == nullptr) return;
    for (void *ptr : e->owned) (void)hipFree(ptr);
    // (allocated lazily or reallocated: not in the owned list)
    (void)hipFree(e->d_gen_scratch);
    (void)hipFree(e->d_gen_adj);
    (void)hipFree(e->d_coop_adj);
    (void)hipFree((void *)e->d_expect_tab);
    (void)hipFree((void *)e->d_grad_ws);
    for (void *ptr : e->p2p_opened) (void)hipIpcCloseMemHandle(ptr);
    (void)hipFree(e->p2p_window);
    (void)hipFree((void *)e->d_p2p_peers);
    delete e;
}

// ---------------------------------------------------------------------------
// sparse operators: host-side analysis and the padded row form of kh_ell.h
// ---------------------------------------------------------------------------
struct HostCsr {  // canonical: column indices sorted within a row, duplicates summed, explicit zeros dropped
    std::vector<int> indptr, indices;
    std::vector<cplx> data;
};

static bool canonical_csr(const int *indptr, const int *indices, const cplx *data, long long nnz, int N, HostCsr &out);

static hipError_t fetch_csr(const kh_csr &c, int N, HostCsr &out) {
    std::vector<int> indptr(N + 1), indices((size_t)c.nnz);
    std::vector<cplx> data((size_t)c.nnz);
    hipError_t err = hipMemcpy(indptr.data(), c.indptr, sizeof(int) * (N + 1), hipMemcpyDeviceToHost);
    if (err == hipSuccess && c.nnz > 0) err = hipMemcpy(indices.data(), c.indices, sizeof(int) * (size_t)c.nnz, hipMemcpyDeviceToHost);
    if (err == hipSuccess && c.nnz > 0) err = hipMemcpy(data.data(), c.data, sizeof(cplx) * (size_t)c.nnz, hipMemcpyDeviceToHost);
    if (err != hipSuccess) return err;
    return canonical_csr(indptr.data(), indices.data(), data.data(), c.nnz, N, out) ? hipSuccess : hipErrorInvalidValue;
}

// host arrays -> canonical form; false on inconsistent arrays
static bool canonical_csr(const int *indptr, const int *indices, const cplx *data, long long nnz, int N, HostCsr &out) {
    out.indptr.assign(N + 1, 0);
    out.indices.clear();
    out.data.clear();
    std::vector<std::pair<int, cplx>> row;
    for (int r = 0; r < N; ++r) {
        row.clear();
        const int lo = indptr[r], hi = indptr[r + 1];
        if (lo < 0 || hi < lo || hi > nnz) return false;
        for (int j = lo; j < hi; ++j) {
            if (indices[j] < 0 || indices[j] >= N) return false;
            row.emplace_back(indices[j], data[j]);
        }
        std::stable_sort(row.begin(), row.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
        for (size_t j = 0; j < row.size();) {
            cplx v = row[j].second;
            size_t q = j + 1;
            for (; q < row.size() && row[q].first == row[j].first; ++q) {
                v.x += row[q].second.x;
                v.y += row[q].second.y;
            }
            if (v.x != 0.0 || v.y != 0.0) {
                out.indices.push_back(row[j].first);
                out.data.push_back(v);
            }
            j = q;
        }
        out.indptr[r + 1] = (int)out.indices.size();
    }
    return true;
}

// does b equal sign * a, entry for entry?
static bool csr_equal(const HostCsr &a, const HostCsr &b, double sign) {
    if (a.indptr != b.indptr || a.indices != b.indices) return false;
    for (size_t j = 0; j < a.data.size(); ++j)
        if (b.data[j].x != sign * a.data[j].x || b.data[j].y != sign * a.data[j].y) return false;
    return true;
}

// || (a + sign adj) / 2 ||_F^2 with adj the conjugate transpose of a, as supplied by the caller
static double csr_part_fro2(const HostCsr &a, const HostCsr &adj, double sign) {
    double acc = 0.0;
    const int N = (int)a.indptr.size() - 1;
    for (int r = 0; r < N; ++r) {
        int i = a.indptr[r], j = adj.indptr[r];
        const int ie = a.indptr[r + 1], je = adj.indptr[r + 1];
        while (i < ie || j < je) {
            double re = 0.0, im = 0.0;
            const int ci = i < ie ? a.indices[i] : INT32_MAX, cj = j < je ? adj.indices[j] : INT32_MAX;
            if (ci <= cj) {
                re += a.data[i].x;
                im += a.data[i].y;
            }
            if (cj <= ci) {
                re += sign * adj.data[j].x;
                im += sign * adj.data[j].y;
            }
            if (ci <= cj) ++i;
            if (cj <= ci) ++j;
            acc += 0.25 * (re * re + im * im);
        }
    }
    return acc;
}

// One operator list (drift + L controls, canonical host copies; NULL: absent) in the padded row form of kh_ell.h:
// the union of the patterns, entries some control touches first.  Returns false when a row is wider than the kernels'
// register budget (kh_ell_emax(N): 32 entries with one row per lane, 16 with two, 8 with three or four).
static bool build_ell_host(const std::vector<const HostCsr *> &ops, int N, std::vector<int> &off, std::vector<cplx> &vals,
                           int &E, int &Ec, bool stream = false, bool any_width = false) {
    const int Lp1 = (int)ops.size();
    std::vector<std::vector<std::pair<int, int>>> rows(N);  // (column, touched by a control)
    E = Ec = 0;
    std::map<int, int> cols;
    for (int r = 0; r < N; ++r) {
        cols.clear();
        for (int o = 0; o < Lp1; ++o) {
            if (ops[o] == nullptr) continue;
            for (int j = ops[o]->indptr[r]; j < ops[o]->indptr[r + 1]; ++j) {
                int &flag = cols[ops[o]->indices[j]];
                if (o > 0) flag = 1;
            }
        }
        int nc = 0;
        for (const auto &kv : cols)
            if (kv.second) rows[r].emplace_back(kv.first, 1), ++nc;
        for (const auto &kv : cols)
            if (!kv.second) rows[r].emplace_back(kv.first, 0);
        E = std::max(E, (int)rows[r].size());
        Ec = std::max(Ec, nc);
    }
    // (stream: the pools of the streamed kernels -- nothing lives in registers, so rows up to 32 entries for any N they take)
    // (any_width: the pools of kh_ellg.h, which loops over a row's entries at run time)
    const int emax = any_width ? INT_MAX - 3 : (stream ? KH_ELL_EMAX : kh_ell_emax(N)), S = stream ? (N + 63) / 64 * 64 : kh_ell_rows(N);
    if (E > emax) return false;
    // every row: its control-touched entries in slots [0, Ec), the others behind them from slot Ec on (so that a rebuild
    // of slots [0, Ec) never touches a drift-only entry); padding: value 0, the lane's own row
    int width = 0;
    for (int r = 0; r < N; ++r) {
        int nc = 0;
        for (const auto &cv : rows[r]) nc += cv.second;
        width = std::max(width, Ec + ((int)rows[r].size() - nc));
    }
    if (width > emax) return false;
    E = (std::max(width, 1) + 3) / 4 * 4;    // the kernels work on groups of four entries
    const int Ec_true = Ec;
    Ec = (Ec + 3) / 4 * 4;                   // (slots [Ec_true, Ec): drift-only entries or padding -- rebuilt to themselves)
    off.assign((size_t)E * S, 0);
    vals.assign((size_t)Lp1 * E * S, make_double2(0.0, 0.0));
    for (int t = 0; t < S; ++t)
        for (int e = 0; e < E; ++e) off[(size_t)e * S + t] = (t < N ? t : 0) * (int)sizeof(cplx);
    auto value_at = [](const HostCsr *m, int r, int c, cplx &v) {
        if (m == nullptr) return false;
        const auto lo = m->indices.begin() + m->indptr[r], hi = m->indices.begin() + m->indptr[r + 1];
        const auto it = std::lower_bound(lo, hi, c);
        if (it == hi || *it != c) return false;
        v = m->data[it - m->indices.begin()];
        return true;
    };
    for (int r = 0; r < N; ++r) {
        int slot_c = 0, slot_d = Ec_true;
        for (const auto &cv : rows[r]) {
            const int slot = cv.second ? slot_c++ : slot_d++;
            off[(size_t)slot * S + r] = cv.first * (int)sizeof(cplx);
            for (int o = 0; o < Lp1; ++o) {
                cplx v;
                if (value_at(ops[o], r, cv.first, v)) vals[((size_t)o * E + slot) * S + r] = v;
            }
        }
    }
    return true;
}

// ---------------------------------------------------------------------------
// kernel families: decided on the host from the problem's facts and the switches (no HIP calls)
// ---------------------------------------------------------------------------
static int max_update_wgs(int num_cus) { return num_cus < 64 * KH_GATHER_CHUNKS ? num_cus : 64 * KH_GATHER_CHUNKS; }

// Ensembles (kh_ens.h): one drift, control operators equal up to a real scale, N <= 64, one control, more objectives
// than CUs (from 257 on it beats the two-workgroups-per-CU tile kernels too: 10.7 against 11.1 us per interval at
// K = 512; one objective per CU: the two-terms-per-phase kernels, 4.8 us per interval against 10.2 there).  The column
// groups where the shape asks for the ensemble detection, else 0.
static int ens_candidate(const KhFacts &f, const KhSwitches &sw) {
    const bool want = sw.ens == 1 || (sw.ens != 0 && !sw.kernel_set && f.K >= sw.ens_min_k);
    if (!want || f.csr || f.N > KH_TILE_N || f.L != 1 || !f.has_h1) return 0;
    const int max_wgs = max_update_wgs(f.num_cus);
    int ncg = 0;
    for (int c = 1; c <= KH_ENS_MAXCG; c *= 2)
        if ((f.K + 2 * c - 1) / (2 * c) <= max_wgs) {
            ncg = c;
            break;
        }
    const int c = sw.ens_ncg;
    if ((c == 1 || c == 2 || c == 4 || c == 8) && (f.K + 2 * c - 1) / (2 * c) <= max_wgs) ncg = c;
    return ncg;
}

// The override order below is the precedence: every family that a later block picks replaces an earlier choice.
static KhPlan plan_families(const KhFacts &f, const KhSwitches &sw) {
    KhPlan p;
    const bool dense = !f.csr, theta_given = f.theta_max > 0.0;
    const bool force = sw.kernel_set, not_generic = !sw.kernel_is("generic");
    const int K = f.K, N = f.N, L = f.L;
    const int max_wgs = max_update_wgs(f.num_cus);
    p.max_wgs = max_wgs;
    p.grid_update = K < max_wgs ? K : max_wgs;
    p.theta_max = theta_given ? f.theta_max : 1.0;
    if (f.lind) {
        // Lindblad form (kh_lind.h): one family for every sweep, one workgroup per objective, objectives in turns beyond
        // the grid; Taylor tables, theta <= 1 per sub-step (a term costs no grid-wide round here)
        p.kind = p.kind_store = KIND_LIND;
        return p;
    }
    p.ell_stream = f.ell_stream;
    p.ell_global = f.ell_global;
    p.ell_E = f.ell_E;
    const bool tile_shape = dense && N <= KH_TILE_N && L >= 1 && L <= 4;
    const bool tile_ok = tile_shape && K <= max_wgs;
    // More objectives than CUs, one control: 256-thread workgroups (one wave per SIMD, 256 VGPRs) fit two per
    // CU, so up to 2 x #CUs objectives stay co-resident -- and the two workgroups of a CU hide each other's
    // phase latency.
    const int max_wgs2 = 2 * f.num_cus < 64 * KH_GATHER_CHUNKS_WIDE ? 2 * f.num_cus : 64 * KH_GATHER_CHUNKS_WIDE;
    const bool tile2_ok = dense && N <= KH_TILE_N && L == 1 && K > max_wgs && K <= max_wgs2;
    if (tile2_ok && not_generic) {
        p.kind = KIND_TILE_RPT2;
        p.grid_update = K;
    }
    // More objectives than can be co-resident (so no in-kernel exchange), tile-sized: the register-tile kernel with
    // ONE LAUNCH PER INTERVAL (the form the sharded sweep uses, kh_update_step) -- every launch re-stages the two
    // operator tiles of its objectives (128 KiB each, from L2 / the Infinity Cache), which still beats the generic
    // kernels' re-streaming of the operators for every term by 5x (K = 1024: 207 -> see DESIGN.md us per interval).
    if (tile_shape && !tile_ok && !tile2_ok && K > max_wgs && sw.stepwise && !force) {
        p.kind = KIND_TILE_RPT1;
        p.grid_update = K;
        p.stepwise_only = true;
        // one workgroup per CU; as few workgroups as give everybody the same number of objectives (K = 384, two controls:
        // 192 x 2 in 23.9 us per interval against 128 x 2 + 128 x 1 in 24.5)
        int G = max_wgs;
        if (K > G) G = (K + (K + G - 1) / G - 1) / ((K + G - 1) / G);
        if (sw.stream_G >= 1 && sw.stream_G <= G) G = sw.stream_G;
        if (G > K) G = K;
        p.stream_G = G;
        p.stream = (long long)G * KH_STREAM_MMAX >= K && sw.stream;
    }
    if (tile_ok && not_generic) {
        // two waves per SIMD are needed to keep the fp64 FMA pipe issuing back to back
        p.kind = L == 1 ? KIND_TILE_Q2 : KIND_TILE_RPT1;  // (one control: two Taylor terms per phase, kh_tile64q2.h)
        if (sw.kernel_is("tile512")) p.kind = KIND_TILE_RPT1;
        if (sw.kernel_is("tile256") && L == 1) p.kind = KIND_TILE_RPT2;  // (two controls: 204 spilled values, never a default choice -- no such instantiation any more)
        p.grid_update = K;
        // small problems: one wave per objective, the objectives of the GPU in one workgroup (kh_mini.h);
        // KH_KERNEL=q2 keeps the workgroup-per-objective kernels, KH_KERNEL=mini is accepted for symmetry
        p.mini = p.kind == KIND_TILE_Q2 && N <= KH_MINI_N && K <= KH_MINI_MAXK && !force;
    }
    if (sw.kernel_is("mini") && tile_ok && L == 1 && N <= KH_MINI_N && K <= KH_MINI_MAXK) {
        p.kind = KIND_TILE_Q2;
        p.grid_update = K;
        p.mini = true;
    }
    p.quad = p.mini && N <= KH_QUAD_N && K <= KH_QUAD_MAXK && !sw.kernel_is("mini");
    // objectives sharing ONE operator list with a state too large for a register tile: one Taylor
    // term of all objectives is a dense (N x N)(N x K) product -> fp64 matrix cores (kh_coop.h)
    {
        // objectives per workgroup: as few as keeps the grid within the co-resident limit (a round is bound by
        // the block fetch, which shrinks with the column count; the MFMA work per workgroup does not grow)
        const int G = (N + 15) / 16;
        int cols = G * ((K + 3) / 4) <= max_wgs ? 4 : KH_COOP_COLS;
        // two objectives per workgroup (half the matrix-core work of a round per workgroup, twice the workgroups)
        // where every column group still gets an XCD of its own (kh_coop_place): up to 8 groups of at most 32
        if (K > 8 && (K + 1) / 2 <= 8 && G <= 32 && G * ((K + 1) / 2) <= max_wgs) cols = 2;
        const int want = sw.coop_cols;
        if ((want == 2 || want == 4 || want == 16) && G * ((K + want - 1) / want) <= max_wgs) cols = want;
        const int Y = (K + cols - 1) / cols;
        const bool fits = dense && f.shared && N <= 480 && L <= KH_COOP_MAX_L && G * Y <= max_wgs;
        if (fits && (sw.kernel_is("coop") || (N > KH_TILE_N && !force))) {
            p.kind = KIND_COOP;
            p.coop_G = G;
            p.coop_Y = Y;
            p.coop_cols = cols;
            p.coop_ks = cols <= 4 ? kh_coop4_slots(N) : (N + 31) / 32;  // operator-fragment slots per lane
            p.coop_xcd = cols <= 4 && Y <= 8 && G <= 32 && sw.coop_xcd;
            p.grid_update = K < max_wgs ? K : max_wgs;  // (stepwise launches use the generic kernel)
            // A round (one Taylor term) costs a cross-workgroup exchange here, so fewer, longer
            // sub-steps pay: theta <= 4 needs ~31 terms per sub-step against 4 x 18 at theta <= 1.
            // Round-off grows like e^theta (55 eps per step at theta = 4), still far inside the
            // parity budget (measured: unchanged 3e-15 vs the oracle on the transmon Liouvillians).
            if (!theta_given) p.theta_max = 4.0;
        }
    }
    // Per-objective operators with 64 < N <= 128: the generator in registers (kh_tilen.h) instead of the generic kernels'
    // re-streaming of every operator for every term.  (Objectives sharing one operator list took the cooperative
    // matrix-core kernels above; KH_KERNEL=tilen forces this family for them too: testing.)
    if (dense && N > KH_TILE_N && N <= KH_TN_NMAX && L >= 1 && L <= KH_MAX_L &&
        ((p.kind == KIND_GENERIC && !force) || sw.kernel_is("tilen"))) {
        p.tilen = true;
        if (sw.kernel_is("tilen")) {
            p.kind = KIND_GENERIC;  // (undo the cooperative choice)
            p.grid_update = K < max_wgs ? K : max_wgs;
            if (!theta_given) p.theta_max = 1.0;
        }
        p.tn_EP = N <= 80 ? 20 : N <= 96 ? 24 : N <= 112 ? 28 : 32;
        p.tn_h1reg = L == 1 && N <= 96 && sw.tn_h1reg && f.all_h1;
        if (K <= max_wgs) {
            p.kind = KIND_TILEN;
            p.grid_update = K;
        }
    }
    // Five to eight controls, N <= 64: the register-tile kernels with the operators beyond the CU's room streamed
    // (kh_tile64x.h) instead of the generic kernels.  The plain sweeps take their objectives in turns (any K); the
    // update sweep needs one resident workgroup per objective, first order and the adjoint-side store (update_route:
    // otherwise the generic kernels, which stay this engine's `kind`).  KH_TX=0: off (A/B switch); KH_KERNEL=tilex: testing
    if (dense && N <= KH_TILE_N && L >= KH_TX_MIN_L && L <= KH_MAX_L && p.kind == KIND_GENERIC &&
        (!force || sw.kernel_is("tilex")) && sw.tx) {
        p.tx = true;
        p.tx_update = K <= max_wgs;
    }
    // Sparse operators in the padded row form: one 1024-thread workgroup per objective, the matrix in registers
    // (kh_ell.h).  The update sweep exchanges the sums in-kernel, so all K workgroups must be resident (one per CU);
    // with more objectives it stays with the generic CSR kernels, the plain sweeps take their objectives in turns.
    const bool near_imag = f.imag_defect >= 0.0 && f.imag_defect <= 0.05;
    const bool ell_cheb = f.ell && (f.real_spectrum || near_imag) && sw.near_imag;
    const double ell_cap = sw.ell_cap > 0.0 && sw.ell_cap < KH_ELL_THETA_CAP ? sw.ell_cap : KH_ELL_THETA_CAP;
    if (f.ell) {
        if (K <= max_wgs) {
            p.kind = KIND_ELL;
            p.grid_update = K;
        }
        // vectors in global memory (kh_ellg.h): a workgroup takes its objectives in turns, so any K runs -- on
        // min(K, #CUs) workgroups, or fewer (kh_set_update_workgroups)
        if (f.ell_global) {
            p.kind = KIND_ELL;
            p.grid_update = K < max_wgs ? K : max_wgs;
        }
        // a term of the series costs a workgroup-wide round whatever it multiplies: fewer, longer sub-steps pay, as
        // for the cooperative kernels (theta <= 4: round-off ~ e^theta eps per step, far inside the parity budget);
        // the long sub-steps only with the Chebyshev form's coefficients, Taylor's at theta <= 4 as before.
        // KH_ELL_CAP (scripts/exp_ell_cap.py): another cap for the Chebyshev-form tables only, never beyond the one
        // they were validated for -- plain Taylor keeps theta <= 4 (its round-off grows like e^theta)
        if (!theta_given) p.theta_max = ell_cheb ? ell_cap : 4.0;
    }
    // The plain sweeps have no cross-objective coupling, so the register-tile kernel serves them for any
    // number of objectives (workgroups simply run in turns) even when the update sweep needs the generic one.
    p.kind_store = f.ell ? KIND_ELL : (p.tilen ? KIND_TILEN : (p.tx ? KIND_TILEX : p.kind));
    if (p.kind == KIND_GENERIC && tile_shape && not_generic) p.kind_store = KIND_TILE_RPT1;
    // ... and with one control that kernel is the two-terms-per-phase one (kh_q2_sweep_store takes its objectives in
    // turns: no co-residency needed), whatever the update sweep has to use: K = 512 on one GPU 7.5 -> 5.8 us per
    // interval of the backward sweep (two turns of the 256-objective sweep instead of the one-term-per-phase kernel
    // with two workgroups per CU).  KH_Q2_STORE=0: the update sweep's own family (A/B switch)
    if ((p.kind_store == KIND_TILE_RPT2 || p.kind_store == KIND_TILE_RPT1) && L == 1 && !force && sw.q2_store)
        p.kind_store = KIND_TILE_Q2;
    // (not for 16 operator slots per lane x 16 objectives per workgroup -- N > 256 with more objectives than 4 per
    // workgroup keep co-resident --: the A^2 chain's second fragment does not fit the registers there, launch_coop_store)
    p.coop_sq = p.kind == KIND_COOP && L == 1 && sw.coop_sq && !(p.coop_cols == 16 && p.coop_ks > 8);
    p.coop_adj = p.coop_sq && f.has_h1 && sw.coop_adj;
    p.stage_sq = p.kind == KIND_TILE_Q2 || p.kind_store == KIND_TILE_Q2 || p.coop_sq;
    // series tables (every kernel family but the cooperative one reads them; the cooperative kernels with the A^2 chain:
    // a term is a cross-workgroup round, so the Chebyshev form is used up to theta = 4 and also for generators that are
    // anti-Hermitian only up to a small defect)
    p.coop_series = p.coop_sq && near_imag;
    p.series_rows = true;
    if (p.coop_series) {
        p.series_cap = 4.0, p.series_defect = f.imag_defect;
    } else if (ell_cheb) {
        // sparse operators in the padded row form: a term costs a workgroup-wide round, so one long sub-step beats
        // several short ones: the Chebyshev form up to theta = 6.  Measured on the reference's three-states problem
        // (scripts/exp_ell_cap.py, theta = 4.4 ... 7.9 per step, 3 iterations x 3 sweeps x 2000 steps): tau within
        // 6e-14 and the pulses within 7e-15 of the same run with theta <= 1 per sub-step, for caps 4, 5, 6 and 8
        // alike; KH_ELL_CAP: A/B switch
        p.series_cap = ell_cap, p.series_defect = f.real_spectrum ? 0.0 : f.imag_defect;
    } else if (f.real_spectrum) {
        p.series_cap = 2.0, p.series_defect = 0.0;
        // the workgroup-per-objective two-terms-per-phase kernels end an odd degree with the A product alone (one
        // product fewer than the next even degree): their launches, and only theirs, get a table with odd degrees.
        // Only for this exactly Hermitian form.  KH_ODD_DEGREES=0: the even-only table for them too (A/B switch)
        p.q2_odd = (p.kind == KIND_TILE_Q2 || p.kind_store == KIND_TILE_Q2) && !p.mini && sw.odd_degrees;
    } else if (f.imag_defect > 0.0 && f.imag_defect <= 0.05 && sw.near_imag) {
        // the same form, with the margin for the Hermitian defect, for the other kernel families (weakly damped
        // Liouvillians, Hamiltonians with a small anti-Hermitian part); KH_NEAR_IMAG=0: Taylor (A/B switch)
        p.series_cap = 2.0, p.series_defect = f.imag_defect;
    } else {
        p.series_rows = false;
    }
    // ensembles: whatever `kind` says, the single-launch update sweep (KH_ENS=0: off; KH_ENS_MINK: smallest K that
    // takes it; KH_ENS_NCG: column groups)
    if (f.ens_ncg > 0) {
        p.ens = true;
        p.ens2 = sw.ens2;
        p.ens_ncg = f.ens_ncg;
        p.ens_G = (K + 2 * f.ens_ncg - 1) / (2 * f.ens_ncg);
    }
    return p;
}

// ---------------------------------------------------------------------------
// engine creation: validate -> gather facts -> plan -> stage what the plan names -> residency demotions
// ---------------------------------------------------------------------------
template <class T>
static int dev_alloc(kh_engine *e, T **ptr, size_t bytes) {
    void *q = nullptr;
    KH_HIP(hipMalloc(&q, bytes));
    e->owned.push_back(q);
    *ptr = (T *)q;
    return KH_OK;
}

template <class T>
static int dev_upload(kh_engine *e, T **ptr, const void *src, size_t bytes) {
    KH_TRY(dev_alloc(e, ptr, bytes));
    KH_HIP(hipMemcpy((void *)*ptr, src, bytes, hipMemcpyHostToDevice));
    return KH_OK;
}

// One device copy per distinct operator (or operator pair): the first request for a key allocates `bytes` and lets
// `fill(dst)` write it; later requests get the same copy.
struct KhCopies {
    std::map<std::pair<const void *, const void *>, cplx *> of;
    template <class Fill>
    int get(kh_engine *e, const void *a, const void *b, size_t bytes, Fill &&fill, const cplx **out) {
        auto it = of.find(std::make_pair(a, b));
        if (it == of.end()) {
            cplx *dst = nullptr;
            int rc = dev_alloc(e, &dst, bytes);
            if (rc == KH_OK) rc = fill(dst);
            if (rc != KH_OK) return rc;
            it = of.emplace(std::make_pair(a, b), dst).first;
        }
        *out = it->second;
        return KH_OK;
    }
};

// the device table [tab.size()] of one copy per distinct operator of `tab` (`absent` where tab has none)
template <class Fill>
static int stage_copies(kh_engine *e, KhCopies &copies, const std::vector<const cplx *> &tab, size_t bytes,
                        const cplx *absent, Fill &&fill, const cplx ***slot) {
    std::vector<const cplx *> out(tab.size(), absent);
    for (size_t i = 0; i < tab.size(); ++i) {
        if (tab[i] == nullptr) continue;
        const int rc = copies.get(e, tab[i], nullptr, bytes, [&](cplx *dst) { return fill(tab[i], dst); }, &out[i]);
        if (rc != KH_OK) return rc;
    }
    KH_HIP(hipGetLastError());
    return dev_upload(e, slot, out.data(), sizeof(cplx *) * out.size());
}

// Operator tables: forward pointers as given, adjoints staged once per distinct operator (dense) or as the caller
// supplies them (CSR); norms, degree table, time steps.  dims: [K] each objective's own dimension (mixed engines:
// its operators are dims[k] x dims[k]), or NULL: every operator is N x N.
static int stage_operators(kh_engine *e, const kh_problem *pr, const kh_csr *csr_fw, const kh_csr *csr_bw,
                           std::vector<const cplx *> &fw, std::vector<const cplx *> &bw, const int32_t *dims = nullptr) {
    const size_t nops = (size_t)e->K * (1 + e->L);
    fw.assign(nops, nullptr);
    bw.assign(nops, nullptr);
    KhCopies adj;
    for (size_t i = 0; i < nops; ++i) {
        const cplx *src = (const cplx *)pr->ops[i];
        fw[i] = src;
        if (src == nullptr) continue;
        if (csr_fw != nullptr) {  // the caller supplies the conjugate transposes
            bw[i] = (const cplx *)csr_bw[i].data;
            continue;
        }
        const int n = dims != nullptr ? dims[i / (size_t)(1 + e->L)] : e->N;
        const int tiles = (n + 31) / 32;
        const int rc = adj.get(e, src, nullptr, sizeof(cplx) * (size_t)n * n, [&](cplx *dst) {
            kh_adjoint_kernel<<<dim3(tiles, tiles), 256>>>(src, dst, n);
            return KH_OK;
        }, &bw[i]);
        if (rc != KH_OK) return rc;
    }
    KH_HIP(hipGetLastError());
    KH_TRY(dev_upload(e, &e->d_ops_fw, fw.data(), sizeof(cplx *) * nops));
    KH_TRY(dev_upload(e, &e->d_ops_bw, bw.data(), sizeof(cplx *) * nops));
    if (csr_fw != nullptr) {
        static_assert(sizeof(KhCsr) == sizeof(kh_csr), "kh_csr layout");
        KH_TRY(dev_upload(e, &e->d_csr_fw, csr_fw, sizeof(KhCsr) * nops));
        KH_TRY(dev_upload(e, &e->d_csr_bw, csr_bw, sizeof(KhCsr) * nops));
    }
    if (pr->op_norms != nullptr) {
        KH_TRY(dev_upload(e, &e->d_norms, pr->op_norms, sizeof(double) * nops));
    } else {
        KH_TRY(dev_alloc(e, &e->d_norms, sizeof(double) * nops));
        if (dims == nullptr) {
            kh_fro_norms<<<(unsigned)nops, 256>>>(e->d_ops_fw, (int)nops, e->N, e->d_norms);
        } else {
            const size_t Lp1 = 1 + e->L;
            for (int k = 0; k < e->K; ++k)
                kh_fro_norms<<<(unsigned)Lp1, 256>>>(e->d_ops_fw + k * Lp1, (int)Lp1, dims[k], e->d_norms + k * Lp1);
        }
        KH_HIP(hipGetLastError());
    }
    double tab[KH_MAX_DEGREE + 1];
    kh_build_degree_table(e->tol, tab);
    KH_TRY(dev_upload(e, &e->d_deg_theta, tab, sizeof(tab)));
    return dev_upload(e, &e->d_dt, pr->dt, sizeof(double) * (e->nt - 1));
}

// `launch(d)` on a zeroed device buffer of `bytes`, copied back to `out` (the set-up kernels that answer a question)
template <class Launch>
static int device_probe(void *out, size_t bytes, Launch &&launch) {
    void *d = nullptr;
    KH_HIP(hipMalloc(&d, bytes));
    hipError_t err = hipMemset(d, 0, bytes);
    if (err == hipSuccess) {
        launch(d);
        err = hipGetLastError();  // (the launch's own verdict, not whatever the copy below reports)
    }
    if (err == hipSuccess) err = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    KH_HIP(err);
    return KH_OK;
}

// What the detection found -> adj_sign, real spectrum, Hermitian defect.  ctl_plus / ctl_minus: every control operator
// equals +/- its adjoint, bit for bit; drift_plus: the drift equals its adjoint; fro2(v): || Hermitian part of the
// drift ||_F^2, asked only where the controls qualify.  Every generator Hermitian and f = -+i: real spectrum (the
// shorter series of kh_common.h); f A anti-Hermitian up to a small Hermitian part of the drift (a weakly damped
// Liouvillian; a Hamiltonian with a small anti-Hermitian part): the same series with a margin.
template <class Fro2>
static int classify_operators(const kh_engine *e, const kh_problem *pr, bool ctl_plus, bool ctl_minus, bool drift_plus,
                              Fro2 &&fro2, KhFacts &f) {
    f.adj_sign = ctl_plus ? 1.0 : (ctl_minus ? -1.0 : 0.0);
    f.real_spectrum = ctl_plus && drift_plus && !e->is_super;
    if (e->is_super ? ctl_minus : ctl_plus) {
        double v = 0.0, dt_max = 0.0;
        KH_TRY(fro2(v));
        for (int n = 0; n < e->nt - 1; ++n) dt_max = pr->dt[n] > dt_max ? pr->dt[n] : dt_max;
        f.imag_defect = sqrt(v) * dt_max;
    }
    return KH_OK;
}

// dense operators: the device-side detection kernels
static int detect_dense(kh_engine *e, const kh_problem *pr, KhFacts &f) {
    const int nops = e->K * (1 + e->L);
    int flags[3] = {1, 1, 1};
    KH_TRY(device_probe(flags, sizeof(flags), [&](void *d) {
        kh_adjoint_sign_kernel<<<(unsigned)(nops < 1024 ? nops : 1024), 256>>>(e->d_ops_fw, e->d_ops_bw, nops, 1 + e->L, e->N, (int *)d);
    }));
    return classify_operators(e, pr, flags[0] == 0, flags[1] == 0, flags[2] == 0, [&](double &v) {
        return device_probe(&v, sizeof(v), [&](void *d) {
            kh_herm_defect_kernel<<<(unsigned)(e->K < 1024 ? e->K : 1024), 256>>>(e->d_ops_fw, e->d_ops_bw, nops, 1 + e->L, e->N,
                                                                                  e->is_super ? 1.0 : -1.0, (unsigned long long *)d);
        });
    }, f);
}

// Sparse operators: the same questions asked of canonical host copies, and the padded row form (kh_ell.h), one structure
// per distinct operator list and direction: the matrix in registers where the rows fit (N <= 2048), else -- or with
// KH_KERNEL=ellstream -- the streamed form (N <= 4096, rows up to 32 entries): the same pools with their own row count,
// read per term.  Where neither applies and the generic kernels cannot hold N either (N > 4096, or N > 2540 with a row
// wider than 32) -- or with KH_KERNEL=ellglobal / ellsplit -- the streamed form's pools with rows of any width and every vector in
// global memory (kh_ellg.h, N <= 2^20).
static int build_sparse(kh_engine *e, const kh_problem *pr, const kh_csr *csr_fw, const kh_csr *csr_bw,
                        const std::vector<const cplx *> &fw, KhFacts &f) {
    const size_t nops = fw.size();
    // canonical host copies of every distinct operator and of its conjugate transpose (small: a few entries per row)
    std::map<const void *, HostCsr> host_fw, host_bw;
    for (size_t i = 0; i < nops; ++i) {
        if (fw[i] == nullptr || host_fw.count(fw[i])) continue;
        KH_HIP(fetch_csr(csr_fw[i], e->N, host_fw[fw[i]]));
        KH_HIP(fetch_csr(csr_bw[i], e->N, host_bw[fw[i]]));
    }
    if (e->L >= 1) {
        bool ctl_plus = true, ctl_minus = true, drift_plus = true;
        double fro2 = 0.0;
        for (size_t i = 0; i < nops; ++i) {
            if (fw[i] == nullptr) continue;
            const HostCsr &a = host_fw[fw[i]], &b = host_bw[fw[i]];
            if (i % (size_t)(1 + e->L) == 0) {
                drift_plus = drift_plus && csr_equal(a, b, 1.0);
                fro2 = std::max(fro2, csr_part_fro2(a, b, e->is_super ? 1.0 : -1.0));
            } else {
                ctl_plus = ctl_plus && csr_equal(a, b, 1.0);
                ctl_minus = ctl_minus && csr_equal(a, b, -1.0);
            }
        }
        KH_TRY(classify_operators(e, pr, ctl_plus, ctl_minus, drift_plus, [&](double &v) { return v = fro2, KH_OK; }, f));
    }
    const bool want_stream = e->sw.kernel_is("ellstream"), want_global = e->sw.kernel_is("ellglobal") || e->sw.kernel_is("ellsplit");
    for (int form = want_global ? 2 : (want_stream ? 1 : 0); form < 3 && !f.ell; ++form) {
        const bool global = form == 2, stream = form >= 1;
        if (e->N > (global ? KH_ELLG_NMAX : (stream ? KH_ELLS_NMAX : KH_ELL_NMAX)) || e->L > KH_MAX_L || e->sw.kernel_is("generic")) continue;
        if (form == 1 && !e->sw.ellstream) continue;
        if (global && !want_global && e->gen_fits) continue;  // (only where nothing else runs: every other dispatch keeps its family)
        bool ok = true;
        int E_max = 0, ec_max = 0;
        std::map<std::vector<const void *>, std::pair<KhEll, KhEll>> made;
        std::vector<KhEll> ell_fw(e->K), ell_bw(e->K);
        std::vector<int> off_pool;
        std::vector<cplx> vals_pool;
        for (int k = 0; k < e->K && ok; ++k) {
            std::vector<const void *> key(fw.begin() + (size_t)k * (1 + e->L), fw.begin() + (size_t)(k + 1) * (1 + e->L));
            auto it = made.find(key);
            if (it == made.end()) {
                KhEll pair[2];
                for (int dir = 0; dir < 2 && ok; ++dir) {
                    std::vector<const HostCsr *> ops_h;
                    for (const void *ptr : key)
                        ops_h.push_back(ptr == nullptr ? nullptr : (dir == 0 ? &host_fw[ptr] : &host_bw[ptr]));
                    std::vector<int> off;
                    std::vector<cplx> vals;
                    int E = 0, Ec = 0;
                    ok = build_ell_host(ops_h, e->N, off, vals, E, Ec, stream, global);
                    if (!ok) break;
                    ec_max = std::max(ec_max, Ec);
                    pair[dir].off_at = (long long)off_pool.size();
                    pair[dir].vals_at = (long long)vals_pool.size();
                    off_pool.insert(off_pool.end(), off.begin(), off.end());
                    vals_pool.insert(vals_pool.end(), vals.begin(), vals.end());
                    pair[dir].E = E;
                    pair[dir].Ec = Ec;
                    pair[dir].rows = stream ? (e->N + 63) / 64 * 64 : kh_ell_rows(e->N);
                    pair[dir].pad_ = 0;
                    E_max = std::max(E_max, E);
                }
                if (!ok) break;
                it = made.emplace(key, std::make_pair(pair[0], pair[1])).first;
            }
            ell_fw[k] = it->second.first;
            ell_bw[k] = it->second.second;
        }
        if (!ok) continue;
        f.ell = true;
        f.ell_stream = stream;
        f.ell_global = global;
        f.ell_E = E_max;
        KH_TRY(dev_upload(e, &e->d_ell_off, off_pool.data(), sizeof(int) * off_pool.size()));
        KH_TRY(dev_upload(e, &e->d_ell_vals, vals_pool.data(), sizeof(cplx) * vals_pool.size()));
        KH_TRY(dev_upload(e, &e->d_ell_fw, ell_fw.data(), sizeof(KhEll) * e->K));
        KH_TRY(dev_upload(e, &e->d_ell_bw, ell_bw.data(), sizeof(KhEll) * e->K));
        if (global) {
            // one workspace per workgroup, here and not at the first launch: the plain sweeps and the update sweep run on
            // at most min(K, #CUs) workgroups
            e->ellg_ws_stride = kh_ellg_ws_stride(e->N, ec_max);
            e->ellg_wgs = e->K < e->num_cus ? e->K : e->num_cus;
            KH_TRY(dev_alloc(e, &e->d_ellg_ws, sizeof(cplx) * (size_t)e->ellg_ws_stride * e->ellg_wgs));
        } else if (stream) {
            // one scratch plane per workgroup (update sweep: K of them; plain sweeps: at most one per CU)
            e->ell_scratch_stride = (long long)std::max(ec_max, 4) * ((e->N + 63) / 64 * 64);
            const int wgs = e->K < e->num_cus ? e->K : e->num_cus;  // (the update sweep takes K <= #CUs workgroups, the plain sweeps at most #CUs)
            KH_TRY(dev_alloc(e, &e->d_ell_scratch, sizeof(cplx) * (size_t)e->ell_scratch_stride * wgs));
        }
    }
    return KH_OK;
}

// Ensembles: is every objective's operator list (H0, s_k H1) with objective 0's H0 and H1?  (kh_ens_detect_kernel;
// the scales s_k stay in d_ens_scale)
static int detect_ensemble(kh_engine *e, const std::vector<const cplx *> &fw, bool &found) {
    found = false;
    // reference element: the largest component of objective 0's control operator
    std::vector<cplx> ref((size_t)e->N * e->N);
    KH_HIP(hipMemcpy(ref.data(), fw[1], sizeof(cplx) * ref.size(), hipMemcpyDeviceToHost));
    int ref_idx = 0, ref_comp = 0;
    double best = 0.0;
    for (size_t i = 0; i < ref.size(); ++i) {
        if (fabs(ref[i].x) > best) best = fabs(ref[i].x), ref_idx = (int)i, ref_comp = 0;
        if (fabs(ref[i].y) > best) best = fabs(ref[i].y), ref_idx = (int)i, ref_comp = 1;
    }
    if (!(best > 0.0)) return KH_OK;
    KH_TRY(dev_alloc(e, &e->d_ens_scale, sizeof(double) * e->K));
    int flags[2] = {1, 1};
    KH_TRY(device_probe(flags, sizeof(flags), [&](void *d) {
        kh_ens_detect_kernel<<<e->K, 256>>>(e->d_ops_fw, e->K, e->N, ref_idx, ref_comp, e->d_ens_scale, (int *)d);
    }));
    found = flags[0] == 0 && flags[1] == 0;
    return KH_OK;
}

// P0 = H0 H0, P1 = H0 H1 + H1 H0, P2 = H1 H1 once per distinct operator (pair), per direction -> d_sq_fw / d_sq_bw
// (sq: the same tables on the host)
static int stage_squares(kh_engine *e, const std::vector<const cplx *> &fw, const std::vector<const cplx *> &bw,
                         std::vector<const cplx *> sq[2]) {
    const unsigned pgrid = (unsigned)(((size_t)e->N * e->N + 255) / 256 < 16 ? 16 : ((size_t)e->N * e->N + 255) / 256);
    const size_t bytes = sizeof(cplx) * (size_t)e->N * e->N;
    for (int dir = 0; dir < 2; ++dir) {
        const std::vector<const cplx *> &tab = dir == 0 ? fw : bw;
        sq[dir].assign((size_t)e->K * 3, nullptr);
        KhCopies p0, p1, p2;
        for (int k = 0; k < e->K; ++k) {
            const cplx *H0 = tab[(size_t)k * 2], *H1 = tab[(size_t)k * 2 + 1];
            auto product = [&](const cplx *X, const cplx *Y, int sym) {
                return [=](cplx *dst) {
                    kh_q2_product<<<pgrid, 256>>>(X, Y, dst, e->N, sym);
                    return KH_OK;
                };
            };
            KH_TRY(p0.get(e, H0, nullptr, bytes, product(H0, H0, 0), &sq[dir][(size_t)k * 3]));
            if (H1 == nullptr) continue;
            KH_TRY(p2.get(e, H1, nullptr, bytes, product(H1, H1, 0), &sq[dir][(size_t)k * 3 + 2]));
            KH_TRY(p1.get(e, H0, H1, bytes, product(H0, H1, 1), &sq[dir][(size_t)k * 3 + 1]));
        }
        KH_HIP(hipGetLastError());
        KH_TRY(dev_upload(e, dir == 0 ? &e->d_sq_fw : &e->d_sq_bw, sq[dir].data(), sizeof(cplx *) * sq[dir].size()));
    }
    return KH_OK;
}

// The cooperative kernels (kh_coop.h): exchange buffers, fragment-ordered copies of the (shared) operators and, for one
// control, of P0, P1, P2; the non-zero blocks of H_1^+ for the adjoint-side sums
static int stage_coop(kh_engine *e, const std::vector<const cplx *> &fw, const std::vector<const cplx *> &bw,
                      const std::vector<const cplx *> sq[2]) {
    const KhPlan &p = e->plan;
    e->coop_vbuf_bytes = sizeof(kh_u64) * KH_COOP_RING * (size_t)p.coop_Y * p.coop_G * 16 * KH_COOP_COLS * 4;
    KH_TRY(dev_alloc(e, &e->d_coop_vbuf, e->coop_vbuf_bytes));
    KH_TRY(dev_alloc(e, &e->d_coop_xcc, sizeof(unsigned int) * (size_t)p.coop_G * p.coop_Y));
    const size_t elems = kh_coop_table_elems(p.coop_G, p.coop_ks);  // (row blocks padded apart: kh_coop_table_stride)
    const size_t frag_elems = (size_t)p.coop_G * KH_COOP_WAVES * p.coop_ks * 64;
    // (+ one zero-slot word per (row block, wave) behind the table: kh_coop_mask_kernel)
    const size_t bytes = sizeof(cplx) * elems + sizeof(unsigned int) * p.coop_G * KH_COOP_WAVES;
    auto permute = [&](const cplx *src, cplx *dst) -> int {
        KH_HIP(hipMemset(dst, 0, sizeof(cplx) * elems));
        kh_coop_permute_kernel<<<(unsigned)((frag_elems + 255) / 256), 256>>>(src, dst, e->N, p.coop_G, p.coop_ks, p.coop_cols);
        kh_coop_mask_kernel<<<p.coop_G * KH_COOP_WAVES, 64>>>(dst, (unsigned int *)(dst + elems), p.coop_ks);
        return KH_OK;
    };
    KhCopies copies;
    for (int dir = 0; dir < 2; ++dir) {
        const std::vector<const cplx *> ops((dir == 0 ? fw : bw).begin(), (dir == 0 ? fw : bw).begin() + 1 + e->L);
        KH_TRY(stage_copies(e, copies, ops, bytes, nullptr, permute, dir == 0 ? &e->d_coop_fops_fw : &e->d_coop_fops_bw));
        if (p.coop_sq) {
            const std::vector<const cplx *> sq3(sq[dir].begin(), sq[dir].begin() + 3);
            KH_TRY(stage_copies(e, copies, sq3, bytes, nullptr, permute, dir == 0 ? &e->d_coop_sq_fw : &e->d_coop_sq_bw));
        }
    }
    if (p.coop_adj) {
        e->coop_adj_op = bw[1];
        KH_TRY(dev_alloc(e, &e->d_coop_adj_nz, (size_t)p.coop_G * p.coop_G));
        kh_coop_adj_mask_kernel<<<p.coop_G * p.coop_G, 256>>>(bw[1], e->N, p.coop_G, e->d_coop_adj_nz);
        KH_HIP(hipGetLastError());
    }
    return KH_OK;
}

// the series tables of the plan (every kernel family but the cooperative one reads them; that one where coop_series)
static int stage_series(kh_engine *e) {
    std::vector<double> tab(KH_MAX_DEGREE + 1), c0(KH_MAX_DEGREE + 1), rows((size_t)(KH_MAX_DEGREE + 1) * KH_Q2_ROWS * 2),
        ratios((size_t)(KH_MAX_DEGREE + 1) * KH_RATIO_STRIDE);
    if (e->plan.q2_odd) {  // (before the even-only tables: the vectors are reused)
        kh_build_real_spectrum_rows(e->tol, tab.data(), c0.data(), rows.data(), ratios.data(), e->plan.series_cap, 0.0, true);
        KH_TRY(dev_upload(e, &e->d_q2o_theta, tab.data(), sizeof(double) * tab.size()));
        KH_TRY(dev_upload(e, &e->d_q2o_c0, c0.data(), sizeof(double) * c0.size()));
        KH_TRY(dev_upload(e, &e->d_q2o_rows, rows.data(), sizeof(double) * rows.size()));
    }
    if (e->plan.series_rows) {
        kh_build_real_spectrum_rows(e->tol, tab.data(), c0.data(), rows.data(), ratios.data(), e->plan.series_cap,
                                    e->plan.series_defect);
    } else {
        kh_build_degree_table(e->tol, tab.data());
        kh_build_taylor_rows(c0.data(), rows.data(), ratios.data());
    }
    KH_TRY(dev_upload(e, &e->d_ratios, ratios.data(), sizeof(double) * ratios.size()));
    KH_TRY(dev_upload(e, &e->d_q2_theta, tab.data(), sizeof(double) * tab.size()));
    KH_TRY(dev_upload(e, &e->d_q2_c0, c0.data(), sizeof(double) * c0.size()));
    return dev_upload(e, &e->d_q2_rows, rows.data(), sizeof(double) * rows.size());
}

template <class F>
static auto with_ens(int ncg, F &&f) {
    switch (ncg) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return f(std::integral_constant<int, 8>{});
    }
}

// the two instantiations of the ensemble kernel with `ncg` column groups (first / second order), their LDS limit raised
static int ens_forms(kh_engine *e, int ncg, const void *forms[2]) {
    with_ens(ncg, [&](auto c) {
        forms[0] = (const void *)kh_ens_forward_update<decltype(c)::value, false>;
        forms[1] = (const void *)kh_ens_forward_update<decltype(c)::value, true>;
        return 0;
    });
    for (int i = 0; i < 2; ++i) {
        KH_TRY(ensure_dynamic_lds(e, forms[i], kh_ens_lds_bytes(ncg)));
    }
    return KH_OK;
}

static int stage_workspaces(kh_engine *e);
static int kh_row_split_auto(int num_cus, int K, int N);

// Everything but the validation of engine_create; on failure the caller destroys the half-built engine.
static int engine_build(kh_engine *e, const kh_problem *pr, const kh_csr *csr_fw, const kh_csr *csr_bw) {
    KH_HIP(hipGetDevice(&e->device));
    hipDeviceProp_t prop;
    KH_HIP(hipGetDeviceProperties(&prop, e->device));
    e->num_cus = prop.multiProcessorCount;
    // the generic kernels -- every engine's last resort -- keep four vectors of N elements in LDS: N <= 2540.  Sparse
    // operators may still run the padded-row kernels -- streamed up to N = 4096, with their vectors in global memory up to
    // N = 2^20 -- (gen_fits stays false then and whatever would need the generic kernels -- one launch per interval -- is
    // refused)
    const size_t gen_lds = kh_gen_lds_bytes(e->N, csr_fw == nullptr);
    e->gen_fits = !(gen_lds > (size_t)prop.sharedMemPerBlock && gen_lds > 160 * 1024);
    if (!e->gen_fits && !(csr_fw != nullptr && e->N <= KH_ELLG_NMAX))
        return kh_fail(KH_ERR_UNSUPPORTED, "N=%d needs %zu bytes of LDS", e->N, gen_lds);

    // ---- facts
    std::vector<const cplx *> fw, bw;
    KH_TRY(stage_operators(e, pr, csr_fw, csr_bw, fw, bw));
    KhFacts f;
    f.K = e->K, f.N = e->N, f.L = e->L, f.num_cus = e->num_cus;
    f.csr = csr_fw != nullptr;
    f.theta_max = pr->theta_max;
    f.shared = true;
    for (size_t i = 0; i < fw.size() && f.shared; ++i) f.shared = fw[i] == fw[i % (size_t)(1 + e->L)];
    f.has_h1 = e->L >= 1 && fw[1] != nullptr;
    f.all_h1 = e->L >= 1;
    for (int k = 0; k < e->K && f.all_h1; ++k) f.all_h1 = fw[(size_t)k * (1 + e->L) + 1] != nullptr;
    if (e->L >= 1) {
        KH_TRY(csr_fw == nullptr ? detect_dense(e, pr, f) : build_sparse(e, pr, csr_fw, csr_bw, fw, f));
        if (e->sw.taylor) f.real_spectrum = false, f.imag_defect = -1.0;  // A/B switch: plain Taylor coefficients everywhere
        if (e->sw.no_adj && csr_fw == nullptr) f.adj_sign = 0.0;        // A/B switch: keep <chi|H phi> on the forward side
    } else if (csr_fw != nullptr) {
        KH_TRY(build_sparse(e, pr, csr_fw, csr_bw, fw, f));
    }
    if (!e->gen_fits && !f.ell)
        return kh_fail(KH_ERR_UNSUPPORTED, "N=%d: no padded-row form for this problem (more than %d controls, or KH_KERNEL) and no room for the generic kernels' vectors in LDS", e->N, KH_MAX_L);
    if (const int ncg = ens_candidate(f, e->sw)) {
        bool found = false;
        KH_TRY(detect_ensemble(e, fw, found));
        if (found) f.ens_ncg = ncg;
    }
    e->adj_sign = f.adj_sign;

    // ---- plan, and what it names
    e->plan = plan_families(f, e->sw);
    KhPlan &p = e->plan;
    if (p.tilen) {
        auto permute = [&](const cplx *src, cplx *dst) {
            kh_tn_permute<<<KH_TN_NMAX / 4, KH_TN_THREADS>>>(src, dst, e->N);
            return KH_OK;
        };
        const size_t bytes = sizeof(cplx) * (KH_TN_NMAX / 4) * KH_TN_THREADS;
        KhCopies copies;  // (one per distinct operator over both directions)
        KH_TRY(stage_copies(e, copies, fw, bytes, nullptr, permute, &e->d_tn_fw));
        KH_TRY(stage_copies(e, copies, bw, bytes, nullptr, permute, &e->d_tn_bw));
    }
    if (p.tx) {
        auto permute = [&](const cplx *src, cplx *dst) {
            kh_tx_permute<<<8, KH_TX_THREADS>>>(src, dst, e->N);
            return KH_OK;
        };
        const size_t bytes = sizeof(cplx) * 8 * KH_TX_THREADS;
        cplx *zero_tile = nullptr;  // stands in for a control an objective does not have (no branches in the kernels' loads)
        KH_TRY(dev_alloc(e, &zero_tile, bytes));
        KH_HIP(hipMemset(zero_tile, 0, bytes));
        KhCopies copies;
        KH_TRY(stage_copies(e, copies, fw, bytes, zero_tile, permute, &e->d_tx_fw));
        KH_TRY(stage_copies(e, copies, bw, bytes, zero_tile, permute, &e->d_tx_bw));
    }
    std::vector<const cplx *> sq[2];
    if (p.stage_sq) KH_TRY(stage_squares(e, fw, bw, sq));
    if (p.kind == KIND_COOP) KH_TRY(stage_coop(e, fw, bw, sq));
    KH_TRY(stage_series(e));
    if (p.kind_store == KIND_TILE_Q2)
        KH_HIP(hipFuncSetAttribute((const void *)kh_q2_sweep_store, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kh_q2_lds_bytes()));
    if (p.kind == KIND_TILE_Q2) {
        // every instantiation a sweep of this engine may launch: one GPU / sharded, first / second order, sums on
        // either side -- their register footprints differ
        const void *forms[] = {(const void *)kh_q2_forward_update<false, true, true>, (const void *)kh_q2_forward_update<false, false, true>,
                               (const void *)kh_q2_forward_update<true, false, true>, (const void *)kh_q2_forward_update<false, true>,
                               (const void *)kh_q2_forward_update<false, false>,      (const void *)kh_q2_forward_update<true, false>};
        for (const void *fn : forms)
            KH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kh_q2_lds_bytes()));
        // every workgroup of the single-launch update sweep must be resident at once: ask the occupancy of the kernel
        // as built (registers, LDS) instead of assuming one per CU; if it does not fit, the generic kernels (which
        // loop over objectives inside at most #CUs workgroups) take over
        int rc = KH_OK;
        if (!p.mini && e->K > 1)
            for (const void *fn : forms)
                if (rc == KH_OK) rc = check_residency(e, fn, KH_Q2_THREADS, kh_q2_lds_bytes(), e->K, "kh_q2_forward_update");
        if (rc != KH_OK) {
            p.kind = KIND_GENERIC;  // (the plain sweeps keep the q2 kernel: its workgroups do not wait for each other)
            p.grid_update = e->K < p.max_wgs ? e->K : p.max_wgs;
        }
    }
    if (p.ens) {  // all ens_G workgroups resident at once?  (as the q2 path asks for its instantiations)
        e->ens_H0 = fw[0];
        e->ens_H1 = fw[1];
        const void *forms[2];
        int rc = ens_forms(e, p.ens_ncg, forms);
        for (const void *fn : forms)
            if (rc == KH_OK) rc = check_residency(e, fn, KH_ENS_THREADS, kh_ens_lds_bytes(p.ens_ncg), p.ens_G, "kh_ens_forward_update");
        if (rc != KH_OK) p.ens = false;
    }

    return stage_workspaces(e);
}

// the sweeps' workspaces (the plan's grids)
static int stage_workspaces(kh_engine *e) {
    const KhPlan &p = e->plan;
    const int Lx = e->L > 0 ? e->L : 1;
    const int slot_wgs = p.kind == KIND_COOP && p.coop_G * p.coop_Y > p.grid_update ? p.coop_G * p.coop_Y : p.grid_update;
    e->slots_bytes = sizeof(kh_u64) * 2 * (size_t)slot_wgs * Lx * 2;
    KH_TRY(dev_alloc(e, &e->d_phi, sizeof(cplx) * (size_t)e->K * e->N));
    KH_TRY(dev_alloc(e, &e->d_slots, e->slots_bytes));
    KH_TRY(dev_alloc(e, &e->d_abort, 2 * sizeof(unsigned int)));  // [0] abort flag, [1] (KH_TIMING) polling rounds
    KH_TRY(dev_alloc(e, &e->d_wait_ticks, 4 * sizeof(unsigned long long)));
    KH_TRY(dev_alloc(e, &e->d_stats, sizeof(double) * 68));
    KH_TRY(dev_alloc(e, &e->d_wg_partial, sizeof(double) * (size_t)p.grid_update * Lx));
    KH_TRY(dev_alloc(e, &e->d_step_partial, sizeof(double) * Lx));
    KH_HIP(hipMemset(e->d_abort, 0, 2 * sizeof(unsigned int)));
    KH_HIP(hipMemset(e->d_wait_ticks, 0, 4 * sizeof(unsigned long long)));
    KH_HIP(hipMemset(e->d_stats, 0, sizeof(double) * 68));
    KH_HIP(hipDeviceSynchronize());
    return KH_OK;
}

// csr_fw / csr_bw: [K*(1+L)] sparse operators and their conjugate transposes (pr->ops then holds their
// data arrays), or both NULL for dense row-major operators
static int validate_problem(const kh_problem *pr) {
    if (pr->K < 1 || pr->N < 1 || pr->L < 0 || pr->nt < 2)
        return kh_fail(KH_ERR_INVALID, "bad sizes K=%d N=%d L=%d nt=%d", pr->K, pr->N, pr->L, pr->nt);
    // (the register-resident families take up to KH_MAX_L controls; with more the generic kernels run, up to KH_GEN_MAX_L)
    if (pr->L > KH_GEN_MAX_L) return kh_fail(KH_ERR_UNSUPPORTED, "L=%d controls > %d", pr->L, KH_GEN_MAX_L);
    if (pr->dt == nullptr || pr->ops == nullptr) return kh_fail(KH_ERR_INVALID, "dt/ops missing");
    for (int n = 0; n < pr->nt - 1; ++n)
        if (!(pr->dt[n] > 0.0)) return kh_fail(KH_ERR_INVALID, "dt[%d] = %g is not positive", n, pr->dt[n]);
    for (int k = 0; k < pr->K; ++k)
        if (pr->ops[(size_t)k * (1 + pr->L)] == nullptr)
            return kh_fail(KH_ERR_INVALID, "objective %d has no drift operator", k);
    return KH_OK;
}

static int engine_create(const kh_problem *pr, const kh_csr *csr_fw, const kh_csr *csr_bw, kh_engine **out) {
    if (pr == nullptr || out == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    *out = nullptr;
    KH_TRY(validate_problem(pr));

    kh_engine *e = new kh_engine();
    e->K = pr->K;
    e->N = pr->N;
    e->L = pr->L;
    e->nt = pr->nt;
    e->is_super = pr->is_super ? 1 : 0;
    e->tol = pr->tol > 0.0 ? pr->tol : ldexp(1.0, -53);
    e->sw = read_switches();
    int rc = engine_build(e, pr, csr_fw, csr_bw);
    // KH_KERNEL=ellsplit: the global form (forced above) on KH_ELL_SPLIT workgroups per objective, or 'auto'
    if (rc == KH_OK && e->sw.kernel_is("ellsplit") && e->plan.kind == KIND_ELL && e->plan.ell_global) {
        const int S = e->sw.ell_split != 0 ? e->sw.ell_split : kh_row_split_auto(e->num_cus, e->K, e->N);
        if (S != 1) rc = kh_set_row_split(e, S);
    }
    if (rc != KH_OK) {
        kh_engine_destroy(e);
        return rc;
    }
    *out = e;
    return KH_OK;
}

extern "C" int kh_engine_create(const kh_problem *pr, kh_engine **out) {
    return engine_create(pr, nullptr, nullptr, out);
}

extern "C" int kh_engine_create_csr(const kh_problem_csr *pc, kh_engine **out) {
    if (pc == nullptr || out == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    *out = nullptr;
    if (pc->ops == nullptr || pc->ops_adj == nullptr || pc->op_norms == nullptr)
        return kh_fail(KH_ERR_INVALID, "ops, ops_adj and op_norms are required for sparse operators");
    if (pc->K < 1 || pc->L < 0) return kh_fail(KH_ERR_INVALID, "bad sizes K=%d L=%d", pc->K, pc->L);
    const size_t nops = (size_t)pc->K * (1 + pc->L);
    std::vector<const kh_cdouble *> data(nops);
    for (size_t i = 0; i < nops; ++i) {
        const kh_csr &a = pc->ops[i], &b = pc->ops_adj[i];
        if ((a.data == nullptr) != (b.data == nullptr))
            return kh_fail(KH_ERR_INVALID, "operator %zu: ops and ops_adj must both be present or both absent", i);
        if (a.data != nullptr && (a.indptr == nullptr || a.indices == nullptr || b.indptr == nullptr ||
                                  b.indices == nullptr || a.nnz != b.nnz))
            return kh_fail(KH_ERR_INVALID, "operator %zu: incomplete CSR arrays", i);
        data[i] = a.data;
    }
    kh_problem pr;
    pr.K = pc->K;
    pr.N = pc->N;
    pr.L = pc->L;
    pr.nt = pc->nt;
    pr.is_super = pc->is_super;
    pr.reserved = 0;
    pr.dt = pc->dt;
    pr.ops = data.data();
    pr.op_norms = pc->op_norms;
    pr.tol = pc->tol;
    pr.theta_max = pc->theta_max;
    return engine_create(&pr, pc->ops, pc->ops_adj, out);
}

// ---- mixed engines (kh_engine_create_mixed): objectives of their own dimension N_k and kind, one launch per sweep
// The generic kernels' MIXED instantiations for every sweep; Taylor series (no real-spectrum form) and the update sums on
// the forward side (no adjoint-side store): a first version, kept simple.
static KhPlan plan_mixed(int K, int num_cus, double theta_max) {
    KhPlan p;  // (kind = kind_store = KIND_GENERIC, Taylor tables)
    p.max_wgs = max_update_wgs(num_cus);
    p.grid_update = K < p.max_wgs ? K : p.max_wgs;
    p.theta_max = theta_max > 0.0 ? theta_max : 1.0;
    return p;
}

static int engine_build_mixed(kh_engine *e, const kh_problem *pr, const int32_t *dims, const int32_t *is_super) {
    KH_HIP(hipGetDevice(&e->device));
    hipDeviceProp_t prop;
    KH_HIP(hipGetDeviceProperties(&prop, e->device));
    e->num_cus = prop.multiProcessorCount;
    const size_t gen_lds = kh_gen_lds_bytes(e->N, true);  // (carved for the stride: S <= 2540)
    if (gen_lds > (size_t)prop.sharedMemPerBlock && gen_lds > 160 * 1024)
        return kh_fail(KH_ERR_UNSUPPORTED, "stride N=%d needs %zu bytes of LDS", e->N, gen_lds);
    std::vector<const cplx *> fw, bw;
    KH_TRY(stage_operators(e, pr, nullptr, nullptr, fw, bw, dims));
    e->plan = plan_mixed(e->K, e->num_cus, pr->theta_max);
    e->gen_adj_failed = true;  // (the update sums stay on the forward side)
    KH_TRY(stage_series(e));
    // per objective: the equation-of-motion factor of each direction (propagators.py:94-99) and the mu factor (mu.py:130-134)
    std::vector<cplx> f_fw(e->K), f_bw(e->K), mu(e->K);
    for (int k = 0; k < e->K; ++k) {
        const bool super = is_super[k] != 0;
        f_fw[k] = super ? make_double2(1.0, 0.0) : make_double2(0.0, -1.0);
        f_bw[k] = super ? make_double2(1.0, 0.0) : make_double2(0.0, 1.0);
        mu[k] = super ? make_double2(0.0, 1.0) : make_double2(1.0, 0.0);
    }
    int *d_dims = nullptr;
    cplx *d_f_fw = nullptr, *d_f_bw = nullptr, *d_mu = nullptr;
    KH_TRY(dev_upload(e, &d_dims, dims, sizeof(int) * e->K));
    KH_TRY(dev_upload(e, &d_f_fw, f_fw.data(), sizeof(cplx) * e->K));
    KH_TRY(dev_upload(e, &d_f_bw, f_bw.data(), sizeof(cplx) * e->K));
    KH_TRY(dev_upload(e, &d_mu, mu.data(), sizeof(cplx) * e->K));
    e->mixed_fw = KhMixedArgs{d_dims, d_f_fw, d_mu};
    e->mixed_bw = KhMixedArgs{d_dims, d_f_bw, d_mu};
    return stage_workspaces(e);
}

extern "C" int kh_engine_create_mixed(const kh_problem *pr, const int32_t *dims, const int32_t *is_super, kh_engine **out) {
    if (pr == nullptr || dims == nullptr || is_super == nullptr || out == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    *out = nullptr;
    KH_TRY(validate_problem(pr));
    int S = 0;
    for (int k = 0; k < pr->K; ++k) {
        if (dims[k] < 1) return kh_fail(KH_ERR_INVALID, "dims[%d] = %d", k, dims[k]);
        S = dims[k] > S ? dims[k] : S;
    }
    if (pr->N != S) return kh_fail(KH_ERR_INVALID, "problem->N = %d must be the stride max(dims) = %d", pr->N, S);
    kh_engine *e = new kh_engine();
    e->K = pr->K;
    e->N = pr->N;
    e->L = pr->L;
    e->nt = pr->nt;
    e->is_super = 0;  // (per objective: mixed_fw / mixed_bw)
    e->mixed = true;
    e->tol = pr->tol > 0.0 ? pr->tol : ldexp(1.0, -53);
    e->sw = read_switches();
    const int rc = engine_build_mixed(e, pr, dims, is_super);
    if (rc != KH_OK) {
        kh_engine_destroy(e);
        return rc;
    }
    *out = e;
    return KH_OK;
}

// ---- Lindblad-form engines (kh_engine_create_lindblad): d x d Hamiltonians and Lindblad operators, kh_lind.h
static int lind_host_norm(const cplx *dev, int d, std::map<const void *, double> &cache, double *out) {
    auto it = cache.find(dev);
    if (it == cache.end()) {
        std::vector<cplx> h((size_t)d * d);
        KH_HIP(hipMemcpy(h.data(), dev, sizeof(cplx) * h.size(), hipMemcpyDeviceToHost));
        double acc = 0.0;
        for (const cplx &v : h) acc += v.x * v.x + v.y * v.y;
        it = cache.emplace(dev, sqrt(acc)).first;
    }
    *out = it->second;
    return KH_OK;
}

static int engine_build_lindblad(kh_engine *e, const kh_problem_lindblad *pl) {
    KH_HIP(hipGetDevice(&e->device));
    hipDeviceProp_t prop;
    KH_HIP(hipGetDeviceProperties(&prop, e->device));
    e->num_cus = prop.multiProcessorCount;
    const int K = e->K, L = e->L, d = pl->d, n_c = pl->n_c, dd = d * d;
    // W buffers: as many of the Lindblad operators at a time as LDS holds
    int nw = n_c > 1 ? n_c : 1;
    while (nw > 1 && kh_lind_lds_bytes(d, n_c, nw) > KH_LIND_LDS_MAX) --nw;
    if (kh_lind_lds_bytes(d, n_c, nw) > KH_LIND_LDS_MAX)
        return kh_fail(KH_ERR_UNSUPPORTED, "d=%d with %d Lindblad operators needs %zu bytes of LDS", d, n_c, kh_lind_lds_bytes(d, n_c, nw));
    // bounds on || Lindbladian ||: n_0 = 2 ||H0|| + 2 sum_j ||C_j||^2, n_l = 2 ||H_l||
    const size_t stride = (size_t)1 + L + n_c;
    std::vector<double> norms((size_t)K * (1 + L), 0.0);
    std::map<const void *, double> fro;
    for (int k = 0; k < K; ++k) {
        auto norm_of = [&](const kh_cdouble *op, size_t j, double *out) {
            *out = 0.0;
            if (op == nullptr) return (int)KH_OK;
            if (pl->op_norms != nullptr) return *out = pl->op_norms[k * stride + j], (int)KH_OK;
            return lind_host_norm((const cplx *)op, d, fro, out);
        };
        double v = 0.0;
        for (int j = 0; j <= L; ++j) {
            KH_TRY(norm_of(pl->ops[(size_t)k * (1 + L) + j], j, &v));
            norms[(size_t)k * (1 + L) + j] = 2.0 * v;
        }
        for (int j = 0; j < n_c; ++j) {
            KH_TRY(norm_of(pl->c_ops[(size_t)k * n_c + j], 1 + L + j, &v));
            norms[(size_t)k * (1 + L)] += 2.0 * v * v;
        }
    }
    kh_problem pr;
    pr.K = K, pr.N = d, pr.L = L, pr.nt = e->nt, pr.is_super = 1, pr.reserved = 0;
    pr.dt = pl->dt, pr.ops = pl->ops, pr.op_norms = norms.data(), pr.tol = pl->tol, pr.theta_max = pl->theta_max;
    const std::vector<int32_t> dims(K, d);
    std::vector<const cplx *> fw, bw;
    KH_TRY(stage_operators(e, &pr, nullptr, nullptr, fw, bw, dims.data()));
    // the Lindblad operators and their adjoints (one copy per distinct operator)
    const size_t ncops = (size_t)K * n_c;
    std::vector<const cplx *> cfw(ncops > 0 ? ncops : 1, nullptr), cbw(ncops > 0 ? ncops : 1, nullptr);
    KhCopies adj;
    for (size_t i = 0; i < ncops; ++i) {
        const cplx *src = (const cplx *)pl->c_ops[i];
        cfw[i] = src;
        if (src == nullptr) continue;
        KH_TRY(adj.get(e, src, nullptr, sizeof(cplx) * dd, [&](cplx *dst) {
            kh_adjoint_kernel<<<dim3(1, 1), 256>>>(src, dst, d);
            return KH_OK;
        }, &cbw[i]));
    }
    KH_HIP(hipGetLastError());
    const cplx **d_cfw = nullptr, **d_cbw = nullptr;
    KH_TRY(dev_upload(e, &d_cfw, cfw.data(), sizeof(cplx *) * cfw.size()));
    KH_TRY(dev_upload(e, &d_cbw, cbw.data(), sizeof(cplx *) * cbw.size()));
    // A0 = -i H0 - M/2, B0 = +i H0 - M/2 per objective, and their adjoints for the backward sweep
    cplx *pool[4] = {nullptr, nullptr, nullptr, nullptr};  // A0 fw, B0 fw, A0 bw, B0 bw
    for (cplx *&q : pool) KH_TRY(dev_alloc(e, &q, sizeof(cplx) * (size_t)K * dd));
    kh_lind_setup_kernel<<<K, 256>>>(e->d_ops_fw, d_cfw, pool[0], pool[1], 1 + L, n_c, d);
    for (int k = 0; k < K; ++k) {
        kh_adjoint_kernel<<<dim3(1, 1), 256>>>(pool[0] + (size_t)k * dd, pool[2] + (size_t)k * dd, d);
        kh_adjoint_kernel<<<dim3(1, 1), 256>>>(pool[1] + (size_t)k * dd, pool[3] + (size_t)k * dd, d);
    }
    KH_HIP(hipGetLastError());
    const cplx **tabs[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int t = 0; t < 4; ++t) {
        std::vector<const cplx *> ptrs(K);
        for (int k = 0; k < K; ++k) ptrs[k] = pool[t] + (size_t)k * dd;
        KH_TRY(dev_upload(e, &tabs[t], ptrs.data(), sizeof(cplx *) * K));
    }
    e->lind_fw = KhLindArgs{d, n_c, nw, -1.0, d_cfw, tabs[0], tabs[1]};
    e->lind_bw = KhLindArgs{d, n_c, nw, +1.0, d_cbw, tabs[2], tabs[3]};

    KhFacts f;
    f.K = K, f.N = e->N, f.L = L, f.num_cus = e->num_cus;
    f.csr = false, f.shared = false, f.has_h1 = f.all_h1 = false;
    f.theta_max = pl->theta_max;
    f.lind = true;
    e->plan = plan_families(f, e->sw);
    e->gen_adj_failed = true;  // (no adjoint-side store: the sums come from one pair of products per interval)
    KH_TRY(stage_series(e));
    return stage_workspaces(e);
}

extern "C" int kh_engine_create_lindblad(const kh_problem_lindblad *pl, kh_engine **out) {
    if (pl == nullptr || out == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    *out = nullptr;
    if (pl->d < 1 || pl->n_c < 0) return kh_fail(KH_ERR_INVALID, "bad sizes d=%d n_c=%d", pl->d, pl->n_c);
    if (pl->n_c > 0 && pl->c_ops == nullptr) return kh_fail(KH_ERR_INVALID, "c_ops missing");
    kh_problem pr;
    pr.K = pl->K, pr.N = pl->d, pr.L = pl->L, pr.nt = pl->nt, pr.is_super = 1, pr.reserved = 0;
    pr.dt = pl->dt, pr.ops = pl->ops, pr.op_norms = nullptr, pr.tol = pl->tol, pr.theta_max = pl->theta_max;
    KH_TRY(validate_problem(&pr));
    if (pl->d > KH_LIND_DMAX || pl->n_c > KH_LIND_MAX_NC || pl->L > KH_LIND_MAX_L)
        return kh_fail(KH_ERR_UNSUPPORTED, "the Lindblad-form kernels take d <= %d, at most %d Lindblad operators and %d controls (d=%d n_c=%d L=%d)",
                       KH_LIND_DMAX, KH_LIND_MAX_NC, KH_LIND_MAX_L, pl->d, pl->n_c, pl->L);
    kh_engine *e = new kh_engine();
    e->K = pl->K;
    e->N = pl->d * pl->d;
    e->L = pl->L;
    e->nt = pl->nt;
    e->is_super = 1;
    e->lind = true;
    e->tol = pl->tol > 0.0 ? pl->tol : ldexp(1.0, -53);
    e->sw = read_switches();
    const int rc = engine_build_lindblad(e, pl);
    if (rc != KH_OK) {
        kh_engine_destroy(e);
        return rc;
    }
    *out = e;
    return KH_OK;
}

// ---- replica engines (kh_engine_create_replicas): B independent small problems in one launch per sweep, kh_replica.h
// One family for every sweep; the coefficient set comes from the analysis of ALL operators of the batch (one set
// serves the whole engine); theta <= 1 per sub-step: a term costs no round here.
static KhPlan plan_replicas(const KhFacts &f, const KhSwitches &sw, int replicas) {
    KhPlan p;
    p.kind = p.kind_store = KIND_REPLICA;
    p.max_wgs = max_update_wgs(f.num_cus);
    p.grid_update = replicas;
    p.theta_max = f.theta_max > 0.0 ? f.theta_max : 1.0;
    p.stage_sq = f.L == 1;  // (one control: the A^2 chain)
    p.series_rows = true;
    if (f.real_spectrum) {
        p.series_cap = 2.0, p.series_defect = 0.0;
    } else if (f.imag_defect > 0.0 && f.imag_defect <= 0.05 && sw.near_imag) {
        p.series_cap = 2.0, p.series_defect = f.imag_defect;
    } else {
        p.series_rows = false;
    }
    return p;
}

// pr->dt: the largest step of every interval over the replicas (what the operator analysis takes); dt_all: [B][nt-1]
static int engine_build_replicas(kh_engine *e, const kh_problem *pr, const double *dt_all) {
    KH_HIP(hipGetDevice(&e->device));
    hipDeviceProp_t prop;
    KH_HIP(hipGetDeviceProperties(&prop, e->device));
    e->num_cus = prop.multiProcessorCount;
    std::vector<const cplx *> fw, bw;
    KH_TRY(stage_operators(e, pr, nullptr, nullptr, fw, bw));
    KH_TRY(dev_upload(e, &e->d_dt, dt_all, sizeof(double) * (size_t)e->replicas * (e->nt - 1)));
    KhFacts f;
    f.K = e->K, f.N = e->N, f.L = e->L, f.num_cus = e->num_cus;
    f.csr = false, f.shared = false;
    f.has_h1 = fw[1] != nullptr;
    f.all_h1 = false;
    f.theta_max = pr->theta_max;
    KH_TRY(detect_dense(e, pr, f));
    if (e->sw.taylor) f.real_spectrum = false, f.imag_defect = -1.0;
    e->adj_sign = 0.0;  // (the sums stay on the forward side)
    e->plan = plan_replicas(f, e->sw, e->replicas);
    e->gen_adj_failed = true;
    std::vector<const cplx *> sq[2];
    if (e->plan.stage_sq) KH_TRY(stage_squares(e, fw, bw, sq));
    KH_TRY(stage_series(e));
    const std::vector<int> ones((size_t)e->replicas, 1);
    KH_TRY(dev_upload(e, &e->d_active, ones.data(), sizeof(int) * ones.size()));
    return stage_workspaces(e);
}

extern "C" int kh_engine_create_replicas(const kh_problem *problem, int32_t replicas, const double *dt_replicas, kh_engine **out) {
    if (problem == nullptr || out == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    *out = nullptr;
    if (replicas < 1 || problem->K < 1 || problem->K % replicas != 0)
        return kh_fail(KH_ERR_INVALID, "K = %d objectives are not %d replicas of equal size", problem->K, replicas);
    if (problem->nt < 2) return kh_fail(KH_ERR_INVALID, "bad sizes K=%d N=%d L=%d nt=%d", problem->K, problem->N, problem->L, problem->nt);
    // the time steps of every replica, [B][nt-1], and the largest of every interval
    const size_t M = (size_t)problem->nt - 1;
    if (dt_replicas == nullptr && problem->dt == nullptr) return kh_fail(KH_ERR_INVALID, "dt/ops missing");
    std::vector<double> dt_all((size_t)replicas * M), dt_max(M, 0.0);
    for (int b = 0; b < replicas; ++b)
        for (size_t n = 0; n < M; ++n) {
            const double v = dt_replicas != nullptr ? dt_replicas[(size_t)b * M + n] : problem->dt[n];
            if (!(v > 0.0)) return kh_fail(KH_ERR_INVALID, "replica %d: dt[%zu] = %g is not positive", b, n, v);
            dt_all[(size_t)b * M + n] = v;
            dt_max[n] = v > dt_max[n] ? v : dt_max[n];
        }
    kh_problem pr = *problem;
    pr.dt = dt_max.data();
    KH_TRY(validate_problem(&pr));
    const int Kr = pr.K / replicas;
    if (pr.N > KH_MINI_N || Kr > KH_MINI_MAXK || pr.L < 1 || pr.L > 4)
        return kh_fail(KH_ERR_UNSUPPORTED, "replica engines take N <= %d, at most %d objectives per replica and 1..4 controls (N=%d K_r=%d L=%d)",
                       KH_MINI_N, KH_MINI_MAXK, pr.N, Kr, pr.L);

    kh_engine *e = new kh_engine();
    e->K = pr.K;
    e->N = pr.N;
    e->L = pr.L;
    e->nt = pr.nt;
    e->is_super = pr.is_super ? 1 : 0;
    e->replicas = replicas;
    e->Kr = Kr;
    e->tol = pr.tol > 0.0 ? pr.tol : ldexp(1.0, -53);
    e->sw = read_switches();
    const int rc = engine_build_replicas(e, &pr, dt_all.data());
    if (rc != KH_OK) {
        kh_engine_destroy(e);
        return rc;
    }
    *out = e;
    return KH_OK;
}

extern "C" int kh_set_active_replicas(kh_engine *e, const int32_t *active_host) {
    if (e == nullptr) return kh_fail(KH_ERR_INVALID, "null engine");
    if (e->replicas < 1) return kh_fail(KH_ERR_UNSUPPORTED, "only replica engines (kh_engine_create_replicas) take an active mask; this one runs %s", kh_engine_kernel(e));
    e->all_active = true;
    if (active_host == nullptr) return KH_OK;
    std::vector<int> mask((size_t)e->replicas);
    for (int b = 0; b < e->replicas; ++b) {
        mask[b] = active_host[b] != 0 ? 1 : 0;
        if (mask[b] == 0) e->all_active = false;
    }
    // (a blocking copy on the null stream: ordered behind the sweeps already launched, done before the next one)
    KH_HIP(hipMemcpy(e->d_active, mask.data(), sizeof(int) * mask.size(), hipMemcpyHostToDevice));
    return KH_OK;
}

// resident workgroups per CU of the replica update kernel as built (hipOccupancyMaxActiveBlocksPerMultiprocessor)
extern "C" int kh_replica_occupancy(kh_engine *e, int32_t *workgroups_per_cu) {
    if (e == nullptr || workgroups_per_cu == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    if (e->replicas < 1) return kh_fail(KH_ERR_UNSUPPORTED, "not a replica engine");
    const void *fn = nullptr;  // (the instantiation the next update sweep launches: kh_set_second_order_replicas)
    if (e->second_order())
        fn = e->L == 1   ? (const void *)kh_rep_forward_update_so<1>
             : e->L == 2 ? (const void *)kh_rep_forward_update_so<2>
             : e->L == 3 ? (const void *)kh_rep_forward_update_so<3>
                         : (const void *)kh_rep_forward_update_so<4>;
    else
        fn = e->L == 1   ? (const void *)kh_rep_forward_update<1>
             : e->L == 2 ? (const void *)kh_rep_forward_update<2>
             : e->L == 3 ? (const void *)kh_rep_forward_update<3>
                         : (const void *)kh_rep_forward_update<4>;
    int per_cu = 0;
    KH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * e->Kr, 0));
    *workgroups_per_cu = per_cu;
    return KH_OK;
}

// ---------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------

// Runtime value -> template parameters: each mapping is written once and called by the plain sweep and the update
// sweep alike, with std::integral_constant / std::bool_constant arguments (`decltype(x)::value` in the callee).
template <int V>
using KhInt = std::integral_constant<int, V>;

template <class F>
static int with_bool(bool b, F &&f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// register-tile kernels (kh_tile64.h, kh_tile64s.h): 1..4 controls
template <class F>
static int with_tile_L(int L, F &&f) {
    switch (L) {
        case 1: return f(KhInt<1>{});
        case 2: return f(KhInt<2>{});
        case 3: return f(KhInt<3>{});
        case 4: return f(KhInt<4>{});
        default: return kh_fail(KH_ERR_UNSUPPORTED, "tile kernels handle 1..4 controls");
    }
}

// ... rows per thread: two (256-thread workgroups) only with one control
template <class F>
static int with_tile(bool rpt2, int L, F &&f) {
    return with_tile_L(L, [&](auto lt) {
        if constexpr (decltype(lt)::value == 1)
            return rpt2 ? f(KhInt<2>{}, lt) : f(KhInt<1>{}, lt);
        else
            return f(KhInt<1>{}, lt);
    });
}

// tile64x kernels (kh_tile64x.h): five to eight controls
template <class F>
static int with_tx(int L, F &&f) {
    switch (L) {
        case 5: return f(KhInt<5>{});
        case 6: return f(KhInt<6>{});
        case 7: return f(KhInt<7>{});
        default: return f(KhInt<8>{});
    }
}

// tilen kernels (kh_tilen.h): elements per lane; the control operator in registers only up to N = 96
template <class F>
static int with_tn(int EP, bool h1reg, F &&f) {
    switch (EP) {
        case 20: return h1reg ? f(KhInt<20>{}, std::true_type{}) : f(KhInt<20>{}, std::false_type{});
        case 24: return h1reg ? f(KhInt<24>{}, std::true_type{}) : f(KhInt<24>{}, std::false_type{});
        case 28: return f(KhInt<28>{}, std::false_type{});
        default: return f(KhInt<32>{}, std::false_type{});
    }
}

// padded-row kernels (kh_ell.h): (threads, rows per lane, row width, streamed form).  One row per lane where the rows'
// entries fit the register budget of that many waves (512 threads: 256 VGPRs, 768: 168, 1024: 128), else two rows
// per lane of a 512-thread workgroup; (12: drift + two controls of a Lindbladian -- the reference's notebook 06 has
// 11.2 entries per row; every padded slot is a gather and four multiply-adds per term); N > 1024: <= 8 entries per
// row (build_ell_host)
template <class F>
static int with_ell(int N, int E, bool stream, F &&f) {
    using F_ = std::false_type;
    if (stream) return f(KhInt<512>{}, KhInt<KH_ELLS_RPL>{}, KhInt<4>{}, std::true_type{});
    if (N <= 512) {
        if (E <= 8) return f(KhInt<512>{}, KhInt<1>{}, KhInt<8>{}, F_{});
        if (E <= 12) return f(KhInt<512>{}, KhInt<1>{}, KhInt<12>{}, F_{});
        if (E <= 16) return f(KhInt<512>{}, KhInt<1>{}, KhInt<16>{}, F_{});
        if (E <= 24) return f(KhInt<512>{}, KhInt<1>{}, KhInt<24>{}, F_{});
        return f(KhInt<512>{}, KhInt<1>{}, KhInt<32>{}, F_{});
    }
    if (N <= 768 && E <= 16) {
        if (E <= 8) return f(KhInt<768>{}, KhInt<1>{}, KhInt<8>{}, F_{});
        if (E <= 12) return f(KhInt<768>{}, KhInt<1>{}, KhInt<12>{}, F_{});
        return f(KhInt<768>{}, KhInt<1>{}, KhInt<16>{}, F_{});
    }
    if (N > 1024) return N <= 1536 ? f(KhInt<512>{}, KhInt<3>{}, KhInt<8>{}, F_{}) : f(KhInt<512>{}, KhInt<4>{}, KhInt<8>{}, F_{});
    if (E <= 8) return f(KhInt<1024>{}, KhInt<1>{}, KhInt<8>{}, F_{});
    return E <= 12 ? f(KhInt<512>{}, KhInt<2>{}, KhInt<12>{}, F_{}) : f(KhInt<512>{}, KhInt<2>{}, KhInt<16>{}, F_{});
}

// Lindblad-form kernels (kh_lind.h): rows per thread
template <class F>
static int with_lind(int d, F &&f) {
    switch (kh_lind_rb(d)) {
        case 1: return f(KhInt<1>{});
        case 2: return f(KhInt<2>{});
        default: return f(KhInt<4>{});
    }
}

// cooperative kernels (kh_coop.h): operator-fragment slots per lane, objectives per workgroup
template <class F>
static int with_coop(int cols, int ks, F &&f) {
    auto by_ks = [&](auto c) { return ks <= 8 ? f(KhInt<8>{}, c) : f(KhInt<16>{}, c); };
    if (cols == 2) return by_ks(KhInt<2>{});
    if (cols == 4) return by_ks(KhInt<4>{});
    return by_ks(KhInt<16>{});
}

// V_lk = H_lk^+ chi_k for the whole co-state store [L][K][nt][N] (kh_generic.h, kh_gen_adjoint_side), in front of an
// update sweep that reads its sums from there
static int gen_adjoint_side(kh_engine *e, const cplx *chi_store, int L, hipStream_t st) {
    const dim3 grid((unsigned)(e->K * L), (unsigned)((e->nt + KH_GEN_ADJ_POINTS - 1) / KH_GEN_ADJ_POINTS));
    // (through the launch registry: a test can tell that the pre-pass ran)
    launch_plain<kh_gen_adjoint_side>(grid, dim3(KH_GEN_ADJ_THREADS), 0, st, e->d_ops_bw, chi_store, e->d_gen_adj, e->K, e->N, L, e->nt);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

static KhExchange exchange_args(const kh_engine *e, bool internal_exchange) {
    KhExchange ex;
    ex.slots = e->d_slots;
    ex.abort_flag = e->d_abort;
    ex.G = (e->plan.kind == KIND_COOP && internal_exchange) ? e->plan.coop_G * e->plan.coop_Y : e->plan.grid_update;
    ex.timeout_ticks = e->sw.timeout_ticks;
    // across GPUs the ranks are separate processes: a host-side hiccup of one of them (garbage collection, page
    // faults) must not look like a lost peer and demote the whole run to the per-interval path
    if (e->p2p_ready && internal_exchange && !e->sw.timeout_set && ex.timeout_ticks < 1000000000LL)
        ex.timeout_ticks = 1000000000LL;  // 10 s
    ex.peer_windows = e->d_p2p_peers;
    ex.my_window = e->p2p_window;
    ex.world = (e->p2p_ready && internal_exchange) ? e->p2p_world : 1;
    ex.rank = e->p2p_rank;
    ex.epoch_base = e->p2p_epoch_base;
    ex.first_poll_delay = e->sw.poll_delay;
    ex.fail_at = (ex.world > 1 && e->p2p_rank == e->sw.p2p_fail_rank && e->p2p_sweeps + 1 == e->sw.p2p_fail_sweep) ? e->sw.p2p_fail_at : -1;
    ex.wait_ticks = ex.world > 1 ? e->d_wait_ticks : nullptr;
    return ex;
}

static KhCoopArgs coop_args(const kh_engine *e, bool backward) {
    KhCoopArgs c;
    c.fops = backward ? e->d_coop_fops_bw : e->d_coop_fops_fw;
    c.sq = backward ? e->d_coop_sq_bw : e->d_coop_sq_fw;  // (NULL unless staged: one control)
    c.vbuf = e->d_coop_vbuf;
    c.epoch_base = 0;  // the buffer is cleared before every launch
    c.G = e->plan.coop_G;
    c.Y = e->plan.coop_Y;
    c.ks = e->plan.coop_ks;
    c.cols = e->plan.coop_cols;
    c.first_poll_delay = e->sw.coop_poll_delay;
    c.xcd_rows = e->plan.coop_xcd ? e->plan.coop_G : 0;
    c.xcc = e->d_coop_xcc;
    c.local = 0;
    c.ring_mask = KH_COOP_RING - 1;
    for (int i = 0; i < 5; ++i) c.tab[i] = nullptr;  // (resolved in the kernel)
    c.ser_theta = e->plan.coop_series ? e->d_q2_theta : nullptr;
    c.ser_c0 = e->plan.coop_series ? e->d_q2_c0 : nullptr;
    c.ser_rows = e->plan.coop_series ? e->d_q2_rows : nullptr;
    return c;
}

// A cooperative kernel: its LDS limit raised (for the largest fragment count of the instantiation), the exchange
// buffers cleared, and launched with one column group per XCD where that is possible: a one-dimensional grid of 8 G
// blocks of which only G Y do anything (kh_coop_place).  The cooperative-launch validation counts all 8 G of them, so
// on a device (or partition, or CU mask) with fewer resident workgroups than that the launch is refused although the
// G Y real ones would fit: the placement is then given up for good (two-dimensional (G, Y) grid, memory-side
// exchange) and the launch repeated.
template <auto Kernel, int COLS, class... Rest>
static int launch_coop(kh_engine *e, hipStream_t st, bool backward, const KhSweepArgs &p, Rest... rest) {
    KhPlan &pl = e->plan;
    KH_TRY(ensure_dynamic_lds(e, (const void *)Kernel, kh_coop_lds_bytes(COLS <= 4 ? 16 : 15, COLS)));
    KH_HIP(hipMemsetAsync(e->d_coop_vbuf, 0, e->coop_vbuf_bytes, st));
    KH_HIP(hipMemsetAsync(e->d_coop_xcc, 0, sizeof(unsigned int) * (size_t)pl.coop_G * pl.coop_Y, st));
    auto launch = [&](dim3 grid) {  // (coop_args: the placement as it stands)
        return launch_persistent<Kernel>(e, grid, dim3(KH_COOP_THREADS), kh_coop_lds_bytes(pl.coop_ks, COLS), st, p,
                                         coop_args(e, backward), rest...);
    };
    int rc2 = launch(pl.coop_xcd ? dim3(8 * pl.coop_G) : dim3(pl.coop_G, pl.coop_Y));
    if (rc2 == KH_ERR_UNSUPPORTED && pl.coop_xcd) {
        pl.coop_xcd = false;
        rc2 = launch(dim3(pl.coop_G, pl.coop_Y));
    }
    return rc2;
}

// (16 operator slots per lane x 16 objectives per workgroup: the A^2 chain's second resident fragment does not fit the
// register file -- 245 .. 343 spilled values --, the engine does not stage the A^2 tables for that shape)
template <int MAXKS, int COLS>
static int launch_coop_store(kh_engine *e, const KhSweepArgs &p, const double *pulses, const cplx *in, cplx *store,
                             cplx *out, int direction, hipStream_t st) {
    const bool bw = direction < 0;
    const KhExchange ex = exchange_args(e, true);
    if constexpr (!(MAXKS == 16 && COLS == 16))
        if ((bw ? e->d_coop_sq_bw : e->d_coop_sq_fw) != nullptr)
            return launch_coop<kh_coop_sweep_store<MAXKS, COLS, true>, COLS>(e, st, bw, p, ex, pulses, in, store, out, direction);
    return launch_coop<kh_coop_sweep_store<MAXKS, COLS, false>, COLS>(e, st, bw, p, ex, pulses, in, store, out, direction);
}

template <int MAXKS, int COLS>
static int launch_coop_update(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u_in, const KhExchange &ex,
                              hipStream_t st) {
    KhUpdateArgs u = u_in;
    const bool so = u.sigma != nullptr;
    if (e->plan.coop_adj && !so && e->L == 1 && e->d_coop_sq_fw != nullptr && e->d_coop_adj == nullptr) {
        // V = H_1^+ X needs a second buffer of the co-state store's size; it is an optimisation (one round per interval
        // less): without the memory the sweep takes the sums by one more round, as it did before the form existed
        const size_t bytes = sizeof(cplx) * (size_t)e->K * e->nt * e->N;
        if (hipMalloc(&e->d_coop_adj, bytes) != hipSuccess) {
            (void)hipGetLastError();
            e->d_coop_adj = nullptr;
            e->plan.coop_adj = false;
        }
    }
    if constexpr (!(MAXKS == 16 && COLS == 16)) {  // (see launch_coop_store)
        if (e->d_coop_sq_fw != nullptr && e->plan.coop_adj && !so && e->L == 1) {
            // V = H_1^+ X over the whole co-state store, block-sparse on the matrix cores (kh_coop.h)
            const long long M = (long long)e->K * e->nt;
            // (through the launch registry: a test can tell that the pre-pass ran)
            launch_plain<kh_coop_adjoint_side>(dim3((unsigned)((M + 63) / 64)), dim3(KH_COOP_ADJ_THREADS), 0, st, e->coop_adj_op,
                                               e->d_coop_adj_nz, u.chi_store, e->d_coop_adj, e->N, e->plan.coop_G, M);
            KH_HIP(hipGetLastError());
            u.adj_store = e->d_coop_adj;
            if (ex.world == 1 && e->sw.coop_single)
                return launch_coop<kh_coop_forward_update<MAXKS, COLS, false, true, true, false>, COLS>(e, st, false, p, u, ex);
            return launch_coop<kh_coop_forward_update<MAXKS, COLS, false, true, true>, COLS>(e, st, false, p, u, ex);
        }
        if (e->d_coop_sq_fw != nullptr)
            return so ? launch_coop<kh_coop_forward_update<MAXKS, COLS, true, false, true>, COLS>(e, st, false, p, u, ex)
                      : launch_coop<kh_coop_forward_update<MAXKS, COLS, false, false, true>, COLS>(e, st, false, p, u, ex);
    }
    return so ? launch_coop<kh_coop_forward_update<MAXKS, COLS, true, false, false>, COLS>(e, st, false, p, u, ex)
              : launch_coop<kh_coop_forward_update<MAXKS, COLS, false, false, false>, COLS>(e, st, false, p, u, ex);
}

// the plain sweeps (forward with storage, backward): one family per engine, kind_store
static int sweep_store(kh_engine *e, bool backward, const double *pulses, const cplx *in, cplx *store, cplx *out,
                       hipStream_t st) {
    const KhPlan &pl = e->plan;
    const KhSweepArgs p = sweep_args(e, backward);
    const int direction = backward ? -1 : +1;
    const cplx *const *sq = backward ? e->d_sq_bw : e->d_sq_fw;
    const int grid_cus = e->K < e->num_cus ? e->K : e->num_cus;  // (objectives in turns: at most one workgroup per CU)
    KH_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(double) * 4, st));
    int rc = KH_OK;
    switch (pl.kind_store) {
        case KIND_TILE_Q2:
            if (pl.quad)
                launch_plain<kh_quad_sweep_store>(dim3(1), dim3(64), 0, st, p, sq, pulses, in, store, out, direction);
            else if (pl.mini)
                launch_plain<kh_mini_sweep_store>(dim3(e->K), dim3(64), 0, st, p, sq, pulses, in, store, out, direction);
            else
                launch_plain<kh_q2_sweep_store>(dim3(e->K), dim3(KH_Q2_THREADS), kh_q2_lds_bytes(), st, sweep_args_q2(e, p), sq, pulses, in, store, out, direction);
            break;
        case KIND_TILEN: {
            const cplx *const *tabs = backward ? e->d_tn_bw : e->d_tn_fw;
            rc = with_tn(pl.tn_EP, pl.tn_h1reg, [&](auto ep, auto hr) {
                launch_plain<kh_tn_sweep_store<decltype(ep)::value, decltype(hr)::value>>(dim3(grid_cus), dim3(KH_TN_THREADS), kh_tn_lds_bytes(),
                                                                                          st, p, tabs, pulses, in, store, out, direction);
                return KH_OK;
            });
            break;
        }
        case KIND_TILEX: {
            const cplx *const *tabs = backward ? e->d_tx_bw : e->d_tx_fw;
            rc = with_tx(e->L, [&](auto lt) {
                return launch_plain_lds<kh_tx_sweep_store<decltype(lt)::value>>(e, dim3(grid_cus), dim3(KH_TX_THREADS), kh_tx_lds_bytes(), st,
                                                                                p, tabs, pulses, in, store, out, direction);
            });
            break;
        }
        case KIND_ELL: {
            const KhEll *ells = backward ? e->d_ell_bw : e->d_ell_fw;
            if (pl.ell_global) {
                const bool split = e->row_split > 1;
                const int G = split ? e->split_groups * e->row_split : e->ellg_wgs;
                auto shared = [&](auto launch) {  // what both forms are launched with
                    return launch(dim3(G), dim3(KH_ELLG_THREADS), kh_ellg_lds_bytes(split), st, p, ells, (const int *)e->d_ell_off,
                                  (const cplx *)e->d_ell_vals, pulses, in, store, out, direction, e->d_ellg_ws, e->ellg_ws_stride);
                };
                if (split) {
                    // all S x groups workgroups wait for each other at every term: resident at once, as an update sweep's
                    KH_HIP(hipMemsetAsync(e->d_split_counters, 0, e->split_counters_bytes, st));
                    KhExchange ex = exchange_args(e, false);
                    ex.G = G;
                    rc = shared([&](auto... a) {
                        return launch_persistent<kh_ellgs_sweep_store<KH_ELLG_THREADS>>(e, a..., ex, e->row_split, e->d_split_counters);
                    });
                } else {
                    shared([](auto... a) { launch_plain<kh_ellg_sweep_store<KH_ELLG_THREADS>>(a...); });
                }
                break;
            }
            const int grid = pl.ell_stream ? grid_cus : (e->K < 4 * e->num_cus ? e->K : 4 * e->num_cus);
            // (two vector buffers of KH_ELL_NMAX elements: more than the 64 KiB a kernel gets without asking)
            const size_t lds = kh_ell_lds_bytes(pl.ell_stream);
            rc = with_ell(e->N, pl.ell_E, pl.ell_stream, [&](auto t, auto r, auto em, auto stm) {
                constexpr int T = decltype(t)::value;
                return launch_plain_lds<kh_ell_sweep_store<T, decltype(r)::value, decltype(em)::value, decltype(stm)::value>>(
                    e, dim3(grid), dim3(T), lds, st, p, ells, e->d_ell_off, e->d_ell_vals, pulses, in, store, out, direction,
                    e->d_ell_scratch, e->ell_scratch_stride);
            });
            break;
        }
        case KIND_LIND: {
            const KhLindArgs la = backward ? e->lind_bw : e->lind_fw;
            rc = with_lind(la.d, [&](auto rb) {
                return launch_plain_lds<kh_lind_sweep_store<decltype(rb)::value>>(e, dim3(grid_cus), dim3(KH_LIND_THREADS),
                                                                                   kh_lind_lds_bytes(la.d, la.n_c, la.nw), st, p, la, pulses,
                                                                                   in, store, out, direction);
            });
            break;
        }
        case KIND_REPLICA:  // one single-wave workgroup per objective; pulses [B][L][nt-1]
            rc = with_tile_L(e->L, [&](auto lt) {
                launch_plain<kh_rep_sweep_store<decltype(lt)::value>>(dim3(e->K), dim3(64), 0, st, p, sq, pulses, in, store, out, direction,
                                                                      e->Kr, e->active_mask());
                return KH_OK;
            });
            break;
        case KIND_TILE_RPT2:
        case KIND_TILE_RPT1:
            rc = with_tile(pl.kind_store == KIND_TILE_RPT2, e->L, [&](auto rpt, auto lt) {
                constexpr int RPT = decltype(rpt)::value, LT = decltype(lt)::value;
                constexpr size_t lds = KhTileLds<RPT, LT>::bytes(KhTileLds<RPT, LT>::STORE);  // operator tiles parked in LDS
                return launch_plain_lds<kh_tile_sweep_store<RPT, LT>>(e, dim3(e->K), dim3(512 / RPT), lds, st, p, pulses, in, store, out, direction);
            });
            break;
        case KIND_COOP:
            rc = with_coop(pl.coop_cols, pl.coop_ks, [&](auto ks, auto cols) {
                return launch_coop_store<decltype(ks)::value, decltype(cols)::value>(e, p, pulses, in, store, out, direction, st);
            });
            if (rc == KH_ERR_UNSUPPORTED) {
                // not even the G x Y grid can be resident at once (fewer CUs than expected): the plain sweeps need no
                // cross-workgroup exchange at all, so the per-objective generic kernel takes them over from here on
                e->plan.kind_store = KIND_GENERIC;
                return sweep_store(e, backward, pulses, in, store, out, st);
            }
            break;
        default: {
            if (!e->gen_fits) return kh_fail(KH_ERR_UNSUPPORTED, "N=%d: the generic kernels' vectors do not fit LDS", e->N);
            int grid = 0;
            const KhSweepArgs pg = gen_sweep_args(e, p, false, &grid);
            const size_t lds = kh_gen_lds_bytes(e->N, e->d_csr_fw == nullptr);
            if (e->mixed)
                rc = launch_plain_lds<kh_gen_sweep_store<true>>(e, dim3(grid), dim3(KH_GEN_THREADS), lds, st, pg,
                                                                backward ? e->mixed_bw : e->mixed_fw, pulses, in, store, out, direction);
            else
                rc = launch_plain_lds<kh_gen_sweep_store<false>>(e, dim3(grid), dim3(KH_GEN_THREADS), lds, st, pg, KhMixedArgs{},
                                                                 pulses, in, store, out, direction);
        }
    }
    if (rc != KH_OK) return rc;
    KH_HIP(hipGetLastError());
    e->last_intervals = e->nt - 1;
    e->last_wgs = pl.kind_store == KIND_ELL && pl.ell_global && e->row_split > 1 ? e->split_groups * e->row_split : e->K;
    return KH_OK;
}

extern "C" int kh_forward_store(kh_engine *e, const double *pulses_dev, const kh_cdouble *init_dev,
                                kh_cdouble *states_dev, kh_cdouble *psi_T_dev, void *stream) {
    if (e == nullptr || pulses_dev == nullptr && e->L > 0 || init_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    return sweep_store(e, false, pulses_dev, (const cplx *)init_dev, (cplx *)states_dev, (cplx *)psi_T_dev,
                       (hipStream_t)stream);
}

extern "C" int kh_backward_store(kh_engine *e, const kh_cdouble *chi_T_dev, const double *pulses_dev,
                                 kh_cdouble *chi_store_dev, void *stream) {
    if (e == nullptr || chi_T_dev == nullptr || chi_store_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    return sweep_store(e, true, pulses_dev, (const cplx *)chi_T_dev, (cplx *)chi_store_dev, nullptr,
                       (hipStream_t)stream);
}

// [a, a + bytes) and [b, b + bytes) share an address
static bool ranges_overlap(const void *a, const void *b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

// The backward sweep of a co-state equation with a source (state-dependent running costs; kh_tile64.h / kh_generic.h, SRC):
// the register-tile form for the engines whose plain sweeps are the q2 (mini and quad included) or the 512-thread tile
// kernels, the generic form for every other engine its vectors fit.
extern "C" int kh_backward_store_source(kh_engine *e, const kh_cdouble *chi_T_dev, const double *pulses_dev,
                                        const kh_cdouble *src_store_dev, const double *chi_norms_dev,
                                        kh_cdouble *chi_store_dev, void *stream) {
    if (e == nullptr || chi_T_dev == nullptr || src_store_dev == nullptr || chi_store_dev == nullptr ||
        pulses_dev == nullptr && e->L > 0)
        return kh_fail(KH_ERR_INVALID, "null argument");
    if (ranges_overlap(src_store_dev, chi_store_dev, sizeof(cplx) * (size_t)e->K * e->nt * e->N))
        return kh_fail(KH_ERR_INVALID, "src_store_dev overlaps chi_store_dev");
    if (e->replicas > 0 || e->lind || e->mixed)
        return kh_fail(KH_ERR_UNSUPPORTED, "the backward sweep with a source takes uniform engines (no replica, Lindblad-form or mixed engine)");
    const KhPlan &pl = e->plan;
    const bool tile = (pl.kind_store == KIND_TILE_Q2 || pl.kind_store == KIND_TILE_RPT1) && e->L >= 1 && e->L <= 4;
    if (!tile && !e->gen_fits)
        return kh_fail(KH_ERR_UNSUPPORTED, "N=%d: the backward sweep with a source runs on the generic kernels, whose vectors do not fit LDS", e->N);
    hipStream_t st = (hipStream_t)stream;
    const KhSweepArgs p = sweep_args(e, true);
    const KhSrcArgs sa{(const cplx *)src_store_dev, chi_norms_dev};
    const cplx *in = (const cplx *)chi_T_dev;
    cplx *store = (cplx *)chi_store_dev;
    KH_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(double) * 4, st));
    int rc = KH_OK;
    if (tile) {
        rc = with_tile_L(e->L, [&](auto lt) {
            constexpr int LT = decltype(lt)::value;
            constexpr size_t lds = KhTileLds<1, LT>::bytes(KhTileLds<1, LT>::STORE);  // operator tiles parked in LDS
            return launch_plain_lds<kh_tile_sweep_store_src<1, LT>>(e, dim3(e->K), dim3(512), lds, st, p, sa, pulses_dev, in, store);
        });
    } else {
        int grid = 0;
        const KhSweepArgs pg = gen_sweep_args(e, p, false, &grid);
        rc = launch_plain_lds<kh_gen_sweep_store_src<false>>(e, dim3(grid), dim3(KH_GEN_THREADS), kh_gen_lds_bytes(e->N, e->d_csr_fw == nullptr),
                                                             st, pg, sa, pulses_dev, in, store);
    }
    if (rc != KH_OK) return rc;
    KH_HIP(hipGetLastError());
    e->last_intervals = e->nt - 1;
    e->last_wgs = e->K;
    return KH_OK;
}

// Out[k][n] = c[n] Op_k In[k][n] over a stored trajectory (kh_generic.h, kh_gen_apply_store)
extern "C" int kh_apply_store(kh_engine *e, const kh_cdouble *const *ops_table_dev, const double *factors_dev,
                              const kh_cdouble *in_store_dev, kh_cdouble *out_store_dev, void *stream) {
    if (e == nullptr || ops_table_dev == nullptr || in_store_dev == nullptr || out_store_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    if (ranges_overlap(in_store_dev, out_store_dev, sizeof(cplx) * (size_t)e->K * e->nt * e->N))
        return kh_fail(KH_ERR_INVALID, "in_store_dev overlaps out_store_dev");
    if (e->mixed || e->lind)
        return kh_fail(KH_ERR_UNSUPPORTED, "kh_apply_store takes uniform engines (one dimension for all objectives, operators of the states' dimension)");
    const dim3 grid((unsigned)e->K, (unsigned)((e->nt + KH_GEN_ADJ_POINTS - 1) / KH_GEN_ADJ_POINTS));
    launch_plain<kh_gen_apply_store>(grid, dim3(KH_GEN_ADJ_THREADS), 0, (hipStream_t)stream, (const cplx *const *)ops_table_dev,
                                     factors_dev, (const cplx *)in_store_dev, (cplx *)out_store_dev, e->K, e->N, e->nt);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

// ---- the update sweep: one route per call (update_route), one small launcher per family

enum KhRoute { ROUTE_ENS, ROUTE_ENS2, ROUTE_STREAM, ROUTE_QUAD, ROUTE_MINI, ROUTE_Q2, ROUTE_COOP, ROUTE_TILEN, ROUTE_ELL, ROUTE_TILE, ROUTE_TILEX, ROUTE_GENERIC, ROUTE_LIND,
               ROUTE_TILE_FORM, ROUTE_GENERIC_FORM };

// Which launcher runs an update call of engine e (read only).  whole: the single launch over all intervals; stepwise: one
// interval per launch (host- or device-indexed: the same route); so: second order; world: ranks of the in-kernel
// exchange; adj_store(): the adjoint-side store can be had (ensure_gen_adj, asked only where a family would read it -- its
// allocation happens at the first such call; never with a form set).
template <class AdjStore>
static KhRoute update_route(const kh_engine *e, bool stepwise, bool whole, bool so, int world, AdjStore &&adj_store) {
    const KhPlan &p = e->plan;
    const int K = e->K, reduced_G = e->reduced_G;
    if (e->form.set()) {
        // pulse parametrizations and non-linear controls: the whole sweep of a register-tile engine on the tile kernel's
        // form for them while its K workgroups are all resident (launch_update: else the generic form after all);
        // everything else -- other families, stepwise launches, reduced grids -- on the generic one
        const bool own_grid = reduced_G == 0 && world == 1 && e->sw.tile_single;  // (the SINGLE exchange on the plan's grid)
        const bool tile_operands = !e->mixed && e->d_csr_fw == nullptr && e->N <= KH_TILE_N && e->L >= 1 && e->L <= 4;
        return whole && p.tile_form(K) && own_grid && tile_operands ? ROUTE_TILE_FORM : ROUTE_GENERIC_FORM;
    }
    if (p.kind == KIND_LIND) return ROUTE_LIND;
    if (p.ens && whole) {
        // first order, four objectives per workgroup (512 < K <= 1024): the A^2 chain with the update sums on the adjoint
        // side (kh_ens2_forward_update; KH_ENS2=0: the term-by-term kernel, A/B switch and what second order and the other
        // column-group counts run -- with one column group it measured 2 % slower, with 4 and 8 its operands do not fit)
        int G = 0;
        const int ncg = p.ens_cols(K, reduced_G, &G);
        return !so && ncg == 2 && p.ens2 && e->d_sq_fw != nullptr && adj_store() ? ROUTE_ENS2 : ROUTE_ENS;
    }
    if (p.kind == KIND_ELL && p.ell_global && !stepwise) return ROUTE_ELL;  // (any grid: kh_ellg.h)
    if ((p.stream || (reduced_G > 0 && reduced_G < p.grid_update && world == 1)) && whole) return ROUTE_STREAM;
    if (p.kind == KIND_TILE_Q2 && p.quad && whole) return ROUTE_QUAD;
    if (p.kind == KIND_TILE_Q2 && p.mini && whole) return ROUTE_MINI;
    if (!stepwise) {
        switch (p.kind) {
            case KIND_TILE_Q2: return ROUTE_Q2;
            case KIND_COOP: return ROUTE_COOP;
            case KIND_TILEN: return ROUTE_TILEN;
            case KIND_ELL: return ROUTE_ELL;
            default: break;
        }
    }
    // One launch per interval (sharded sweep): every launch re-stages its operator tiles, so the q2 kernels (5 tiles,
    // 320 KiB per objective) lose to the plain tile kernel (2 tiles) there -- measured 39 vs ~20 us per interval.
    if (p.kind == KIND_TILE_RPT1 || p.kind == KIND_TILE_RPT2 || p.kind == KIND_TILE_Q2) return ROUTE_TILE;
    if (p.tx_update && whole && !so && reduced_G == 0 && p.grid_update >= K && adj_store()) return ROUTE_TILEX;
    return ROUTE_GENERIC;
}

// the ensemble kernels (ens2: the A^2 chain with the sums on the adjoint side)
static int update_ens(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st, bool ens2) {
    KhExchange exe = ex;
    const int ncg = e->plan.ens_cols(e->K, e->reduced_G, &exe.G);
    KhEnsArgs en;
    en.H0 = e->ens_H0;
    en.H1 = e->ens_H1;
    en.scale = e->d_ens_scale;
    e->last_update_grid = exe.G;
    if (ens2) {
        KH_TRY(gen_adjoint_side(e, u.chi_store, 1, st));
        KhUpdateArgs ua = u;
        ua.adj_store = e->d_gen_adj;
        // (the interval's first pass sits between the sums' stores and the first poll: no head start on top -- 16.08 -> 15.75 us)
        if (!e->sw.poll_delay_set) exe.first_poll_delay = 0;
        return launch_persistent_lds<kh_ens2_forward_update<2>>(e, dim3(exe.G), dim3(KH_ENS_THREADS), kh_ens2_lds_bytes(ncg), st, p, en,
                                                                e->d_sq_fw, ua, exe);
    }
    return with_ens(ncg, [&](auto c) {
        return with_bool(u.sigma != nullptr, [&](auto s) {
            constexpr int NCG = decltype(c)::value;
            return launch_persistent<kh_ens_forward_update<NCG, decltype(s)::value>>(e, dim3(exe.G), dim3(KH_ENS_THREADS),
                                                                                     kh_ens_lds_bytes(NCG), st, p, en, u, exe);
        });
    });
}

// more objectives than co-resident workgroups -- or (kh_set_update_workgroups) fewer workgroups than the register-tile
// family of this engine would use: G workgroups walk through K / G objectives each (kh_tile64s.h)
static int update_stream(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st) {
    int G = e->plan.stream ? e->plan.stream_G : e->plan.grid_update;
    if (e->reduced_G > 0 && e->reduced_G < G) G = e->reduced_G;
    KhExchange exs = ex;
    exs.G = G;
    exs.world = 1;
    e->last_update_grid = G;
    return with_tile_L(e->L, [&](auto lt) {
        return with_bool(u.sigma != nullptr, [&](auto so) {
            return with_bool(e->N == KH_TILE_N, [&](auto n64) {
                return launch_persistent<kh_stream_forward_update<decltype(lt)::value, decltype(so)::value, decltype(n64)::value>>(
                    e, dim3(G), dim3(512), 0, st, p, u, exs);
            });
        });
    });
}

static int update_mini(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st, bool quad) {
    return with_bool(u.sigma != nullptr, [&](auto so) {
        constexpr bool SO = decltype(so)::value;
        if (quad)
            launch_plain<kh_quad_forward_update<SO>>(dim3(1), dim3(64), 0, st, p, e->d_sq_fw, u, ex);
        else
            launch_plain<kh_mini_forward_update<SO>>(dim3(1), dim3(64 * e->K), 0, st, p, e->d_sq_fw, u, ex);
        return KH_OK;
    });
}

static int update_q2(kh_engine *e, const KhSweepArgs &p_in, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st) {
    const KhSweepArgs p = sweep_args_q2(e, p_in);
    const dim3 g(e->K), b(KH_Q2_THREADS);
    const size_t lds = kh_q2_lds_bytes();
    // (KH_Q2_SINGLE=0: the instantiations with the cross-GPU stage on one GPU too -- A/B switch)
    const bool single = ex.world == 1 && e->sw.q2_single;
    if (u.sigma != nullptr)
        return single ? launch_persistent<kh_q2_forward_update<true, false, true>>(e, g, b, lds, st, p, e->d_sq_fw, u, ex)
                      : launch_persistent<kh_q2_forward_update<true, false>>(e, g, b, lds, st, p, e->d_sq_fw, u, ex);
    if (u.adj_sign != 0.0) {
        KhExchange exa = ex;
        exa.first_poll_delay = e->sw.adj_poll_delay;
        // (the default form on one GPU: an instantiation without the cross-GPU stage)
        return single ? launch_persistent<kh_q2_forward_update<false, true, true>>(e, g, b, lds, st, p, e->d_sq_fw, u, exa)
                      : launch_persistent<kh_q2_forward_update<false, true>>(e, g, b, lds, st, p, e->d_sq_fw, u, exa);
    }
    return single ? launch_persistent<kh_q2_forward_update<false, false, true>>(e, g, b, lds, st, p, e->d_sq_fw, u, ex)
                  : launch_persistent<kh_q2_forward_update<false, false>>(e, g, b, lds, st, p, e->d_sq_fw, u, ex);
}

static int update_tilen(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st) {
    const bool so = u.sigma != nullptr;
    // first order with the control operators NOT in registers (several controls, or N > 96): the update sums on the
    // adjoint side, H_lk^+ chi_k for the whole store in front of the sweep (kh_generic.h, kh_gen_adjoint_side) instead
    // of L streamed control products per interval (N = 100, L = 6: 60 of the update sweep's 106 us per interval)
    KhUpdateArgs ut = u;
    if (!so && !e->plan.tn_h1reg && ensure_gen_adj(e)) {
        KH_TRY(gen_adjoint_side(e, u.chi_store, e->L, st));
        ut.adj_store = e->d_gen_adj;
    }
    // (several waves poll side by side: a later first poll, as for the tile64x kernels -- N = 100, L = 6: 68.8 -> 64.9 us per
    // interval, N = 81, L = 4: 38.2 -> 35.5; KH_POLL_DELAY overrides)
    KhExchange ext = ex;
    if (!e->sw.poll_delay_set && e->L >= 2) ext.first_poll_delay = e->L == 2 ? 32 : 64;
    return with_tn(e->plan.tn_EP, e->plan.tn_h1reg, [&](auto ep, auto hr) {
        return with_bool(so, [&](auto s) {
            return launch_persistent<kh_tn_forward_update<decltype(ep)::value, decltype(s)::value, decltype(hr)::value>>(
                e, dim3(e->K), dim3(KH_TN_THREADS), kh_tn_lds_bytes(), st, p, (const cplx *const *)e->d_tn_fw, ut, ext);
        });
    });
}

// the padded-row form with its vectors in global memory (kh_ellg.h): a workgroup takes its objectives in turns, so the
// grid is min(K, #CUs) or what kh_set_update_workgroups allows
static int update_ellg(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st) {
    const int S = e->row_split;
    const bool split = S > 1;  // the split form: every workgroup of every group takes part in the exchange
    int G = split ? e->split_groups * S : e->plan.grid_update;
    if (!split && e->reduced_G > 0 && e->reduced_G < G) G = e->reduced_G;
    if (split) {
        KH_HIP(hipMemsetAsync(e->d_split_counters, 0, e->split_counters_bytes, st));
    }
    KhExchange exg = ex;
    exg.G = G;
    e->last_update_grid = G;
    return with_bool(u.sigma != nullptr, [&](auto so) {
        constexpr bool SO = decltype(so)::value;
        auto shared = [&](auto launch) {  // what both forms are launched with
            return launch(e, dim3(G), dim3(KH_ELLG_THREADS), kh_ellg_lds_bytes(split), st, p, (const KhEll *)e->d_ell_fw,
                          (const int *)e->d_ell_off, (const cplx *)e->d_ell_vals, u, exg, e->d_ellg_ws, e->ellg_ws_stride);
        };
        if (split)
            return shared([&](auto... a) {
                return launch_persistent<kh_ellgs_forward_update<KH_ELLG_THREADS, SO>>(a..., S, e->d_split_counters);
            });
        return shared([](auto... a) { return launch_persistent<kh_ellg_forward_update<KH_ELLG_THREADS, SO>>(a...); });
    });
}

static int update_ell(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st) {
    if (e->plan.ell_global) return update_ellg(e, p, u, ex, st);
    const size_t lds = kh_ell_lds_bytes(e->plan.ell_stream);
    return with_ell(e->N, e->plan.ell_E, e->plan.ell_stream, [&](auto t, auto r, auto em, auto stm) {
        return with_bool(u.sigma != nullptr, [&](auto so) {
            constexpr int T = decltype(t)::value;
            return launch_persistent_lds<kh_ell_forward_update<T, decltype(r)::value, decltype(em)::value, decltype(so)::value, decltype(stm)::value>>(
                e, dim3(e->K), dim3(T), lds, st, p, (const KhEll *)e->d_ell_fw, (const int *)e->d_ell_off, (const cplx *)e->d_ell_vals, u, ex,
                e->d_ell_scratch, e->ell_scratch_stride);
        });
    });
}

// The register-tile update kernels' first poll with several controls: L waves gather side by side (kh_tile64.h) and a failed
// polling round costs L times the loads, so the stores get a longer head start -- measured best on config-5 shapes:
// 24 / 28 / 32 x 64 cycles for L = 2 / 3 / 4 (update sweep 7.47 / - / 9.86 us per interval against 7.92 / - / 11.21 with 16);
// KH_POLL_DELAY overrides
template <int LT>
static KhExchange tile_exchange(const kh_engine *e, KhExchange ex) {
    if (LT >= 2 && !e->sw.poll_delay_set) ex.first_poll_delay = 24 + 4 * (LT - 2);
    return ex;
}

template <int RPT, int LT>
static int launch_tile_update(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex,
                              hipStream_t st) {
    constexpr size_t lds = KhTileLds<RPT, LT>::bytes(KhTileLds<RPT, LT>::UPDATE);
    const dim3 g(e->K), b(512 / RPT);
    return with_bool(u.sigma != nullptr, [&](auto so) {
        constexpr bool SO = decltype(so)::value;
        if (!u.internal_exchange)  // one launch per interval (sharded sweep): nothing waits inside the kernel
            return launch_plain_lds<kh_tile_forward_update<RPT, LT, SO>>(e, g, b, lds, st, p, u, ex);
        const KhExchange exl = tile_exchange<LT>(e, ex);
        if (exl.world == 1 && exl.G > 1 && e->sw.tile_single)
            return launch_persistent_lds<kh_tile_forward_update<RPT, LT, SO, true>>(e, g, b, lds, st, p, u, exl);
        return launch_persistent_lds<kh_tile_forward_update<RPT, LT, SO>>(e, g, b, lds, st, p, u, exl);
    });
}

static KhParArgs par_args(const kh_engine *e) {
    return KhParArgs{e->form.dfdu, e->form.u_opt, e->form.d_kind, e->form.d_ab, e->form.d_ab + e->L};
}

static KhNlArgs nl_args(const kh_engine *e) {
    return KhNlArgs{e->form.dcde, e->form.d_tab, e->form.d_tab + e->L, e->form.C};
}

// the register-tile kernel's form with pulse parametrizations or non-linear controls (LT: its terms): one launch over the
// sweep, one GPU, K > 1 resident workgroups (update_route)
template <int RPT, int LT>
static int launch_tile_update_form(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex,
                                   hipStream_t st) {
    constexpr size_t lds = KhTileLds<RPT, LT>::bytes(KhTileLds<RPT, LT>::UPDATE);
    const dim3 g(e->K), b(512 / RPT);
    const KhExchange exl = tile_exchange<LT>(e, ex);
    e->last_update_grid = e->K;
    return with_bool(u.sigma != nullptr, [&](auto so) {
        constexpr bool SO = decltype(so)::value;
        if (e->form.tag == FORM_NL)
            return launch_persistent_lds<kh_tile_forward_update_nl<RPT, LT, SO>>(e, g, b, lds, st, p, u, exl, nl_args(e));
        return launch_persistent_lds<kh_tile_forward_update_par<RPT, LT, SO>>(e, g, b, lds, st, p, u, exl, par_args(e));
    });
}

// The generic update kernel `Kernel` -- update_generic names it -- with the arguments `form_args` of its form behind the
// shared ones.  With a form set every update sweep that is not the tile kernel's comes here, whatever the engine's family:
// the single launch then runs on min(K, max_wgs) workgroups (or what kh_set_update_workgroups allows), each taking its
// objectives in turns.
template <auto Kernel, class... FormArgs>
static int launch_gen_update(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex_in, hipStream_t st,
                             const KhMixedArgs &mx, FormArgs... form_args) {
    const size_t lds = kh_gen_lds_bytes(e->N, e->d_csr_fw == nullptr);
    const int rc = ensure_dynamic_lds(e, (const void *)Kernel, lds);
    int G = 0;
    const KhSweepArgs pg = gen_sweep_args(e, p, true, &G);
    if (rc != KH_OK) return rc;
    // first order, dense operators: V_lk = H_lk^+ chi_k for the whole store in front of the sweep -- at the sweep's first
    // launch (the single launch, or kh_update_begin's); the launches of a stepwise sweep that follow reuse it
    KhUpdateArgs ug = u;
    const bool first_launch = u.internal_exchange || (u.n_dev == nullptr && u.n_begin == 0 && u.n_end == 0);
    if (first_launch) {
        e->gen_adj_ready = false;
        if (u.sigma == nullptr && e->d_csr_fw == nullptr && ensure_gen_adj(e)) {
            KH_TRY(gen_adjoint_side(e, u.chi_store, e->L, st));
            e->gen_adj_ready = true;
        }
    }
    if (e->gen_adj_ready && u.sigma == nullptr) ug.adj_store = e->d_gen_adj;
    KhExchange ex = ex_in;
    if (e->form.set() && ug.internal_exchange) {
        // (an engine of another family may hold more workgroups than the exchange of this kernel takes, or fewer
        // were asked for: the workgroups walk through the objectives)
        if (G > e->plan.max_wgs) G = e->plan.max_wgs;
        if (e->reduced_G > 0 && e->reduced_G < G) G = e->reduced_G;
        ex.G = G;
        ex.world = 1;
        e->last_update_grid = G;
    }
    const dim3 g(G), b(KH_GEN_THREADS);
    if (ug.internal_exchange) return launch_persistent<Kernel>(e, g, b, lds, st, pg, ug, ex, mx, form_args...);
    launch_plain<Kernel>(g, b, lds, st, pg, ug, ex, mx, form_args...);
    return KH_OK;
}

static int update_generic(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st) {
    if (!e->gen_fits)
        return kh_fail(KH_ERR_UNSUPPORTED, "N=%d: this form of the update sweep needs the generic kernels, whose vectors do not fit LDS", e->N);
    return with_bool(e->mixed, [&](auto mixed) {
        constexpr bool MIXED = decltype(mixed)::value;
        const KhMixedArgs mx = MIXED ? e->mixed_fw : KhMixedArgs{};
        switch (e->form.tag) {
            case FORM_PAR: return launch_gen_update<kh_gen_forward_update_par<MIXED>>(e, p, u, ex, st, mx, par_args(e));
            case FORM_NL: return launch_gen_update<kh_gen_forward_update_nl<MIXED>>(e, p, u, ex, st, mx, nl_args(e));
            default: return launch_gen_update<kh_gen_forward_update<MIXED>>(e, p, u, ex, st, mx);
        }
    });
}

// five to eight controls, N <= 64, one resident workgroup per objective, first order: the register-tile form with
// streamed operators (kh_tile64x.h); V_lk = H_lk^+ chi_k for the whole store in front of the sweep
static int update_tilex(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st) {
    KH_TRY(gen_adjoint_side(e, u.chi_store, e->L, st));
    KhUpdateArgs ux = u;
    ux.adj_store = e->d_gen_adj;
    KhExchange exx = ex;
    exx.G = e->K;
    // (five to eight waves poll side by side: their first poll later than the register-tile kernels' -- measured best at
    // K = 256, N = 64: 32 / 44 / 64 / 64 for L = 5 / 6 / 7 / 8, profiles/r06/ab_tile64x.txt; KH_POLL_DELAY overrides)
    if (!e->sw.poll_delay_set) exx.first_poll_delay = e->L <= 5 ? 32 : e->L == 6 ? 44 : 64;
    e->last_update_grid = e->K;
    return with_tx(e->L, [&](auto lt) {
        return launch_persistent_lds<kh_tx_forward_update<decltype(lt)::value>>(e, dim3(e->K), dim3(KH_TX_THREADS), kh_tx_lds_bytes(), st, p,
                                                                                (const cplx *const *)e->d_tx_fw, ux, exx);
    });
}

// Lindblad form (kh_lind.h): first order, the whole sweep in one launch
static int update_lind(kh_engine *e, const KhSweepArgs &p, const KhUpdateArgs &u, const KhExchange &ex, hipStream_t st) {
    if (u.sigma != nullptr || !u.internal_exchange)
        return kh_fail(KH_ERR_UNSUPPORTED, "the Lindblad-form kernels run the first-order update sweep in one launch only");
    const KhLindArgs la = e->lind_fw;
    return with_lind(la.d, [&](auto rb) {
        return launch_persistent_lds<kh_lind_forward_update<decltype(rb)::value>>(e, dim3(e->plan.grid_update), dim3(KH_LIND_THREADS),
                                                                                  kh_lind_lds_bytes(la.d, la.n_c, la.nw), st, p, la, u, ex);
    });
}

static int launch_update(kh_engine *e, const KhUpdateArgs &u, hipStream_t st) {
    const KhSweepArgs p = sweep_args(e, false);
    const KhExchange ex = exchange_args(e, u.internal_exchange != 0);
    if (u.internal_exchange) KH_HIP(hipMemsetAsync(e->d_slots, 0, e->slots_bytes, st));
    if (u.internal_exchange && ex.world > 1) KH_HIP(hipMemsetAsync(e->d_wait_ticks, 0, 2 * sizeof(unsigned long long), st));
    const bool stepwise = !u.internal_exchange;
    const bool whole = !stepwise && u.n_begin == 0 && u.n_end == e->nt - 1;
    e->last_update_grid = 0;
    int rc = KH_OK;
    switch (update_route(e, stepwise, whole, u.sigma != nullptr, ex.world, [e] { return ensure_gen_adj(e); })) {
        case ROUTE_ENS: rc = update_ens(e, p, u, ex, st, false); break;
        case ROUTE_ENS2: rc = update_ens(e, p, u, ex, st, true); break;
        case ROUTE_STREAM: rc = update_stream(e, p, u, ex, st); break;
        case ROUTE_QUAD: rc = update_mini(e, p, u, ex, st, true); break;
        case ROUTE_MINI: rc = update_mini(e, p, u, ex, st, false); break;
        case ROUTE_Q2: rc = update_q2(e, p, u, ex, st); break;
        case ROUTE_COOP:
            rc = with_coop(e->plan.coop_cols, e->plan.coop_ks, [&](auto ks, auto cols) {
                return launch_coop_update<decltype(ks)::value, decltype(cols)::value>(e, p, u, ex, st);
            });
            break;
        case ROUTE_TILEN: rc = update_tilen(e, p, u, ex, st); break;
        case ROUTE_ELL: rc = update_ell(e, p, u, ex, st); break;
        case ROUTE_TILE:
            rc = with_tile(e->plan.kind == KIND_TILE_RPT2, e->L, [&](auto rpt, auto lt) {
                return launch_tile_update<decltype(rpt)::value, decltype(lt)::value>(e, p, u, ex, st);
            });
            break;
        case ROUTE_TILEX: rc = update_tilex(e, p, u, ex, st); break;
        case ROUTE_LIND: rc = update_lind(e, p, u, ex, st); break;
        case ROUTE_TILE_FORM:
            rc = with_tile(e->plan.kind == KIND_TILE_RPT2, e->L, [&](auto rpt, auto lt) {
                return launch_tile_update_form<decltype(rpt)::value, decltype(lt)::value>(e, p, u, ex, st);
            });
            if (rc != KH_ERR_UNSUPPORTED) break;  // (unsupported: the grid cannot be resident -- the generic form takes the sweep)
            [[fallthrough]];
        case ROUTE_GENERIC_FORM:  // (update_generic takes the form's kernel)
        case ROUTE_GENERIC: rc = update_generic(e, p, u, ex, st); break;
    }
    if (rc != KH_OK) return rc;
    KH_HIP(hipGetLastError());
    return KH_OK;
}

static KhUpdateArgs update_args(kh_engine *e, const kh_cdouble *chi_store, const double *chi_norms,
                                const double *guess, const double *shape, const double *lambda, double *opt,
                                double *g_a) {
    KhUpdateArgs u;
    u.mu_re = e->is_super ? 0.0 : 1.0;  // mu.py:130-134
    u.mu_im = e->is_super ? 1.0 : 0.0;
    u.chi_store = (const cplx *)chi_store;
    u.chi_norms = chi_norms;
    u.phi = e->d_phi;
    u.guess = guess;
    u.shape = shape;
    u.lambda = lambda;
    u.opt = opt;
    u.g_a = g_a;
    u.wg_partial = e->d_wg_partial;
    u.D_in = nullptr;
    u.n_dev = nullptr;
    u.fw_prev = e->so.fw_prev;
    u.fw_store = e->so.fw_store;
    u.sigma = e->so.sigma;
    u.n_begin = 0;
    u.n_end = e->nt - 1;
    u.internal_exchange = 1;
    u.adj_sign = e->adj_sign;
    u.adj_store = nullptr;
    if (e->form.tag == FORM_PAR) u.guess = e->form.u_guess;  // (the sweep updates u; eps = f(u) goes to `opt`)
    return u;
}

// One interval per launch (no in-kernel exchange): [n_begin, n_end) or, with n_dev, the interval read on the device;
// then, if `reduce`, the workgroups' sums summed in a fixed order into `partial`
static int update_interval(kh_engine *e, KhUpdateArgs u, const double *D, int n_begin, int n_end, int32_t *n_dev,
                           double *partial, bool reduce, hipStream_t st) {
    u.internal_exchange = 0;
    u.D_in = D;
    u.n_dev = n_dev;
    u.n_begin = n_begin;
    u.n_end = n_end;
    KH_TRY(launch_update(e, u, st));
    if (!reduce) return KH_OK;
    kh_reduce_partials<<<1, 64, 0, st>>>(e->d_wg_partial, e->plan.grid_update, e->L, partial, n_dev);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

extern "C" int kh_forward_update(kh_engine *e, const kh_cdouble *chi_store_dev, const double *chi_norms_dev,
                                 const kh_cdouble *init_dev, const double *guess_dev, const double *shape_dev,
                                 const double *lambda_dev, double *opt_dev, kh_cdouble *psi_T_dev, double *g_a_dev,
                                 void *stream) {
    if (e == nullptr || chi_store_dev == nullptr || chi_norms_dev == nullptr || init_dev == nullptr ||
        guess_dev == nullptr || shape_dev == nullptr || lambda_dev == nullptr || opt_dev == nullptr ||
        psi_T_dev == nullptr || g_a_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    if (e->L < 1) return kh_fail(KH_ERR_INVALID, "no controls to update");
    if (opt_dev == guess_dev) return kh_fail(KH_ERR_INVALID, "opt_dev must not alias guess_dev");
    hipStream_t st = (hipStream_t)stream;
    if (e->replicas > 0) {
        // replica engines (kh_replica.h): one workgroup per replica, wave w = objective b K_r + w; the kernel reads init_dev
        // and writes psi_T_dev itself, so that an inactive replica's rows keep what they held
        KH_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(double) * 4, st));
        const KhUpdateArgs u = update_args(e, chi_store_dev, chi_norms_dev, guess_dev, shape_dev, lambda_dev, opt_dev, g_a_dev);
        const KhSweepArgs p = sweep_args(e, false);
        KH_TRY(with_tile_L(e->L, [&](auto lt) {
            constexpr int LT = decltype(lt)::value;
            if (u.sigma != nullptr)  // second order: kh_set_second_order_replicas
                launch_plain<kh_rep_forward_update_so<LT>>(dim3(e->replicas), dim3(64 * e->Kr), 0, st, p, e->d_sq_fw, u,
                                                           (const cplx *)init_dev, (cplx *)psi_T_dev, e->Kr, e->active_mask());
            else
                launch_plain<kh_rep_forward_update<LT>>(dim3(e->replicas), dim3(64 * e->Kr), 0, st, p, e->d_sq_fw, u,
                                                        (const cplx *)init_dev, (cplx *)psi_T_dev, e->Kr, e->active_mask());
            return KH_OK;
        }));
        KH_HIP(hipGetLastError());
        e->last_intervals = e->nt - 1;
        e->last_wgs = e->replicas;
        return KH_OK;
    }
    if (e->plan.per_interval()) {
        // one launch per interval; on one GPU the "all-reduced" sums are the local ones (kh_reduce_partials has
        // summed the workgroups' pieces in a fixed order)
        KH_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(double) * 4, st));
        int rc = kh_update_begin(e, chi_store_dev, chi_norms_dev, init_dev, guess_dev, opt_dev, g_a_dev,
                                 e->d_step_partial, stream);
        for (int n = 0; rc == KH_OK && n < e->nt - 1; ++n)
            rc = kh_update_step(e, n, e->d_step_partial, chi_store_dev, chi_norms_dev, shape_dev, lambda_dev, opt_dev,
                                g_a_dev, e->d_step_partial, stream);
        if (rc == KH_OK) rc = kh_update_end(e, psi_T_dev, stream);
        e->last_intervals = e->nt - 1;
        e->last_wgs = e->plan.grid_update;
        return rc;
    }
#ifdef KH_TIMING
    KH_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(double) * 68, st));
#else
    KH_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(double) * 4, st));
#endif
    KH_HIP(hipMemcpyAsync(e->d_phi, init_dev, sizeof(cplx) * (size_t)e->K * e->N, hipMemcpyDeviceToDevice, st));
    KhUpdateArgs u =
        update_args(e, chi_store_dev, chi_norms_dev, guess_dev, shape_dev, lambda_dev, opt_dev, g_a_dev);
    KH_TRY(launch_update(e, u, st));
    if (e->p2p_ready) {
        e->p2p_epoch_base += (unsigned int)e->nt;  // every rank advances identically
        e->p2p_sweeps += 1;
    }
    KH_HIP(hipMemcpyAsync(psi_T_dev, e->d_phi, sizeof(cplx) * (size_t)e->K * e->N, hipMemcpyDeviceToDevice, st));
    e->last_intervals = e->nt - 1;
    e->last_wgs = e->last_update_grid > 0 ? e->last_update_grid : e->plan.grid_update;
    return KH_OK;
}

// Fewer workgroups for the single-launch update sweep: what a caller asks for after KH_ERR_TIMEOUT (co-tenants hold
// compute units, so the sweep's workgroups were not all resident at once) before it gives up on the single launch.
extern "C" int kh_set_update_workgroups(kh_engine *e, int32_t max_workgroups, int32_t *chosen) {
    if (e == nullptr || max_workgroups < 0) return kh_fail(KH_ERR_INVALID, "bad argument");
    if (chosen != nullptr) *chosen = e->plan.single_grid();
    if (e->row_split > 1 && chosen != nullptr) *chosen = e->split_groups * e->row_split;
    if (max_workgroups == 0) {
        e->reduced_G = 0;
        e->form.reduced = false;
        return KH_OK;
    }
    if (e->replicas > 0) return kh_fail(KH_ERR_UNSUPPORTED, "replica engines (kh_engine_create_replicas) run one workgroup per replica: no form with fewer workgroups");
    if (e->row_split > 1) return kh_fail(KH_ERR_UNSUPPORTED, "a split engine (kh_set_row_split) keeps its own grid: set the row split to 1 first");
    if (e->lind) return kh_fail(KH_ERR_UNSUPPORTED, "Lindblad-form engines (kh_engine_create_lindblad) have no form with fewer workgroups");
    if (e->p2p_ready) return kh_fail(KH_ERR_UNSUPPORTED, "sharded sweeps keep their grid (all ranks must agree on the form)");
    const KhPlan &p = e->plan;
    int G = 0;
    if (e->form.set()) {
        // a parametrized or non-linear engine (kh_set_parametrization, kh_set_nonlinear): the generic kernels take their objectives in turns on any grid
        G = p.grid_update < p.max_wgs ? p.grid_update : p.max_wgs;
        if (max_workgroups < G) G = max_workgroups;
        e->form.reduced = true;  // (not a grid the engine's own family was asked about: dropped with the form)
    } else if (p.ens) {
        const int widest = (e->K + 2 * KH_ENS_MAXCG - 1) / (2 * KH_ENS_MAXCG);
        if (max_workgroups < widest)
            return kh_fail(KH_ERR_UNSUPPORTED, "the ensemble kernel needs at least %d workgroups for %d objectives", widest, e->K);
        const void *forms[2];
        KH_TRY(ens_forms(e, p.ens_cols(e->K, max_workgroups, &G), forms));
    } else if (p.kind == KIND_ELL && p.ell_global) {
        const int fewest = (e->K + KH_ELLG_MMAX - 1) / KH_ELLG_MMAX;
        if (max_workgroups < fewest)
            return kh_fail(KH_ERR_UNSUPPORTED, "%d objectives need at least %d workgroups (%d per workgroup)", e->K, fewest, KH_ELLG_MMAX);
        G = p.grid_update < max_workgroups ? p.grid_update : max_workgroups;
    } else {
        if (!p.tile_family() || e->d_csr_fw != nullptr || e->N > KH_TILE_N || e->L < 1 || e->L > 4)
            return kh_fail(KH_ERR_UNSUPPORTED, "only the register-tile families (N <= 64, 1..4 controls) and the sparse form with global vectors have a form with fewer workgroups");
        const int fewest = (e->K + KH_STREAM_MMAX - 1) / KH_STREAM_MMAX;
        if (max_workgroups < fewest)
            return kh_fail(KH_ERR_UNSUPPORTED, "%d objectives need at least %d workgroups (%d per workgroup)", e->K, fewest, KH_STREAM_MMAX);
        G = p.stream ? p.stream_G : p.grid_update;
        if (max_workgroups < G) G = max_workgroups;
    }
    e->reduced_G = max_workgroups;
    if (chosen != nullptr) *chosen = G;
    return KH_OK;
}

// 'auto': the largest power of two <= min(CUs / K, chunks / 8, 64); 1 where N <= 4096.  The N floor and the chunks / 8
// term (at least 512 rows per part) are PLACEHOLDERS until scripts/perf_ellsplit.py has been run.
static int kh_row_split_auto(int num_cus, int K, int N) {
    if (N <= 4096 || K < 1) return 1;
    const int chunks = (int)(kh_ellg_rows(N) / 64);
    int cap = num_cus / K;
    if (chunks / 8 < cap) cap = chunks / 8;
    if (cap > 64) cap = 64;
    int S = 1;
    while (2 * S <= cap) S *= 2;
    return S;
}

extern "C" int kh_ellsplit_rows(int32_t N, int32_t S, int32_t part, int32_t *first, int32_t *count) {
    if (first == nullptr || count == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    if (N < 1 || N > KH_ELLG_NMAX || S < 1 || part < 0 || part >= S) return kh_fail(KH_ERR_INVALID, "bad N = %d, S = %d or part = %d", N, S, part);
    int f = 0, c = 0;
    kh_ellsplit_range(N, S, part, &f, &c);
    *first = f;
    *count = c;
    return KH_OK;
}

// S workgroups per objective for both sweeps of a CSR engine in the global form (kh_ellg.h's split form); 1: its plain form
extern "C" int kh_set_row_split(kh_engine *e, int workgroups_per_objective) {
    if (e == nullptr) return kh_fail(KH_ERR_INVALID, "null engine");
    const int S = workgroups_per_objective;
    if (!(e->plan.kind == KIND_ELL && e->plan.ell_global && e->d_csr_fw != nullptr))
        return kh_fail(KH_ERR_UNSUPPORTED, "only sparse (CSR) engines in the form with global vectors (\"ellglobal/csr\") split an objective's rows; this one runs %s", kh_engine_kernel(e));
    if (S < 1) return kh_fail(KH_ERR_UNSUPPORTED, "%d workgroups per objective: at least 1", S);
    if (S == 1) {
        e->row_split = 1;
        return KH_OK;
    }
    if (e->form.set()) return kh_fail(KH_ERR_UNSUPPORTED, "%s keeps one workgroup per objective", kh_form_words[e->form.tag].engine);
    const int max_wgs = e->plan.max_wgs;  // (what the exchange takes: at most 256, at most one per CU)
    if (S > e->num_cus || S > max_wgs)
        return kh_fail(KH_ERR_UNSUPPORTED, "%d workgroups per objective: this device runs at most %d at once", S, e->num_cus < max_wgs ? e->num_cus : max_wgs);
    const int chunks = (int)(kh_ellg_rows(e->N) / 64);
    if (S > chunks && chunks == 1 && S > 64)
        return kh_fail(KH_ERR_UNSUPPORTED, "%d workgroups per objective for one 64-row chunk: every part but one would be empty", S);
    if (e->p2p_ready) return kh_fail(KH_ERR_UNSUPPORTED, "sharded sweeps keep one workgroup per objective");
    if (e->reduced_G > 0) return kh_fail(KH_ERR_UNSUPPORTED, "the update sweep's grid was reduced (kh_set_update_workgroups): restore it first");
    int groups = e->K < max_wgs / S ? e->K : max_wgs / S;
    if (e->sw.ell_groups > 0 && e->sw.ell_groups < groups) groups = e->sw.ell_groups;
    if (groups > e->ellg_wgs) groups = e->ellg_wgs;  // (one workspace per group)
    if ((e->K + groups - 1) / groups > KH_ELLG_MMAX)
        return kh_fail(KH_ERR_UNSUPPORTED, "%d objectives on %d groups of %d workgroups: more than %d per group", e->K, groups, S, KH_ELLG_MMAX);
    const int Lx = e->L > 0 ? e->L : 1;
    const size_t slots = sizeof(kh_u64) * 2 * (size_t)groups * S * Lx * 2;
    if (slots > e->slots_bytes) {  // (the earlier block stays with the engine until it is destroyed)
        KH_TRY(dev_alloc(e, &e->d_slots, slots));
        e->slots_bytes = slots;
    }
    const size_t counters = (size_t)groups * KH_ELLGS_LINE;  // (a multiple of 16 bytes from its allocation's start)
    if (counters > e->split_counters_bytes) {
        KH_TRY(dev_alloc(e, &e->d_split_counters, counters));
        e->split_counters_bytes = counters;
    }
    e->row_split = S;
    e->split_groups = groups;
    return KH_OK;
}

// kh_set_second_order, and kh_set_second_order_replicas with one sigma row per replica ([B][nt-1]; kh_replica.h,
// kh_rep_forward_update_so)
static int set_second_order(kh_engine *e, const kh_cdouble *fw_prev_dev, kh_cdouble *fw_store_dev, const double *sigma_dev,
                            bool replicas) {
    if (e == nullptr) return kh_fail(KH_ERR_INVALID, "null engine");
    if (replicas && e->replicas < 1) return kh_fail(KH_ERR_UNSUPPORTED, "only replica engines (kh_engine_create_replicas) take one sigma row per replica; this one runs %s (kh_set_second_order)", kh_engine_kernel(e));
    const int given = (fw_prev_dev != nullptr) + (fw_store_dev != nullptr) + (sigma_dev != nullptr);
    if (given != 0 && given != 3)
        return kh_fail(KH_ERR_INVALID, "fw_prev, fw_store and sigma must be given together (or all NULL)");
    if (!replicas && e->lind && given != 0) return kh_fail(KH_ERR_UNSUPPORTED, "Lindblad-form engines (kh_engine_create_lindblad) run the first-order update only");
    if (!replicas && e->replicas > 0 && given != 0) return kh_fail(KH_ERR_UNSUPPORTED, "replica engines (kh_engine_create_replicas) run the first-order update only");
    if (fw_prev_dev != nullptr && (const void *)fw_prev_dev == (const void *)fw_store_dev)
        return kh_fail(KH_ERR_INVALID, "fw_store must not alias fw_prev");
    e->so = KhSecondOrder{(const cplx *)fw_prev_dev, (cplx *)fw_store_dev, sigma_dev};
    return KH_OK;
}

extern "C" int kh_set_second_order(kh_engine *e, const kh_cdouble *fw_prev_dev, kh_cdouble *fw_store_dev,
                                   const double *sigma_dev) {
    return set_second_order(e, fw_prev_dev, fw_store_dev, sigma_dev, false);
}

extern "C" int kh_set_second_order_replicas(kh_engine *e, const kh_cdouble *fw_prev_dev, kh_cdouble *fw_store_dev,
                                            const double *sigma_dev) {
    return set_second_order(e, fw_prev_dev, fw_store_dev, sigma_dev, true);
}

// What the two setters of a form refuse alike, in the words of the form asked for (kh_form_words)
static int refuse_form(const kh_engine *e, int tag) {
    const KhFormWords &w = kh_form_words[tag];
    if (e->lind) return kh_fail(KH_ERR_UNSUPPORTED, "Lindblad-form engines (kh_engine_create_lindblad) take no %s: build the Liouvillian and use kh_engine_create", w.noun);
    if (e->replicas > 0) return kh_fail(KH_ERR_UNSUPPORTED, "replica engines (kh_engine_create_replicas) take no %s", w.noun);
    if (e->p2p_ready || e->p2p_window != nullptr) return kh_fail(KH_ERR_UNSUPPORTED, "sharded engines take no %s (one GPU)", w.noun);
    if (e->row_split > 1) return kh_fail(KH_ERR_UNSUPPORTED, "a split engine (kh_set_row_split) takes no %s: set the row split to 1 first", w.noun);
    if (!e->gen_fits) return kh_fail(KH_ERR_UNSUPPORTED, "N=%d: %s run on the generic kernels, whose vectors do not fit LDS", e->N, w.plural);
    if (e->L < 1) return kh_fail(KH_ERR_INVALID, "%s", w.no_rows);
    if (e->form.set() && e->form.tag != tag) return kh_fail(KH_ERR_INVALID, "%s: the two are not combined", kh_form_words[e->form.tag].is_set);
    return KH_OK;
}

// a setter's "off": the form `tag` unset, and a reduced grid that was set while a form was on dropped with it
static void clear_form(kh_engine *e, int tag) {
    KhUpdateForm &f = e->form;
    if (f.tag == tag) {
        f.tag = FORM_LINEAR, f.C = 0;
        f.u_guess = f.dfdu = f.dcde = nullptr;
        f.u_opt = nullptr;
    }
    if (f.reduced) e->reduced_G = 0;
    f.reduced = false;
}

// The engine's own copy of a setter's host table: allocated at the first use, uploaded when it changes (an optimisation
// sets the same one before every sweep) -- a blocking copy behind a device-wide wait for an earlier sweep that may still
// read it
template <class T>
static int upload_table(kh_engine *e, T **dev, std::vector<T> &mirror, const std::vector<T> &host) {
    if (*dev == nullptr) KH_TRY(dev_alloc(e, dev, sizeof(T) * host.size()));
    if (host == mirror) return KH_OK;
    KH_HIP(hipDeviceSynchronize());
    KH_HIP(hipMemcpy(*dev, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice));
    mirror = host;
    return KH_OK;
}

// Pulse parametrizations eps_l = f_l(u_l) (include/krotov_hip.h): the following update sweeps update u and propagate with
// f(u) -- on the register-tile kernel's parametrized form or the generic kernels', by update_route's rule
extern "C" int kh_set_parametrization(kh_engine *e, const int32_t *kind, const double *a, const double *b,
                                      const double *u_guess_dev, const double *dfdu_dev, double *u_opt_dev) {
    if (e == nullptr) return kh_fail(KH_ERR_INVALID, "null engine");
    if (kind == nullptr) {
        clear_form(e, FORM_PAR);
        return KH_OK;
    }
    KH_TRY(refuse_form(e, FORM_PAR));
    if (a == nullptr || b == nullptr || u_guess_dev == nullptr || dfdu_dev == nullptr || u_opt_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    if (u_opt_dev == u_guess_dev) return kh_fail(KH_ERR_INVALID, "u_opt_dev must not alias u_guess_dev");
    for (int l = 0; l < e->L; ++l)
        if (kind[l] < KH_PAR_NONE || kind[l] > KH_PAR_TANH) return kh_fail(KH_ERR_INVALID, "control %d: unknown parametrization kind %d", l, (int)kind[l]);
    std::vector<double> ab(a, a + e->L);
    ab.insert(ab.end(), b, b + e->L);
    KhUpdateForm &f = e->form;
    KH_TRY(upload_table(e, &f.d_kind, f.kind_host, std::vector<int>(kind, kind + e->L)));
    KH_TRY(upload_table(e, &f.d_ab, f.ab_host, ab));
    f.tag = FORM_PAR, f.u_guess = u_guess_dev, f.dfdu = dfdu_dev, f.u_opt = u_opt_dev;
    return KH_OK;
}

// Non-linear controls (include/krotov_hip.h): the engine's L slots become terms eps_c^p H_j of C controls; the following
// update sweeps run kh_tile_forward_update_nl or kh_gen_forward_update_nl, by update_route's rule
extern "C" int kh_set_nonlinear(kh_engine *e, int32_t C, const int32_t *term_control, const int32_t *term_power,
                                const double *dcde_dev) {
    if (e == nullptr) return kh_fail(KH_ERR_INVALID, "null engine");
    if (term_control == nullptr) {
        clear_form(e, FORM_NL);
        return KH_OK;
    }
    KH_TRY(refuse_form(e, FORM_NL));
    if (term_power == nullptr || dcde_dev == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    if (C < 1 || C > e->L) return kh_fail(KH_ERR_INVALID, "%d controls for %d terms", (int)C, e->L);
    std::vector<int> tab(term_control, term_control + e->L);
    tab.insert(tab.end(), term_power, term_power + e->L);
    std::vector<bool> seen((size_t)C, false);
    for (int j = 0; j < e->L; ++j) {
        if (tab[j] < 0 || tab[j] >= C) return kh_fail(KH_ERR_INVALID, "term %d: control %d outside 0..%d", j, tab[j], (int)C - 1);
        if (tab[e->L + j] < 1 || tab[e->L + j] > 4) return kh_fail(KH_ERR_INVALID, "term %d: power %d outside 1..4", j, tab[e->L + j]);
        seen[(size_t)tab[j]] = true;
    }
    for (int c = 0; c < C; ++c)
        if (!seen[(size_t)c]) return kh_fail(KH_ERR_INVALID, "control %d has no term", c);
    KhUpdateForm &f = e->form;
    KH_TRY(upload_table(e, &f.d_tab, f.tab_host, tab));
    f.tag = FORM_NL, f.dcde = dcde_dev, f.C = C;
    return KH_OK;
}

// what the four kh_update_* entry points refuse
static int refuse_stepwise(const kh_engine *e) {
    if (e->lind) return kh_fail(KH_ERR_UNSUPPORTED, "Lindblad-form engines (kh_engine_create_lindblad) have no per-interval update sweep");
    if (e->replicas > 0) return kh_fail(KH_ERR_UNSUPPORTED, "replica engines (kh_engine_create_replicas) have no per-interval update sweep");
    return KH_OK;
}

// rows of the update sweep's pulse-like arrays: the C controls of kh_set_nonlinear (the pulses are rows of eps), else L
static int update_rows(const kh_engine *e) { return e->form.tag == FORM_NL ? e->form.C : e->L; }

extern "C" int kh_update_begin(kh_engine *e, const kh_cdouble *chi_store_dev, const double *chi_norms_dev,
                               const kh_cdouble *init_dev, const double *guess_dev, double *opt_dev,
                               double *g_a_dev, double *partial_dev, void *stream) {
    if (e == nullptr || chi_store_dev == nullptr || chi_norms_dev == nullptr || init_dev == nullptr ||
        guess_dev == nullptr || opt_dev == nullptr || g_a_dev == nullptr || partial_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    if (e->L < 1) return kh_fail(KH_ERR_INVALID, "no controls to update");
    KH_TRY(refuse_stepwise(e));
    hipStream_t st = (hipStream_t)stream;
    e->guess_dev = guess_dev;
    KH_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(double) * 4, st));
    KH_HIP(hipMemcpyAsync(e->d_phi, init_dev, sizeof(cplx) * (size_t)e->K * e->N, hipMemcpyDeviceToDevice, st));
    const int rows = update_rows(e);
    KH_HIP(hipMemcpyAsync(opt_dev, guess_dev, sizeof(double) * (size_t)rows * (e->nt - 1),
                          hipMemcpyDeviceToDevice, st));
    KH_HIP(hipMemsetAsync(g_a_dev, 0, sizeof(double) * rows, st));
    if (e->form.tag == FORM_PAR)
        KH_HIP(hipMemcpyAsync(e->form.u_opt, e->form.u_guess, sizeof(double) * (size_t)e->L * (e->nt - 1), hipMemcpyDeviceToDevice, st));
    const KhUpdateArgs u = update_args(e, chi_store_dev, chi_norms_dev, guess_dev, nullptr, nullptr, opt_dev, g_a_dev);
    return update_interval(e, u, nullptr, 0, 0, nullptr, partial_dev, true, st);
}

extern "C" int kh_update_step(kh_engine *e, int32_t n, const double *D_dev, const kh_cdouble *chi_store_dev,
                              const double *chi_norms_dev, const double *shape_dev, const double *lambda_dev,
                              double *opt_dev, double *g_a_dev, double *partial_dev, void *stream) {
    if (e == nullptr || D_dev == nullptr || chi_store_dev == nullptr || chi_norms_dev == nullptr ||
        shape_dev == nullptr || lambda_dev == nullptr || opt_dev == nullptr || g_a_dev == nullptr ||
        partial_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    KH_TRY(refuse_stepwise(e));
    if (e->guess_dev == nullptr) return kh_fail(KH_ERR_INVALID, "kh_update_begin was not called");
    if (n < 0 || n >= e->nt - 1) return kh_fail(KH_ERR_INVALID, "interval %d out of range", n);
    const KhUpdateArgs u = update_args(e, chi_store_dev, chi_norms_dev, e->guess_dev, shape_dev, lambda_dev, opt_dev, g_a_dev);
    return update_interval(e, u, D_dev, n, n + 1, nullptr, partial_dev, n + 1 < e->nt - 1, (hipStream_t)stream);
}

extern "C" int kh_update_step_dev(kh_engine *e, int32_t *n_dev, const double *D_dev,
                                  const kh_cdouble *chi_store_dev, const double *chi_norms_dev,
                                  const double *shape_dev, const double *lambda_dev, double *opt_dev,
                                  double *g_a_dev, double *partial_dev, void *stream) {
    if (e == nullptr || n_dev == nullptr || D_dev == nullptr || chi_store_dev == nullptr ||
        chi_norms_dev == nullptr || shape_dev == nullptr || lambda_dev == nullptr || opt_dev == nullptr ||
        g_a_dev == nullptr || partial_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    KH_TRY(refuse_stepwise(e));
    if (e->guess_dev == nullptr) return kh_fail(KH_ERR_INVALID, "kh_update_begin was not called");
    const KhUpdateArgs u = update_args(e, chi_store_dev, chi_norms_dev, e->guess_dev, shape_dev, lambda_dev, opt_dev, g_a_dev);
    return update_interval(e, u, D_dev, 0, 1, n_dev, partial_dev, true, (hipStream_t)stream);  // (n_begin: overridden on the device)
}

extern "C" int kh_update_end(kh_engine *e, kh_cdouble *psi_T_dev, void *stream) {
    if (e == nullptr || psi_T_dev == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    KH_TRY(refuse_stepwise(e));
    KH_HIP(hipMemcpyAsync(psi_T_dev, e->d_phi, sizeof(cplx) * (size_t)e->K * e->N, hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    e->guess_dev = nullptr;
    return KH_OK;
}

// ---------------------------------------------------------------------------
// cross-GPU exchange windows (sharded objectives, one rank per GPU)
// ---------------------------------------------------------------------------

// in-kernel ping-pong over the windows: every rank publishes (rank + round) and
// must read the same total from its own window
__global__ void kh_p2p_selftest_kernel(KhExchange ex, int L, int rounds, unsigned int epoch0, int *result) {
    const int lane = threadIdx.x;
    int ok_all = 1;
    long long t_first = 0;
    for (int r = 0; r < rounds; ++r) {
        if (r == 1) t_first = wall_clock64();  // (the first round absorbs the ranks' launch skew)
        double vals[KH_MAX_L], out[KH_MAX_L];
        for (int l = 0; l < KH_MAX_L; ++l) vals[l] = (double)(ex.rank + 1) * (l + 1) + 0.25 * r;
        const unsigned int epoch = epoch0 + (unsigned)r + 1u;
        kh_p2p_publish(ex, r & 1, L, lane, vals, epoch);
        if (!kh_p2p_gather<KH_MAX_L>(ex, r & 1, L, epoch, lane, out)) {
            ok_all = 0;
            break;
        }
        for (int l = 0; l < L; ++l) {
            const double want = (double)(ex.world * (ex.world + 1) / 2) * (l + 1) + 0.25 * r * ex.world;
            if (out[l] != want) ok_all = 0;
        }
    }
    if (lane == 0) *result = ok_all;
    if (lane == 0 && ex.wait_ticks != nullptr && rounds > 1) {  // publish -> all ranks' values read back, per round
        ex.wait_ticks[2] = (unsigned long long)(wall_clock64() - t_first);
        ex.wait_ticks[3] = (unsigned long long)(rounds - 1);
    }
}

extern "C" int kh_p2p_create_window(kh_engine *e, int32_t world, int32_t rank, unsigned char *ipc_handle_out) {
    if (e == nullptr || ipc_handle_out == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    if (world < 1 || rank < 0 || rank >= world) return kh_fail(KH_ERR_INVALID, "bad world/rank %d/%d", rank, world);
    if (e->mixed) return kh_fail(KH_ERR_UNSUPPORTED, "mixed engines (kh_engine_create_mixed) are not sharded");
    if (e->lind) return kh_fail(KH_ERR_UNSUPPORTED, "Lindblad-form engines (kh_engine_create_lindblad) are not sharded");
    if (e->replicas > 0) return kh_fail(KH_ERR_UNSUPPORTED, "replica engines (kh_engine_create_replicas) are not sharded");
    if (e->form.set()) return kh_fail(KH_ERR_UNSUPPORTED, "%s is not sharded", kh_form_words[e->form.tag].engine);
    const int Lx = e->L > 0 ? e->L : 1;
    if (world * Lx * 2 > 64 || Lx > KH_MAX_L)
        return kh_fail(KH_ERR_UNSUPPORTED, "world * L = %d exceeds the 32 exchange lanes (or more than %d controls)", world * Lx, KH_MAX_L);
    if (!e->plan.exchanges_in_kernel())  // (the caller falls back to kh_update_step + an all-reduce per interval)
        return kh_fail(KH_ERR_UNSUPPORTED, "%d objectives per GPU are not co-resident: no in-kernel exchange", e->K);
    if (e->p2p_window != nullptr) return kh_fail(KH_ERR_INVALID, "window already created");
    e->p2p_world = world;
    e->p2p_rank = rank;
    e->p2p_window_bytes = sizeof(kh_u64) * 2 * (size_t)world * Lx * 2;
    if (e->p2p_window_bytes < 4096) e->p2p_window_bytes = 4096;
    void *ptr = nullptr;
    // fine-grained (uncached, system-coherent) device memory for cross-GPU visibility
    hipError_t err = hipExtMallocWithFlags(&ptr, e->p2p_window_bytes, hipDeviceMallocFinegrained);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        KH_HIP(hipMalloc(&ptr, e->p2p_window_bytes));
    }
    e->p2p_window = (kh_u64 *)ptr;
    KH_HIP(hipMemset(ptr, 0, e->p2p_window_bytes));
    hipIpcMemHandle_t h;
    KH_HIP(hipIpcGetMemHandle(&h, ptr));
    static_assert(sizeof(hipIpcMemHandle_t) <= 64, "IPC handle larger than the ABI's 64 bytes");
    memset(ipc_handle_out, 0, 64);
    memcpy(ipc_handle_out, &h, sizeof(h));
    KH_HIP(hipDeviceSynchronize());
    return KH_OK;
}

extern "C" int kh_p2p_open_peers(kh_engine *e, const unsigned char *all_handles) {
    if (e == nullptr || all_handles == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    if (e->p2p_window == nullptr) return kh_fail(KH_ERR_INVALID, "kh_p2p_create_window was not called");
    std::vector<kh_u64 *> peers(e->p2p_world, nullptr);
    for (int r = 0; r < e->p2p_world; ++r) {
        if (r == e->p2p_rank) {
            peers[r] = e->p2p_window;
            continue;
        }
        hipIpcMemHandle_t h;
        memcpy(&h, all_handles + (size_t)r * 64, sizeof(h));
        void *ptr = nullptr;
        KH_HIP(hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess));
        e->p2p_opened.push_back(ptr);
        peers[r] = (kh_u64 *)ptr;
    }
    KH_HIP(hipMalloc((void **)&e->d_p2p_peers, sizeof(kh_u64 *) * e->p2p_world));
    KH_HIP(hipMemcpy((void *)e->d_p2p_peers, peers.data(), sizeof(kh_u64 *) * e->p2p_world, hipMemcpyHostToDevice));
    return KH_OK;
}

// Collective over all ranks (each calls it at the same point): returns KH_OK when
// `rounds` in-kernel exchanges over the windows produced the expected totals on
// THIS rank; the caller combines the verdicts of all ranks.  Marks the engine
// ready for the cross-GPU update sweep on success.
extern "C" int kh_p2p_selftest(kh_engine *e, int32_t rounds, void *stream) {
    if (e == nullptr) return kh_fail(KH_ERR_INVALID, "null engine");
    if (e->d_p2p_peers == nullptr) return kh_fail(KH_ERR_INVALID, "kh_p2p_open_peers was not called");
    hipStream_t st = (hipStream_t)stream;
    KhExchange ex;
    memset(&ex, 0, sizeof(ex));
    ex.abort_flag = e->d_abort;
    ex.timeout_ticks = 20000000LL;  // 0.2 s
    ex.peer_windows = e->d_p2p_peers;
    ex.my_window = e->p2p_window;
    ex.world = e->p2p_world;
    ex.rank = e->p2p_rank;
    ex.fail_at = -1;
    ex.wait_ticks = e->d_wait_ticks;
    int *d_res = nullptr;
    KH_HIP(hipMalloc(&d_res, sizeof(int)));
    KH_HIP(hipMemsetAsync(d_res, 0, sizeof(int), st));
    const int Lx = e->L > 0 ? e->L : 1;
    kh_p2p_selftest_kernel<<<1, 64, 0, st>>>(ex, Lx, rounds, e->p2p_epoch_base, d_res);
    KH_HIP(hipGetLastError());
    e->p2p_epoch_base += (unsigned int)rounds + 1u;
    int res = 0;
    KH_HIP(hipMemcpyAsync(&res, d_res, sizeof(int), hipMemcpyDeviceToHost, st));
    KH_HIP(hipStreamSynchronize(st));
    (void)hipFree(d_res);
    unsigned int flag = 0;
    KH_HIP(hipMemcpy(&flag, e->d_abort, sizeof(flag), hipMemcpyDeviceToHost));
    if (flag != 0) KH_HIP(hipMemset(e->d_abort, 0, sizeof(flag)));
    if (res != 1 || flag != 0) {
        e->p2p_ready = false;
        return kh_fail(KH_ERR_TIMEOUT, "cross-GPU exchange self-test failed on rank %d", e->p2p_rank);
    }
    e->p2p_ready = true;
    return KH_OK;
}

extern "C" int kh_p2p_stats(kh_engine *e, double out[4]) {
    if (e == nullptr || out == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    unsigned long long t[4] = {0, 0, 0, 0};
    KH_HIP(hipMemcpy(t, e->d_wait_ticks, sizeof(t), hipMemcpyDeviceToHost));
    const double n = e->last_intervals > 0 ? e->last_intervals : 1.0;
    out[0] = (double)t[0] * 0.01 / n;                       // 100 MHz ticks -> us
    out[1] = (double)t[1] * 0.01 / n;
    out[2] = t[3] > 0 ? (double)t[2] * 0.01 / (double)t[3] : 0.0;
    out[3] = (double)e->p2p_world;
    return KH_OK;
}

extern "C" int kh_p2p_disable(kh_engine *e) {
    if (e == nullptr) return kh_fail(KH_ERR_INVALID, "null engine");
    e->p2p_ready = false;
    return KH_OK;
}

extern "C" int kh_tau(kh_engine *e, const kh_cdouble *targets_dev, const kh_cdouble *psi_T_dev,
                      kh_cdouble *tau_dev, void *stream) {
    if (e == nullptr || targets_dev == nullptr || psi_T_dev == nullptr || tau_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    const int waves_per_block = 4;
    const int blocks = (e->K + waves_per_block - 1) / waves_per_block;
    kh_tau_kernel<<<blocks, 64 * waves_per_block, 0, (hipStream_t)stream>>>(
        (const cplx *)targets_dev, (const cplx *)psi_T_dev, (cplx *)tau_dev, e->K, e->N);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

// Expectation values of a stored trajectory (kh_expect.h): <psi|O|psi> on Hilbert-space engines, tr(O rho) on
// Liouville-space ones, KH_EXPECT_MAX_OPS operators per pass over the store.
extern "C" int kh_expect(kh_engine *e, const kh_cdouble *states_dev, const kh_cdouble *const *e_ops, int32_t n_e,
                         kh_cdouble *out_dev, void *stream) {
    if (e == nullptr || states_dev == nullptr || e_ops == nullptr || out_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    if (n_e < 1) return kh_fail(KH_ERR_INVALID, "n_e = %d: at least one operator", n_e);
    if (e->mixed)
        return kh_fail(KH_ERR_UNSUPPORTED, "mixed engines (kh_engine_create_mixed) have no expectation-value kernel: "
                                           "their objectives would need operators of their own dimensions");
    const bool super = e->is_super != 0;
    const int points = super ? KH_EXPECT_L_POINTS : KH_EXPECT_H_POINTS;
    const long long blocks = ((long long)e->nt + points - 1) / points;
    if (blocks > 65535) return kh_fail(KH_ERR_UNSUPPORTED, "nt = %d: more than 65535 blocks of %d time points", e->nt, points);
    hipStream_t st = (hipStream_t)stream;
    const size_t entries = (size_t)e->K * (size_t)n_e;
    if (entries > e->expect_tab_entries) {
        (void)hipFree((void *)e->d_expect_tab);  // (waits for whatever still reads it)
        e->d_expect_tab = nullptr, e->expect_tab_entries = 0;
        void *mem = nullptr;
        if (hipMalloc(&mem, entries * sizeof(cplx *)) != hipSuccess) {
            (void)hipGetLastError();
            return kh_fail(KH_ERR_NOMEM, "no device memory for a table of %zu operator pointers", entries);
        }
        e->d_expect_tab = (const cplx **)mem, e->expect_tab_entries = entries;
    }
    // (ordered on the stream behind an earlier call's kernels, which read the same table)
    KH_HIP(hipMemcpyAsync((void *)e->d_expect_tab, (const void *)e_ops, entries * sizeof(cplx *), hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)e->K, (unsigned)blocks), block(KH_EXPECT_THREADS);
    for (int e0 = 0; e0 < n_e; e0 += KH_EXPECT_MAX_OPS) {
        const int ne = n_e - e0 < KH_EXPECT_MAX_OPS ? n_e - e0 : KH_EXPECT_MAX_OPS;
        cplx *plane = (cplx *)out_dev + (size_t)e0 * e->K * e->nt;
        if (super)
            launch_plain<kh_expect_liouville>(grid, block, 0, st, e->d_expect_tab + e0, (int)n_e, ne, (const cplx *)states_dev, plane,
                                              e->K, e->N, e->nt);
        else
            launch_plain<kh_expect_hilbert>(grid, block, 0, st, e->d_expect_tab + e0, (int)n_e, ne, (const cplx *)states_dev, plane,
                                            e->K, e->N, e->nt);
    }
    KH_HIP(hipGetLastError());
    return KH_OK;
}

extern "C" int kh_chi_boundary(kh_engine *e, const kh_cdouble *targets_dev, const kh_cdouble *psi_T_dev,
                               const kh_cdouble *c_dev, const kh_cdouble *d_dev, kh_cdouble *chi_T_dev,
                               double *chi_norms_dev, void *stream) {
    if (e == nullptr || targets_dev == nullptr || psi_T_dev == nullptr || c_dev == nullptr || d_dev == nullptr ||
        chi_T_dev == nullptr || chi_norms_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    const int waves_per_block = 4;
    const int blocks = (e->K + waves_per_block - 1) / waves_per_block;
    kh_chi_kernel<<<blocks, 64 * waves_per_block, 0, (hipStream_t)stream>>>(
        (const cplx *)targets_dev, (const cplx *)psi_T_dev, (const cplx *)c_dev, (const cplx *)d_dev,
        (cplx *)chi_T_dev, chi_norms_dev, e->K, e->N);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

// Boundary co-states of the perfect-entangler / local-invariants functionals (kh_chi_li.h): one wave per gate
extern "C" int kh_chi_local_invariants(kh_engine *e, const kh_cdouble *psi_T_dev, const kh_cdouble *bell_dev,
                                       int32_t bell_per_gate, int32_t mode, const double *invariants_dev,
                                       int32_t invariants_per_gate, double unitarity_weight, double scale,
                                       kh_cdouble *chi_T_dev, double *chi_norms_dev, double *J_dev, void *stream) {
    if (e == nullptr || psi_T_dev == nullptr || bell_dev == nullptr || chi_T_dev == nullptr || chi_norms_dev == nullptr ||
        J_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    if (mode != KH_LI_MODE_PE && mode != KH_LI_MODE_LI) return kh_fail(KH_ERR_INVALID, "mode = %d: KH_LI_PE or KH_LI_LI", mode);
    if (mode == KH_LI_MODE_LI && invariants_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument: KH_LI_LI needs the target gate's invariants");
    if (!(unitarity_weight >= 0.0 && unitarity_weight <= 1.0))
        return kh_fail(KH_ERR_INVALID, "unitarity_weight must be in [0, 1]");
    if (e->mixed || e->lind || e->is_super)
        return kh_fail(KH_ERR_UNSUPPORTED, "the local-invariants functionals are defined on Hilbert-space states: "
                                           "Liouville-space, Lindblad-form and mixed engines keep the host constructor");
    if (e->K % 4 != 0 || (e->replicas > 0 && e->Kr % 4 != 0))
        return kh_fail(KH_ERR_INVALID, "%d objectives%s: a gate is 4 consecutive objectives", e->replicas > 0 ? e->Kr : e->K,
                       e->replicas > 0 ? " per replica" : "");
    KhLiArgs a;
    a.psi = (const cplx *)psi_T_dev, a.bell = (const cplx *)bell_dev, a.inv = invariants_dev;
    a.chi = (cplx *)chi_T_dev, a.norms = chi_norms_dev, a.J = J_dev;
    a.active = e->replicas > 0 ? e->active_mask() : nullptr;
    a.M = e->K / 4, a.N = e->N;
    a.gates_per_replica = e->replicas > 0 ? e->Kr / 4 : 1;
    a.bell_per_gate = bell_per_gate != 0, a.inv_per_gate = invariants_per_gate != 0;
    a.w = unitarity_weight, a.scale = scale;
    const dim3 grid((unsigned)((a.M + KH_LI_WAVES - 1) / KH_LI_WAVES)), block(64 * KH_LI_WAVES);
    if (mode == KH_LI_MODE_PE)
        launch_plain<kh_chi_li_kernel<KH_LI_MODE_PE>>(grid, block, 0, (hipStream_t)stream, a);
    else
        launch_plain<kh_chi_li_kernel<KH_LI_MODE_LI>>(grid, block, 0, (hipStream_t)stream, a);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

// the limits of kh_pulse_gradient that a problem's sizes decide
static int grad_limits(int N, int L, int nt) {
    if (L < 1) return kh_fail(KH_ERR_INVALID, "L = %d: no control to differentiate for", L);
    if (nt < 2 || N < 1) return kh_fail(KH_ERR_INVALID, "nt = %d, N = %d: at least one interval and one dimension", nt, N);
    if (N > KH_GRAD_NMAX) return kh_fail(KH_ERR_UNSUPPORTED, "N = %d: the pulse gradient serves N <= %d", N, KH_GRAD_NMAX);
    if (L > KH_GRAD_MAX_L)
        return kh_fail(KH_ERR_UNSUPPORTED, "L = %d: the pulse gradient serves L <= %d controls (terms)", L, KH_GRAD_MAX_L);
    if (((long long)nt - 1 + KH_GRAD_CHUNK - 1) / KH_GRAD_CHUNK > 65535)
        return kh_fail(KH_ERR_UNSUPPORTED, "nt = %d: more than 65535 chunks of %d intervals", nt, KH_GRAD_CHUNK);
    return KH_OK;
}

extern "C" int kh_pulse_gradient_limits(const kh_problem *pr) {
    if (pr == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    return grad_limits(pr->N, pr->L, pr->nt);
}

// Exact gradient of J_T for the pulse values (kh_grad.h): one slot per (objective, control, interval), then the sum over
// the objectives in their order.
extern "C" int kh_pulse_gradient(kh_engine *e, const kh_cdouble *fw_store_dev, const kh_cdouble *chi_store_dev,
                                 const double *chi_norms_dev, const double *pulses_dev, double *grad_dev,
                                 double *per_objective_dev, void *stream) {
    if (e == nullptr || fw_store_dev == nullptr || chi_store_dev == nullptr || pulses_dev == nullptr || grad_dev == nullptr)
        return kh_fail(KH_ERR_INVALID, "null argument");
    if (e->d_csr_fw != nullptr || e->mixed || e->lind || e->replicas > 0 || e->p2p_world > 1)
        return kh_fail(KH_ERR_UNSUPPORTED, "the pulse gradient serves dense uniform engines on one GPU: not %s engines",
                       e->d_csr_fw != nullptr ? "sparse (CSR)" : e->mixed ? "mixed" : e->lind ? "Lindblad-form"
                                                                : e->replicas > 0 ? "replica" : "sharded");
    KH_TRY(grad_limits(e->N, e->L, e->nt));
    const long long nI = (long long)e->nt - 1;
    const long long chunks = (nI + KH_GRAD_CHUNK - 1) / KH_GRAD_CHUNK;
    hipStream_t st = (hipStream_t)stream;
    const long long count = (long long)e->L * nI;
    if (per_objective_dev == nullptr) {
        if (e->d_grad_ws == nullptr) {
            void *mem = nullptr;
            if (hipMalloc(&mem, sizeof(double) * (size_t)e->K * (size_t)count) != hipSuccess) {
                (void)hipGetLastError();
                return kh_fail(KH_ERR_NOMEM, "no device memory for the per-objective gradients (%d x %lld doubles)", e->K, count);
            }
            e->d_grad_ws = (double *)mem;
        }
        per_objective_dev = e->d_grad_ws;
    }
    KhGradArgs a;
    a.ops = e->d_ops_fw, a.norms = e->d_norms, a.dt = e->d_dt, a.deg_theta = e->d_deg_theta;
    a.fw = (const cplx *)fw_store_dev, a.chi = (const cplx *)chi_store_dev, a.chi_norms = chi_norms_dev;
    a.pulses = pulses_dev, a.per_obj = per_objective_dev;
    a.K = e->K, a.N = e->N, a.nt = e->nt, a.is_super = e->is_super;
    const int gx = e->sw.grad_grid > 0 && e->sw.grad_grid < e->K ? e->sw.grad_grid : e->K;
    const dim3 grid((unsigned)gx, (unsigned)chunks), block(KH_GRAD_THREADS);
    const size_t lds = kh_grad_lds_bytes(e->N, e->L);
    // (row blocks of 16 per wave: one up to N = 64, two beyond)
    auto launch = [&](auto l, auto ng) {
        return launch_plain_lds<kh_grad_items<decltype(l)::value, decltype(ng)::value>>(e, grid, block, lds, st, a);
    };
    auto by_rows = [&](auto l) {
        return e->N <= 64 ? launch(l, std::integral_constant<int, 1>{}) : launch(l, std::integral_constant<int, 2>{});
    };
    switch (e->L) {
        case 1: KH_TRY(by_rows(std::integral_constant<int, 1>{})); break;
        case 2: KH_TRY(by_rows(std::integral_constant<int, 2>{})); break;
        case 3: KH_TRY(by_rows(std::integral_constant<int, 3>{})); break;
        default: KH_TRY(by_rows(std::integral_constant<int, 4>{})); break;
    }
    launch_plain<kh_grad_reduce>(dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const double *)per_objective_dev, grad_dev,
                                 e->K, count);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

extern "C" int kh_check(kh_engine *e) {
    if (e == nullptr) return kh_fail(KH_ERR_INVALID, "null engine");
    unsigned int flag = 0;
    KH_HIP(hipMemcpy(&flag, e->d_abort, sizeof(flag), hipMemcpyDeviceToHost));
    if (flag != 0) {
        KH_HIP(hipMemset(e->d_abort, 0, sizeof(flag)));
        return kh_fail(KH_ERR_TIMEOUT, "in-kernel exchange timed out: outputs of the last update sweep are invalid");
    }
    return KH_OK;
}

extern "C" int kh_series_tables(int32_t real_spectrum, double tol, double *theta, double *ratios) {
    if (theta == nullptr || ratios == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    static_assert(KH_MAX_DEGREE == 64 && KH_RATIO_STRIDE == 65, "documented table sizes");
    if (!(tol > 0.0)) tol = ldexp(1.0, -53);
    std::vector<double> c0(KH_MAX_DEGREE + 1), rows((size_t)(KH_MAX_DEGREE + 1) * KH_Q2_ROWS * 2);
    if (real_spectrum) {
        kh_build_real_spectrum_rows(tol, theta, c0.data(), rows.data(), ratios);
    } else {
        kh_build_degree_table(tol, theta);
        kh_build_taylor_rows(c0.data(), rows.data(), ratios);
    }
    return KH_OK;
}

extern "C" int kh_series_tables_odd(double tol, double *theta, double *c0, double *rows) {
    if (theta == nullptr || c0 == nullptr || rows == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    if (!(tol > 0.0)) tol = ldexp(1.0, -53);
    std::vector<double> ratios((size_t)(KH_MAX_DEGREE + 1) * KH_RATIO_STRIDE);
    kh_build_real_spectrum_rows(tol, theta, c0, rows, ratios.data(), 2.0, 0.0, true);
    return KH_OK;
}

extern "C" int kh_series_tables_defect(double tol, double theta_cap, double defect, double *theta, double *ratios) {
    if (theta == nullptr || ratios == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    if (!(theta_cap > 0.0) || theta_cap > 8.0 || !(defect >= 0.0))
        return kh_fail(KH_ERR_INVALID, "theta_cap must be in (0, 8], defect >= 0");
    if (!(tol > 0.0)) tol = ldexp(1.0, -53);
    std::vector<double> c0(KH_MAX_DEGREE + 1), rows((size_t)(KH_MAX_DEGREE + 1) * KH_Q2_ROWS * 2);
    kh_build_real_spectrum_rows(tol, theta, c0.data(), rows.data(), ratios, theta_cap, defect);
    return KH_OK;
}

// holds one CU per workgroup (all of its LDS) until `ticks` of the 100 MHz wall clock have passed
__global__ void __launch_bounds__(512) kh_occupy_kernel(long long ticks, int *sink) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const long long t0 = wall_clock64();
    // all ones (a NaN as a double) in all of the 128 KiB: what a later kernel on this CU finds in its uninitialised LDS
    for (int i = threadIdx.x; i < 128 * 1024 / 16; i += blockDim.x) ((uint4 *)smem)[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
    __syncthreads();
    smem[threadIdx.x] = (char)threadIdx.x;
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
    if (smem[(threadIdx.x + 1) & 511] == 77 && ticks < 0) *sink = 1;
}

extern "C" int kh_debug_occupy(kh_engine *e, int32_t workgroups, double milliseconds, void *stream) {
    if (e == nullptr || workgroups < 1 || !(milliseconds >= 0.0) || milliseconds > 1000.0)
        return kh_fail(KH_ERR_INVALID, "bad argument");
    const size_t lds = 128 * 1024;
    KH_TRY(ensure_dynamic_lds(e, (const void *)kh_occupy_kernel, lds));
    kh_occupy_kernel<<<workgroups, 512, lds, (hipStream_t)stream>>>((long long)(milliseconds * 1e5), (int *)e->d_abort + 0);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

extern "C" int kh_debug_launched(int32_t which, char *buf, int32_t cap) {
    std::string out;
    if (which == 2) {  // forget what this process has launched so far (not what it has logged)
        for (KhKernelRecord &rec : kh_kernel_registry()) rec.launched = false;
        return 0;
    }
    for (const KhKernelRecord &rec : kh_kernel_registry())
        if (which != 0 || rec.launched) out += rec.name + "\n";
    if (buf != nullptr && cap > 0) {
        const size_t n = out.size() < (size_t)cap - 1 ? out.size() : (size_t)cap - 1;
        memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return (int)out.size() + 1;
}

extern "C" int kh_last_stats(kh_engine *e, double stats[4]) {
    if (e == nullptr || stats == nullptr) return kh_fail(KH_ERR_INVALID, "null argument");
    double d[4] = {0, 0, 0, 0};
    KH_HIP(hipMemcpy(d, e->d_stats, sizeof(d), hipMemcpyDeviceToHost));
    stats[0] = d[0];
    stats[1] = e->last_intervals;
    stats[2] = e->last_wgs;
    stats[3] = 0.0;
#ifdef KH_TIMING
    stats[0] = d[0];
    stats[1] = d[1];
    stats[2] = d[2];
    stats[3] = d[3];
    if (getenv("KH_TRACE")) {  // per-point clock stamps of one interval of workgroup 0 (kernels that record them)
        double tr[64];
        KH_HIP(hipMemcpy(tr, e->d_stats + 4, sizeof(tr), hipMemcpyDeviceToHost));
        fprintf(stderr, "KH_TRACE (cycles since the interval's start):");
        for (int i = 0; i < 64 && (i == 0 || tr[i] != 0.0); ++i) fprintf(stderr, " %d:%.0f", i, tr[i] - tr[0]);
        fprintf(stderr, "\n");
        unsigned int ab[2] = {0, 0};
        KH_HIP(hipMemcpy(ab, e->d_abort, sizeof(ab), hipMemcpyDeviceToHost));
        fprintf(stderr, "KH_TRACE polling rounds of workgroup 0 since the engine was created: %u\n", ab[1]);
        fprintf(stderr, "KH_TRACE raw [16..31]:");
        for (int i = 16; i < 32; ++i) fprintf(stderr, " %.0f", tr[i]);
        fprintf(stderr, "\n");
    }
#endif
    return KH_OK;
}

extern "C" int32_t kh_ell_rows_of(int32_t N) { return N >= 1 && N <= KH_ELL_NMAX ? kh_ell_rows(N) : 0; }

extern "C" int kh_debug_q2_lane_map(int32_t wave, int32_t lane, int32_t *out) {
    if (out == nullptr || wave < 0 || wave >= KH_Q2_THREADS / 64 || lane < 0 || lane >= 64)
        return kh_fail(KH_ERR_INVALID, "bad argument");
    out[0] = KhLanesR16::row_in(wave, lane);
    out[1] = KhLanesR16::col0(wave, lane);
    out[2] = KhLanesR16::x_index(wave, lane);
    out[3] = KhLanesR16::landing_lane(lane);
    out[4] = KhLanesR16::row_out(wave, lane);
    out[5] = KhLanesR16::writer(lane) ? 1 : 0;
    out[6] = KhLanesR16::half(wave);
    return KH_OK;
}

static int ell_layout(int32_t N, int32_t n_ops, const kh_csr *ops_host, int32_t *E_out, int32_t *Ec_out, int32_t *off_out,
                      kh_cdouble *vals_out, int32_t E_cap, bool global) {
    if (ops_host == nullptr || E_out == nullptr || Ec_out == nullptr || n_ops < 1 || N < 1)
        return kh_fail(KH_ERR_INVALID, "bad argument");
    const int nmax = global ? KH_ELLG_NMAX : KH_ELL_NMAX;
    if (N > nmax) return kh_fail(KH_ERR_UNSUPPORTED, "N = %d: the padded row form serves N <= %d", N, nmax);
    std::vector<HostCsr> host(n_ops);
    std::vector<const HostCsr *> ptrs(n_ops, nullptr);
    for (int o = 0; o < n_ops; ++o) {
        if (ops_host[o].data == nullptr) continue;
        if (!canonical_csr(ops_host[o].indptr, ops_host[o].indices, (const cplx *)ops_host[o].data, ops_host[o].nnz, N, host[o]))
            return kh_fail(KH_ERR_INVALID, "operator %d: inconsistent CSR arrays", o);
        ptrs[o] = &host[o];
    }
    std::vector<int> off;
    std::vector<cplx> vals;
    int E = 0, Ec = 0;
    if (!build_ell_host(ptrs, N, off, vals, E, Ec, global, global))
        return kh_fail(KH_ERR_UNSUPPORTED, "rows wider than the kernels' register budget (%d entries for N = %d)", kh_ell_emax(N), N);
    *E_out = E;
    *Ec_out = Ec;
    if (off_out != nullptr || vals_out != nullptr) {
        if (E_cap < E) return kh_fail(KH_ERR_INVALID, "E_cap = %d < E = %d", E_cap, E);
        if (off_out != nullptr) memcpy(off_out, off.data(), sizeof(int) * off.size());
        if (vals_out != nullptr) memcpy(vals_out, vals.data(), sizeof(cplx) * vals.size());
    }
    return KH_OK;
}

extern "C" int kh_ell_layout(int32_t N, int32_t n_ops, const kh_csr *ops_host, int32_t *E_out, int32_t *Ec_out, int32_t *off_out,
                             kh_cdouble *vals_out, int32_t E_cap) {
    return ell_layout(N, n_ops, ops_host, E_out, Ec_out, off_out, vals_out, E_cap, false);
}

extern "C" int kh_ell_layout_global(int32_t N, int32_t n_ops, const kh_csr *ops_host, int32_t *E_out, int32_t *Ec_out,
                                    int32_t *off_out, kh_cdouble *vals_out, int32_t E_cap) {
    return ell_layout(N, n_ops, ops_host, E_out, Ec_out, off_out, vals_out, E_cap, true);
}
