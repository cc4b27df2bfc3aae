// Sparse operators in the padded row form with NOTHING of size N in LDS or registers: the global-vector forms of the
// family of kh_ell.h, for what neither the register form (N <= 2048) nor the streamed form (N <= 4096, rows up to 32
// entries, two vectors in 2 x 64 KiB of LDS) can hold -- a 13-qubit spin chain (N = 8192), a d = 65 Lindbladian
// (N = 4225), a ladder whose rows are wider than 32.  One body per sweep (template <bool SPLIT>), two forms:
//   * PLAIN ("ellglobal/csr", kh_ellg_*): one 512-thread workgroup per group;
//   * SPLIT ("ellsplit/csr", kh_ellgs_*): S workgroups per group, for problems with a handful of large objectives (a
//     17-qubit chain: N = 131 072, K = 1 .. 3), where the plain form leaves all but K compute units idle.  Workgroup b
//     belongs to group b / S as part b % S.
// Common to both:
//   * a group owns the objectives k = group, group + groups, ... in turns (as kh_lind_forward_update does): more
//     objectives than CUs run, and the plain form runs on any grid the caller asks for (kh_set_update_workgroups);
//   * the rows are dealt in whole 64-row chunks of kh_ellg_rows(N), a contiguous range [first, end) per part
//     (kh_ellsplit_range; a part may own no row at all; plain: [0, N)); inside its range a workgroup loops
//     row = first + tid + 512 i at RUN TIME, and a row's arithmetic (kh_ells_row / kh_ells_control_row / kh_ellg_rebuild)
//     does not depend on S;
//   * the pools of the streamed form as they are (KhEll, rows = N rounded up to 64, any row width that is a multiple of
//     four): lane = row, so every pool load is coalesced;
//   * a per-GROUP workspace in global memory, allocated at engine creation: the two term planes xa / xb, the running
//     sum of the series and the plane of the interval's control-touched values (kh_ells_rebuild's scratch plane).  The
//     running sum and the values plane are row-private (the lane that writes an element is the one that reads it); the
//     term planes (and, in the update sweep, u.phi) are written by the lane that owns the row and gathered by every lane
//     of the group -- as the generic kernels' scratch matrix and kh_lind.h's non-resident state are -- through plain
//     pointers: a workgroup's waves share their CU's vector cache, and nothing may move these loads to the scalar or
//     read-only path;
//   * a term of the series: E coalesced pool loads (20 B per entry), E gathers from L2 (16 B each), one store, one
//     read-modify-write of the running sum and ONE sync (kh_ellg_sync), as in kh_ells_expm_action.  Plain: the sync is
//     __syncthreads().  Split: a barrier among the group's S workgroups (kh_group_barrier): plain stores, every storing
//     wave's vmcnt(0), __syncthreads(), lane 0's agent-scope release fence and vmcnt(0), one agent-scope add to the
//     group's counter; one wave polls the counter relaxed, then ONE agent-scope acquire fence, vmcnt(0), __syncthreads(),
//     plain vector loads.  The ping-pong needs no second sync per term: nobody starts term j + 1 before everybody has
//     finished reading in term j.  The handed-off planes are read through plain pointers only (kh_ells_row's `x`);
//   * split: every spin is bounded (kh_poll_gave_up: KH_TIMEOUT_MS and the abort flag); a wave that gives up leaves the
//     verdict in LDS, every thread of its workgroup returns behind the workgroup barrier and kh_check reports
//     KH_ERR_TIMEOUT.  All S x groups workgroups must be resident at once: both sweeps are launched through
//     launch_persistent.  (The plain sweep_store runs on launch_plain with any K.)
// Degree lookup, sub-steps, ratios and the pulse update are the family's (kh_degree_cached, kh_ell_load_ratios,
// kh_pulse_update); so is the exchange (kh_exchange_waves_*).
// Indices: N <= 2^20, so a column's byte offset (N * 16 <= 2^24) stays int32; pool offsets, (k nt + n) N and the
// workspace strides are 64-bit.
#pragma once

#include "kh_ell.h"

#define KH_ELLG_THREADS 512
#define KH_ELLG_NMAX (1 << 20)  // 16 MiB per state: a stated limit, not a measured one
#define KH_ELLG_MMAX 16         // objectives per workgroup of the update sweep at most (kh_set_update_workgroups)
#define KH_ELLGS_LINE 128       // bytes between two groups' barrier counters: a memory line each

// rows of the pools and of every workspace plane
__host__ __device__ inline long long kh_ellg_rows(int N) { return ((long long)N + 63) / 64 * 64; }
// elements of one group's workspace: xa, xb, the running sum, ec_max value planes
__host__ __device__ inline long long kh_ellg_ws_stride(int N, int ec_max) { return (3 + (long long)(ec_max > 4 ? ec_max : 4)) * kh_ellg_rows(N); }

struct KhEllgWs {
    cplx *xa, *xb;  // the series' term planes (gathered across lanes)
    cplx *sum;      // the running sum = the state (row-private)
    cplx *scr;      // [Ec][rows] the interval's values of the control-touched slots (row-private)
};

__device__ __forceinline__ KhEllgWs kh_ellg_carve_ws(cplx *ws, long long ws_stride, int N, int group) {
    const long long rows = kh_ellg_rows(N);
    KhEllgWs w;
    w.xa = ws + (long long)group * ws_stride;
    w.xb = w.xa + rows;
    w.sum = w.xb + rows;
    w.scr = w.sum + rows;
    return w;
}

// LDS: the family's small arrays (KhEllLds, no vectors), the workgroup's partial sums over its objectives and, in the
// split form, the word a polling wave leaves its verdict in
__host__ __device__ inline size_t kh_ellg_lds_bytes(bool split) {
    return kh_ell_lds_bytes() - (size_t)2 * KH_ELL_XB_BYTES + KH_MAX_L * sizeof(double) + (split ? 16 : 0);
}

// rows [*first, *first + *count) of part `part` of S: the chunk count split as evenly as possible, earlier parts take the
// remainder, empty parts come last (and start at N)
__host__ __device__ inline void kh_ellsplit_range(int N, int S, int part, int *first, int *count) {
    const int chunks = (int)(kh_ellg_rows(N) / 64);
    const int q = chunks / S, r = chunks % S;
    const long long c0 = (long long)part * q + (part < r ? part : r), c1 = c0 + q + (part < r ? 1 : 0);
    const long long lo = 64 * c0 < N ? 64 * c0 : N, hi = 64 * c1 < N ? 64 * c1 : N;
    *first = (int)lo;
    *count = (int)(hi - lo);
}

// a workgroup's place: its group, its part of the group and the rows [first, end) the part owns.  !SPLIT: one workgroup
// per group that owns every row -- nothing but blockIdx.x and gridDim.x is left at run time
struct KhEllgPlace {
    int group, groups, part, first, end;
};

template <bool SPLIT>
__device__ __forceinline__ KhEllgPlace kh_ellg_place(int N, int S) {
    if constexpr (!SPLIT) return {(int)blockIdx.x, (int)gridDim.x, 0, 0, N};
    int first, count;
    kh_ellsplit_range(N, S, blockIdx.x % S, &first, &count);
    return {(int)(blockIdx.x / S), (int)(gridDim.x / S), (int)(blockIdx.x % S), first, first + count};
}

struct KhGroupBarrier {
    unsigned int *counter;  // the group's arrivals, monotonic within a launch (zeroed by the launch function)
    unsigned int target;    // S x barriers passed so far
    int S;
    int *gave_up;           // LDS: != 0 once a wait of this workgroup gave up
};

// the group's counter and the verdict word behind the partial sums.  !SPLIT: neither -- the word would lie beyond
// kh_ellg_lds_bytes(false)
template <bool SPLIT>
__device__ __forceinline__ KhGroupBarrier kh_ellg_barrier_init(const KhEllLds &s, int group, int S, unsigned int *counters) {
    if constexpr (!SPLIT) return {nullptr, 0u, 1, nullptr};
    return {counters + (size_t)group * (KH_ELLGS_LINE / sizeof(unsigned int)), 0u, S, (int *)(s.g_a + 2 * KH_MAX_L)};
}

// All threads of every workgroup of the group.  Before it: plain stores other parts will read; after it (true): plain
// vector loads of them.  false: a wait gave up -- every thread of the workgroup gets false and must return.
__device__ __forceinline__ bool kh_group_barrier(KhGroupBarrier &gb, const KhExchange &ex, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave
    __syncthreads();
    gb.target += (unsigned int)gb.S;
    if (tid < 64) {
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the compiler may drop the fence's own wait)
            __hip_atomic_fetch_add(gb.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        long long t0 = 0;
        unsigned int spins = 0;
        for (;;) {
            const unsigned int seen = __hip_atomic_load(gb.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((int)(seen - gb.target) >= 0) break;  // (a faster part may already have arrived at the next barrier)
            if (kh_poll_gave_up(ex, tid, t0, spins)) {
                if (tid == 0) *gb.gave_up = 1;
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // holds the barrier below until the invalidate has completed
    }
    __syncthreads();
    return *gb.gave_up == 0;
}

// what orders a term plane between its writers and its readers: the group's barrier, or the workgroup's
template <bool SPLIT>
__device__ __forceinline__ bool kh_ellg_sync(KhGroupBarrier &gb, const KhExchange &ex, int tid) {
    if constexpr (SPLIT) return kh_group_barrier(gb, ex, tid);
    __syncthreads();
    return true;
}

// kh_ells_rebuild with the run-time row loop: rows first, first + T, ... below `end`
template <int T>
__device__ __forceinline__ void kh_ellg_rebuild(const KhEll &el, const cplx *__restrict__ vals, cplx *scr, int first, int L,
                                                const double *eps, int end) {
    const long long plane = (long long)el.E * el.rows;
    for (int row = first; row < end; row += T) {
        for (int e0 = 0; e0 < el.Ec; e0 += 4) {
            cplx v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = (vals + (el.vals_at + (long long)(e0 + q) * el.rows))[row];
            for (int l = 0; l < L; ++l) {
                const double w = eps[l];
                cplx c[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) c[q] = (vals + (el.vals_at + (1 + l) * plane + (long long)(e0 + q) * el.rows))[row];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q].x = fma(w, c[q].x, v[q].x);
                    v[q].y = fma(w, c[q].y, v[q].y);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) scr[(long long)(e0 + q) * el.rows + row] = v[q];
        }
    }
}

// sum <- exp(f A dt) sum on the rows [first, end) of this part, term by term (kh_ells_expm_action with the vectors in
// global memory), the term planes ordered by kh_ellg_sync.  All threads; on entry the previous reads of xa / xb are
// behind a sync.  Returns nsub * m, or -1 when a barrier gave up.  On exit (>= 0) every part's rows of `sum` are
// visible to every part.
template <int T, bool SPLIT>
__device__ __forceinline__ int kh_ellg_expm_action(const KhEll &el, const int *__restrict__ offs, const cplx *__restrict__ vals,
                                                   const cplx *scr, cplx *sum, cplx *xa, cplx *xb, const double *ratio,
                                                   double fre, double fim, double dt, int nsub, int m, int tid, int first,
                                                   int end, KhGroupBarrier &gb, const KhExchange &ex) {
    const double h = dt / nsub;
    auto term = [&](int j, const cplx *xin, cplx *xout) {
        const double hj = h * ratio[j];
        const cplx coef = c_make(fre * hj, fim * hj);
        for (int row = first + tid; row < end; row += T) {
            const cplx t = c_mul(coef, kh_ells_row(el, offs, vals, scr, row, (const char *)xin));
            xout[row] = t;
            cplx s = sum[row];
            s.x += t.x;
            s.y += t.y;
            sum[row] = s;
        }
        return kh_ellg_sync<SPLIT>(gb, ex, tid);
    };
    for (int sub = 0; sub < nsub; ++sub) {
        const double c0 = ratio[0];
        for (int row = first + tid; row < end; row += T) {
            const cplx v = sum[row];
            xa[row] = v;  // the chain starts from v itself, the sum from T_0 = c_0 v
            sum[row] = c_make(c0 * v.x, c0 * v.y);
        }
        if (!kh_ellg_sync<SPLIT>(gb, ex, tid)) return -1;
        for (int j = 1; j <= m; j += 2) {
            if (!term(j, xa, xb)) return -1;
            if (j + 1 > m) break;
            if (!term(j + 1, xb, xa)) return -1;
        }
    }
    return nsub * m;
}

// ---------------------------------------------------------------------------
// plain propagation with storage (backward sweep / iteration-0 forward sweep): groups take the objectives in turns
// ---------------------------------------------------------------------------
template <int T, bool SPLIT>
__device__ __forceinline__ void kh_ellg_sweep_store_body(char *smem, const KhSweepArgs &p, const KhEll *__restrict__ ells,
                                                         const int *__restrict__ offs, const cplx *__restrict__ vals,
                                                         const double *__restrict__ pulses, const cplx *__restrict__ state_in,
                                                         cplx *__restrict__ store, cplx *__restrict__ state_out, int direction,
                                                         cplx *ws, long long ws_stride, const KhExchange &ex, int S,
                                                         unsigned int *counters) {
    const KhEllLds s = kh_ell_carve<0>(smem);
    const int tid = threadIdx.x, N = p.N, L = p.L, nt = p.nt;
    const KhEllgPlace pl = kh_ellg_place<SPLIT>(N, S);
    const int first = pl.first, end = pl.end;
    const KhEllgWs w = kh_ellg_carve_ws(ws, ws_stride, N, pl.group);
    KhGroupBarrier gb = kh_ellg_barrier_init<SPLIT>(s, pl.group, S, counters);
    double matvecs = 0.0;
    int m_cur = -1;
    if (tid <= KH_MAX_DEGREE) s.deg[tid] = p.q2_theta[tid];
    if (SPLIT && tid == 0) *gb.gave_up = 0;
    __syncthreads();
    for (int k = pl.group; k < p.K; k += pl.groups) {
        const KhEll el = ells[k];
        const double *norms_k = p.op_norms + (size_t)k * (1 + L);
        auto put = [&](cplx *dst) {
            for (int row = first + tid; row < end; row += T) dst[row] = w.sum[row];
        };
        for (int row = first + tid; row < end; row += T) w.sum[row] = state_in[(size_t)k * N + row];
        if (store != nullptr) put(store + ((size_t)k * nt + (direction > 0 ? 0 : nt - 1)) * N);
        KhDegreeCache dc = {12, 1.0, 0.0};
        for (int step = 0; step < nt - 1; ++step) {
            const int n = direction > 0 ? step : nt - 2 - step;
            // theta decides nsub, m, the ratio reload and the number of terms, that is the number of group barriers:
            // every part of a group must form it from identical inputs -- the objective's op_norms and the caller's
            // pulse values, the same memory for every workgroup.  A part that counted differently would stall its group.
            double theta = norms_k[0];
            for (int l = 0; l < L; ++l) {
                const double v = pulses[(size_t)l * (nt - 1) + n];
                if (tid == l) s.eps[l] = v;
                theta += fabs(v) * norms_k[1 + l];
            }
            const double dt = p.dt[n];
            __syncthreads();  // (s.eps)
            kh_ellg_rebuild<T>(el, vals, w.scr, first + tid, L, s.eps, end);
            int nsub, m;
            kh_degree_cached(theta * dt, s.deg, p.theta_max, p.inv_theta_max, dc, &nsub, &m);
            if (m != m_cur) {
                kh_ell_load_ratios(p, s, m, tid);
                m_cur = m;
            }
            const int done = kh_ellg_expm_action<T, SPLIT>(el, offs, vals, w.scr, w.sum, w.xa, w.xb, s.ratio, p.fre, p.fim, dt, nsub,
                                                           m, tid, first, end, gb, ex);
            if (SPLIT && done < 0) return;
            matvecs += done;
            if (store != nullptr) put(store + ((size_t)k * nt + (direction > 0 ? n + 1 : n)) * N);
        }
        if (state_out != nullptr) put(state_out + (size_t)k * N);
    }
    if (tid == 0 && pl.part == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);  // a product counts once per group
}

template <int T>
__global__ void __launch_bounds__(T)
kh_ellg_sweep_store(KhSweepArgs p, const KhEll *__restrict__ ells, const int *__restrict__ offs, const cplx *__restrict__ vals,
                    const double *__restrict__ pulses, const cplx *__restrict__ state_in, cplx *__restrict__ store,
                    cplx *__restrict__ state_out, int direction, cplx *ws, long long ws_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    kh_ellg_sweep_store_body<T, false>(smem, p, ells, offs, vals, pulses, state_in, store, state_out, direction, ws, ws_stride,
                                       KhExchange(), 1, nullptr);
}

template <int T>
__global__ void __launch_bounds__(T)
kh_ellgs_sweep_store(KhSweepArgs p, const KhEll *__restrict__ ells, const int *__restrict__ offs, const cplx *__restrict__ vals,
                     const double *__restrict__ pulses, const cplx *__restrict__ state_in, cplx *__restrict__ store,
                     cplx *__restrict__ state_out, int direction, cplx *ws, long long ws_stride, KhExchange ex, int S,
                     unsigned int *counters) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    kh_ellg_sweep_store_body<T, true>(smem, p, ells, offs, vals, pulses, state_in, store, state_out, direction, ws, ws_stride, ex,
                                      S, counters);
}

// ---------------------------------------------------------------------------
// forward sweep with sequential pulse update (optimize.py:444-508): ONE launch, sums exchanged among ALL workgroups
// ---------------------------------------------------------------------------
// The states of a group's objectives live in u.phi, which is also the series' running sum (row-private) and, between the
// intervals, the vector the control products gather from.  Every workgroup forms the partial sums over its own rows of its
// group's objectives (added in order) and publishes them as one of the ex.G = gridDim.x workgroups of the exchange, whose
// fixed-order gather gives every workgroup the bit-identical eps[n].  In the split form the exchange is also what keeps a
// part from rewriting u.phi (the next interval's sub-step start) while another part of its group still gathers from it:
// nobody passes it before everybody has published, and a part publishes what its gathers returned.
template <int T, bool SO, bool SPLIT>
__device__ __forceinline__ void kh_ellg_forward_update_body(char *smem, const KhSweepArgs &p, const KhEll *__restrict__ ells,
                                                            const int *__restrict__ offs, const cplx *__restrict__ vals,
                                                            const KhUpdateArgs &u, const KhExchange &ex, cplx *ws,
                                                            long long ws_stride, int S, unsigned int *counters) {
    const KhEllLds s = kh_ell_carve<0>(smem);
    double *part_sh = s.g_a + KH_MAX_L;  // [KH_MAX_L] the workgroup's partial sums, its objectives added in order
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, N = p.N, L = p.L, nt = p.nt;
    const int wg = blockIdx.x;
    const KhEllgPlace pl = kh_ellg_place<SPLIT>(N, S);
    const int group = pl.group, groups = pl.groups, first = pl.first, end = pl.end;
    const KhEllgWs w = kh_ellg_carve_ws(ws, ws_stride, N, group);
    KhGroupBarrier gb = kh_ellg_barrier_init<SPLIT>(s, group, S, counters);
    double matvecs = 0.0;
    if (tid < KH_MAX_L) s.g_a[tid] = 0.0;
    if (SPLIT && tid == 0) *gb.gave_up = 0;
    int m_cur = -1;
    KhDegreeCache dc = {12, 1.0, 0.0};
    if (tid <= KH_MAX_DEGREE) s.deg[tid] = p.q2_theta[tid];  // (visible after the first barrier below)
    if constexpr (SO) {
        for (int k = group; k < p.K; k += groups)
            for (int row = first + tid; row < end; row += T) u.fw_store[((size_t)k * nt) * N + row] = u.phi[(size_t)k * N + row];
    }

    // part_sh[l] = sum over the group's objectives of ||chi_k|| Im(mu <chi_k(t_n) + 0.5 sigma/||chi_k|| (phi_k - phi_prev)
    // | A_lk phi_k(t_n)>) over THIS part's rows; phi_k(t_n) = u.phi[k]: the caller's copy, or every part's rows of it
    // behind the sync of the previous interval's last term
    auto partial_sums = [&](int n) {
        if (tid < KH_MAX_L) part_sh[tid] = 0.0;
        for (int k = group; k < p.K; k += groups) {
            const KhEll el = ells[k];
            const double chi_norm = u.chi_norms[k];
            const cplx *phi = u.phi + (size_t)k * N;
            const cplx *chi = u.chi_store + ((size_t)k * nt + n) * N;
            for (int l = 0; l < L; ++l) {
                double v = 0.0;
                for (int row = first + tid; row < end; row += T) {
                    cplx bra = chi[row];
                    if constexpr (SO) {
                        const cplx cur = phi[row], prev = u.fw_prev[((size_t)k * nt + n) * N + row];
                        const double hs = 0.5 * u.sigma[n] / chi_norm;
                        bra.x = fma(hs, cur.x - prev.x, bra.x);
                        bra.y = fma(hs, cur.y - prev.y, bra.y);
                    }
                    const cplx z = kh_ells_control_row(el, offs, vals, l, row, (const char *)phi);
                    cplx ov = c_make(0.0, 0.0);
                    c_fma_conj(ov, bra, z);
                    v += u.mu_re * ov.y + u.mu_im * ov.x;  // Im(mu <bra|A_l phi>): one real combination
                }
                v = sum64(v);
                if (lane == 0) s.red[wave * KH_MAX_L + l] = v;
            }
            if (pl.part == 0) matvecs += (double)L;
            __syncthreads();
            if (tid < L) {
                double acc = 0.0;
                for (int wv = 0; wv < T / 64; ++wv) acc += s.red[wv * KH_MAX_L + tid];
                part_sh[tid] += chi_norm * acc;
            }
            __syncthreads();
        }
    };

    __syncthreads();
    partial_sums(0);

    for (int n = 0; n < nt - 1; ++n) {
        // ---- cross-objective sum (optimize.py:470): wave 0 publishes, wave l gathers control l ----
        if (wave == 0) {
            double part_v[KH_MAX_L];
            for (int l = 0; l < KH_MAX_L; ++l) part_v[l] = l < L ? part_sh[l] : 0.0;
            kh_exchange_waves_publish(ex, n, wg, L, lane, part_v, s.D, s.ok);
        }
        kh_exchange_waves_gather(ex, n, L, wave, lane, s.D, s.ok);
        __syncthreads();
        if (!kh_exchange_waves_finish(ex, n, wg, L, wave, lane, s.D, s.ok)) return;
        // ---- pulse update (optimize.py:471-477): once per workgroup; workgroup 0 stores the values ----
        const double dt = p.dt[n];
        kh_pulse_update(u, p.op_norms, s.D, n, nt, L, wg, tid, dt, s.eps, s.g_a);
        __syncthreads();
        // ---- propagate every objective of the group over interval n (optimize.py:479-491) ----
        for (int k = group; k < p.K; k += groups) {
            const KhEll el = ells[k];
            const double *norms_k = p.op_norms + (size_t)k * (1 + L);
            cplx *phi = u.phi + (size_t)k * N;
            // theta decides nsub, m, the ratio reload and the number of terms, that is the number of group barriers:
            // every part of a group must form it from identical inputs -- the objective's op_norms and s.eps, the
            // bit-identical eps[n] the exchange's fixed-order gather gives every workgroup.  A part that counted
            // differently would stall its group.
            double theta = norms_k[0];
            for (int l = 0; l < L; ++l) theta += fabs(s.eps[l]) * norms_k[1 + l];
            kh_ellg_rebuild<T>(el, vals, w.scr, first + tid, L, s.eps, end);
            int nsub, m;
            kh_degree_cached(theta * dt, s.deg, p.theta_max, p.inv_theta_max, dc, &nsub, &m);
            if (m != m_cur) {
                kh_ell_load_ratios(p, s, m, tid);
                m_cur = m;
            }
            const int done = kh_ellg_expm_action<T, SPLIT>(el, offs, vals, w.scr, phi, w.xa, w.xb, s.ratio, p.fre, p.fim, dt, nsub, m,
                                                           tid, first, end, gb, ex);
            if (SPLIT && done < 0) return;
            if (pl.part == 0) matvecs += done;
            if constexpr (SO) {
                for (int row = first + tid; row < end; row += T) u.fw_store[((size_t)k * nt + n + 1) * N + row] = phi[row];
            }
        }
        // ---- partial sums of the next interval ----
        if (n + 1 < nt - 1) partial_sums(n + 1);
    }
    if (wg == 0 && tid < L) u.g_a[tid] = s.g_a[tid];
    if (tid == 0 && pl.part == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);
}

template <int T, bool SO>
__global__ void __launch_bounds__(T)
kh_ellg_forward_update(KhSweepArgs p, const KhEll *__restrict__ ells, const int *__restrict__ offs,
                       const cplx *__restrict__ vals, KhUpdateArgs u, KhExchange ex, cplx *ws, long long ws_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    kh_ellg_forward_update_body<T, SO, false>(smem, p, ells, offs, vals, u, ex, ws, ws_stride, 1, nullptr);
}

template <int T, bool SO>
__global__ void __launch_bounds__(T)
kh_ellgs_forward_update(KhSweepArgs p, const KhEll *__restrict__ ells, const int *__restrict__ offs,
                        const cplx *__restrict__ vals, KhUpdateArgs u, KhExchange ex, cplx *ws, long long ws_stride, int S,
                        unsigned int *counters) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    kh_ellg_forward_update_body<T, SO, true>(smem, p, ells, offs, vals, u, ex, ws, ws_stride, S, counters);
}
