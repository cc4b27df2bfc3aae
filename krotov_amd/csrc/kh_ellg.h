// Sparse operators in the padded row form with NOTHING of size N in LDS or registers: the third form of the family of
// kh_ell.h ("ellglobal/csr"), for what neither the register form (N <= 2048) nor the streamed form (N <= 4096, rows up
// to 32 entries, two vectors in 2 x 64 KiB of LDS) can hold -- a 13-qubit spin chain (N = 8192), a d = 65 Lindbladian
// (N = 4225), a ladder whose rows are wider than 32.
//   * one 512-thread workgroup per objective, lane = row with a RUN-TIME loop row = tid + 512 i over all rows;
//   * the pools of the streamed form as they are (KhEll, rows = N rounded up to 64, any row width that is a multiple of
//     four): lane = row, so every pool load is coalesced (kh_ells_row, kh_ells_control_row);
//   * a per-workgroup workspace in global memory, allocated at engine creation: the two term planes xa / xb, the running
//     sum of the series and the plane of the interval's control-touched values (kh_ells_rebuild's scratch plane).  The
//     running sum and the values plane are row-private (the lane that writes an element is the one that reads it); the
//     term planes are written by every lane and gathered by other lanes of the SAME workgroup after __syncthreads() --
//     as the generic kernels' scratch matrix and kh_lind.h's non-resident state are -- through plain pointers: a
//     workgroup's waves share their CU's vector cache, and nothing may move these loads to the scalar or read-only path;
//   * a term of the series: E coalesced pool loads (20 B per entry), E gathers from L2 (16 B each), one store, one
//     read-modify-write of the running sum and ONE barrier, as in kh_ells_expm_action.
// Degree lookup, sub-steps, ratios and the pulse update are the family's (kh_degree_cached, kh_ell_load_ratios,
// kh_pulse_update); so is the exchange (kh_exchange_waves_*).  Unlike kh_ell_forward_update a workgroup of the update
// sweep owns the objectives k = blockIdx.x, + gridDim.x, ... (as kh_lind_forward_update does): more objectives than CUs
// run, and the sweep runs on any grid the caller asks for (kh_set_update_workgroups).
// Indices: N <= 2^20, so a column's byte offset (N * 16 <= 2^24) stays int32; pool offsets, (k nt + n) N and the
// workspace strides are 64-bit.
#pragma once

#include "kh_ell.h"

#define KH_ELLG_THREADS 512
#define KH_ELLG_NMAX (1 << 20)  // 16 MiB per state: a stated limit, not a measured one
#define KH_ELLG_MMAX 16         // objectives per workgroup of the update sweep at most (kh_set_update_workgroups)

// rows of the pools and of every workspace plane
__host__ __device__ inline long long kh_ellg_rows(int N) { return ((long long)N + 63) / 64 * 64; }
// elements of one workgroup's workspace: xa, xb, the running sum, ec_max value planes
__host__ __device__ inline long long kh_ellg_ws_stride(int N, int ec_max) { return (3 + (long long)(ec_max > 4 ? ec_max : 4)) * kh_ellg_rows(N); }

struct KhEllgWs {
    cplx *xa, *xb;  // the series' term planes (gathered across lanes)
    cplx *sum;      // the running sum = the state (row-private)
    cplx *scr;      // [Ec][rows] the interval's values of the control-touched slots (row-private)
};

__device__ __forceinline__ KhEllgWs kh_ellg_carve_ws(cplx *ws, long long ws_stride, int N) {
    const long long rows = kh_ellg_rows(N);
    KhEllgWs w;
    w.xa = ws + (long long)blockIdx.x * ws_stride;
    w.xb = w.xa + rows;
    w.sum = w.xb + rows;
    w.scr = w.sum + rows;
    return w;
}

// LDS: the family's small arrays (KhEllLds, no vectors) and the workgroup's partial sums over its objectives
__host__ __device__ inline size_t kh_ellg_lds_bytes() { return kh_ell_lds_bytes() - (size_t)2 * KH_ELL_XB_BYTES + KH_MAX_L * sizeof(double); }

// kh_ells_rebuild with the run-time row loop
template <int T>
__device__ __forceinline__ void kh_ellg_rebuild(const KhEll &el, const cplx *__restrict__ vals, cplx *scr, int tid, int L,
                                                const double *eps, int N) {
    const long long plane = (long long)el.E * el.rows;
    for (int row = tid; row < N; row += T) {
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

// sum <- exp(f A dt) sum, term by term (kh_ells_expm_action with the vectors in global memory).  All threads; on entry
// the previous reads of xa / xb are behind a barrier, on exit every lane's rows of `sum` are its own writes.
template <int T>
__device__ __forceinline__ int kh_ellg_expm_action(const KhEll &el, const int *__restrict__ offs, const cplx *__restrict__ vals,
                                                   const cplx *scr, cplx *sum, cplx *xa, cplx *xb, const double *ratio,
                                                   double fre, double fim, double dt, int nsub, int m, int tid, int N) {
    const double h = dt / nsub;
    auto term = [&](int j, const cplx *xin, cplx *xout) {
        const double hj = h * ratio[j];
        const cplx coef = c_make(fre * hj, fim * hj);
        for (int row = tid; row < N; row += T) {
            const cplx t = c_mul(coef, kh_ells_row(el, offs, vals, scr, row, (const char *)xin));
            xout[row] = t;
            cplx s = sum[row];
            s.x += t.x;
            s.y += t.y;
            sum[row] = s;
        }
        __syncthreads();
    };
    for (int sub = 0; sub < nsub; ++sub) {
        const double c0 = ratio[0];
        for (int row = tid; row < N; row += T) {
            const cplx v = sum[row];
            xa[row] = v;  // the chain starts from v itself, the sum from T_0 = c_0 v
            sum[row] = c_make(c0 * v.x, c0 * v.y);
        }
        __syncthreads();
        for (int j = 1; j <= m; j += 2) {
            term(j, xa, xb);
            if (j + 1 > m) break;
            term(j + 1, xb, xa);
        }
    }
    return nsub * m;
}

// ---------------------------------------------------------------------------
// plain propagation with storage (backward sweep / iteration-0 forward sweep): objectives in turns
// ---------------------------------------------------------------------------
template <int T>
__global__ void __launch_bounds__(T)
kh_ellg_sweep_store(KhSweepArgs p, const KhEll *__restrict__ ells, const int *__restrict__ offs, const cplx *__restrict__ vals,
                    const double *__restrict__ pulses, const cplx *__restrict__ state_in, cplx *__restrict__ store,
                    cplx *__restrict__ state_out, int direction, cplx *ws, long long ws_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KhEllLds s = kh_ell_carve<0>(smem);
    const KhEllgWs w = kh_ellg_carve_ws(ws, ws_stride, p.N);
    const int tid = threadIdx.x, N = p.N, L = p.L, nt = p.nt;
    double matvecs = 0.0;
    int m_cur = -1;
    if (tid <= KH_MAX_DEGREE) s.deg[tid] = p.q2_theta[tid];
    __syncthreads();
    for (int k = blockIdx.x; k < p.K; k += gridDim.x) {
        const KhEll el = ells[k];
        const double *norms_k = p.op_norms + (size_t)k * (1 + L);
        auto put = [&](cplx *dst) {
            for (int row = tid; row < N; row += T) dst[row] = w.sum[row];
        };
        for (int row = tid; row < N; row += T) w.sum[row] = state_in[(size_t)k * N + row];
        if (store != nullptr) put(store + ((size_t)k * nt + (direction > 0 ? 0 : nt - 1)) * N);
        KhDegreeCache dc = {12, 1.0, 0.0};
        for (int step = 0; step < nt - 1; ++step) {
            const int n = direction > 0 ? step : nt - 2 - step;
            double theta = norms_k[0];
            for (int l = 0; l < L; ++l) {
                const double v = pulses[(size_t)l * (nt - 1) + n];
                if (tid == l) s.eps[l] = v;
                theta += fabs(v) * norms_k[1 + l];
            }
            const double dt = p.dt[n];
            __syncthreads();  // (s.eps; also: the previous interval's last term has been read by everybody)
            kh_ellg_rebuild<T>(el, vals, w.scr, tid, L, s.eps, N);
            int nsub, m;
            kh_degree_cached(theta * dt, s.deg, p.theta_max, p.inv_theta_max, dc, &nsub, &m);
            if (m != m_cur) {
                kh_ell_load_ratios(p, s, m, tid);
                m_cur = m;
            }
            matvecs += kh_ellg_expm_action<T>(el, offs, vals, w.scr, w.sum, w.xa, w.xb, s.ratio, p.fre, p.fim, dt, nsub, m, tid, N);
            if (store != nullptr) put(store + ((size_t)k * nt + (direction > 0 ? n + 1 : n)) * N);
        }
        if (state_out != nullptr) put(state_out + (size_t)k * N);
    }
    if (tid == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);
}

// ---------------------------------------------------------------------------
// forward sweep with sequential pulse update (optimize.py:444-508): ONE launch on any grid, sums exchanged in-kernel
// ---------------------------------------------------------------------------
// Workgroup g owns the objectives k = g, g + gridDim.x, ...; their states live in u.phi, which is also the series'
// running sum (row-private) and, between the intervals, the vector the control products gather from.
template <int T, bool SO>
__global__ void __launch_bounds__(T)
kh_ellg_forward_update(KhSweepArgs p, const KhEll *__restrict__ ells, const int *__restrict__ offs,
                       const cplx *__restrict__ vals, KhUpdateArgs u, KhExchange ex, cplx *ws, long long ws_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KhEllLds s = kh_ell_carve<0>(smem);
    double *part_sh = s.g_a + KH_MAX_L;  // [KH_MAX_L] the workgroup's partial sums, its objectives added in order
    const KhEllgWs w = kh_ellg_carve_ws(ws, ws_stride, p.N);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, N = p.N, L = p.L, nt = p.nt;
    const int wg = blockIdx.x;
    double matvecs = 0.0;
    if (tid < KH_MAX_L) s.g_a[tid] = 0.0;
    int m_cur = -1;
    KhDegreeCache dc = {12, 1.0, 0.0};
    if (tid <= KH_MAX_DEGREE) s.deg[tid] = p.q2_theta[tid];  // (visible after the first barrier below)
    if constexpr (SO) {
        for (int k = wg; k < p.K; k += gridDim.x)
            for (int row = tid; row < N; row += T) u.fw_store[((size_t)k * nt) * N + row] = u.phi[(size_t)k * N + row];
    }

    // part_sh[l] = sum over the workgroup's objectives of ||chi_k|| Im(mu <chi_k(t_n) + 0.5 sigma/||chi_k|| (phi_k -
    // phi_prev) | A_lk phi_k(t_n)>); phi_k(t_n) = u.phi[k], written by this workgroup in front of a barrier
    auto partial_sums = [&](int n) {
        if (tid < KH_MAX_L) part_sh[tid] = 0.0;
        for (int k = wg; k < p.K; k += gridDim.x) {
            const KhEll el = ells[k];
            const double chi_norm = u.chi_norms[k];
            const cplx *phi = u.phi + (size_t)k * N;
            const cplx *chi = u.chi_store + ((size_t)k * nt + n) * N;
            for (int l = 0; l < L; ++l) {
                double v = 0.0;
                for (int row = tid; row < N; row += T) {
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
            matvecs += (double)L;
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
            double part[KH_MAX_L];
            for (int l = 0; l < KH_MAX_L; ++l) part[l] = l < L ? part_sh[l] : 0.0;
            kh_exchange_waves_publish(ex, n, wg, L, lane, part, s.D, s.ok);
        }
        kh_exchange_waves_gather(ex, n, L, wave, lane, s.D, s.ok);
        __syncthreads();
        if (!kh_exchange_waves_finish(ex, n, wg, L, wave, lane, s.D, s.ok)) return;
        // ---- pulse update (optimize.py:471-477): once per workgroup; workgroup 0 stores the values ----
        const double dt = p.dt[n];
        kh_pulse_update(u, p.op_norms + (size_t)wg * (1 + L), s.D, n, nt, L, wg, tid, dt, s.eps, s.g_a);
        __syncthreads();
        // ---- propagate every objective of the workgroup over interval n (optimize.py:479-491) ----
        for (int k = wg; k < p.K; k += gridDim.x) {
            const KhEll el = ells[k];
            const double *norms_k = p.op_norms + (size_t)k * (1 + L);
            cplx *phi = u.phi + (size_t)k * N;
            double theta = norms_k[0];
            for (int l = 0; l < L; ++l) theta += fabs(s.eps[l]) * norms_k[1 + l];
            kh_ellg_rebuild<T>(el, vals, w.scr, tid, L, s.eps, N);
            int nsub, m;
            kh_degree_cached(theta * dt, s.deg, p.theta_max, p.inv_theta_max, dc, &nsub, &m);
            if (m != m_cur) {
                kh_ell_load_ratios(p, s, m, tid);
                m_cur = m;
            }
            matvecs += kh_ellg_expm_action<T>(el, offs, vals, w.scr, phi, w.xa, w.xb, s.ratio, p.fre, p.fim, dt, nsub, m, tid, N);
            if constexpr (SO) {
                for (int row = tid; row < N; row += T) u.fw_store[((size_t)k * nt + n + 1) * N + row] = phi[row];
            }
        }
        // ---- partial sums of the next interval ----
        if (n + 1 < nt - 1) partial_sums(n + 1);
    }
    if (wg == 0 && tid < L) u.g_a[tid] = s.g_a[tid];
    if (tid == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);
}
