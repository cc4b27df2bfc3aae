// Many independent small optimisations in one launch ("replica16/wave"): B replicas of one shape -- K_r <= 8 objectives,
// N <= 16, 1..4 controls, nt grid points, one kind -- each a complete optimize_pulses problem of its own.
//
// The mappings are kh_mini.h's: a 16 x 16 complex tile is 4 elements per lane of one wave (lane = row * 4 + column
// quarter), the vector stays in registers and is fetched with ds_bpermute, and a replica's objectives are the waves of
// ONE workgroup, so its update sums cross through LDS with one __syncthreads per interval.  Replicas never talk to each
// other: no exchange slots, no polling, no co-residency requirement -- with more replicas than the device holds at
// once the later workgroups simply run later, and nothing here waits on another workgroup.
//
// Objective k belongs to replica b = k / K_r.  Pulses, shapes and output pulses are [B][L][nt-1], lambda and g_a are
// [B][L], the time steps (KhSweepArgs::dt) are [B][nt-1].  The series plan (theta, sub-steps, degree) is formed per
// wave from the objective's own op_norms and its replica's pulse values and dt: two waves of a workgroup may run
// different numbers of products; every barrier is outside the series.
//
// Arithmetic.  L = 1: kh_mini_forward_update's A^2 chain (q2_rows tables, staged P0, P1, P2), instruction for
// instruction.  L = 2..4: the generator tile a = h0 + sum_l eps_l h_l is built per interval in registers by fused
// multiply-adds in control order and the series goes term by term from the engine's `ratios` rows -- the
// one-term-per-phase form of kh_tile64.h, one kh_mini_matvec per term; the row of the current degree sits in the
// lanes of the wave (lane j holds ratio j) and is read with v_readlane: no LDS, no table load inside the series.
//
// `active` ([B], or NULL: all): a workgroup whose replica is inactive returns before its first barrier and before any
// store; every slice of every output buffer that belongs to that replica keeps what it held.
//
// Second order (kh_rep_forward_update_so): sigma is [B][nt-1], one row per replica; the forward trajectories are [K][nt][N]
// like the co-state store.  See the update kernel below.
#pragma once

#include "kh_mini.h"

template <int LT>
struct KhRepLds {
    double deg[KH_MAX_DEGREE + 1];
    double part[2][LT][KH_MINI_MAXK];  // the objectives' partial sums per control, by interval parity
    __device__ __forceinline__ const double *degrees() const { return deg; }
    __device__ __forceinline__ double &sum(int par, int l, int w) { return part[par][l][w]; }
};
template <>
struct KhRepLds<1> {
    KhMiniLds m;  // (the series tables of the A^2 chain; its part[][] serves the one control)
    __device__ __forceinline__ const double *degrees() const { return m.deg; }
    __device__ __forceinline__ double &sum(int par, int, int w) { return m.part[par][w]; }
};

template <int LT>
__device__ __forceinline__ void kh_rep_stage_tables(const KhSweepArgs &p, KhRepLds<LT> &s, int tid, int nthreads) {
    if constexpr (LT == 1) {
        kh_mini_stage_tables(p, s.m, tid, nthreads);
    } else {
        for (int i = tid; i <= KH_MAX_DEGREE; i += nthreads) s.deg[i] = p.q2_theta[i];
    }
}

// The `ratios` row of the current degree, spread over the wave: lane j holds ratio j (j < 64), `top` ratio 64.
struct KhRepRatios {
    int m;
    double lanes, top;
};

__device__ __forceinline__ void kh_rep_load_ratios(const KhSweepArgs &p, KhRepRatios &c, int m, int lane) {
    if (c.m == m) return;  // (wave-uniform; the usual case along a smooth pulse)
    c.m = m;
    const double *row = p.ratios + (size_t)m * KH_RATIO_STRIDE;
    c.lanes = row[lane];
    c.top = kh_uniform(row[KH_MAX_DEGREE]);
}

// state <- series(f A dt) state, term by term: T_0 = c_0 v, T_j = ratio_j (f h A) T_{j-1} (kh_tile64.h's form)
__device__ __forceinline__ int kh_rep_expm_action(const cplx (&a)[4], cplx &state, const KhRepRatios &c, double fre,
                                                  double fim, double dt, int nsub, int m, int lane) {
    const double h = nsub == 1 ? dt : dt / nsub;
    const double c0 = readlane_f64(c.lanes, 0);
    for (int sub = 0; sub < nsub; ++sub) {
        cplx term = state;  // (ratio 1 is relative to v itself)
        state = c_make(c0 * state.x, c0 * state.y);
        for (int j = 1; j <= m; ++j) {
            const double hj = h * (j < 64 ? readlane_f64(c.lanes, j) : c.top);
            term = c_mul(c_make(fre * hj, fim * hj), kh_mini_matvec(a, term, lane));
            state.x += term.x;
            state.y += term.y;
        }
    }
    return nsub * m;
}

// The operator tiles of one objective, its norm bounds, and the interval's propagation in either arithmetic
template <int LT>
struct KhRepTiles {
    cplx h[1 + LT][4];
    cplx sq[LT == 1 ? 3 : 1][4];  // P0, P1, P2 of A^2 (one control)
    double nrm[1 + LT];

    __device__ __forceinline__ void load(const KhSweepArgs &p, const cplx *const *sqp, int k, int lane) {
#pragma unroll
        for (int o = 0; o <= LT; ++o) {
            kh_mini_load_tile(p.ops[(size_t)k * (1 + LT) + o], p.N, lane, h[o]);
            nrm[o] = kh_uniform(p.op_norms[(size_t)k * (1 + LT) + o]);
        }
        if constexpr (LT == 1) {
#pragma unroll
            for (int o = 0; o < 3; ++o) kh_mini_load_tile(sqp[(size_t)k * 3 + o], p.N, lane, sq[o]);
        }
    }
};

struct KhRepSeries {
    KhDegreeCache dc;
    KhMiniCoef coef;   // one control
    KhRepRatios rat;   // several
    __device__ __forceinline__ void reset() {
        dc = {12, 1.0, 0.0};
        coef.m = -1;
        rat.m = -1;
    }
};

// one interval of this wave's objective under the pulse values eps[]; returns the products issued
template <int LT>
__device__ __forceinline__ int kh_rep_interval(const KhSweepArgs &p, const KhRepTiles<LT> &t, KhRepLds<LT> &s,
                                               KhRepSeries &ser, const double (&eps)[LT], double dt, cplx &state,
                                               int lane) {
    int nsub, m;
    if constexpr (LT == 1) {
        kh_degree_cached((t.nrm[0] + fabs(eps[0]) * t.nrm[1]) * dt, s.degrees(), p.theta_max, p.inv_theta_max, ser.dc, &nsub, &m);
        kh_mini_coefficients(ser.coef, s.m, m, nsub, dt, p.fre, p.fim);
        cplx a[4], b[4];
        kh_mini_build(eps[0], t.h[0], t.h[1], t.sq[0], t.sq[1], t.sq[2], a, b);
        return kh_mini_expm_action(a, b, state, s.m, ser.coef, p.fre, p.fim, dt, nsub, m, lane);
    } else {
        double theta = t.nrm[0];
#pragma unroll
        for (int l = 0; l < LT; ++l) theta += fabs(eps[l]) * t.nrm[1 + l];
        kh_degree_cached(theta * dt, s.degrees(), p.theta_max, p.inv_theta_max, ser.dc, &nsub, &m);
        nsub = __builtin_amdgcn_readfirstlane(nsub);  // (wave-uniform: the series' loops run on scalar counters)
        m = __builtin_amdgcn_readfirstlane(m);
        kh_rep_load_ratios(p, ser.rat, m, lane);
        cplx a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cplx v = t.h[0][j];
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                v.x = fma(eps[l], t.h[1 + l][j].x, v.x);
                v.y = fma(eps[l], t.h[1 + l][j].y, v.y);
            }
            a[j] = v;
        }
        return kh_rep_expm_action(a, state, ser.rat, p.fre, p.fim, dt, nsub, m, lane);
    }
}

// ---------------------------------------------------------------------------
// plain propagation with storage: one single-wave workgroup per objective, grid B * K_r
// ---------------------------------------------------------------------------
template <int LT>
__global__ void __launch_bounds__(64)
kh_rep_sweep_store(KhSweepArgs p, const cplx *const *__restrict__ sq, const double *__restrict__ pulses,
                   const cplx *__restrict__ state_in, cplx *__restrict__ store, cplx *__restrict__ state_out,
                   int direction, int Kr, const int *__restrict__ active) {
    __shared__ KhRepLds<LT> s;
    const int lane = threadIdx.x, r = lane >> 2, k = blockIdx.x, b = k / Kr;
    if (active != nullptr && active[b] == 0) return;
    const bool writer = (lane & 3) == 0;
    const int N = p.N, nt = p.nt;
    const double *dts = p.dt + (size_t)b * (nt - 1);
    const double *eps_b = pulses + (size_t)b * LT * (nt - 1);
    kh_rep_stage_tables(p, s, lane, 64);
    KhRepTiles<LT> t;
    t.load(p, sq, k, lane);
    cplx state = r < N ? state_in[(size_t)k * N + r] : c_make(0.0, 0.0);
    __syncthreads();  // (the tables)
    const bool stores = store != nullptr && writer && r < N;
    if (stores) store[((size_t)k * nt + (direction > 0 ? 0 : nt - 1)) * N + r] = state;
    double matvecs = 0.0;
    KhRepSeries ser;
    ser.reset();
    // the interval's scalars are fetched one interval ahead and consumed before the interval's state is stored
    // (kh_mini.h, kh_mini_sweep_store: loads and stores share one in-order counter)
    const int n0 = direction > 0 ? 0 : nt - 2;
    double eps_next[LT], dt_next = kh_uniform(dts[n0]);
#pragma unroll
    for (int l = 0; l < LT; ++l) eps_next[l] = kh_uniform(eps_b[(size_t)l * (nt - 1) + n0]);
    for (int step = 0; step < nt - 1; ++step) {
        const int n = direction > 0 ? step : nt - 2 - step;
        const double dt = dt_next;
        double eps[LT], eps_ld[LT], dt_ld = 0.0;
#pragma unroll
        for (int l = 0; l < LT; ++l) eps[l] = eps_next[l], eps_ld[l] = 0.0;
        if (step + 1 < nt - 1) {
            const int nn = direction > 0 ? n + 1 : n - 1;
            dt_ld = dts[nn];
#pragma unroll
            for (int l = 0; l < LT; ++l) eps_ld[l] = eps_b[(size_t)l * (nt - 1) + nn];
        }
        matvecs += kh_rep_interval<LT>(p, t, s, ser, eps, dt, state, lane);
        dt_next = kh_uniform(dt_ld);
#pragma unroll
        for (int l = 0; l < LT; ++l) eps_next[l] = kh_uniform(eps_ld[l]);
        if (stores) store[((size_t)k * nt + (direction > 0 ? n + 1 : n)) * N + r] = state;
    }
    if (state_out != nullptr && writer && r < N) state_out[(size_t)k * N + r] = state;
    if (lane == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);
}

// ---------------------------------------------------------------------------
// forward sweep with sequential pulse update (optimize.py:444-508): ONE workgroup per replica, grid B, block 64 K_r,
// wave w = objective b K_r + w.  init / psi_T: [K][N] (read and written directly: an inactive replica's rows are never
// touched); u.guess / u.shape / u.opt: [B][L][nt-1]; u.lambda / u.g_a: [B][L].
//
// SO (second order, kh_set_second_order_replicas): u.fw_prev / u.fw_store are [K][nt][N], u.sigma is [B][nt-1] -- every
// replica its own row.  The bra of interval n is chi + sigma_n / (2 ||chi||) (phi - phi_prev) (optimize.py:468-469;
// kh_mini_forward_update<true>'s two fused multiply-adds, once per interval: all L controls share it), phi_prev's row
// and sigma_n come one interval ahead with chi's, and fw_store[k][n] takes the state before interval n is propagated,
// fw_store[k][nt-1] the final one.  One body serves both orders; the two kernels below differ in SO only, and the
// first-order one keeps its name (kh_debug_launched) and its code.
// ---------------------------------------------------------------------------
template <int LT, bool SO>
__device__ __forceinline__ void kh_rep_update_body(const KhSweepArgs &p, const cplx *const *__restrict__ sq,
                                                   const KhUpdateArgs &u, const cplx *__restrict__ init,
                                                   cplx *__restrict__ psi_T, int Kr, const int *__restrict__ active,
                                                   KhRepLds<LT> &s) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane >> 2, b = blockIdx.x, k = b * Kr + w;
    if (active != nullptr && active[b] == 0) return;  // (uniform over the workgroup: before the first barrier)
    const bool writer = (lane & 3) == 0;
    const int N = p.N, nt = p.nt;
    const double *dts = p.dt + (size_t)b * (nt - 1);
    const double *guess_b = u.guess + (size_t)b * LT * (nt - 1), *shape_b = u.shape + (size_t)b * LT * (nt - 1);
    double *opt_b = u.opt + (size_t)b * LT * (nt - 1);
    kh_rep_stage_tables(p, s, tid, blockDim.x);
    KhRepTiles<LT> t;  // (h[1 + l] is also dH/d eps_l, mu.py:123-134)
    t.load(p, sq, k, lane);
    const double chi_norm = u.chi_norms[k];
    cplx state = r < N ? init[(size_t)k * N + r] : c_make(0.0, 0.0);
    __syncthreads();  // (the tables)
    double matvecs = 0.0;

    // chi(t_n) (and, second order, phi_prev(t_n), sigma_n of this replica) of this lane's row, fetched one interval ahead
    cplx chi = c_make(0.0, 0.0), prev = c_make(0.0, 0.0);
    double sig = 0.0;
    const double *sigma_b = SO ? u.sigma + (size_t)b * (nt - 1) : nullptr;
    auto load_bra = [&](int n) {
        if (writer && r < N) {
            chi = u.chi_store[((size_t)k * nt + n) * N + r];
            if constexpr (SO) prev = u.fw_prev[((size_t)k * nt + n) * N + r];
        }
        if constexpr (SO) sig = sigma_b[n];
    };
    // this objective's  ||chi|| Im(mu <bra(t_n)|H_l phi>)  -> part[n & 1][l][w]
    auto partial = [&](int n) {
        cplx bra = chi;
        if constexpr (SO) {  // bra = chi + sigma / (2 ||chi||) (phi - phi_prev)  (optimize.py:468-469)
            if (writer && r < N) {
                const double hs = 0.5 * sig / chi_norm;
                bra = c_make(fma(hs, state.x - prev.x, chi.x), fma(hs, state.y - prev.y, chi.y));
            }
        }
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            const cplx y = kh_mini_matvec(t.h[1 + l], state, lane);
            cplx ov = c_make(0.0, 0.0);
            c_fma_conj(ov, bra, y);
            const double v = sum64(u.mu_re * ov.y + u.mu_im * ov.x);
            if (lane == 0) s.sum(n & 1, l, w) = chi_norm * v;
        }
        matvecs += LT;
    };

    if (nt - 1 > 0) {
        load_bra(0);
        partial(0);
    }
    __syncthreads();
    double g_a_loc[LT], lam[LT], guess_next[LT], shape_next[LT];
    double dt_next = dts[0];
#pragma unroll
    for (int l = 0; l < LT; ++l) {
        g_a_loc[l] = 0.0;
        lam[l] = u.lambda[(size_t)b * LT + l];
        guess_next[l] = guess_b[(size_t)l * (nt - 1)];
        shape_next[l] = shape_b[(size_t)l * (nt - 1)];
    }
    KhRepSeries ser;
    ser.reset();
    for (int n = 0; n < nt - 1; ++n) {
        const int par = n & 1;
        const double dt = kh_uniform(dt_next);
        double guess[LT], shape[LT];
#pragma unroll
        for (int l = 0; l < LT; ++l) guess[l] = guess_next[l], shape[l] = shape_next[l];
        if (n + 1 < nt - 1) {  // next interval's scalars and co-state row: in flight during this interval
            dt_next = dts[n + 1];
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                guess_next[l] = guess_b[(size_t)l * (nt - 1) + n + 1];
                shape_next[l] = shape_b[(size_t)l * (nt - 1) + n + 1];
            }
            load_bra(n + 1);
        }
        // ---- cross-objective sum (optimize.py:470) through LDS, in objective order; pulse update (optimize.py:471-477) ----
        double eps[LT];
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            double d1 = 0.0;
            for (int q = 0; q < Kr; ++q) d1 += s.sum(par, l, q);
            const double stepw = shape[l] / lam[l];
            eps[l] = kh_uniform(guess[l] + stepw * d1);
            g_a_loc[l] += stepw * (d1 * d1) * dt;
            if (tid == 0) opt_b[(size_t)l * (nt - 1) + n] = eps[l];
        }
        if constexpr (SO) {  // (behind the next interval's loads: kh_mini.h, kh_mini_sweep_store, on the shared counter)
            if (writer && r < N) u.fw_store[((size_t)k * nt + n) * N + r] = state;
        }
        // ---- propagate over interval n with the updated pulse (optimize.py:479-491) ----
        matvecs += kh_rep_interval<LT>(p, t, s, ser, eps, dt, state, lane);
        if (n + 1 < nt - 1) partial(n + 1);
        __syncthreads();  // everybody's partial sums of the next interval are in LDS
    }
    if (writer && r < N) {
        psi_T[(size_t)k * N + r] = state;
        if constexpr (SO) u.fw_store[((size_t)k * nt + nt - 1) * N + r] = state;
    }
    if (tid == 0) {
#pragma unroll
        for (int l = 0; l < LT; ++l) u.g_a[(size_t)b * LT + l] = g_a_loc[l];
    }
    if (lane == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);
}

template <int LT>
__global__ void __launch_bounds__(64 * KH_MINI_MAXK)
kh_rep_forward_update(KhSweepArgs p, const cplx *const *__restrict__ sq, KhUpdateArgs u, const cplx *__restrict__ init,
                      cplx *__restrict__ psi_T, int Kr, const int *__restrict__ active) {
    __shared__ KhRepLds<LT> s;
    kh_rep_update_body<LT, false>(p, sq, u, init, psi_T, Kr, active, s);
}

template <int LT>
__global__ void __launch_bounds__(64 * KH_MINI_MAXK)
kh_rep_forward_update_so(KhSweepArgs p, const cplx *const *__restrict__ sq, KhUpdateArgs u,
                         const cplx *__restrict__ init, cplx *__restrict__ psi_T, int Kr,
                         const int *__restrict__ active) {
    __shared__ KhRepLds<LT> s;
    kh_rep_update_body<LT, true>(p, sq, u, init, psi_T, Kr, active, s);
}
