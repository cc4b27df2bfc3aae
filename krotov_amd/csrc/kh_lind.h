// Lindblad-form sweep kernels ("lindblad/matrix"): density matrices under a d x d Hamiltonian and Lindblad operators,
// propagated in MATRIX form -- no d^2 x d^2 Liouvillian is ever built.
//
//   d/dt rho = A rho + rho B + sum_j C_j rho C_j^+,   A = -i H(eps) - M/2,  B = +i H(eps) - M/2,  M = sum_j C_j^+ C_j
//
// (A and B are kept apart: for a non-Hermitian H this is exactly -i (H rho - rho H), what liouvillian(H, c_ops) builds).
// The backward sweep runs the same form on the adjoint operators: A^+ chi + chi B^+ + sum_j C_j^+ chi C_j.  States stay
// what they are everywhere else in the library: column-stacked vec(rho) of length N = d^2 in every buffer.
//
// One 256-thread workgroup per objective (objectives in turns where K exceeds the grid).  Everything a series term
// touches sits in LDS: A (column-major), B, the Lindblad operators (column-major), the term matrix ping-ponging between
// two buffers, and W_j = T C_j^+ of the term at hand.  A thread owns RB consecutive rows of one column of the result
// (RB = 1 for d <= 16, 2 for d <= 22, 4 for d <= 32: RB * 256 >= d^2); a term is 2 + 2 n_c complex d x d x d products
// on fp64 vector FMAs, two workgroup barriers (one without Lindblad operators), no global memory.
// The update sums need no product per control: tr(chi^+ [H_l, rho]) = sum_rc Y[r][c] H_l[c][r] with
// Y = rho chi^+ - chi^+ rho formed once per interval.
#pragma once

#include "kh_common.h"
#include "kh_generic.h"

#define KH_LIND_THREADS 256
#define KH_LIND_DMAX 32     // d x d density matrices up to this d
#define KH_LIND_MAX_NC 4    // Lindblad operators per objective
#define KH_LIND_MAX_L 4     // controls
#define KH_LIND_LDS_MAX (160 * 1024)

struct KhLindArgs {
    int d, n_c;
    int nw;                    // W buffers in LDS (1 .. n_c; the Lindblad operators are taken nw at a time)
    double sgn;                // A = A0 + sgn i sum eps_l G_l, B = B0 - sgn i sum eps_l G_l: -1 forward (G = H_l), +1 backward (G = H_l^+)
    const cplx *const *cops;   // [K*n_c] Lindblad operators of this direction (row-major d x d; backward: adjoints), NULL: absent
    const cplx *const *A0;     // [K] -i H0 - M/2 (backward: its adjoint), row-major
    const cplx *const *B0;     // [K] +i H0 - M/2 (backward: its adjoint), row-major
};

__host__ __device__ inline int kh_lind_rb(int d) { return d <= 16 ? 1 : (d <= 22 ? 2 : 4); }

// LDS: At B T0 T1 | Ct[n_c] | W[max(nw, 1)] (d x d each), then the per-control scalars
__host__ __device__ inline size_t kh_lind_lds_bytes(int d, int n_c, int nw) {
    const size_t mats = 4 + (size_t)n_c + (size_t)(nw > 1 ? nw : 1);
    return mats * d * d * sizeof(cplx) + ((KH_LIND_THREADS / 64) * 2 * KH_MAX_L + 4 * KH_MAX_L + KH_RATIO_STRIDE) * sizeof(double) + 64;
}

struct KhLindLds {
    cplx *At, *B, *T0, *T1, *Ct, *W;
    double *red, *D, *eps, *part, *ga, *ratio;
    int *ok;
};

__device__ __forceinline__ KhLindLds kh_lind_carve(char *smem, int d, int n_c, int nw) {
    const int dd = d * d;
    KhLindLds s;
    s.At = (cplx *)smem;
    s.B = s.At + dd;
    s.T0 = s.B + dd;
    s.T1 = s.T0 + dd;
    s.Ct = s.T1 + dd;
    s.W = s.Ct + (size_t)n_c * dd;
    s.red = (double *)(s.W + (size_t)(nw > 1 ? nw : 1) * dd);
    s.D = s.red + (KH_LIND_THREADS / 64) * 2 * KH_MAX_L;
    s.eps = s.D + KH_MAX_L;
    s.part = s.eps + KH_MAX_L;
    s.ga = s.part + KH_MAX_L;
    s.ratio = s.ga + KH_MAX_L;
    s.ok = (int *)(s.ratio + KH_RATIO_STRIDE);
    return s;
}

// which entries of the d x d result this thread owns: rows r0 .. r0 + RB - 1 of column c (column-stacked index c d + r)
template <int RB>
struct KhLindOwn {
    int r0, c;
    bool active;
    int rr[RB];   // row indices clamped into the matrix (reads of rows past the end repeat the last row)
    bool in[RB];  // the row exists
};

template <int RB>
__device__ __forceinline__ KhLindOwn<RB> kh_lind_own(int d) {
    KhLindOwn<RB> o;
    const int nrb = (d + RB - 1) / RB, tid = threadIdx.x;
    o.active = tid < nrb * d;
    o.c = o.active ? tid / nrb : 0;
    o.r0 = o.active ? (tid % nrb) * RB : 0;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        o.in[i] = o.active && o.r0 + i < d;
        o.rr[i] = o.r0 + i < d ? o.r0 + i : d - 1;
    }
    return o;
}

// the Lindblad operators of objective k -> LDS, column-major (Ct[j][kk d + r] = C_j[r][kk]); absent: zeros.  All threads;
// the caller's next barrier completes it.
__device__ __forceinline__ void kh_lind_load_cops(const KhLindArgs &la, int k, const KhLindLds &s) {
    const int d = la.d, dd = d * d;
    for (int j = 0; j < la.n_c; ++j) {
        const cplx *C = la.cops[(size_t)k * la.n_c + j];
        for (int e = threadIdx.x; e < dd; e += KH_LIND_THREADS) {
            const int r = e / d, kk = e - r * d;
            s.Ct[(size_t)j * dd + kk * d + r] = C != nullptr ? C[e] : c_make(0.0, 0.0);
        }
    }
}

// A(eps) -> s.At (column-major), B(eps) -> s.B (row-major) of objective k.  All threads; ends with a barrier.
__device__ __forceinline__ void kh_lind_build(const KhSweepArgs &p, const KhLindArgs &la, int k, const double *eps,
                                              const KhLindLds &s) {
    const int d = la.d, dd = d * d, L = p.L;
    const cplx *A0 = la.A0[k], *B0 = la.B0[k];
    const cplx *const *ops_k = p.ops + (size_t)k * (1 + L);
    for (int e = threadIdx.x; e < dd; e += KH_LIND_THREADS) {
        cplx a = A0[e], b = B0[e];
        for (int l = 0; l < L; ++l) {
            const cplx *g = ops_k[1 + l];
            if (g == nullptr) continue;
            const cplx v = g[e];
            const double w = la.sgn * eps[l];  // w i v = (-w v.y, w v.x)
            a.x = fma(-w, v.y, a.x);
            a.y = fma(w, v.x, a.y);
            b.x = fma(w, v.y, b.x);
            b.y = fma(-w, v.x, b.y);
        }
        const int r = e / d, kk = e - r * d;
        s.At[kk * d + r] = a;
        s.B[e] = b;
    }
    __syncthreads();
}

// acc (this thread's entries of rho) <- exp(dt Lindbladian) rho, by nsub Taylor sub-steps of degree m.  s.At, s.B, s.Ct
// hold the interval's operators.  All threads of the workgroup call this; returns the terms issued.
template <int RB>
__device__ __forceinline__ int kh_lind_expm(const KhSweepArgs &p, const KhLindArgs &la, const double *norms_k,
                                            const double *eps, double dt, const KhLindLds &s, const KhLindOwn<RB> &o,
                                            cplx (&acc)[RB]) {
    const int tid = threadIdx.x, d = la.d, dd = d * d, L = p.L, n_c = la.n_c;
    double theta = norms_k[0];
    for (int l = 0; l < L; ++l) theta += fabs(eps[l]) * norms_k[1 + l];
    theta *= dt;
    int nsub, m;
    kh_degree_lookup(theta, p.q2_theta, p.theta_max, p.inv_theta_max, 12, &nsub, &m);
    // (every thread passes here with the same m; the previous call's readers of s.ratio are behind a barrier)
    if (tid <= m) s.ratio[tid] = p.ratios[(size_t)m * KH_RATIO_STRIDE + tid];
    const double h = dt / nsub;
    const int own0 = o.c * d + o.r0;
    for (int sub = 0; sub < nsub; ++sub) {
#pragma unroll
        for (int i = 0; i < RB; ++i)
            if (o.in[i]) s.T0[own0 + i] = acc[i];
        __syncthreads();
        const double c0 = s.ratio[0];
#pragma unroll
        for (int i = 0; i < RB; ++i) acc[i] = c_make(c0 * acc[i].x, c0 * acc[i].y);
        const cplx *xin = s.T0;
        cplx *xout = s.T1;
        for (int j = 1; j <= m; ++j) {
            const double hj = h * s.ratio[j];
            cplx P[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) P[i] = c_make(0.0, 0.0);
            if (o.active) {
                // A T + T B
                for (int kk = 0; kk < d; ++kk) {
                    const cplx tc = xin[o.c * d + kk], bc = s.B[kk * d + o.c];
#pragma unroll
                    for (int i = 0; i < RB; ++i) {
                        c_fma(P[i], s.At[kk * d + o.rr[i]], tc);
                        c_fma(P[i], xin[kk * d + o.rr[i]], bc);
                    }
                }
            }
            for (int j0 = 0; j0 < n_c; j0 += la.nw) {
                const int j1 = j0 + la.nw < n_c ? j0 + la.nw : n_c;
                if (j0 > 0) __syncthreads();  // (the previous group's W is read no more)
                if (o.active) {
                    // W_q = T C_q^+
                    for (int q = j0; q < j1; ++q) {
                        const cplx *Ct = s.Ct + (size_t)q * dd;
                        cplx w[RB];
#pragma unroll
                        for (int i = 0; i < RB; ++i) w[i] = c_make(0.0, 0.0);
                        for (int kk = 0; kk < d; ++kk) {
                            cplx cc = Ct[kk * d + o.c];  // C[c][kk]
                            cc.y = -cc.y;
#pragma unroll
                            for (int i = 0; i < RB; ++i) c_fma(w[i], xin[kk * d + o.rr[i]], cc);
                        }
                        cplx *W = s.W + (size_t)(q - j0) * dd;
#pragma unroll
                        for (int i = 0; i < RB; ++i)
                            if (o.in[i]) W[own0 + i] = w[i];
                    }
                }
                __syncthreads();
                if (o.active) {
                    // + C_q W_q
                    for (int q = j0; q < j1; ++q) {
                        const cplx *Ct = s.Ct + (size_t)q * dd, *W = s.W + (size_t)(q - j0) * dd;
                        for (int kk = 0; kk < d; ++kk) {
                            const cplx wc = W[o.c * d + kk];
#pragma unroll
                            for (int i = 0; i < RB; ++i) c_fma(P[i], Ct[kk * d + o.rr[i]], wc);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const cplx t = c_make(hj * P[i].x, hj * P[i].y);
                if (o.in[i]) xout[own0 + i] = t;
                acc[i].x += t.x;
                acc[i].y += t.y;
            }
            __syncthreads();
            cplx *tmp = (cplx *)xin;
            xin = xout;
            xout = tmp;
        }
    }
    return nsub * m;
}

template <int RB>
__device__ __forceinline__ void kh_lind_get(const cplx *__restrict__ src, const KhLindOwn<RB> &o, int d, cplx (&acc)[RB]) {
#pragma unroll
    for (int i = 0; i < RB; ++i) acc[i] = o.in[i] ? src[o.c * d + o.r0 + i] : c_make(0.0, 0.0);
}

template <int RB>
__device__ __forceinline__ void kh_lind_put(cplx *__restrict__ dst, const KhLindOwn<RB> &o, int d, const cplx (&acc)[RB]) {
#pragma unroll
    for (int i = 0; i < RB; ++i)
        if (o.in[i]) dst[o.c * d + o.r0 + i] = acc[i];
}

// ---------------------------------------------------------------------------
// plain propagation with storage (direction +1: forward, -1: backward; as kh_gen_sweep_store)
// ---------------------------------------------------------------------------
template <int RB>
__global__ void __launch_bounds__(KH_LIND_THREADS)
kh_lind_sweep_store(KhSweepArgs p, KhLindArgs la, const double *__restrict__ pulses, const cplx *__restrict__ state_in,
                    cplx *__restrict__ store, cplx *__restrict__ state_out, int direction) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KhLindLds s = kh_lind_carve(smem, la.d, la.n_c, la.nw);
    const int tid = threadIdx.x, d = la.d, N = p.N, L = p.L, nt = p.nt;
    const KhLindOwn<RB> o = kh_lind_own<RB>(d);
    double terms = 0.0;
    for (int k = blockIdx.x; k < p.K; k += gridDim.x) {
        const double *norms_k = p.op_norms + (size_t)k * (1 + L);
        kh_lind_load_cops(la, k, s);
        cplx acc[RB];
        kh_lind_get<RB>(state_in + (size_t)k * N, o, d, acc);
        if (store != nullptr) kh_lind_put<RB>(store + ((size_t)k * nt + (direction > 0 ? 0 : nt - 1)) * N, o, d, acc);
        for (int step = 0; step < nt - 1; ++step) {
            const int n = direction > 0 ? step : nt - 2 - step;
            if (tid < L) s.eps[tid] = pulses[(size_t)tid * (nt - 1) + n];
            __syncthreads();
            kh_lind_build(p, la, k, s.eps, s);
            terms += kh_lind_expm<RB>(p, la, norms_k, s.eps, p.dt[n], s, o, acc);
            if (store != nullptr) kh_lind_put<RB>(store + ((size_t)k * nt + (direction > 0 ? n + 1 : n)) * N, o, d, acc);
        }
        if (state_out != nullptr) kh_lind_put<RB>(state_out + (size_t)k * N, o, d, acc);
        __syncthreads();
    }
    if (tid == 0 && p.stats != nullptr) atomicAdd(p.stats, terms);
}

// ---------------------------------------------------------------------------
// forward sweep with sequential pulse update, first order, one launch (as kh_gen_forward_update with the in-kernel exchange)
// ---------------------------------------------------------------------------
// s.part[l] <- sum over this workgroup's objectives of norm_k Im tr(chi_k(t_n)^+ [H_lk, rho_k]); complete behind the
// function's last barrier.  resident: the workgroup's one objective keeps its state in acc.
template <int RB>
__device__ __forceinline__ void kh_lind_partials(const KhSweepArgs &p, const KhLindArgs &la, const KhUpdateArgs &u, int n,
                                                 const KhLindLds &s, const KhLindOwn<RB> &o, bool resident,
                                                 const cplx (&acc)[RB]) {
    const int tid = threadIdx.x, d = la.d, dd = d * d, N = p.N, L = p.L, nt = p.nt;
    const int wave = tid >> 6, lane = tid & 63;
    if (tid < L) s.part[tid] = 0.0;
    __syncthreads();
    cplx *R = s.T0, *X = s.W;  // rho and chi, column-stacked
    for (int k = blockIdx.x; k < p.K; k += gridDim.x) {
        if (resident) {
            kh_lind_put<RB>(R, o, d, acc);
        } else {
            for (int e = tid; e < dd; e += KH_LIND_THREADS) R[e] = u.phi[(size_t)k * N + e];
        }
        for (int e = tid; e < dd; e += KH_LIND_THREADS) X[e] = u.chi_store[((size_t)k * nt + n) * N + e];
        __syncthreads();
        // Y = rho chi^+ - chi^+ rho, this thread's entries
        cplx Y[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) Y[i] = c_make(0.0, 0.0);
        if (o.active) {
            for (int kk = 0; kk < d; ++kk) {
                cplx xc = X[kk * d + o.c];  // chi[c][kk]
                xc.y = -xc.y;
                const cplx rc = R[o.c * d + kk];  // rho[kk][c]
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    c_fma(Y[i], R[kk * d + o.rr[i]], xc);
                    cplx xr = X[o.rr[i] * d + kk];  // chi[kk][r]
                    xr.x = -xr.x;                   // -conj
                    c_fma(Y[i], xr, rc);
                }
            }
        }
        for (int l = 0; l < L; ++l) {
            const cplx *h = p.ops[(size_t)k * (1 + L) + 1 + l];
            double im = 0.0;
            if (h != nullptr) {
#pragma unroll
                for (int i = 0; i < RB; ++i)
                    if (o.in[i]) {
                        const cplx g = h[o.c * d + o.r0 + i];  // H_l[c][r]
                        im = fma(Y[i].x, g.y, im);
                        im = fma(Y[i].y, g.x, im);
                    }
            }
            im = sum64(im);
            if (lane == 0) s.red[wave * KH_MAX_L + l] = im;
        }
        __syncthreads();
        if (tid < L) {
            double im = 0.0;
            for (int w = 0; w < KH_LIND_THREADS / 64; ++w) im += s.red[w * KH_MAX_L + tid];
            s.part[tid] += u.chi_norms[k] * im;
        }
        __syncthreads();
    }
}

template <int RB>
__global__ void __launch_bounds__(KH_LIND_THREADS)
kh_lind_forward_update(KhSweepArgs p, KhLindArgs la, KhUpdateArgs u, KhExchange ex) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KhLindLds s = kh_lind_carve(smem, la.d, la.n_c, la.nw);
    const int tid = threadIdx.x, d = la.d, N = p.N, L = p.L, nt = p.nt;
    const int wave = tid >> 6, lane = tid & 63;
    const KhLindOwn<RB> o = kh_lind_own<RB>(d);
    double terms = 0.0;
    if (tid < L) s.ga[tid] = 0.0;
    // one objective per workgroup: its Lindblad operators and its state stay here for the whole sweep
    const bool resident = (int)gridDim.x >= p.K;
    cplx acc[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) acc[i] = c_make(0.0, 0.0);
    if (resident) {
        kh_lind_load_cops(la, blockIdx.x, s);
        kh_lind_get<RB>(u.phi + (size_t)blockIdx.x * N, o, d, acc);
    }
    kh_lind_partials<RB>(p, la, u, 0, s, o, resident, acc);
    for (int n = 0; n < nt - 1; ++n) {
        // ---- cross-objective sum D_l (optimize.py:470) ----
        if (wave == 0) {
            double part[KH_LIND_MAX_L], D[KH_LIND_MAX_L];
#pragma unroll
            for (int l = 0; l < KH_LIND_MAX_L; ++l) part[l] = l < L ? s.part[l] : 0.0;
            const bool ok = kh_exchange<KH_LIND_MAX_L, KH_GATHER_CHUNKS, false>(ex, n, blockIdx.x, L, lane, part, D);
            if (lane == 0) {
                for (int l = 0; l < L; ++l) s.D[l] = D[l];
                *s.ok = ok ? 1 : 0;
            }
        }
        __syncthreads();
        if (!*s.ok) return;
        // ---- pulse update (optimize.py:471-477): thread l takes control l ----
        const double dt = p.dt[n];
        if (tid < L) {
            const int l = tid;
            const double S = u.shape[(size_t)l * (nt - 1) + n];
            const double lam = u.lambda[l];
            const double d1 = s.D[l];
            const double e = u.guess[(size_t)l * (nt - 1) + n] + (S / lam) * d1;
            s.eps[l] = e;
            s.ga[l] += (S / lam) * (d1 * d1) * dt;
            if (blockIdx.x == 0) u.opt[(size_t)l * (nt - 1) + n] = e;
        }
        __syncthreads();
        // ---- propagate every local objective over interval n (optimize.py:479-491) ----
        for (int k = blockIdx.x; k < p.K; k += gridDim.x) {
            if (!resident) {
                kh_lind_load_cops(la, k, s);
                kh_lind_get<RB>(u.phi + (size_t)k * N, o, d, acc);
            }
            kh_lind_build(p, la, k, s.eps, s);
            terms += kh_lind_expm<RB>(p, la, p.op_norms + (size_t)k * (1 + L), s.eps, dt, s, o, acc);
            if (!resident || n + 1 == nt - 1) kh_lind_put<RB>(u.phi + (size_t)k * N, o, d, acc);
            __syncthreads();
        }
        // ---- partial sums of the next interval (phi written above by this same workgroup: visible after the barrier) ----
        if (n + 1 < nt - 1) kh_lind_partials<RB>(p, la, u, n + 1, s, o, resident, acc);
    }
    if (blockIdx.x == 0 && tid < L) u.g_a[tid] = s.ga[tid];
    if (tid == 0 && p.stats != nullptr) atomicAdd(p.stats, terms);
}

// A0 = -i H0 - M/2, B0 = +i H0 - M/2 with M = sum_j C_j^+ C_j, one workgroup per objective (engine creation)
__global__ void kh_lind_setup_kernel(const cplx *const *__restrict__ ops /*[K*(1+L)]*/, const cplx *const *__restrict__ cops /*[K*n_c]*/,
                                     cplx *__restrict__ A0 /*[K][d*d]*/, cplx *__restrict__ B0, int Lp1, int n_c, int d)
#if KH_DEFINES(KH_TU_MAIN)
{
    const int k = blockIdx.x, dd = d * d;
    const cplx *H0 = ops[(size_t)k * Lp1];
    for (int e = threadIdx.x; e < dd; e += blockDim.x) {
        const int r = e / d, c = e - r * d;
        cplx M = c_make(0.0, 0.0);
        for (int j = 0; j < n_c; ++j) {
            const cplx *C = cops[(size_t)k * n_c + j];
            if (C == nullptr) continue;
            for (int kk = 0; kk < d; ++kk) c_fma_conj(M, C[kk * d + r], C[kk * d + c]);
        }
        const cplx h = H0[e];
        A0[(size_t)k * dd + e] = c_make(h.y - 0.5 * M.x, -h.x - 0.5 * M.y);
        B0[(size_t)k * dd + e] = c_make(-h.y - 0.5 * M.x, h.x - 0.5 * M.y);
    }
}
#else
    ;  // (defined in the translation unit that owns it: kh_common.h, KH_DEFINES)
#endif
