// Expectation values of a stored trajectory, on the device (kh_expect of include/krotov_hip.h).
//
// What every workflow does after a propagation -- populations, energies, <O>(t) for a list of operators (the
// reference's Objective.propagate(..., e_ops=...), objectives.py:338-433, evaluates them state by state on the host) --
// for all K objectives and all nt grid points at once, without the trajectory leaving the device.
//
//   states [K][nt][N]   a stored trajectory in the layout every sweep writes, read only
//   tab    [K][n_e]     device pointers to dense row-major operators; equal pointers: a shared operator; NULL: that
//                       objective / operator pair is skipped and its outputs are exact zeros
//   out    [n_e][K][nt] written, every element exactly once
//
// Two forms, chosen by the engine's kind:
//
//   kh_expect_hilbert     out[e][k][n] = <psi_k(t_n)| O_ke |psi_k(t_n)>, O is N x N.  A batch of (N x N)(N x nt) products
//       whose result is contracted with conj(psi) at once: the operand mapping of kh_gen_adjoint_side (kh_generic.h) on
//       v_mfma_f64_16x16x4 -- A = operator block [row lane & 15][k lane >> 4], B = sixteen states [k lane >> 4][time
//       point lane & 15], D = [row 4 reg + (lane >> 4)][time point lane & 15] -- but the product tile never reaches
//       memory: each lane multiplies its four D entries by the conjugated state entries of its rows and its time point
//       and keeps one running sum over the row groups; the sum over lane >> 4 ends it.  Any N (a run-time loop over
//       16-blocks, nothing of size N in LDS or registers); rows >= N, columns >= N and time points >= nt are masked as
//       there.  blockIdx.x: objective, blockIdx.y: KH_EXPECT_H_POINTS time points (every wave takes KH_EXPECT_VG groups
//       of sixteen with one fetch of an operator block).  The operators of a pass are taken one after the other by the
//       SAME workgroup, so its slab of the store (KH_EXPECT_H_POINTS x N x 16 bytes) comes from HBM once and from the
//       caches afterwards.
//       Bound: max(16 K nt N bytes at the memory side's rate, 8 N^2 n_e K nt flops on the fp64 MFMA).  K = 256, N = 64,
//       nt = 4001, n_e = 2: 1.05 GB against 67 GFLOP -- the matrix cores decide from N ~ 16 on.
//
//   kh_expect_liouville   out[e][k][n] = tr(O_ke rho_k(t_n)), N = d^2, O is d x d, states are column-stacked vec(rho):
//       tr(O rho) = sum_ij O_ij rho_ji = sum_ij O_ij vec(rho)[j + d i], and j + d i is O_ij's own place in the row-major
//       operator: a NON-conjugated dot product of the state row with the operator read as a vector of length N.  Pure
//       streaming: a wave per objective and KH_EXPECT_L_POINTS time points, every operator of the pass accumulated from
//       ONE read of the state row (the operators, n_e N x 16 bytes per objective, stay in the caches).
//       Bound: 16 K nt N bytes at the memory side's rate.
//
// One pass takes up to KH_EXPECT_MAX_OPS operators (the accumulators of the Liouville form live in registers); kh_expect
// makes ceil(n_e / KH_EXPECT_MAX_OPS) passes, each of which reads the store once.
// Summation order: fixed (per lane in index order, then a fixed tree over the lanes): two runs give the same bits.  No
// atomics.
#pragma once

#include "kh_common.h"

#define KH_EXPECT_MAX_OPS 8   // operators per pass
#define KH_EXPECT_THREADS 256 // 4 waves
#define KH_EXPECT_VG 4        // Hilbert form: groups of 16 time points per wave
#define KH_EXPECT_H_POINTS (4 * 16 * KH_EXPECT_VG)  // ... time points per workgroup
#define KH_EXPECT_L_WAVE_POINTS 4                   // Liouville form: time points per wave
#define KH_EXPECT_L_POINTS (4 * KH_EXPECT_L_WAVE_POINTS)  // ... per workgroup

typedef double kh_expect_d4 __attribute__((ext_vector_type(4)));

// v + (the same of the lanes 16, 32 and 48 further on): every lane of a column ends with the same sum, added in the
// same order
__device__ __forceinline__ double kh_expect_sum_rows(double v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// `tab` points at the pass's first operator of objective 0, `stride` is n_e of the whole call, `ne` (<=
// KH_EXPECT_MAX_OPS) the operators of this pass; `out` at the pass's first plane [K][nt]
__global__ void __launch_bounds__(KH_EXPECT_THREADS)
kh_expect_hilbert(const cplx *const *__restrict__ tab, int stride, int ne, const cplx *__restrict__ states /*[K][nt][N]*/,
                  cplx *__restrict__ out /*[ne][K][nt]*/, int K, int N, int nt)
#if KH_DEFINES(KH_TU_EXPECT)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = lane & 15, kq = lane >> 4;
    const int k = blockIdx.x;
    // this lane's time points (B operand columns): one per group
    const int n0 = (blockIdx.y * 4 + wave) * 16 * KH_EXPECT_VG + j;
    const cplx *xk = states + (size_t)k * nt * N;
    const int G = (N + 15) / 16;
    for (int e = 0; e < ne; ++e) {
        const cplx *op = tab[(size_t)k * stride + e];
        cplx *ok = out + ((size_t)e * K + k) * nt;
        double sr[KH_EXPECT_VG], si[KH_EXPECT_VG];
#pragma unroll
        for (int vg = 0; vg < KH_EXPECT_VG; ++vg) sr[vg] = si[vg] = 0.0;
        if (op != nullptr) {  // (uniform over the workgroup)
            for (int g = 0; g < G; ++g) {
                kh_expect_d4 dr[KH_EXPECT_VG], di[KH_EXPECT_VG];
#pragma unroll
                for (int vg = 0; vg < KH_EXPECT_VG; ++vg) dr[vg] = di[vg] = kh_expect_d4{0.0, 0.0, 0.0, 0.0};
                const int arow = 16 * g + j;  // A operand: row lane & 15
                for (int kb = 0; kb < G; ++kb) {
                    cplx a[4];
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        const int kk = 16 * kb + 4 * ks + kq;
                        a[ks] = (kk < N && arow < N) ? op[(size_t)arow * N + kk] : c_make(0.0, 0.0);
                    }
#pragma unroll
                    for (int vg = 0; vg < KH_EXPECT_VG; ++vg) {
                        const int n = n0 + 16 * vg;
                        cplx b[4];
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) {
                            const int kk = 16 * kb + 4 * ks + kq;
                            b[ks] = (kk < N && n < nt) ? xk[(size_t)n * N + kk] : c_make(0.0, 0.0);
                        }
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) {
                            dr[vg] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks].x, b[ks].x, dr[vg], 0, 0, 0);
                            dr[vg] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks].y, -b[ks].y, dr[vg], 0, 0, 0);
                            di[vg] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks].x, b[ks].y, di[vg], 0, 0, 0);
                            di[vg] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks].y, b[ks].x, di[vg], 0, 0, 0);
                        }
                    }
                }
                // conj(psi[row]) (O psi)[row] of this lane's rows 16 g + 4 reg + kq, added to the lane's running sums
#pragma unroll
                for (int vg = 0; vg < KH_EXPECT_VG; ++vg) {
                    const int n = n0 + 16 * vg;
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int row = 16 * g + 4 * reg + kq;
                        const cplx x = (row < N && n < nt) ? xk[(size_t)n * N + row] : c_make(0.0, 0.0);
                        sr[vg] = fma(x.x, dr[vg][reg], sr[vg]);
                        sr[vg] = fma(x.y, di[vg][reg], sr[vg]);
                        si[vg] = fma(x.x, di[vg][reg], si[vg]);
                        si[vg] = fma(-x.y, dr[vg][reg], si[vg]);
                    }
                }
            }
        }
#pragma unroll
        for (int vg = 0; vg < KH_EXPECT_VG; ++vg) {
            const int n = n0 + 16 * vg;
            const double re = kh_expect_sum_rows(sr[vg]), im = kh_expect_sum_rows(si[vg]);
            if (kq == 0 && n < nt) ok[n] = c_make(re, im);
        }
    }
}
#else
    ;  // (defined in the translation unit that owns it: kh_common.h, KH_DEFINES)
#endif

__global__ void __launch_bounds__(KH_EXPECT_THREADS)
kh_expect_liouville(const cplx *const *__restrict__ tab, int stride, int ne, const cplx *__restrict__ states /*[K][nt][N]*/,
                    cplx *__restrict__ out /*[ne][K][nt]*/, int K, int N, int nt)
#if KH_DEFINES(KH_TU_EXPECT)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x;
    const cplx *ops[KH_EXPECT_MAX_OPS];
#pragma unroll
    for (int e = 0; e < KH_EXPECT_MAX_OPS; ++e) ops[e] = e < ne ? tab[(size_t)k * stride + e] : nullptr;
    const int first = (blockIdx.y * 4 + wave) * KH_EXPECT_L_WAVE_POINTS;
    for (int n = first; n < first + KH_EXPECT_L_WAVE_POINTS && n < nt; ++n) {  // (uniform over the wave)
        const cplx *x = states + ((size_t)k * nt + n) * N;
        cplx acc[KH_EXPECT_MAX_OPS];
#pragma unroll
        for (int e = 0; e < KH_EXPECT_MAX_OPS; ++e) acc[e] = c_make(0.0, 0.0);
        for (int m = lane; m < N; m += 64) {
            const cplx v = x[m];
#pragma unroll
            for (int e = 0; e < KH_EXPECT_MAX_OPS; ++e)
                if (ops[e] != nullptr) c_fma(acc[e], ops[e][m], v);
        }
#pragma unroll
        for (int e = 0; e < KH_EXPECT_MAX_OPS; ++e) {
            if (e >= ne) continue;
            cplx r = c_make(0.0, 0.0);
            if (ops[e] != nullptr) r = c_make(sum64(acc[e].x), sum64(acc[e].y));
            if (lane == 0) out[((size_t)e * K + k) * nt + n] = r;
        }
    }
}
#else
    ;  // (defined in the translation unit that owns it: kh_common.h, KH_DEFINES)
#endif
