// Exact gradient of J_T for the pulse values, on the device (kh_pulse_gradient of include/krotov_hip.h).
//
//   dJ_T/d eps_l[n] = -2 sum_k ||chi_k|| Re < chi^_k(t_{n+1}) | L_exp(f dt_n A_kn)[ f dt_n H_lk ] | phi_k(t_n) >
//
// with A_kn = H0_k + sum_l eps_l[n] H_lk, f = -i (Hilbert) or 1 (Liouville), phi the stored forward states and chi^ the
// stored, normalised co-states of the SAME pulses, and L_exp(X)[E] the Frechet derivative of the matrix exponential: the
// top-right block of exp([[X, E], [0, X]]).  Krotov's update sum is only the first order in dt of this.
//
// Series.  The pair (d_l; t) is propagated under the block matrix [[Z, E_l], [0, Z]], Z = f h A_kn, E_l = f h H_lk,
// h = dt_n / s, term by term
//     t_j = (1/j) Z t_{j-1},     d_{l,j} = (1/j) (Z d_{l,j-1} + E_l t_{j-1}),     t_0 = phi_k(t_n), d_{l,0} = 0,
// and over the s sub-steps the pair (sum_j d_{l,j}; sum_j t_j) carries on as the next (d_{l,0}; t_0): after s sub-steps
// sum d_l = L_exp(f dt_n A_kn)[f dt_n H_lk] phi_k(t_n) exactly (it IS the exponential of the block matrix at the full dt).
// Plain Taylor coefficients for every engine, theta = dt_n (||H0|| + sum_l |eps_l[n]| ||H_l||) from the engine's norms,
// theta_max = 1 (s = ceil(theta)), and the degree ONE ABOVE the Taylor table's (kh_build_degree_table, what
// kh_series_tables(0, tol) exports):
//     the d block of the degree-m polynomial of the block matrix is the derivative of p_m(Z) = sum_{j<=m} Z^j / j! in the
//     direction E, sum_{j<=m} (1/j!) sum_{i<j} Z^i E Z^{j-1-i}, whose j-th term is bounded by ||E|| theta^{j-1}/(j-1)!.
//     It therefore misses L_exp by at most ||E|| sum_{i>=m} theta^i / i!  -- the remainder of exp after degree m - 1.
//     The table's entry for m bounds the remainder after degree m (sum_{i>m} theta^i/i! <= tol), so the derivative
//     meets that bound at degree m + 1, not at m.
// The real-spectrum / defect forms of the sweeps would need a derivative bound of their own: not used here.
//
// Mapping.  All (objective k, interval n) items are independent; what they share is the operator list of k.  Re-read
// per term and item, (1 + L) N^2 16 bytes each, K = 256, N = 64, nt = 4001, L = 1 would move 1e6 x ~15 x 128 KiB ~ 2e15
// bytes: such a form is priced by that, not by its flops.  So the INTERVAL INDEX is the second matrix dimension (as the
// ensemble index in kh_ens.h): a workgroup takes one objective and KH_GRAD_CHUNK intervals, sixteen at a time as the
// columns of N x 16 matrices T = (t of 16 intervals) and D_l, and a term is
//     H_o T (o = 0..L) and H_o D_l    on v_mfma_f64_16x16x4, combined per column with eps_l[n] and h_n / j:
// (1 + L)^2 products per term instead of the 1 + 2 L matrix-vector products of a generator formed per item in LDS -- but
// every operator entry fetched serves 16 (1 + L) columns, and for N <= 64, L <= KH_GRAD_REG_L the operators do not move
// at all: wave w keeps the row block 16 w .. 16 w + 15 of every operator in registers as MFMA A operands (64 VGPRs per
// operator) for all intervals of the chunk.  A workgroup then reads its operators once per KH_GRAD_CHUNK items (2 GB
// per evaluation at the size above) and the kernel is bound by the fp64 MFMA: 8 N^2 (1 + L)^2 flops per term and item,
// 1.9 TFLOP at that size (measured: profiles/gradient.txt).  N > 64 (a wave then has two row blocks: twice the sums and
// accumulators per lane, no room for operators) and L > KH_GRAD_REG_L stream the A tiles from L2, each serving
// 16 (1 + L) columns.  The eps_l[n] of a column commute with the product: H_o (eps D_l) accumulates all o into ONE
// accumulator per D_l; only H_o T is kept apart (it is E_o T as well).
// The form with A_kn per item in LDS was not built: at N = 96 its 144 KiB leave 16 KiB for the 2 (1 + L) vectors of ONE
// item per CU at a time, and every matrix entry is read from LDS once per product and item.
//
// Operand mapping (that of kh_expect_hilbert): A = operator block [row lane & 15][k lane >> 4], B = sixteen columns
// [k lane >> 4][column lane & 15], D = [row 4 reg + (lane >> 4)][column lane & 15].  A lane's four D entries of row block
// g are exactly its B entries of k block g: the term vectors live in LDS as [vector][4 g + reg][lane], every lane writes
// and reads 16 contiguous bytes next to its neighbours' (no bank conflicts), and the running sums stay in registers.
// The series' (s, m) are those of the largest theta among the sixteen columns (uniform over the workgroup: the barriers
// are); a column with a smaller theta gets more terms than it needs, never fewer.  Columns beyond the grid and rows /
// columns of the operators beyond N are zeros.
//
// Determinism: every item writes its own slot of per_objective [K][L][nt-1] (fixed order inside: registers, then the
// lanes 16 / 32 / 48 further on, then the waves 0..3); kh_grad_reduce adds over k in objective order.  No atomics; the
// result does not depend on the grid.
#pragma once

#include "kh_common.h"

#define KH_GRAD_MAX_L 4
#define KH_GRAD_NMAX 96
#define KH_GRAD_THREADS 256  // 4 waves: wave w takes the row blocks w and w + 4
#define KH_GRAD_CHUNK 64     // intervals per workgroup (sixteen at a time)
#define KH_GRAD_REG_L 2      // N <= 64: up to this many controls the operators stay in registers

typedef double kh_grad_d4 __attribute__((ext_vector_type(4)));

struct KhGradArgs {
    const cplx *const *ops;    // [K*(1+L)] dense row-major operators (forward direction); NULL: absent
    const double *norms;       // [K*(1+L)]
    const double *dt;          // [nt-1]
    const double *deg_theta;   // [KH_MAX_DEGREE+1] Taylor thresholds (kh_build_degree_table)
    const cplx *fw, *chi;      // [K][nt][N] stored forward states / normalised co-states
    const double *chi_norms;   // [K] or NULL: 1
    const double *pulses;      // [L][nt-1]
    double *per_obj;           // [K][L][nt-1]
    int K, N, nt, is_super;
};

__host__ __device__ inline size_t kh_grad_lds_bytes(int N, int L) {
    const size_t G = (size_t)(N + 15) / 16;
    return (size_t)(1 + L) * G * 256 * sizeof(cplx) + (size_t)4 * KH_GRAD_MAX_L * 16 * sizeof(double);
}

// One k block of the products of an operator's row block with the term vectors: y += tile x t (kept apart: it is E t
// too), and acc[v] += tile x (c d_v) for v = 1 .. L -- the column factor c (1, or eps of the lane's column) commutes with
// the product, so the d vectors need no accumulators of their own
template <int L, int NG>
__device__ __forceinline__ void kh_grad_mac(const cplx (&at)[4], const cplx *T, size_t vstride, int kb, int lane, double c,
                                            kh_grad_d4 &yr, kh_grad_d4 &yi, kh_grad_d4 (&accr)[1 + L][NG],
                                            kh_grad_d4 (&acci)[1 + L][NG], int gi) {
#pragma unroll
    for (int v = 0; v <= L; ++v) {
        cplx b[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            b[ks] = T[v * vstride + (size_t)(kb * 4 + ks) * 64 + lane];
            if (v > 0) b[ks] = c_make(c * b[ks].x, c * b[ks].y);
        }
        kh_grad_d4 &dr = v == 0 ? yr : accr[v][gi], &di = v == 0 ? yi : acci[v][gi];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            dr = __builtin_amdgcn_mfma_f64_16x16x4f64(at[ks].x, b[ks].x, dr, 0, 0, 0);
            dr = __builtin_amdgcn_mfma_f64_16x16x4f64(at[ks].y, -b[ks].y, dr, 0, 0, 0);
            di = __builtin_amdgcn_mfma_f64_16x16x4f64(at[ks].x, b[ks].y, di, 0, 0, 0);
            di = __builtin_amdgcn_mfma_f64_16x16x4f64(at[ks].y, b[ks].x, di, 0, 0, 0);
        }
    }
}

// NG: row blocks per wave -- 1 for N <= 64, 2 for N <= 96 (twice the sums and accumulators per lane: an instantiation of
// its own, or the N <= 64 form would carry them)
template <int L, int NG>
__global__ void __launch_bounds__(KH_GRAD_THREADS) kh_grad_items(KhGradArgs a) {
    static_assert(L >= 1 && L <= KH_GRAD_MAX_L && (NG == 1 || NG == 2), "controls, row blocks per wave");
    constexpr bool CANREG = NG == 1 && L <= KH_GRAD_REG_L;  // the operators stay in registers
    extern __shared__ __attribute__((aligned(16))) char kh_grad_smem[];
    const int N = a.N, G = (N + 15) >> 4, nt = a.nt, nI = a.nt - 1;
    const size_t vstride = (size_t)G * 256;
    cplx *T = (cplx *)kh_grad_smem;                       // [1+L][4 G][64] the term vectors t, d_1 .. d_L
    double *red = (double *)(T + (1 + L) * vstride);  // [4 waves][L][16 columns]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, kq = lane >> 4;
    constexpr bool regs = CANREG;
    const bool super = a.is_super != 0;

    for (int k = blockIdx.x; k < a.K; k += gridDim.x) {  // objectives in turns
        const cplx *const *ops_k = a.ops + (size_t)k * (1 + L);
        const double *norms_k = a.norms + (size_t)k * (1 + L);
        const cplx *fw_k = a.fw + (size_t)k * nt * N, *chi_k = a.chi + (size_t)k * nt * N;
        const double cn = a.chi_norms != nullptr ? a.chi_norms[k] : 1.0;

        // the row block `wave` of every operator as A operands
        cplx areg[CANREG ? 1 + L : 1][4][4];
        if constexpr (CANREG) {
            if (regs) {
                const int arow = 16 * wave + j;
#pragma unroll
                for (int o = 0; o <= L; ++o) {
                    const cplx *op = ops_k[o];
#pragma unroll
                    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) {
                            const int kk = 16 * kb + 4 * ks + kq;
                            areg[o][kb][ks] = (op != nullptr && arow < N && kk < N) ? op[(size_t)arow * N + kk] : c_make(0.0, 0.0);
                        }
                }
            }
        }

        for (int cg = 0; cg < KH_GRAD_CHUNK / 16; ++cg) {
            const int n0 = blockIdx.y * KH_GRAD_CHUNK + cg * 16;
            if (n0 >= nI) break;  // (uniform)
            const int n = n0 + j;  // this lane's column
            const bool valid = n < nI;
            const double dtn = valid ? a.dt[n] : 0.0;
            double eps[L];
            double theta = norms_k[0];
#pragma unroll
            for (int l = 0; l < L; ++l) {
                eps[l] = valid ? a.pulses[(size_t)l * nI + n] : 0.0;
                theta += fabs(eps[l]) * norms_k[1 + l];
            }
            theta *= dtn;
            // the largest theta of the sixteen columns: the same value in every lane of every wave
            theta = fmax(theta, __shfl_xor(theta, 1, 64));
            theta = fmax(theta, __shfl_xor(theta, 2, 64));
            theta = fmax(theta, __shfl_xor(theta, 4, 64));
            theta = fmax(theta, __shfl_xor(theta, 8, 64));
            int s_l, m_l;
            kh_degree_lookup(theta, a.deg_theta, 1.0, 1.0, 12, &s_l, &m_l);
            const int s = __builtin_amdgcn_readfirstlane(s_l);
            const int m = __builtin_amdgcn_readfirstlane(m_l) + 1;  // one above the table's: the header comment
            const double h = dtn / (double)s;

            // t_0 = phi_k(t_n), d_l0 = 0; the running sums start with them
            kh_grad_d4 sr[1 + L][NG], si[1 + L][NG];
#pragma unroll
            for (int gi = 0; gi < NG; ++gi) {
                const int g = wave + 4 * gi;
#pragma unroll
                for (int v = 0; v <= L; ++v) sr[v][gi] = si[v][gi] = kh_grad_d4{0.0, 0.0, 0.0, 0.0};
                if (g >= G) continue;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = 16 * g + 4 * reg + kq;
                    const cplx x = (valid && row < N) ? fw_k[(size_t)n * N + row] : c_make(0.0, 0.0);
                    sr[0][gi][reg] = x.x;
                    si[0][gi][reg] = x.y;
                    T[(size_t)(g * 4 + reg) * 64 + lane] = x;
#pragma unroll
                    for (int v = 1; v <= L; ++v) T[v * vstride + (size_t)(g * 4 + reg) * 64 + lane] = c_make(0.0, 0.0);
                }
            }
            __syncthreads();

            for (int sub = 0; sub < s; ++sub) {
                for (int jt = 1; jt <= m; ++jt) {
                    const double sc = h / (double)jt;
                    kh_grad_d4 nr[1 + L][NG], ni[1 + L][NG];
#pragma unroll
                    for (int gi = 0; gi < NG; ++gi) {
                        const int g = wave + 4 * gi;
#pragma unroll
                        for (int v = 0; v <= L; ++v) nr[v][gi] = ni[v][gi] = kh_grad_d4{0.0, 0.0, 0.0, 0.0};
                        if (g >= G) continue;  // (uniform over the wave)
                        const int arow = 16 * g + j;
#pragma unroll
                        for (int o = 0; o <= L; ++o) {
                            const cplx *op = ops_k[o];
                            if (op == nullptr) continue;  // an absent control: no term (uniform)
                            const double c = o == 0 ? 1.0 : eps[o == 0 ? 0 : o - 1];  // (of this lane's column)
                            kh_grad_d4 yr = kh_grad_d4{0.0, 0.0, 0.0, 0.0}, yi = yr;
                            bool done = false;
                            if constexpr (CANREG) {
                                if (regs) {  // (then g == wave: gi == 0)
#pragma unroll
                                    for (int kb = 0; kb < 4; ++kb)
                                        if (kb < G) kh_grad_mac<L, NG>(areg[o][kb], T, vstride, kb, lane, c, yr, yi, nr, ni, gi);
                                    done = true;
                                }
                            }
                            if (!done) {
                                for (int kb = 0; kb < G; ++kb) {
                                    cplx at[4];
#pragma unroll
                                    for (int ks = 0; ks < 4; ++ks) {
                                        const int kk = 16 * kb + 4 * ks + kq;
                                        at[ks] = (arow < N && kk < N) ? op[(size_t)arow * N + kk] : c_make(0.0, 0.0);
                                    }
                                    kh_grad_mac<L, NG>(at, T, vstride, kb, lane, c, yr, yi, nr, ni, gi);
                                }
                            }
                            // Z t += c_o H_o t (c_0 = 1, c_o = eps_{o-1}[n]); E_{o-1} t = H_o t
                            nr[0][gi] += c * yr;
                            ni[0][gi] += c * yi;
                            if (o >= 1) {
                                nr[o][gi] += yr;
                                ni[o][gi] += yi;
                            }
                        }
                        // times f h / j
#pragma unroll
                        for (int v = 0; v <= L; ++v) {
                            const kh_grad_d4 xr = nr[v][gi], xi = ni[v][gi];
                            if (super) {
                                nr[v][gi] = sc * xr;
                                ni[v][gi] = sc * xi;
                            } else {  // -i (x + i y) = y - i x
                                nr[v][gi] = sc * xi;
                                ni[v][gi] = -sc * xr;
                            }
                        }
                    }
                    __syncthreads();  // every wave has read the terms j - 1
#pragma unroll
                    for (int gi = 0; gi < NG; ++gi) {
                        const int g = wave + 4 * gi;
                        if (g >= G) continue;
#pragma unroll
                        for (int v = 0; v <= L; ++v) {
                            sr[v][gi] += nr[v][gi];
                            si[v][gi] += ni[v][gi];
#pragma unroll
                            for (int reg = 0; reg < 4; ++reg)
                                T[v * vstride + (size_t)(g * 4 + reg) * 64 + lane] = c_make(nr[v][gi][reg], ni[v][gi][reg]);
                        }
                    }
                    __syncthreads();
                }
                if (sub + 1 < s) {  // the pair carries on: the sums are the next sub-step's t_0, d_l0
#pragma unroll
                    for (int gi = 0; gi < NG; ++gi) {
                        const int g = wave + 4 * gi;
                        if (g >= G) continue;
#pragma unroll
                        for (int v = 0; v <= L; ++v)
#pragma unroll
                            for (int reg = 0; reg < 4; ++reg)
                                T[v * vstride + (size_t)(g * 4 + reg) * 64 + lane] = c_make(sr[v][gi][reg], si[v][gi][reg]);
                    }
                    __syncthreads();
                }
            }

            // Re <chi^(t_{n+1}) | sum d_l>: this lane's rows, then the lanes 16 / 32 / 48 further on, then the waves
            double part[L];
#pragma unroll
            for (int l = 0; l < L; ++l) part[l] = 0.0;
#pragma unroll
            for (int gi = 0; gi < NG; ++gi) {
                const int g = wave + 4 * gi;
                if (g >= G) continue;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = 16 * g + 4 * reg + kq;
                    const cplx x = (valid && row < N) ? chi_k[(size_t)(n + 1) * N + row] : c_make(0.0, 0.0);
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        part[l] = fma(x.x, sr[1 + l][gi][reg], part[l]);
                        part[l] = fma(x.y, si[1 + l][gi][reg], part[l]);
                    }
                }
            }
#pragma unroll
            for (int l = 0; l < L; ++l) {
                double p = part[l];
                p += __shfl_xor(p, 16, 64);
                p += __shfl_xor(p, 32, 64);
                if (kq == 0) red[(wave * KH_GRAD_MAX_L + l) * 16 + j] = p;
            }
            __syncthreads();
            if (wave == 0 && kq == 0 && valid) {
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    double tot = 0.0;
#pragma unroll
                    for (int w = 0; w < 4; ++w) tot += red[(w * KH_GRAD_MAX_L + l) * 16 + j];
                    a.per_obj[((size_t)k * L + l) * nI + n] = ops_k[1 + l] == nullptr ? 0.0 : -2.0 * cn * tot;
                }
            }
            // (the next writes of `red` lie behind the barriers of the next group of columns)
        }
    }
}

// grad[i] = sum_k per_obj[k][i] in objective order, i over [L][nt-1]
__global__ void __launch_bounds__(256) kh_grad_reduce(const double *__restrict__ per_obj, double *__restrict__ grad, int K,
                                                      long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc += per_obj[(size_t)k * count + i];
    grad[i] = acc;
}
