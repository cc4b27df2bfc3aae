// Register-resident sweep kernels for state dimension N <= 64 (CDNA4 / gfx950).
//
// One workgroup per objective.  The step generator A = H0 + sum_l eps_l H_l and
// the operators it is rebuilt from stay in VGPRs for the whole sweep (a 64x64
// complex128 operator is 64 KiB = 64 dwords/lane over 256 lanes, 32 over 512);
// only the Taylor-term vector goes through LDS (1 KiB, double-buffered), read as
// conflict-free broadcast ds_read_b128s.  Each lane owns RPT rows x 8 columns
// (columns cg, cg+8, ... so the 8 column-group lanes of a row hit 8 consecutive
// 16-byte LDS slots); row sums are all-reduced over the 8 adjacent lanes with
// DPP (quad_perm, quad_perm, row_half_mirror), never through LDS.
//
//   RPT = 2 : 256 threads, 4 waves, 16 rows per wave
//   RPT = 1 : 512 threads, 8 waves,  8 rows per wave (half the registers/lane)
//
// Stored states are written as one coalesced 1 KiB store per interval.
#pragma once

#include "kh_common.h"
#include "kh_generic.h"

#define KH_TILE_N 64

// Lane roles inside a wave (8 rows x 8 column groups), in two flavours:
//   KhLanes<false>: the row's 8 column groups are 8 adjacent lanes; row sums are a three-step DPP butterfly
//     (quad_perm, quad_perm, row_half_mirror: 18 VALU instructions for a complex value).
//   KhLanes<true>: the matrix core adds them.  v_mfma_f64_4x4x4 with a constant B operand sums its A operand
//     over the four lanes 16 k + i (k = 0..3), so the column group's low bits are lane >> 4; the result for
//     i = 4 blk + r4 lands on lanes 16 r4 + 4 blk + (0..3), and ONE DPP half-mirror step adds the blk-parity
//     partner: 2 MFMA + 6 VALU per complex value.  Pays in the two-terms-per-phase kernels (VALU-issue
//     bound: -3 % on the backward sweep); the one-term-per-phase kernels are latency-bound and keep DPP
//     (measured +1 % with the MFMA form).
//   input side  (operator tiles, products):  column group cg(lane),  row row_in(lane)
//   output side (row sums, state, co-state): row row_out(lane), replicated over 8 adjacent lanes; lane & 7 == 0
//     writes
template <bool MFMA>
struct KhLanes;
template <>
struct KhLanes<true> {
    static __device__ __forceinline__ int cg(int lane) { return (lane >> 4) + 4 * ((lane >> 2) & 1); }
    static __device__ __forceinline__ int row_in(int lane) { return (lane & 3) + 4 * ((lane >> 3) & 1); }
    static __device__ __forceinline__ int row_out(int lane) { return (lane >> 4) + 4 * ((lane >> 3) & 1); }
    // scale * (sum of v over the 8 column groups of a row), on the row's output lanes
    static __device__ __forceinline__ double rowsum(double v, double scale) {
        const double d = __builtin_amdgcn_mfma_f64_4x4x4f64(v, scale, 0.0, 0, 0, 0);
        return d + dpp_move<KH_DPP_HALF_MIRROR>(d);
    }
    // sum over the wave of a value that is zero except on the 8 writer lanes (lane & 7 == 0); valid on lane 0.
    // The same MFMA adds lanes {0,16,32,48} into lane 0 and {8,24,40,56} into lane 8; one row rotation joins
    // them: 1 MFMA + 3 VALU instead of the ~30 dependent instructions of a full 64-lane butterfly.
    static __device__ __forceinline__ double writers_sum(double v) {
        const double d = __builtin_amdgcn_mfma_f64_4x4x4f64(v, 1.0, 0.0, 0, 0, 0);
        return d + dpp_move<KH_DPP_ROR8>(d);
    }
};
template <>
struct KhLanes<false> {
    static __device__ __forceinline__ int cg(int lane) { return lane & 7; }
    static __device__ __forceinline__ int row_in(int lane) { return lane >> 3; }
    static __device__ __forceinline__ int row_out(int lane) { return lane >> 3; }
    static __device__ __forceinline__ double rowsum(double v, double scale) { return scale * sum8(v); }
    static __device__ __forceinline__ double writers_sum(double v) { return sum64(v); }
};
typedef KhLanes<false> KhTileLanes;

// Lane roles of the row-broadcast map (512 threads; the two-terms-per-phase kernels, kh_tile64q2.h).  A wave is
// (rb, half) = (wave >> 1, wave & 1); lane i of its DPP row d (lane = 16 d + i) holds matrix row 16 rb + i and the 8
// columns 8 (d + 4 half) + 0..7: a wave covers 16 rows x 32 columns, the pair (rb, 0), (rb, 1) the full rows.
//   input side:  lane n of a DPP row holds ONE element of the vector, x[8 (d + 4 half) + (n & 7)] (lanes 8..15 repeat
//     lanes 0..7: no load under a branch); product j takes it from lane j of the row as the FMA's own DPP operand
//     (row_newbcast:j) -- one or two ds_read_b128 per lane and product instead of eight, and no registers for the vector.
//   output side: the four column blocks of a row are the lanes 16 k + i, which ONE v_mfma_f64_4x4x4 with a constant B
//     operand adds; the sum for i = 4 blk + r4 lands on lanes 16 r4 + 4 blk + (0..3), whose first is the writer.  What
//     lands is the wave's HALF of the row sum: everything kept on these lanes is the partial that belongs to the wave's
//     column half, and the two are added where a complete vector is read.
struct KhLanesR16 {
    static __host__ __device__ __forceinline__ int half(int wave) { return wave & 1; }
    static __host__ __device__ __forceinline__ int row_in(int wave, int lane) { return 16 * (wave >> 1) + (lane & 15); }
    static __host__ __device__ __forceinline__ int col0(int wave, int lane) { return 8 * ((lane >> 4) + 4 * (wave & 1)); }
    static __host__ __device__ __forceinline__ int x_index(int wave, int lane) { return col0(wave, lane) + (lane & 7); }
    // where the row sum of input lane `lane` lands (first of four lanes), and the row whose sum an output lane holds
    static __host__ __device__ __forceinline__ int landing_lane(int lane) { return 16 * (lane & 3) + 4 * ((lane >> 2) & 3); }
    static __host__ __device__ __forceinline__ int row_out(int wave, int lane) {
        return 16 * (wave >> 1) + 4 * ((lane >> 2) & 3) + (lane >> 4);
    }
    static __host__ __device__ __forceinline__ bool writer(int lane) { return (lane & 3) == 0; }
    static __device__ __forceinline__ double rowsum(double v, double scale) {
        return __builtin_amdgcn_mfma_f64_4x4x4f64(v, scale, 0.0, 0, 0, 0);
    }
    // acc += sum_j t[j] * x(lane j of this lane's DPP row).  The compiler neither folds a DPP move into an fp64 FMA nor
    // sees inside the string: 2 wait states in front (x may come straight from a VALU add; a DPP read after a VALU
    // write needs them) and 2 behind (acc goes to the matrix core next).
    // Preconditions, both the caller's: (1) all 64 lanes active -- a row_newbcast from a disabled lane leaves the
    // destination unwritten, so never call this inside a divergent branch; (2) no VALU write of EXEC (v_cmpx, ...)
    // directly in front: a DPP instruction needs 5 wait states behind one, which the string does not carry.
#define KH_R16_FMAC(J, RE, IM)                                                           \
    "v_fmac_f64_dpp %0, %2, %" #RE " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"  \
    "v_fmac_f64_dpp %1, %3, %" #RE " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"  \
    "v_fmac_f64_dpp %0, -%3, %" #IM " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t" \
    "v_fmac_f64_dpp %1, %2, %" #IM " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
    static __device__ __forceinline__ void dot8(cplx &acc, const cplx (&t)[8], cplx x) {
        asm("s_nop 1\n\t"
            KH_R16_FMAC(0, 4, 5) KH_R16_FMAC(1, 6, 7) KH_R16_FMAC(2, 8, 9) KH_R16_FMAC(3, 10, 11)
            KH_R16_FMAC(4, 12, 13) KH_R16_FMAC(5, 14, 15) KH_R16_FMAC(6, 16, 17) KH_R16_FMAC(7, 18, 19)
            "s_nop 1"
            : "+v"(acc.x), "+v"(acc.y)
            : "v"(x.x), "v"(x.y), "v"(t[0].x), "v"(t[0].y), "v"(t[1].x), "v"(t[1].y), "v"(t[2].x), "v"(t[2].y),
              "v"(t[3].x), "v"(t[3].y), "v"(t[4].x), "v"(t[4].y), "v"(t[5].x), "v"(t[5].y), "v"(t[6].x), "v"(t[6].y),
              "v"(t[7].x), "v"(t[7].y));
    }
#undef KH_R16_FMAC
};

template <int RPT>
struct KhTile {
    static constexpr int THREADS = 512 / RPT;
    static constexpr int WAVES = THREADS / 64;
    // rows of (wave, lane) for r in [0, RPT): whose operator elements it holds / whose sums and state it holds
    static __device__ __forceinline__ int row_in(int wave, int lane, int r) {
        return wave * (8 * RPT) + r * 8 + KhTileLanes::row_in(lane);
    }
    static __device__ __forceinline__ int row(int wave, int lane, int r) {
        return wave * (8 * RPT) + r * 8 + KhTileLanes::row_out(lane);
    }
    static __device__ __forceinline__ bool writer(int lane) { return (lane & 7) == 0; }
};

template <int RPT>
__device__ __forceinline__ void kh_tile_load_op(const cplx *op, int N, int wave, int lane, cplx (&a)[RPT][8]) {
    const int cg = KhTileLanes::cg(lane);
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int row = KhTile<RPT>::row_in(wave, lane, r);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = cg + 8 * j;
            a[r][j] = (op != nullptr && row < N && col < N) ? op[(size_t)row * N + col] : c_make(0.0, 0.0);
        }
    }
}

// y[r] = sum_c a[r][c] x[c], summed over the row's 8 column groups (on the row's 8 output lanes)
template <int RPT>
__device__ __forceinline__ void kh_tile_matvec(const cplx (&a)[RPT][8], const cplx *x, int cg, cplx (&y)[RPT]) {
    cplx xv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) xv[j] = x[cg + 8 * j];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        cplx acc = c_make(0.0, 0.0);
#pragma unroll
        for (int j = 0; j < 8; ++j) c_fma(acc, a[r][j], xv[j]);
        y[r].x = KhTileLanes::rowsum(acc.x, 1.0);
        y[r].y = KhTileLanes::rowsum(acc.y, 1.0);
    }
}

// state (in registers of every lane of the row group) <- exp(f A dt) state.
// buf: LDS ping-pong vectors.  On entry buf[cur] holds the state (all rows
// written, barrier passed); on exit buf[cur] (updated) holds the NEW state, so
// consecutive intervals chain without an extra write + barrier: the last
// Taylor term is never needed in LDS, its slot receives the state instead.
// One barrier per matrix-vector product.  Returns the matvec count.
template <int RPT>
__device__ __forceinline__ int kh_tile_expm_action(const cplx (&a)[RPT][8], cplx (&state)[RPT],
                                                   cplx (*buf)[KH_TILE_N], const double *inv, int &cur, double fre,
                                                   double fim,
                                                   double dt, int nsub, int m, int wave, int lane) {
    const int cg = KhTileLanes::cg(lane);
    const bool writer = KhTile<RPT>::writer(lane);
    const double h = nsub == 1 ? dt : dt / nsub;
    for (int sub = 0; sub < nsub; ++sub) {
        const double c0 = inv[0];  // T_0 = c_0 v (1 for Taylor); ratio 1 is relative to v itself
#pragma unroll
        for (int r = 0; r < RPT; ++r) state[r] = c_make(c0 * state[r].x, c0 * state[r].y);
        for (int j = 1; j <= m; ++j) {
            const double hj = h * inv[j];  // series ratio of term j (Taylor: 1/j); LDS: no SMEM loads in the loop
            const cplx coef = c_make(fre * hj, fim * hj);
            cplx y[RPT];
            kh_tile_matvec<RPT>(a, buf[cur], cg, y);
            const bool last = (j == m);
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const cplx t = c_mul(coef, y[r]);
                state[r].x += t.x;
                state[r].y += t.y;
                const double wx = last ? state[r].x : t.x, wy = last ? state[r].y : t.y;
                if (writer) buf[cur ^ 1][KhTile<RPT>::row(wave, lane, r)] = c_make(wx, wy);
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    return nsub * m;
}

// The 1+LT operator tiles of one objective.  With more than three operators they do not all fit
// in the register file next to the generator tile (32 VGPRs each at RPT = 1): the first NL of them
// are parked in LDS instead, each lane's 8 elements at stride THREADS so a wave reads 64
// consecutive 16-byte slots (no bank conflicts), and only the lane itself ever reads its slots
// (no barrier needed after the fill).
template <int RPT, int LT, int NL>
struct KhTileOps {
    static constexpr int THREADS = 512 / RPT;
    cplx reg[1 + LT - NL][RPT][8];
    cplx *lds;  // this lane's column of the LDS-resident tiles

    __device__ __forceinline__ cplx at(int o, int r, int j) const {
        if (o < NL) return lds[(size_t)((o * RPT + r) * 8 + j) * THREADS];
        return reg[o < NL ? 0 : o - NL][r][j];
    }
    __device__ __forceinline__ void load(const cplx *const *ops_k, int N, int wave, int lane, cplx *lds_base,
                                         int tid) {
        lds = lds_base + tid;
#pragma unroll
        for (int o = 0; o <= LT; ++o) {
            if (o < NL) {
                cplx t[RPT][8];
                kh_tile_load_op<RPT>(ops_k[o], N, wave, lane, t);
#pragma unroll
                for (int r = 0; r < RPT; ++r)
#pragma unroll
                    for (int j = 0; j < 8; ++j) lds[(size_t)((o * RPT + r) * 8 + j) * THREADS] = t[r][j];
            } else {
                kh_tile_load_op<RPT>(ops_k[o], N, wave, lane, reg[o < NL ? 0 : o - NL]);
            }
        }
    }
    // a = op[0] + sum_l eps_l op[1+l]
    __device__ __forceinline__ void build(const double *eps, cplx (&a)[RPT][8]) const {
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                cplx v = at(0, r, j);
#pragma unroll
                for (int l = 0; l < LT; ++l) {
                    const cplx hl = at(1 + l, r, j);
                    v.x = fma(eps[l], hl.x, v.x);
                    v.y = fma(eps[l], hl.y, v.y);
                }
                a[r][j] = v;
            }
    }
    // this lane's share of (op[o] x)[row]: its 8 columns only, NOT summed over the row's lanes; xv = x[cg + 8 j]
    __device__ __forceinline__ void matvec_part(int o, const cplx (&xv)[8], cplx (&y)[RPT]) const {
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            cplx acc = c_make(0.0, 0.0);
#pragma unroll
            for (int j = 0; j < 8; ++j) c_fma(acc, at(o, r, j), xv[j]);
            y[r] = acc;
        }
    }
    // y = op[o] x, reduced over the row's 8 lanes
    __device__ __forceinline__ void matvec(int o, const cplx *x, int cg, cplx (&y)[RPT]) const {
        cplx xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = x[cg + 8 * j];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            cplx acc = c_make(0.0, 0.0);
#pragma unroll
            for (int j = 0; j < 8; ++j) c_fma(acc, at(o, r, j), xv[j]);
            y[r].x = KhTileLanes::rowsum(acc.x, 1.0);
            y[r].y = KhTileLanes::rowsum(acc.y, 1.0);
        }
    }
};

// operators parked in LDS: none up to three operators; for L = 3, 4 the update sweep parks L - 2
// (it also keeps chi, the partial sums and, second order, phi_prev), the plain sweep one for L = 4
template <int RPT, int LT>
struct KhTileLds {
    // RPT = 2 (256-thread workgroups, two per CU, K > #CUs): a tile is 64 VGPRs per lane there, so with one control the
    // drift is parked as well (64 KiB per workgroup, 128 KiB per CU) -- generator + control + broadcast vector then fit
    static constexpr int UPDATE = (RPT == 1 && LT >= 3) ? LT - 2 : (RPT == 2 && LT == 1) ? 1 : 0;
    static constexpr int STORE = (RPT == 1 && LT >= 4) ? 1 : (RPT == 2 && LT == 1) ? 1 : 0;
    // the update kernel's single-GPU instantiation has registers to spare (kh_tile_forward_update: SINGLE): three controls
    // park nothing there
    static constexpr int UPDATE_SINGLE = (RPT == 1 && LT == 3) ? 0 : UPDATE;
    static constexpr size_t bytes(int nl) { return (size_t)nl * KH_TILE_N * KH_TILE_N * sizeof(cplx); }
};

extern __shared__ __attribute__((aligned(16))) cplx kh_tile_dyn_lds[];

// the series' ratios of degree m -> LDS (workgroup-uniform m; between intervals; contains barriers)
__device__ __forceinline__ void kh_tile_load_ratios(const KhSweepArgs &p, double *inv_sh, int m, int tid) {
    __syncthreads();  // (no phase is still reading the previous ratios)
    if (tid <= KH_MAX_DEGREE) inv_sh[tid] = p.ratios[(size_t)m * KH_RATIO_STRIDE + tid];
    __syncthreads();
}

// ---------------------------------------------------------------------------
// plain propagation with storage (backward sweep / iteration-0 forward sweep)
// ---------------------------------------------------------------------------
// SRC (kh_tile_sweep_store_src): the backward sweep of a co-state equation with a source term (state-dependent running
// costs, kh_backward_store_source) -- a kernel of its own, so that the sweep without a source keeps its code; both include
// one body (kh_tile64_store.inc).  KhSrcArgs: kh_generic.h.
template <int RPT, int LT>
__global__ void __launch_bounds__(512 / RPT, 2)
kh_tile_sweep_store(KhSweepArgs p, const double *__restrict__ pulses, const cplx *__restrict__ state_in,
                    cplx *__restrict__ store, cplx *__restrict__ state_out, int direction) {
    constexpr bool SRC = false;
    const KhSrcArgs sa{};
#include "kh_tile64_store.inc"
}

// backward direction only: chi_T -> store[:, nt-1], then n = nt-2 .. 0
template <int RPT, int LT>
__global__ void __launch_bounds__(512 / RPT, 2)
kh_tile_sweep_store_src(KhSweepArgs p, KhSrcArgs sa, const double *__restrict__ pulses, const cplx *__restrict__ state_in,
                        cplx *__restrict__ store) {
    constexpr bool SRC = true;
    constexpr int direction = -1;
    cplx *const state_out = nullptr;
#include "kh_tile64_store.inc"
}

// ---------------------------------------------------------------------------
// forward sweep with sequential pulse update (optimize.py:444-508)
// ---------------------------------------------------------------------------
// Requires gridDim.x == K (one resident workgroup per objective): operators
// and the running state never leave the registers / LDS of their workgroup.
// Barriers per interval: 1 (partial sums) + 1 (broadcast of the reduced sums)
// + one per Taylor term.
// SO: second-order update, compiled separately.  SINGLE: launched on ONE GPU as one launch over the sweep with more than one
// workgroup (ex.world == 1, ex.G > 1, u.internal_exchange): the sums' exchange without the cross-GPU stage and without the
// forms it does not take -- an instantiation of its own because the kernel sits at the register limit
// PAR (kh_tile_forward_update_par): with pulse parametrizations (kh_set_parametrization) -- u_guess and f'(u_guess) are
// prefetched with the other per-interval scalars, f is applied where eps[l] is formed.  A kernel of its own, so that the
// unparametrized one keeps its code; both include one body (kh_tile64_update.inc).
template <int RPT, int LT, bool SO, bool SINGLE = false>
__global__ void __launch_bounds__(512 / RPT, 2)
kh_tile_forward_update(KhSweepArgs p, KhUpdateArgs u, KhExchange ex) {
    constexpr bool PAR = false, NL = false;
    const KhParArgs pa{};
    const KhNlArgs na{};
#include "kh_tile64_update.inc"
}

// the whole sweep in one launch on one GPU (SINGLE)
template <int RPT, int LT, bool SO>
__global__ void __launch_bounds__(512 / RPT, 2)
kh_tile_forward_update_par(KhSweepArgs p, KhUpdateArgs u, KhExchange ex, KhParArgs pa) {
    constexpr bool PAR = true, NL = false, SINGLE = true;
    const KhNlArgs na{};
#include "kh_tile64_update.inc"
}

// NL (kh_tile_forward_update_nl): with non-linear controls (kh_set_nonlinear) -- the LT slots are the terms
// eps_c(l)^p_l H_l of C <= LT controls; the weights w_l are prefetched with the other per-interval scalars, the sums of a
// control's terms are weighted and added after the exchange, h.build takes the powers.  The whole sweep in one launch on
// one GPU (SINGLE), and a kernel of its own for the reason above; the PAR note on parked operators holds for it.
template <int RPT, int LT, bool SO>
__global__ void __launch_bounds__(512 / RPT, 2)
kh_tile_forward_update_nl(KhSweepArgs p, KhUpdateArgs u, KhExchange ex, KhNlArgs na) {
    constexpr bool PAR = false, NL = true, SINGLE = true;
    const KhParArgs pa{};
#include "kh_tile64_update.inc"
}
