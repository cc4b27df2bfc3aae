// Micro-benchmark: one register-tile matvec phase chain (LDS read -> FMAs -> row sums -> LDS write -> barrier) of a
// 64 x 64 complex operator, today's q2 lane map against a map that feeds the term vector by DPP row broadcast
// (dev tool):
//   M18 : lane = 1 row x 8 columns (the kernels' map, copied from ubench_lanemap.hip: 8 broadcast ds_read_b128 per
//         lane and phase, row sum over 8 lanes)
//   R16 : lane i of DPP row d of wave (rb, half) = matrix row 16 rb + i x columns 8 (d + 4 half) + 0..7.  Lane n of
//         a DPP row holds ONE vector element, x[8 (d + 4 half) + (n & 7)]; product j takes it from lane j of the
//         row (row_newbcast:j).  The four column blocks of a wave are lanes 16 k + i, which one v_mfma_f64_4x4x4
//         with a constant B operand adds; the two waves of a pair write their halves to part[half][64] and the
//         reader adds them: 2 ds_read_b128 per lane and phase.
//         (a) __builtin_amdgcn_update_dpp: v_mov_b64_dpp + plain FMAs
//         (b) inline v_fmac_f64_dpp, the broadcast folded into the FMA
//         (d) as (b), with four accumulator chains per product instead of two
//   R16c: 4 waves of 16 rows x 64 columns (256 threads, one wave per SIMD, 16 elements per lane, no pair add;
//         1 ds_read_b128 per lane and phase), builtin form
// A first launch of three phases on a random operator checks every map's vector against M18's.
// hipcc --offload-arch=gfx950 -O3 -I krotov_amd/csrc scripts/ubench_dppbcast.hip -o /tmp/ubench_dppbcast && /tmp/ubench_dppbcast
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "kh_common.h"

enum { M18 = 0, R16A = 1, R16B = 2, R16C = 3, R16D = 4 };

// v <- lane J of the caller's 16-lane DPP row
template <int J>
__device__ __forceinline__ double row_bcast(double v) {
    return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + J, 0xF, 0xF, false);
}

template <int J, int NJ>
struct BcastFma {
    static __device__ __forceinline__ void run(cplx &acc, const cplx *a, cplx x) {
        c_fma(acc, a[J], c_make(row_bcast<J>(x.x), row_bcast<J>(x.y)));
        BcastFma<J + 1, NJ>::run(acc, a, x);
    }
};
template <int NJ>
struct BcastFma<NJ, NJ> {
    static __device__ __forceinline__ void run(cplx &, const cplx *, cplx) {}
};

// acc += a[j] * x(lane j of the DPP row), j = 0..7, the broadcast as the FMA's own DPP operand.  The compiler does not
// see inside the string: x was just written by a VALU add (2 wait states before a DPP read), and acc goes to an MFMA
// next (2 wait states after the last VALU write).
#define KH_FMAC_DPP(J, A)                                                                  \
    "v_fmac_f64_dpp %0, %2, %" #A " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"    \
    "v_fmac_f64_dpp %1, %3, %" #A " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
#define KH_FMAC_DPP_IM(J, A)                                                               \
    "v_fmac_f64_dpp %0, -%3, %" #A " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"   \
    "v_fmac_f64_dpp %1, %2, %" #A " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ void fmac_dpp8(cplx &acc, const cplx *a, cplx x) {
    asm("s_nop 1\n\t"
        KH_FMAC_DPP(0, 4) KH_FMAC_DPP_IM(0, 5) KH_FMAC_DPP(1, 6) KH_FMAC_DPP_IM(1, 7)
        KH_FMAC_DPP(2, 8) KH_FMAC_DPP_IM(2, 9) KH_FMAC_DPP(3, 10) KH_FMAC_DPP_IM(3, 11)
        KH_FMAC_DPP(4, 12) KH_FMAC_DPP_IM(4, 13) KH_FMAC_DPP(5, 14) KH_FMAC_DPP_IM(5, 15)
        KH_FMAC_DPP(6, 16) KH_FMAC_DPP_IM(6, 17) KH_FMAC_DPP(7, 18) KH_FMAC_DPP_IM(7, 19)
        "s_nop 1"
        : "+v"(acc.x), "+v"(acc.y)
        : "v"(x.x), "v"(x.y), "v"(a[0].x), "v"(a[0].y), "v"(a[1].x), "v"(a[1].y), "v"(a[2].x), "v"(a[2].y),
          "v"(a[3].x), "v"(a[3].y), "v"(a[4].x), "v"(a[4].y), "v"(a[5].x), "v"(a[5].y), "v"(a[6].x), "v"(a[6].y),
          "v"(a[7].x), "v"(a[7].y));
}

// the same with four accumulator chains (re.re, im.im, re.im, im.re) instead of two: does the dependent-issue latency of
// the fp64 FMA show at two waves per SIMD?
#define KH_FMAC_DPP4(J, RE, IM)                                                            \
    "v_fmac_f64_dpp %0, %4, %" #RE " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"   \
    "v_fmac_f64_dpp %1, -%5, %" #IM " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"  \
    "v_fmac_f64_dpp %2, %5, %" #RE " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"   \
    "v_fmac_f64_dpp %3, %4, %" #IM " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ void fmac_dpp8_4chains(cplx &acc, const cplx *a, cplx x) {
    double rr = 0.0, ii = 0.0, ri = 0.0, ir = 0.0;
    asm("s_nop 1\n\t"
        KH_FMAC_DPP4(0, 6, 7) KH_FMAC_DPP4(1, 8, 9) KH_FMAC_DPP4(2, 10, 11) KH_FMAC_DPP4(3, 12, 13)
        KH_FMAC_DPP4(4, 14, 15) KH_FMAC_DPP4(5, 16, 17) KH_FMAC_DPP4(6, 18, 19) KH_FMAC_DPP4(7, 20, 21)
        "s_nop 0"
        : "+v"(rr), "+v"(ii), "+v"(ri), "+v"(ir)
        : "v"(x.x), "v"(x.y), "v"(a[0].x), "v"(a[0].y), "v"(a[1].x), "v"(a[1].y), "v"(a[2].x), "v"(a[2].y),
          "v"(a[3].x), "v"(a[3].y), "v"(a[4].x), "v"(a[4].y), "v"(a[5].x), "v"(a[5].y), "v"(a[6].x), "v"(a[6].y),
          "v"(a[7].x), "v"(a[7].y));
    acc.x += rr + ii;
    acc.y += ri + ir;
}

// scale * (sum of v over the lanes 16 k + i, k = 0..3); the sum for i = 4 blk + r4 lands on lanes 16 r4 + 4 blk + 0..3
__device__ __forceinline__ double rowsum_mfma(double v, double scale) {
    return __builtin_amdgcn_mfma_f64_4x4x4f64(v, scale, 0.0, 0, 0, 0);
}

template <int MAP>
struct Threads {
    static constexpr int value = MAP == R16C ? 256 : 512;
};

template <int MAP, int PRODUCTS>
__global__ void __launch_bounds__(Threads<MAP>::value)
    k(const cplx *op, cplx *out, cplx *vec, long long *cyc, int iters) {
    constexpr int NJ = MAP == R16C ? 16 : 8;      // operator elements per lane and product
    constexpr int PARTS = (MAP == R16A || MAP == R16B || MAP == R16D) ? 2 : 1;  // partial vectors a reader adds
    __shared__ __attribute__((aligned(16))) cplx buf[2][PARTS][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    cplx a[PRODUCTS][NJ];
    int row_w = 0, part_w = 0;  // the row this lane writes, and into which partial vector
    int x_idx = 0;              // the vector element this lane reads (R16 maps)
    bool writer = false;
    if (MAP == M18) {
        const int cg = lane & 7, r = wave * 8 + (lane >> 3);
        for (int p = 0; p < PRODUCTS; ++p)
            for (int j = 0; j < 8; ++j) a[p][j] = op[(p * 64 + r) * 64 + cg + 8 * j];
        row_w = r;
        writer = cg == 0;
    } else {
        const int rb = MAP == R16C ? wave : wave >> 1, half = MAP == R16C ? 0 : wave & 1;
        const int d = lane >> 4, i = lane & 15, col0 = MAP == R16C ? 16 * d : 8 * (d + 4 * half);
        for (int p = 0; p < PRODUCTS; ++p)
            for (int j = 0; j < NJ; ++j) a[p][j] = op[(p * 64 + 16 * rb + i) * 64 + col0 + j];
        x_idx = col0 + (i & (NJ - 1));
        row_w = 16 * rb + 4 * ((lane >> 2) & 3) + (lane >> 4);
        part_w = half;
        writer = (lane & 3) == 0;
    }
    if (tid < 64) {
        buf[0][0][tid] = c_make(1.0 / (tid + 1), 0.5);
        if constexpr (PARTS == 2) buf[0][1][tid] = c_make(0.0, 0.0);
    }
    __syncthreads();
    cplx state = c_make(0, 0);
    int cur = 0;
    const long long t0 = clock64();
    for (int it = 0; it < iters; ++it) {
        const double cf = -1e-3 * kh_inv_table[(it & 15) + 1];
        cplx t[PRODUCTS];
        if (MAP == M18) {
            const int cg = lane & 7;
            cplx xv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = buf[cur][0][cg + 8 * j];
#pragma unroll
            for (int p = 0; p < PRODUCTS; ++p) {
                cplx acc = c_make(0.0, 0.0);
#pragma unroll
                for (int j = 0; j < 8; ++j) c_fma(acc, a[p][j], xv[j]);
                t[p] = c_make(cf * sum8(acc.x), cf * sum8(acc.y));
            }
        } else {
            cplx x = buf[cur][0][x_idx];
            if constexpr (PARTS == 2) {
                const cplx x1 = buf[cur][1][x_idx];
                x.x += x1.x;
                x.y += x1.y;
            }
#pragma unroll
            for (int p = 0; p < PRODUCTS; ++p) {
                cplx acc = c_make(0.0, 0.0);
                if (MAP == R16B)
                    fmac_dpp8(acc, a[p], x);
                else if (MAP == R16D)
                    fmac_dpp8_4chains(acc, a[p], x);
                else
                    BcastFma<0, NJ>::run(acc, a[p], x);
                t[p] = c_make(rowsum_mfma(acc.x, cf), rowsum_mfma(acc.y, cf));
            }
        }
#pragma unroll
        for (int p = 0; p < PRODUCTS; ++p) {
            state.x += t[p].x;
            state.y += t[p].y;
        }
        if (writer) buf[cur ^ 1][part_w][row_w] = t[0];
        __syncthreads();
        cur ^= 1;
    }
    const long long t1 = clock64();
    out[blockIdx.x * Threads<MAP>::value + tid] = state;
    if (vec != nullptr && blockIdx.x == 0 && tid < 64) {
        cplx v = buf[cur][0][tid];
        if constexpr (PARTS == 2) {
            v.x += buf[cur][1][tid].x;
            v.y += buf[cur][1][tid].y;
        }
        vec[tid] = v;
    }
    if (tid == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}

template <int MAP, int PRODUCTS>
double run(const char *name, const cplx *op, cplx *out, long long *cyc, int grid) {
    const int iters = 20000;
    constexpr int threads = Threads<MAP>::value;
    k<MAP, PRODUCTS><<<grid, threads>>>(op, out, nullptr, cyc, iters);
    hipDeviceSynchronize();
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    hipEventRecord(a);
    k<MAP, PRODUCTS><<<grid, threads>>>(op, out, nullptr, cyc, iters);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    long long h[1];
    hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);
    printf("%-52s grid=%3d: %7.1f ns/phase  %7.1f clk/phase\n", name, grid, ms * 1e6 / iters, (double)h[0] / iters);
    return ms * 1e6 / iters;
}

// the vector after three phases on a random operator
template <int MAP>
std::vector<cplx> check_vec(const cplx *op, cplx *out, cplx *vec, long long *cyc) {
    std::vector<cplx> h(64);
    k<MAP, 1><<<1, Threads<MAP>::value>>>(op, out, vec, cyc, 3);
    hipDeviceSynchronize();
    hipMemcpy(h.data(), vec, 64 * sizeof(cplx), hipMemcpyDeviceToHost);
    return h;
}

static bool same_vec(const char *name, const std::vector<cplx> &ref, const std::vector<cplx> &v) {
    double err = 0.0, mag = 0.0;
    for (int i = 0; i < 64; ++i) {
        err = fmax(err, fmax(fabs(ref[i].x - v[i].x), fabs(ref[i].y - v[i].y)));
        mag = fmax(mag, fmax(fabs(ref[i].x), fabs(ref[i].y)));
    }
    const bool ok = mag > 0.0 && err <= 1e-13 * mag;
    printf("check %-5s against M18 after 3 phases: max |diff| %.3e of %.3e  %s\n", name, err, mag, ok ? "ok" : "WRONG");
    return ok;
}

int main() {
    cplx *op, *out, *vec;
    long long *cyc;
    const size_t op_elems = 2 * 64 * 64;
    if (hipMalloc(&op, op_elems * sizeof(cplx)) != hipSuccess || hipMalloc(&out, 256 * 512 * sizeof(cplx)) != hipSuccess ||
        hipMalloc(&vec, 64 * sizeof(cplx)) != hipSuccess || hipMalloc(&cyc, 16) != hipSuccess) {
        fprintf(stderr, "no device memory\n");
        return 2;
    }
    std::vector<cplx> h_op(op_elems);
    srand(7);
    for (size_t i = 0; i < op_elems; ++i) h_op[i] = make_double2(rand() / (double)RAND_MAX - 0.5, rand() / (double)RAND_MAX - 0.5);
    hipMemcpy(op, h_op.data(), op_elems * sizeof(cplx), hipMemcpyHostToDevice);
    const std::vector<cplx> ref = check_vec<M18>(op, out, vec, cyc);
    bool ok = same_vec("R16a", ref, check_vec<R16A>(op, out, vec, cyc));
    ok = same_vec("R16b", ref, check_vec<R16B>(op, out, vec, cyc)) && ok;
    ok = same_vec("R16c", ref, check_vec<R16C>(op, out, vec, cyc)) && ok;
    ok = same_vec("R16d", ref, check_vec<R16D>(op, out, vec, cyc)) && ok;
    if (hipGetLastError() != hipSuccess || !ok) {
        fprintf(stderr, "a map computes another vector than M18: no timings\n");
        return 1;
    }
    for (int grid : {1, 256}) {
        const double m1 = run<M18, 1>("M18  1 row x 8 cols, LDS broadcast, one product", op, out, cyc, grid);
        const double a1 = run<R16A, 1>("R16a row broadcast, v_mov_b64_dpp, one product", op, out, cyc, grid);
        const double b1 = run<R16B, 1>("R16b row broadcast, v_fmac_f64_dpp, one product", op, out, cyc, grid);
        const double c1 = run<R16C, 1>("R16c 4 waves x 16 rows x 64 cols, one product", op, out, cyc, grid);
        const double d1 = run<R16D, 1>("R16d as R16b, four accumulator chains, one product", op, out, cyc, grid);
        const double m2 = run<M18, 2>("M18  two products per phase (A and B)", op, out, cyc, grid);
        const double a2 = run<R16A, 2>("R16a two products per phase", op, out, cyc, grid);
        const double b2 = run<R16B, 2>("R16b two products per phase", op, out, cyc, grid);
        const double c2 = run<R16C, 2>("R16c two products per phase", op, out, cyc, grid);
        const double d2 = run<R16D, 2>("R16d two products per phase", op, out, cyc, grid);
        printf("grid=%3d: best R16 / M18 = %.3f (one product), %.3f (two products)\n", grid, fmin(fmin(a1, d1), fmin(b1, c1)) / m1,
               fmin(fmin(a2, d2), fmin(b2, c2)) / m2);
    }
    return 0;
}
