// The body of the batched operator-times-stored-trajectory kernels (kh_generic.h: kh_gen_adjoint_side,
// kh_gen_apply_store), included into each of them so that the adjoint-side pre-pass compiles to exactly the code it had
// as a function of its own.  Expects op (row-major N x N), xk / vk (this objective's [nt][N] input / output), N, nt,
// APPLY (constant expression) and factors ([nt] or NULL; read only where APPLY): vk[n] = factors[n] op xk[n].
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = lane & 15, kq = lane >> 4;
    // this lane's time points (B operand columns): one per vector group
    const int n0 = (blockIdx.y * 4 + wave) * 16 * KH_GEN_ADJ_VG + j;
    const int G = (N + 15) / 16;
    for (int g = 0; g < G; ++g) {
        kh_gen_d4 dr[KH_GEN_ADJ_VG], di[KH_GEN_ADJ_VG];
#pragma unroll
        for (int vg = 0; vg < KH_GEN_ADJ_VG; ++vg) dr[vg] = di[vg] = kh_gen_d4{0.0, 0.0, 0.0, 0.0};
        const int arow = 16 * g + j;  // A operand: row lane & 15
        for (int kb = 0; kb < G; ++kb) {
            cplx a[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int kk = 16 * kb + 4 * ks + kq;
                a[ks] = (kk < N && arow < N) ? op[(size_t)arow * N + kk] : c_make(0.0, 0.0);
            }
#pragma unroll
            for (int vg = 0; vg < KH_GEN_ADJ_VG; ++vg) {
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
#pragma unroll
        for (int vg = 0; vg < KH_GEN_ADJ_VG; ++vg) {
            const int n = n0 + 16 * vg;
            const double fac = (APPLY && factors != nullptr && n < nt) ? factors[n] : 1.0;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = 16 * g + 4 * reg + kq;
                if (n < nt && row < N)
                    vk[(size_t)n * N + row] = APPLY ? c_make(fac * dr[vg][reg], fac * di[vg][reg]) : c_make(dr[vg][reg], di[vg][reg]);
            }
        }
    }
