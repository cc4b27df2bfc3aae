// Boundary co-states of the two gate functionals in the local invariants of a two-qubit gate (kh_chi_local_invariants;
// krotov_amd/functionals.py: PerfectEntanglerChi, LocalInvariantsChi -- the reference takes both from the weylchamber
// package and runs them on the host).  A gate is 4 consecutive objectives whose initial states are the Bell states B_i:
//
//   U[i][k] = <B_i|phi_k(T)>,  m = U^T U,  t = tr m,  d = det U,  G = t^2 / (16 d),  H = (t^2 - tr m^2) / (4 d),  g3 = Re H
//   PE:  F = g3 |G| - Re G                   J_G = g3 conj(G) / (2 |G|) - 1/2  (0 - 1/2 at |G| = 0),  J_H = |G| / 2
//   LI:  F = |G - G_O|^2 + (g3 - g3_O)^2     J_G = conj(G - G_O),                                     J_H = g3 - g3_O
//   J = (1 - w) F + w (1 - tr(U^+ U) / 4)
//   dG/dU = t U / (4 d) - G U^-T,   dH/dU = (t U - U m) / d - H U^-T,   U^-T = cof(U) / d
//   D = dJ / d conj U = (1 - w) conj(J_G dG/dU + J_H dH/dU) - (w / 4) U
//   chi_k = -scale sum_i D[i][k] B_i,   chi_T[k] = chi_k / ||chi_k||,  chi_norms[k] = ||chi_k||
//
// One wavefront per gate.  The 16 inner products go to the 16 groups of four adjacent lanes (group 4 i + k, lane s of it
// takes the components s, s + 4, ...; DPP sum over the four); every lane then reads all 16 and runs the 4 x 4 algebra in
// registers (wave-uniform: the compiler keeps most of it in scalar registers); the chi rows are written with a loop over
// N in steps of 64.  Every sum has a fixed order: results are bitwise repeatable and do not depend on the gate's place in
// the batch.  No LDS, no scratch, no atomics.
#pragma once

#include "kh_common.h"

#define KH_LI_WAVES 4              // gates per workgroup
#define KH_LI_MODE_PE 0
#define KH_LI_MODE_LI 1
#define KH_LI_SINGULAR_RTOL 1e-10  // |det U| <= this x (||U||_F / 2)^4: singular (functionals.py: LI_SINGULAR_RTOL)

#define KH_LI_HD __device__ __forceinline__

struct KhLiArgs {
    const cplx *psi;      // [K][N] phi_k(T)
    const cplx *bell;     // [4][N], or [M][4][N] with bell_per_gate
    const double *inv;    // LI: (Re G_O, Im G_O, g3_O) [3], or [M][3] with inv_per_gate; PE: not read
    cplx *chi;            // [K][N]
    double *norms;        // [K]
    double *J;            // [M]
    const int *active;    // replica engines: [B] (0: the replica's gates are skipped), or NULL
    int M, N;             // gates, state dimension
    int gates_per_replica;
    int bell_per_gate, inv_per_gate;
    double w, scale;
};

KH_LI_HD cplx li_mul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
KH_LI_HD cplx li_add(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }
KH_LI_HD cplx li_sub(cplx a, cplx b) { return make_double2(a.x - b.x, a.y - b.y); }
KH_LI_HD cplx li_scale(double s, cplx a) { return make_double2(s * a.x, s * a.y); }
KH_LI_HD cplx li_conj(cplx a) { return make_double2(a.x, -a.y); }
// a b - c d
KH_LI_HD cplx li_minor(cplx a, cplx b, cplx c, cplx d) { return li_sub(li_mul(a, b), li_mul(c, d)); }
// a x - b y + c z
KH_LI_HD cplx li_three(cplx a, cplx x, cplx b, cplx y, cplx c, cplx z) {
    return li_add(li_sub(li_mul(a, x), li_mul(b, y)), li_mul(c, z));
}

// The 4 x 4 algebra of one gate: C[i][k] = -scale D[i][k] (chi_k = sum_i C[i][k] B_i) and the value J.  Returns false
// -- C zero, J NaN -- where U is singular.  target = (Re G_O, Im G_O, g3_O), read in LI mode only.
template <int MODE>
KH_LI_HD bool kh_li_gate_terms(const cplx (&U)[4][4], const double (&target)[3], double w, double scale, cplx (&C)[4][4],
                               double *J_out) {
    // m = U^T U (symmetric), t, tr m^2, ||U||_F^2
    cplx m[4][4];
    double fro2 = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            fro2 += U[r][c].x * U[r][c].x + U[r][c].y * U[r][c].y;
            cplx acc = make_double2(0.0, 0.0);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = li_add(acc, li_mul(U[i][r], U[i][c]));
            m[r][c] = acc;
        }
    const cplx t = li_add(li_add(m[0][0], m[1][1]), li_add(m[2][2], m[3][3]));
    cplx trm2 = make_double2(0.0, 0.0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) trm2 = li_add(trm2, li_mul(m[r][c], m[c][r]));
    // determinant and adjugate A (U^-1 = A / d) from the 2 x 2 minors of the upper and the lower two rows
    const cplx s0 = li_minor(U[0][0], U[1][1], U[1][0], U[0][1]), s1 = li_minor(U[0][0], U[1][2], U[1][0], U[0][2]);
    const cplx s2 = li_minor(U[0][0], U[1][3], U[1][0], U[0][3]), s3 = li_minor(U[0][1], U[1][2], U[1][1], U[0][2]);
    const cplx s4 = li_minor(U[0][1], U[1][3], U[1][1], U[0][3]), s5 = li_minor(U[0][2], U[1][3], U[1][2], U[0][3]);
    const cplx c5 = li_minor(U[2][2], U[3][3], U[3][2], U[2][3]), c4 = li_minor(U[2][1], U[3][3], U[3][1], U[2][3]);
    const cplx c3 = li_minor(U[2][1], U[3][2], U[3][1], U[2][2]), c2 = li_minor(U[2][0], U[3][3], U[3][0], U[2][3]);
    const cplx c1 = li_minor(U[2][0], U[3][2], U[3][0], U[2][2]), c0 = li_minor(U[2][0], U[3][1], U[3][0], U[2][1]);
    const cplx d = li_add(li_three(s0, c5, s1, c4, s2, c3), li_three(s3, c2, s4, c1, s5, c0));
    const double absd = sqrt(d.x * d.x + d.y * d.y);
    const double unit = 0.25 * fro2;
    if (!(absd > KH_LI_SINGULAR_RTOL * (unit * unit))) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) C[i][k] = make_double2(0.0, 0.0);
        *J_out = __builtin_nan("");
        return false;
    }
    cplx A[4][4];
    A[0][0] = li_three(U[1][1], c5, U[1][2], c4, U[1][3], c3);
    A[0][1] = li_scale(-1.0, li_three(U[0][1], c5, U[0][2], c4, U[0][3], c3));
    A[0][2] = li_three(U[3][1], s5, U[3][2], s4, U[3][3], s3);
    A[0][3] = li_scale(-1.0, li_three(U[2][1], s5, U[2][2], s4, U[2][3], s3));
    A[1][0] = li_scale(-1.0, li_three(U[1][0], c5, U[1][2], c2, U[1][3], c1));
    A[1][1] = li_three(U[0][0], c5, U[0][2], c2, U[0][3], c1);
    A[1][2] = li_scale(-1.0, li_three(U[3][0], s5, U[3][2], s2, U[3][3], s1));
    A[1][3] = li_three(U[2][0], s5, U[2][2], s2, U[2][3], s1);
    A[2][0] = li_three(U[1][0], c4, U[1][1], c2, U[1][3], c0);
    A[2][1] = li_scale(-1.0, li_three(U[0][0], c4, U[0][1], c2, U[0][3], c0));
    A[2][2] = li_three(U[3][0], s4, U[3][1], s2, U[3][3], s0);
    A[2][3] = li_scale(-1.0, li_three(U[2][0], s4, U[2][1], s2, U[2][3], s0));
    A[3][0] = li_scale(-1.0, li_three(U[1][0], c3, U[1][1], c1, U[1][2], c0));
    A[3][1] = li_three(U[0][0], c3, U[0][1], c1, U[0][2], c0);
    A[3][2] = li_scale(-1.0, li_three(U[3][0], s3, U[3][1], s1, U[3][2], s0));
    A[3][3] = li_three(U[2][0], s3, U[2][1], s1, U[2][2], s0);
    const cplx inv_d = li_scale(1.0 / (absd * absd), li_conj(d));
    const cplx t2 = li_mul(t, t);
    const cplx G = li_scale(1.0 / 16.0, li_mul(t2, inv_d));
    const cplx H = li_scale(0.25, li_mul(li_sub(t2, trm2), inv_d));
    const double g3 = H.x;
    cplx J_G;
    double J_H, F;
    if (MODE == KH_LI_MODE_PE) {
        const double absG = sqrt(G.x * G.x + G.y * G.y);
        F = g3 * absG - G.x;
        J_G = make_double2(-0.5, 0.0);
        if (absG > 0.0) J_G = li_add(J_G, li_scale(g3 / (2.0 * absG), li_conj(G)));
        J_H = 0.5 * absG;
    } else {
        const cplx dG = make_double2(G.x - target[0], G.y - target[1]);
        const double d3 = g3 - target[2];
        F = (dG.x * dG.x + dG.y * dG.y) + d3 * d3;
        J_G = li_conj(dG);
        J_H = d3;
    }
    *J_out = (1.0 - w) * F + w * (1.0 - unit);
    // per element: dG/dU = (t / 4d) U - (G / d) A^T,  dH/dU = (t U - U m) / d - (H / d) A^T
    const cplx t_4d = li_scale(0.25, li_mul(t, inv_d));
    const cplx t_d = li_mul(t, inv_d);
    const cplx G_d = li_mul(G, inv_d), H_d = li_mul(H, inv_d);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cplx Um = make_double2(0.0, 0.0);
#pragma unroll
            for (int j = 0; j < 4; ++j) Um = li_add(Um, li_mul(U[i][j], m[j][k]));
            const cplx dG = li_sub(li_mul(t_4d, U[i][k]), li_mul(G_d, A[k][i]));
            const cplx dH = li_sub(li_sub(li_mul(t_d, U[i][k]), li_mul(inv_d, Um)), li_mul(H_d, A[k][i]));
            const cplx grad = li_conj(li_add(li_mul(J_G, dG), li_scale(J_H, dH)));
            const cplx D = li_sub(li_scale(1.0 - w, grad), li_scale(0.25 * w, U[i][k]));
            C[i][k] = li_scale(-scale, D);
        }
    return true;
}

template <int MODE>
__global__ void __launch_bounds__(64 * KH_LI_WAVES) kh_chi_li_kernel(KhLiArgs a) {
    const int gate = blockIdx.x * KH_LI_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gate >= a.M) return;
    if (a.active != nullptr && a.active[gate / a.gates_per_replica] == 0) return;  // (wave-uniform; nothing to meet at)
    const int N = a.N;
    const cplx *psi = a.psi + (size_t)gate * 4 * N;
    const cplx *bell = a.bell + (a.bell_per_gate ? (size_t)gate * 4 * N : (size_t)0);
    cplx *chi = a.chi + (size_t)gate * 4 * N;

    // U[i][k] = <B_i|phi_k>: lane group 4 i + k
    const int grp = lane >> 2, sub = lane & 3;
    const cplx *bi = bell + (size_t)(grp >> 2) * N, *pk = psi + (size_t)(grp & 3) * N;
    cplx acc = c_make(0.0, 0.0);
    for (int n = sub; n < N; n += 4) c_fma_conj(acc, bi[n], pk[n]);
    acc.x = sum4(acc.x);
    acc.y = sum4(acc.y);
    cplx U[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) U[i][k] = c_make(readlane_f64(acc.x, 4 * (4 * i + k)), readlane_f64(acc.y, 4 * (4 * i + k)));

    double target[3] = {0.0, 0.0, 0.0};
    if (MODE == KH_LI_MODE_LI) {
        const double *inv = a.inv + (a.inv_per_gate ? (size_t)gate * 3 : (size_t)0);
        target[0] = inv[0], target[1] = inv[1], target[2] = inv[2];
    }
    cplx C[4][4];
    double J;
    kh_li_gate_terms<MODE>(U, target, a.w, a.scale, C, &J);

    // chi_k = sum_i C[i][k] B_i: the norms first, then the rows (a singular U: C = 0, zero rows)
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
    for (int n = lane; n < N; n += 64) {
        const cplx b0 = bell[n], b1 = bell[(size_t)N + n], b2 = bell[(size_t)2 * N + n], b3 = bell[(size_t)3 * N + n];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cplx v = c_mul(C[0][k], b0);
            c_fma(v, C[1][k], b1);
            c_fma(v, C[2][k], b2);
            c_fma(v, C[3][k], b3);
            sq[k] = fma(v.x, v.x, fma(v.y, v.y, sq[k]));
        }
    }
    double nrm[4], rinv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nrm[k] = sqrt(sum64(sq[k]));
        rinv[k] = nrm[k] > 0.0 ? 1.0 / nrm[k] : 0.0;  // zero norm: a zero row, norm 0
    }
    for (int n = lane; n < N; n += 64) {
        const cplx b0 = bell[n], b1 = bell[(size_t)N + n], b2 = bell[(size_t)2 * N + n], b3 = bell[(size_t)3 * N + n];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cplx v = c_mul(C[0][k], b0);
            c_fma(v, C[1][k], b1);
            c_fma(v, C[2][k], b2);
            c_fma(v, C[3][k], b3);
            chi[(size_t)k * N + n] = nrm[k] > 0.0 ? c_make(v.x * rinv[k], v.y * rinv[k]) : c_make(0.0, 0.0);
        }
    }
    if (lane < 4) a.norms[(size_t)gate * 4 + lane] = lane == 0 ? nrm[0] : (lane == 1 ? nrm[1] : (lane == 2 ? nrm[2] : nrm[3]));
    if (lane == 0) a.J[gate] = J;
}
