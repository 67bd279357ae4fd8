// Per-voxel arithmetic of the posterior comparison ("Posterior comparison"): the distances between the
// 3-D Gaussians fitted to two Welford states A and B of the displacement (covariance_device.h).  Plain host / device functions
// over scalars, all in double, so the kernel and a host build compute the same thing.
//
// The three eigen-solves run one after another: A's, then B's, after which the overlaps G_ik = e^B_i . e^A_k carry everything
// that needs both bases; then the one of R, of which only the eigenvalues are read.  Every trace below is a sum of
// non-negative terms over those overlaps: no inverse matrix is ever formed.
#pragma once
#include "covariance_device.h"

namespace irs {

// the comparison of two covariances and a shift, before anything is rounded to float32
struct CompareCore {
    double shift2;     // |Delta|^2
    double half_log;   // 1/2 ln(t_A / t_B)
    double bures2;     // the squared Bures distance, clamped at 0
    double jeffreys;   // KL(A|B) + KL(B|A) of the floored covariances
    double terms;      // the sum of the absolute values of the terms of jeffreys (what its rounding error scales with)
    double tr_a, tr_b;
    bool floored;      // one of the six eigenvalues was raised to floor2
};

// SA, SB: a00, a11, a22, a01, a02, a12 of the two covariances; dl: the shift; floor2 = std_floor^2
__host__ __device__ inline CompareCore compare_core(const double (&SA)[6], const double (&SB)[6], const double (&dl)[3], double floor2) {
    CompareCore o;
    o.shift2 = dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2];
    o.tr_a = SA[0] + SA[1] + SA[2];
    o.tr_b = SB[0] + SB[1] + SB[2];
    // eigenvalues la, lb and eigenvectors ea[k], eb[i]
    double la[3], ea[3][3], lb[3], eb[3][3];
    cov_eigen(SA[0], SA[1], SA[2], SA[3], SA[4], SA[5], la[0], la[1], la[2], ea[0], ea[1], ea[2]);
    cov_eigen(SB[0], SB[1], SB[2], SB[3], SB[4], SB[5], lb[0], lb[1], lb[2], eb[0], eb[1], eb[2]);
    bool floored = false;
    double fa[3], fb[3], rb[3];  // the floored eigenvalues, and the square roots of B's clamped ones
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        la[i] = fmax(la[i], 0.0), lb[i] = fmax(lb[i], 0.0);  // a rounded M need not be positive semi-definite
        floored = floored || la[i] < floor2 || lb[i] < floor2;
        fa[i] = fmax(la[i], floor2), fb[i] = fmax(lb[i], floor2);
        rb[i] = sqrt(lb[i]);
    }
    o.floored = floored;

    // everything that needs both bases: the overlaps G[i][k] = e^B_i . e^A_k
    double G[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) G[i][k] = eb[i][0] * ea[k][0] + eb[i][1] * ea[k][1] + eb[i][2] * ea[k][2];
    // Jeffreys: tr(B~^-1 A~) + tr(A~^-1 B~) = sum_ik G_ik^2 (fa_k / fb_i + fb_i / fa_k); the shift under both inverses
    double tr = 0.0, quad = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tr += G[i][k] * G[i][k] * (fa[k] / fb[i] + fb[i] / fa[k]);
        const double pa = ea[i][0] * dl[0] + ea[i][1] * dl[1] + ea[i][2] * dl[2];
        const double pb = eb[i][0] * dl[0] + eb[i][1] * dl[1] + eb[i][2] * dl[2];
        quad += pa * pa / fa[i] + pb * pb / fb[i];
    }
    o.jeffreys = 0.5 * (tr - 6.0 + quad);
    o.terms = 0.5 * (tr + 6.0 + quad);
    // Bures: R = B^1/2 A B^1/2 in B's eigenbasis, R_ij = rb_i rb_j sum_k la_k G_ik G_jk -- symmetric as it is formed
    double R[6];
    {
        const int I[6] = {0, 1, 2, 0, 0, 1}, J[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            const int i = I[e], j = J[e];
            R[e] = rb[i] * rb[j] * (la[0] * G[i][0] * G[j][0] + la[1] * G[i][1] * G[j][1] + la[2] * G[i][2] * G[j][2]);
        }
    }
    double lr[3], u0[3], u1[3], u2[3];
    cov_eigen(R[0], R[1], R[2], R[3], R[4], R[5], lr[0], lr[1], lr[2], u0, u1, u2);
    const double cross = sqrt(fmax(lr[0], 0.0)) + sqrt(fmax(lr[1], 0.0)) + sqrt(fmax(lr[2], 0.0));
    o.bures2 = fmax(o.tr_a + o.tr_b - 2.0 * cross, 0.0);
    // 1/2 ln(ta / tb) through log1p of the difference over the smaller: exactly 0 for ta == tb, exactly antisymmetric under
    // A <-> B, and relatively accurate where the ratio is close to 1 (ln of a rounded quotient is only absolutely so)
    const double ta = fmax(o.tr_a, 3.0 * floor2), tb = fmax(o.tr_b, 3.0 * floor2);
    o.half_log = ta >= tb ? 0.5 * log1p((ta - tb) / tb) : -0.5 * log1p((tb - ta) / ta);
    return o;
}

struct CompareMaps {
    float shift, log_std_ratio, bures, jeffreys;  // the four planes; NaN where !finite
    double tr_a, tr_b;                            // tr S_A, tr S_B
    bool finite;                                  // false: one of the 18 state values was not finite
    bool floored;                                 // one of the six eigenvalues was raised to floor^2
};

// S = diag(sc) M diag(sc) * inv as a00, a11, a22, a01, a02, a12
__host__ __device__ inline void compare_matrix(const float (&M)[6], double inv, const double (&sc)[3], double (&S)[6]) {
    S[0] = sc[0] * sc[0] * (double)M[0] * inv, S[1] = sc[1] * sc[1] * (double)M[1] * inv, S[2] = sc[2] * sc[2] * (double)M[2] * inv;
    S[3] = sc[0] * sc[1] * (double)M[3] * inv, S[4] = sc[0] * sc[2] * (double)M[4] * inv, S[5] = sc[1] * sc[2] * (double)M[5] * inv;
}

// mu_x, M_x: the states; inv_x = 1 / (n_x - 1); sc: the per-channel scale; floor2 = std_floor^2
__host__ __device__ inline CompareMaps compare_maps(const float (&mu_a)[3], const float (&M_a)[6], double inv_a, const float (&mu_b)[3],
                                                    const float (&M_b)[6], double inv_b, const double (&sc)[3], double floor2) {
    CompareMaps o;
    float chk = 0.0f;  // finite exactly when all 18 values are: x * 0 is 0 for a finite x and NaN otherwise
#pragma unroll
    for (int i = 0; i < 3; ++i) chk += mu_a[i] * 0.0f + mu_b[i] * 0.0f;
#pragma unroll
    for (int i = 0; i < 6; ++i) chk += M_a[i] * 0.0f + M_b[i] * 0.0f;
    o.finite = chk == 0.0f;
    double dl[3], SA[6], SB[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) dl[i] = sc[i] * ((double)mu_a[i] - (double)mu_b[i]);
    compare_matrix(M_a, inv_a, sc, SA);
    compare_matrix(M_b, inv_b, sc, SB);
    const CompareCore c = compare_core(SA, SB, dl, floor2);
    const float nan = __builtin_nanf("");
    o.tr_a = c.tr_a, o.tr_b = c.tr_b, o.floored = c.floored;
    o.shift = o.finite ? (float)sqrt(c.shift2) : nan;
    o.log_std_ratio = o.finite ? (float)c.half_log : nan;
    o.bures = o.finite ? (float)sqrt(c.bures2) : nan;
    o.jeffreys = o.finite ? (float)c.jeffreys : nan;
    return o;
}

}  // namespace irs
