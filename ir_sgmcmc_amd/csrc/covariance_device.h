// Per-voxel arithmetic of the displacement covariance posterior: the Welford fold of one record into
// the mean and the six co-moments, and the eigen-decomposition of the 3 x 3 sample covariance behind the final maps.  Both are
// plain host / device functions over scalars, so every kernel variant computes the same thing and a host build can check them.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace irs {

constexpr int kCovSweeps = 5;  // cyclic Jacobi sweeps: 4 reach an off-diagonal norm of 2e-16 |S|_F, one spare

// x: one record's displacement at a voxel, the k-th record of all (k >= 1).  mu: mean, M: co-moments xx, yy, zz, xy, xz, yz.
// k = 1 overwrites; otherwise delta_a = x_a - mu_a, mu_a += delta_a / k, M_ab += delta_a * (x_b - mu_b) with the new mu_b.
__host__ __device__ inline void cov_fold(float x0, float x1, float x2, int k, float (&mu)[3], float (&M)[6]) {
    if (k == 1) {
        mu[0] = x0;
        mu[1] = x1;
        mu[2] = x2;
        M[0] = M[1] = M[2] = M[3] = M[4] = M[5] = 0.0f;
        return;
    }
    const float fk = (float)k;
    const float d0 = x0 - mu[0], d1 = x1 - mu[1], d2 = x2 - mu[2];
    mu[0] += d0 / fk;
    mu[1] += d1 / fk;
    mu[2] += d2 / fk;
    const float e0 = x0 - mu[0], e1 = x1 - mu[1], e2 = x2 - mu[2];
    M[0] += d0 * e0;
    M[1] += d1 * e1;
    M[2] += d2 * e2;
    M[3] += d0 * e1;
    M[4] += d0 * e2;
    M[5] += d1 * e2;
}

// one Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix: app, aqq the diagonal entries, apq the entry it
// annihilates, arp, arq the third row's; (v0p, v0q), ... the two columns of the accumulated rotations.  apq == 0: identity.
__host__ __device__ inline void cov_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                           double& v1p, double& v1q, double& v2p, double& v2q) {
    const double tau = (aqq - app) / (2.0 * apq);
    double t = 1.0 / (fabs(tau) + sqrt(1.0 + tau * tau));  // tau^2 = inf gives t = 0
    t = tau < 0.0 ? -t : t;
    t = apq == 0.0 ? 0.0 : t;
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0, v0q = b0, v1p = a1, v1q = b1, v2p = a2, v2q = b2;
}

__host__ __device__ inline void cov_swap_if_less(double& la, double& lb, double (&va)[3], double (&vb)[3]) {
    const bool sw = la < lb;
    const double l = la;
    la = sw ? lb : la;
    lb = sw ? l : lb;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double v = va[i];
        va[i] = sw ? vb[i] : va[i];
        vb[i] = sw ? v : vb[i];
    }
}

struct CovMaps {
    float std[3];  // sqrt of the eigenvalues, descending
    float dir[3];  // unit eigenvector of the largest one, its component of largest magnitude positive; 0 where std[0] is 0
    float fa;      // fractional anisotropy
    bool finite;   // false: the state held a non-finite value and everything above is NaN
};

// the 3 x 3 symmetric eigen-solver: kCovSweeps cyclic Jacobi sweeps over the pairs (0,1), (0,2), (1,2) of the matrix with the
// diagonal a00, a11, a22 and the off-diagonal a01, a02, a12 -> the eigenvalues l0 >= l1 >= l2 (as the sweeps leave them: a
// rounded matrix need not be positive semi-definite) and their unit eigenvectors e0, e1, e2
__host__ __device__ inline void cov_eigen(double a00, double a11, double a22, double a01, double a02, double a12, double& l0,
                                          double& l1, double& l2, double (&e0)[3], double (&e1)[3], double (&e2)[3]) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
    for (int sweep = 0; sweep < kCovSweeps; ++sweep) {
        cov_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0,1); the third index is 2
        cov_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0,2); the third index is 1
        cov_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1,2); the third index is 0
    }
    l0 = a00, l1 = a11, l2 = a22;
    e0[0] = v00, e0[1] = v10, e0[2] = v20;
    e1[0] = v01, e1[1] = v11, e1[2] = v21;
    e2[0] = v02, e2[1] = v12, e2[2] = v22;
    cov_swap_if_less(l0, l1, e0, e1);
    cov_swap_if_less(l0, l2, e0, e2);
    cov_swap_if_less(l1, l2, e1, e2);
}

// mu, M: the state after n >= 1 records; inv = 1 / max(n - 1, 1); sc: the per-channel scale
__host__ __device__ inline CovMaps cov_maps(const float (&mu)[3], const float (&M)[6], double inv, const double (&sc)[3]) {
    CovMaps o;
    float chk = 0.0f;  // finite exactly when all nine values are: x * 0 is 0 for a finite x and NaN otherwise
#pragma unroll
    for (int i = 0; i < 3; ++i) chk += mu[i] * 0.0f;
#pragma unroll
    for (int i = 0; i < 6; ++i) chk += M[i] * 0.0f;
    o.finite = chk == 0.0f;
    const double a00 = sc[0] * sc[0] * (double)M[0] * inv, a11 = sc[1] * sc[1] * (double)M[1] * inv, a22 = sc[2] * sc[2] * (double)M[2] * inv;
    const double a01 = sc[0] * sc[1] * (double)M[3] * inv, a02 = sc[0] * sc[2] * (double)M[4] * inv, a12 = sc[1] * sc[2] * (double)M[5] * inv;
    double l0, l1, l2, e0[3], e1[3], e2[3];
    cov_eigen(a00, a11, a22, a01, a02, a12, l0, l1, l2, e0, e1, e2);
    l0 = fmax(l0, 0.0), l1 = fmax(l1, 0.0), l2 = fmax(l2, 0.0);  // a rounded M need not be positive semi-definite
    const float nan = __builtin_nanf("");
    o.std[0] = o.finite ? (float)sqrt(l0) : nan;
    o.std[1] = o.finite ? (float)sqrt(l1) : nan;
    o.std[2] = o.finite ? (float)sqrt(l2) : nan;
    float d0 = (float)e0[0], d1 = (float)e0[1], d2 = (float)e0[2];
    float big = d0;  // the stored component of largest magnitude, the lowest channel on a tie
    big = fabsf(d1) > fabsf(big) ? d1 : big;
    big = fabsf(d2) > fabsf(big) ? d2 : big;
    const bool none = !(l0 > 0.0), flip = big < 0.0f;  // no spread, no direction
    o.dir[0] = !o.finite ? nan : none ? 0.0f : flip ? -d0 : d0;
    o.dir[1] = !o.finite ? nan : none ? 0.0f : flip ? -d1 : d1;
    o.dir[2] = !o.finite ? nan : none ? 0.0f : flip ? -d2 : d2;
    const double lm = (l0 + l1 + l2) / 3.0, den = l0 * l0 + l1 * l1 + l2 * l2;
    const double num = (l0 - lm) * (l0 - lm) + (l1 - lm) * (l1 - lm) + (l2 - lm) * (l2 - lm);
    o.fa = !o.finite ? nan : den > 0.0 ? (float)sqrt(1.5 * num / den) : 0.0f;
    return o;
}

}  // namespace irs
