// The normalised gradient field distance (Haber & Modersitzki 2006; include/irsgmcmc.h carries the definition): the one place its
// arithmetic lives.  Used by both kernels of ngf_kernels.hip.
//
// Per voxel, float32, every operation rounded once (the __f*_rn intrinsics: nothing contracts into an FMA, so numpy float32
// reproduces d, c and g bit for bit -- tests/_ngf.py).  With a = grad F and b = grad M (ngf_diff per axis, axes in the order z, y, x),
// ef2 = fmul(eps_f, eps_f) and em2 = fmul(eps_m, eps_m):
//   P   = fadd(fadd(fmul(az, bz), fmul(ay, by)), fmul(ax, bx))
//   Nf  = fadd(fadd(fadd(fmul(az, az), fmul(ay, ay)), fmul(ax, ax)), ef2)          Nm alike from b and em2
//   r   = fdiv(P, fmul(Nf, Nm))            d = fsub(1, fmul(P, r))
//   s   = fdiv(P, Nm)                      k = fmul(fmul(-2, u), r)
//   c_i = fmul(k, fsub(a_i, fmul(s, b_i)))
// and the adjoint of the clamped central difference on one axis of length n at index y, from cm = c[max(y - 1, 0)] and
// cp = c[min(y + 1, n - 1)]:
//   g_axis = fmul(0.5, fsub(fmul(sm, cm), fmul(sp, cp)))      sm = y == 0 ? -1 : 1,  sp = y == n - 1 ? -1 : 1
// (interior: 0.5 (c[y-1] - c[y+1]); low face: 0.5 (-c[0] - c[1]); high face: 0.5 (c[n-2] + c[n-1]); n = 1: -c[0] + c[0] = 0),
//   g = fadd(fadd(g_z, g_y), g_x).
#pragma once
#include "common.h"

namespace irs {

#if defined(__HIPCC__)
// the clamped central difference in voxel units from the two neighbours (the caller clamps the indices)
__device__ __forceinline__ float ngf_diff(float hi, float lo) { return __fmul_rn(0.5f, __fsub_rn(hi, lo)); }

__device__ __forceinline__ float ngf_dot(const float (&p)[3], const float (&q)[3]) {
    return __fadd_rn(__fadd_rn(__fmul_rn(p[0], q[0]), __fmul_rn(p[1], q[1])), __fmul_rn(p[2], q[2]));
}

// one voxel: the gradients a of the fixed and b of the moving image, the upstream weight u -> d and the coefficients c = u dd/db
__device__ __forceinline__ void ngf_point(const float (&a)[3], const float (&b)[3], float u, float ef2, float em2, float& d,
                                          float (&c)[3]) {
    const float P = ngf_dot(a, b);
    const float Nf = __fadd_rn(ngf_dot(a, a), ef2);
    const float Nm = __fadd_rn(ngf_dot(b, b), em2);
    const float r = __fdiv_rn(P, __fmul_rn(Nf, Nm));
    d = __fsub_rn(1.0f, __fmul_rn(P, r));
    const float s = __fdiv_rn(P, Nm);
    const float k = __fmul_rn(__fmul_rn(-2.0f, u), r);
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = __fmul_rn(k, __fsub_rn(a[i], __fmul_rn(s, b[i])));
}

// the tap weights of the adjoint difference at index y of an axis of length n: -1 where the neighbour is the clamped voxel itself
__device__ __forceinline__ float ngf_tap_lo(int y) { return y == 0 ? -1.0f : 1.0f; }
__device__ __forceinline__ float ngf_tap_hi(int y, int n) { return y == n - 1 ? -1.0f : 1.0f; }

// one axis of grad^T c from the two clamped neighbours and their tap weights
__device__ __forceinline__ float ngf_adjoint_axis(float cm, float cp, float sm, float sp) {
    return __fmul_rn(0.5f, __fsub_rn(__fmul_rn(sm, cm), __fmul_rn(sp, cp)));
}
#endif

}  // namespace irs
