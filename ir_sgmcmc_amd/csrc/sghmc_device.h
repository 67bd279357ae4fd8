// SGHMC (Chen, Fox & Guestrin 2014, eq. 15 with beta_hat = 0): the one place its arithmetic lives.  Used by the SGHMC instantiations
// of the fused update kernels (stencil_kernels.hip, bending_kernels.hip) and by the stateless sghmc_update_kernel (field_kernels.hip).
//
// Per element of the velocity grid, float32, every operation rounded once (the __f*_rn intrinsics: nothing contracts into an FMA,
// so numpy float32 reproduces the step bit for bit -- tests/_sghmc.py):
//   t  = fsub(fmul(oma, m), fmul(lr, gs))                      oma = (float)(1 - (double)friction), host
//   m' = T > 0 ? fadd(t, fmul(fmul(amp, sigma), n)) : t        amp = (float)sqrt(2 friction lr T), host
//   v' = fadd(v, m')
// gs is grad_v (sigma^2 already applied), n a standard normal.  friction = 1: Langevin dynamics whose noise is persisted in v;
// friction < 1: momentum; T = 0: no noise is drawn, a heavy-ball optimiser.
//
// The noise is perturb_kernel's (field_kernels.hip) with another stream word: one Philox4x32-10 call per voxel pair (z even, z + 1)
// and chain, counter (idx lo, idx hi, iteration lo, 0x484D ^ iteration hi), idx = chain * Vg + voxel index of the pair's even plane,
// the six normals assigned e0 e1 / e2 o0 / o1 o2 -- never a draw the forward perturbation (stream word 0x5347) has used.
#pragma once
#include "common.h"

namespace irs {

constexpr uint32_t kSghmcStream = 0x484Du;

// what an SGHMC update needs on top of an SGLD one (by value into the kernels)
struct SghmcArgs {
    float* m;          // momentum, shape and layout of v; read and written
    const float* eps;  // injected standard normals or nullptr (Philox)
    float oma, amp;    // 1 - friction; sqrt(2 friction lr T)
    int noisy;         // T > 0
    uint64_t seed;
};

// the host-side constants of a step
inline SghmcArgs sghmc_args(float* m, const float* eps, float lr, float friction, float temperature, uint64_t seed) {
    SghmcArgs a;
    a.m = m;
    a.eps = eps;
    a.oma = (float)(1.0 - (double)friction);
    a.amp = (float)sqrt(2.0 * (double)friction * (double)lr * (double)temperature);
    a.noisy = temperature > 0.0f ? 1 : 0;
    a.seed = seed;
    return a;
}

#if defined(__HIPCC__)
// one element: (v, m) -> (v1, m1)
__device__ __forceinline__ void sghmc_step(float v, float m, float gs, float sigma, float n, float lr, float oma, float amp, bool noisy,
                                           float& v1, float& m1) {
    const float t = __fsub_rn(__fmul_rn(oma, m), __fmul_rn(lr, gs));
    m1 = noisy ? __fadd_rn(t, __fmul_rn(__fmul_rn(amp, sigma), n)) : t;
    v1 = __fadd_rn(v, m1);
}

// the six normals of the pair whose even plane holds the voxel `voxa` (index within a chain's volume): n[plane parity][channel]
__device__ __forceinline__ void sghmc_pair_draw(int chain, int64_t Vg, int64_t voxa, uint64_t it, uint64_t seed, float (&n)[2][3]) {
    const uint64_t idx = (uint64_t)chain * (uint64_t)Vg + (uint64_t)voxa;
    const U4 r = philox4x32_10(U4{(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)it, kSghmcStream ^ (uint32_t)(it >> 32)}, (uint32_t)seed,
                               (uint32_t)(seed >> 32));
    uint32_t w[6];
    split21(r, w);
    box_muller21(w[0], w[1], n[0][0], n[0][1]);
    box_muller21(w[2], w[3], n[0][2], n[1][0]);
    box_muller21(w[4], w[5], n[1][1], n[1][2]);
}
#endif

}  // namespace irs
