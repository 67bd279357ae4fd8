// Bending-energy prior: the second-order differential operator (HessianOperator = GradientOperator applied twice, forward
// differences with the difference array replicate-padded, both times) as z-marching kernels.
//
// Per chain and component f, with w(q) = 2 for q = n - 2 and 1 otherwise (the replicated last difference counted twice):
//   y = sum_a sum_{i <= n_a - 3} (f[i+2] - 2 f[i+1] + f[i])^2                                            "pure" terms
//     + 2 sum_{a<b} sum_{i <= n_a - 2, j <= n_b - 2} w_a(i) w_b(j) (f[i+1,j+1] - f[i,j+1] - f[i+1,j] + f[i,j])^2   "mixed" terms
// (the replicated planes of a second difference along its own axis contribute exactly 0).  Its gradient 2 H^T W H f splits into
// one-dimensional operators, which is how it is evaluated here:
//   H^T W H f = sum_a P_a f + 2 sum_{a<b} L_a L_b f
//   L_a = D_a^T W_a D_a   the weighted 3-tap operator of the first-order prior (stencil_kernels.hip: sgld_update_march_kernel)
//   P_a = (D_a^2)^T M_a D_a^2   5 taps; M_a keeps the second differences based at i <= n_a - 3
// In the interior this is the 25-tap stencil {centre 84, axis neighbours -24, axis distance two +2, in-plane diagonals +4} / 2;
// at the faces the weights below decide, nothing is special-cased.
//
// Schedule: a 256-thread workgroup owns a 32 x 8 column tile of ONE component of one chain and marches along z over a segment.
// The planes zc - 2 .. zc + 2 sit in an LDS ring of 8 planes of (32 + 4) x (8 + 4) values (two-voxel halo, 1.7 x the tile's own
// voxels; 13.5 KB, so LDS never limits the 8 workgroups a CU holds); replicate padding by clamped loads at staging time, as in
// the other marching kernels -- a clamped value only ever meets a zero weight.  A segment re-stages two planes on either side.
// One device function (bending_point) holds the stencil: the energy, the gradient and the fused update call it.
#include "common.h"
#include "kernels.h"
#include "scalar_kernels.h"

namespace irs {

namespace {

constexpr int kBdBlock = 256;
constexpr int BTX = 32, BTY = 8, BHALO = 2, BPX = BTX + 2 * BHALO, BPY = BTY + 2 * BHALO, BPN = BPX * BPY, BNS = 8;
constexpr int BNIT = (BPN + kBdBlock - 1) / kBdBlock;
#ifndef IRS_SWZ_BENDING_ROWS
#define IRS_SWZ_BENDING_ROWS 4
#endif

__device__ __forceinline__ float ldg_off(const float* __restrict__ base, unsigned byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}

// weights of one axis at position `pos` of `n`:
//   lm, lp   the two first differences touching pos, (pos - 1, pos) and (pos, pos + 1): w(q), 0 where the difference does not exist
//   pa, pb, pc   the three second differences touching pos, based at pos - 2, pos - 1, pos: 1 where the base k has 0 <= k <= n - 3
struct BendAxis {
    float lm, lp, pa, pb, pc;
};
__device__ __forceinline__ BendAxis bend_axis(int pos, int n) {
    BendAxis w;
    w.lm = pos >= 1 ? (pos - 1 == n - 2 ? 2.0f : 1.0f) : 0.0f;
    w.lp = pos <= n - 2 ? (pos == n - 2 ? 2.0f : 1.0f) : 0.0f;
    w.pa = pos >= 2 ? 1.0f : 0.0f;
    w.pb = pos >= 1 && pos <= n - 2 ? 1.0f : 0.0f;
    w.pc = pos <= n - 3 ? 1.0f : 0.0f;
    return w;
}

// P_a f at the centre from the five values along the axis; e: + the pure energy term based at the centre.
// Roundings (products with the weights 0 / 1 / 2 are exact): 2 per second difference, 2 to combine = 8
template <bool ENERGY>
__device__ __forceinline__ float bend_pure(float m2, float m1, float c, float p1, float p2, const BendAxis& w, float& e) {
    const float sa = (c - 2.0f * m1) + m2, sb = (p1 - 2.0f * c) + m1, sc = (p2 - 2.0f * p1) + c;
    if (ENERGY) e += w.pc * sc * sc;
    return (w.pa * sa + w.pc * sc) - 2.0f * (w.pb * sb);
}

// L_a of one line (m, c, p) along axis a.  Roundings: 3
__device__ __forceinline__ float bend_l(float m, float c, float p, const BendAxis& w) { return w.lm * (c - m) - w.lp * (p - c); }

// L_b L_a f at the centre of a 3 x 3 neighbourhood q[b][a]; e: + the mixed energy term based at the centre.
// Roundings: 3 lines of 3, 3 across = 12
template <bool ENERGY>
__device__ __forceinline__ float bend_mixed(const float (&q)[3][3], const BendAxis& wa, const BendAxis& wb, float& e) {
    if (ENERGY) {
        const float d = (q[2][2] - q[2][1]) - (q[1][2] - q[1][1]);
        e += 2.0f * (wa.lp * wb.lp) * d * d;
    }
    return bend_l(bend_l(q[0][0], q[0][1], q[0][2], wa), bend_l(q[1][0], q[1][1], q[1][2], wa), bend_l(q[2][0], q[2][1], q[2][2], wa), wb);
}

// The stencil at one voxel: m2 .. p2 are the LDS planes z - 2 .. z + 2, ci the voxel's index in a plane.
// Returns H^T W H f (GRAD); e receives the energy terms based at the voxel (ENERGY).
// Roundings that feed the returned value: 3 x 8 (pure) + 3 x 12 (mixed) + 2 + 2 (the two sums of three) + 1 (pure + 2 mixed) = 65
template <bool GRAD, bool ENERGY>
__device__ __forceinline__ float bending_point(const float* __restrict__ m2, const float* __restrict__ m1, const float* __restrict__ c0,
                                               const float* __restrict__ p1, const float* __restrict__ p2, int ci, const BendAxis& wx,
                                               const BendAxis& wy, const BendAxis& wz, float& e) {
    float q[3][3];
    // x y plane
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) q[j][i] = c0[ci + (j - 1) * BPX + (i - 1)];
    const float f = q[1][1];
    const float px = bend_pure<ENERGY>(c0[ci - 2], q[1][0], f, q[1][2], c0[ci + 2], wx, e);
    const float py = bend_pure<ENERGY>(c0[ci - 2 * BPX], q[0][1], f, q[2][1], c0[ci + 2 * BPX], wy, e);
    const float zm = m1[ci], zp = p1[ci];
    const float pz = bend_pure<ENERGY>(m2[ci], zm, f, zp, p2[ci], wz, e);
    const float mxy = bend_mixed<ENERGY>(q, wx, wy, e);
    // x z plane: rows z - 1, z, z + 1 of (x - 1, x, x + 1)
    float r[3][3] = {{m1[ci - 1], zm, m1[ci + 1]}, {q[1][0], f, q[1][2]}, {p1[ci - 1], zp, p1[ci + 1]}};
    const float mxz = bend_mixed<ENERGY>(r, wx, wz, e);
    // y z plane: rows z - 1, z, z + 1 of (y - 1, y, y + 1)
    float s[3][3] = {{m1[ci - BPX], zm, m1[ci + BPX]}, {q[0][1], f, q[2][1]}, {p1[ci - BPX], zp, p1[ci + BPX]}};
    const float myz = bend_mixed<ENERGY>(s, wy, wz, e);
    if (!GRAD) return 0.0f;
    return ((px + py) + pz) + 2.0f * ((mxy + mxz) + myz);
}

template <int P>
struct Par {
    static constexpr int value = P;
};

// One tile, one segment [z0, z1) of one component f (D, H, W): stages the ring and calls, per plane,
//   prefetch(z, Par)      before the plane prefetch of that step -- the own-voxel streams of plane z, requested one plane ahead
//                         (stencil_kernels.hip, sgld_update_march_kernel: why the order matters); Par alternates between planes
//   emit(z, x, y, h, e, Par)   for the threads whose column lies in the volume
// F: BNS * BPN floats of LDS.  Leaves with a barrier behind the last read of the ring.
template <bool GRAD, bool ENERGY, class Pre, class Emit>
__device__ __forceinline__ void bending_march_tile(float* __restrict__ F, const float* __restrict__ f, const Vol& vol, int ox, int oy, int z0,
                                                   int z1, Pre&& prefetch, Emit&& emit) {
    const int64_t HW = (int64_t)vol.H * vol.W;
    const int lx = threadIdx.x % BTX, ly = threadIdx.x / BTX;
    const int x = ox + lx, y = oy + ly;
    const bool col_in = x < vol.W && y < vol.H;
    const BendAxis wx = bend_axis(x, vol.W), wy = bend_axis(y, vol.H);
    const int ci = (ly + BHALO) * BPX + lx + BHALO;
    unsigned off[BNIT];
#pragma unroll
    for (int it = 0; it < BNIT; ++it) {
        const int i = threadIdx.x + it * kBdBlock;
        const int ex = i % BPX, ey = i / BPX;
        off[it] = (unsigned)(min(max(oy - BHALO + ey, 0), vol.H - 1) * vol.W + min(max(ox - BHALO + ex, 0), vol.W - 1)) * 4u;
    }
    auto load_plane = [&](int p, float (&dst)[BNIT]) {
        const float* __restrict__ base = f + (int64_t)min(max(p, 0), vol.D - 1) * HW;
#pragma unroll
        for (int it = 0; it < BNIT; ++it)
            if (threadIdx.x + it * kBdBlock < BPN) dst[it] = ldg_off(base, off[it]);
    };
    auto commit = [&](int p, const float (&src)[BNIT]) {
        float* __restrict__ S = F + ((p + BNS) & (BNS - 1)) * BPN;  // p >= -2
#pragma unroll
        for (int it = 0; it < BNIT; ++it) {
            const int i = threadIdx.x + it * kBdBlock;
            if (i < BPN) S[i] = src[it];
        }
    };
    auto plane = [&](int p) -> const float* { return F + ((p + BNS) & (BNS - 1)) * BPN; };
    float pre[BNIT];
    {
        float run[4][BNIT];  // the run-in: four planes requested at once
#pragma unroll
        for (int k = 0; k < 4; ++k) load_plane(z0 - 2 + k, run[k]);
        prefetch(z0, Par<0>());
        load_plane(z0 + 2, pre);
#pragma unroll
        for (int k = 0; k < 4; ++k) commit(z0 - 2 + k, run[k]);
    }
    auto step = [&](int zc, auto par) {
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the commit needs the newest loads, and it tells the compiler that the own-voxel streams have arrived
        commit(zc + 2, pre);
        if (zc + 1 < z1) {
            prefetch(zc + 1, Par<1 - decltype(par)::value>());
            load_plane(zc + 3, pre);
        }
        __syncthreads();  // ring of 8: plane zc + 2 landed in the slot of plane zc - 6; the slowest wavefront still reads zc - 3
        if (col_in) {
            float e = 0.0f;
            const float h = bending_point<GRAD, ENERGY>(plane(zc - 2), plane(zc - 1), plane(zc), plane(zc + 1), plane(zc + 2), ci, wx, wy,
                                                        bend_axis(zc, vol.D), e);
            emit(zc, x, y, h, e, par);
        }
    };
    for (int zc = z0; zc < z1; zc += 2) {
        step(zc, Par<0>());
        if (zc + 1 < z1) step(zc + 1, Par<1>());
    }
    __syncthreads();
}

// blockIdx.x -> (component, x tile, y tile, segment) of a chain's `total` = 3 ntx nty nseg tiles; x-neighbouring tiles and
// IRS_SWZ_BENDING_ROWS rows of them on one XCD, as for the first-order update
struct BendTile {
    int comp, ox, oy, z0, z1;
};
__device__ __forceinline__ BendTile bend_tile(int id, int total, const Vol& vol, int seg_len, int nseg, int ntx, int nty) {
    const int t = xcd_swizzle_runs(id, total, ntx * IRS_SWZ_BENDING_ROWS);
    const int per = ntx * nty * nseg, comp = t / per, r = t - comp * per, seg = r / (ntx * nty);
    BendTile b;
    b.comp = comp;
    b.ox = (r % ntx) * BTX;
    b.oy = ((r / ntx) % nty) * BTY;
    b.z0 = vol.z0 + seg * seg_len;
    b.z1 = min(b.z0 + seg_len, vol.z0 + vol.nz);
    return b;
}

struct NoPrefetch {
    template <class P>
    __device__ __forceinline__ void operator()(int, P) const {}
};

}  // namespace

// ------------------------------------------------------------------------------------------------
// y_c partials, [C][gridDim.x] in double: a capped grid walks the tiles in a fixed order, a thread adds its voxels' terms (float32,
// six non-negative squares each) to a double in marching order, block_sum adds the threads in a fixed tree.  No atomics.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBdBlock) void bending_energy_march_kernel(const float* __restrict__ v, double* __restrict__ partials, Vol vol,
                                                                        int seg_len, int nseg, int ntx, int nty) {
    __shared__ float F[BNS * BPN];
    __shared__ double smem[kBdBlock / kWave];
    double acc[1] = {0.0};
    const int total = 3 * ntx * nty * nseg;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
        const BendTile b = bend_tile(id, total, vol, seg_len, nseg, ntx, nty);
        const float* __restrict__ f = v + ((int64_t)blockIdx.y * 3 + b.comp) * vol.V;
        bending_march_tile<false, true>(F, f, vol, b.ox, b.oy, b.z0, b.z1, NoPrefetch(),
                                        [&](int, int, int, float, float e, auto) { acc[0] += (double)e; });
    }
    block_sum<1, kBdBlock / kWave>(acc, smem);
    if (threadIdx.x == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

// ------------------------------------------------------------------------------------------------
// out = scale_c * 2 H^T W H v (scale: C floats or nullptr = 1).  Stateless: the autograd backward and the tests.
// One more rounding than bending_point (the product with scale_c; the factor 2 is exact): 66 feed one output.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBdBlock) void bending_grad_march_kernel(const float* __restrict__ v, const float* __restrict__ scale,
                                                                      float* __restrict__ out, Vol vol, int seg_len, int nseg, int ntx,
                                                                      int nty) {
    __shared__ float F[BNS * BPN];
    const BendTile b = bend_tile((int)blockIdx.x, (int)gridDim.x, vol, seg_len, nseg, ntx, nty);
    const int64_t cb = ((int64_t)blockIdx.y * 3 + b.comp) * vol.V;
    const float sc2 = 2.0f * (scale ? scale[blockIdx.y] : 1.0f);
    float* __restrict__ o = out + cb;
    const int64_t HW = (int64_t)vol.H * vol.W;
    bending_march_tile<true, false>(F, v + cb, vol, b.ox, b.oy, b.z0, b.z1, NoPrefetch(), [&](int z, int x, int y, float h, float, auto) {
        o[(int64_t)z * HW + (unsigned)(y * vol.W + x)] = sc2 * h;
    });
}

// ------------------------------------------------------------------------------------------------
// SGLD / SGD update with the bending prior: the contract of sgld_update_march_kernel (stencil_kernels.hip), the stencil swapped
//   grad_v = sigma^2 (g * s_c + 2 coef H^T W H v_s),   v <- v - lr grad_v     (v stays when the transition is frozen)
// coef from state->coef[chain]: the energy and the scalar stage always run in front of this kernel.
// ------------------------------------------------------------------------------------------------
// HMC (compile-time, sghmc_device.h): 0 the update above; 1 / 2 the SGHMC step in its place, noise from Philox / from hm.eps, as in
// sgld_update_march_kernel.  A workgroup marches ONE component: of the six normals of a voxel pair a thread keeps the two of its
// component (the three components of a voxel make the same call -- thrice the generator's work of the first-order kernel, which
// this kernel's 125-point stencil hides).  With HMC = 0 nothing of `hm` is touched.
template <bool SIGMA, int HMC>
__device__ __forceinline__ void sgld_update_bending_march_body(float* __restrict__ v, const float* __restrict__ sigma,
                                                               const float* __restrict__ g, const float* __restrict__ v_s,
                                                               const DevState* __restrict__ state, float lr, float s0,
                                                               float s1, float s2, float* __restrict__ grad_out, Vol vol,
                                                               int seg_len, int nseg, int ntx, int nty, const SghmcArgs& hm) {
    __shared__ float F[BNS * BPN];
    const BendTile b = bend_tile((int)blockIdx.x, (int)gridDim.x, vol, seg_len, nseg, ntx, nty);
    const int chain = blockIdx.y;
    const int64_t cb = ((int64_t)chain * 3 + b.comp) * vol.V;
    const int64_t HW = (int64_t)vol.H * vol.W;
    const float coef2 = 2.0f * (float)state->coef[chain];
    const bool frozen = state->bad_now != 0u || comm_bad(state);
    const float sc = b.comp == 0 ? s0 : (b.comp == 1 ? s1 : s2);
    const int ox_ = b.ox + (int)(threadIdx.x % BTX), oy_ = b.oy + (int)(threadIdx.x / BTX);
    const bool col_in = ox_ < vol.W && oy_ < vol.H;
    const unsigned own = col_in ? (unsigned)(oy_ * vol.W + ox_) * 4u : 0u;
    struct OwnIn {
        float g, v, s;
        float m, e;  // SGHMC: momentum, injected noise
    };
    OwnIn qa = {}, qb = {};  // used alternately (no copies: a copy would have to wait for the loads it copies)
    auto load_own = [&](int z, OwnIn& q) {
        const int64_t base = cb + (int64_t)z * HW;
        q.g = ldg_off(g + base, own);
        q.v = ldg_off(v + base, own);
        if (SIGMA) q.s = ldg_off(sigma + base, own);
        if (HMC) q.m = ldg_off(hm.m + base, own);
        if (HMC == 2) q.e = ldg_off(hm.eps + base, own);
    };
    float n_even = 0.0f, n_odd = 0.0f;  // SGHMC, Philox: this component's normals of the pair the plane in hand belongs to
    const uint64_t iter = HMC == 1 ? state->st.iteration : 0ull;
    bending_march_tile<true, false>(
        F, v_s + cb, vol, b.ox, b.oy, b.z0, b.z1, [&](int z, auto par) { load_own(z, decltype(par)::value ? qb : qa); },
        [&](int z, int, int, float h, float, auto par) {
            const OwnIn& cur = decltype(par)::value ? qb : qa;
            const int64_t base = cb + (int64_t)z * HW;
            const float gr = cur.g * sc + coef2 * h;
            const float sg = SIGMA ? cur.s : 1.0f;
            const float gs = sg * sg * gr;  // SGLD.backward: sigma^2 * grad == v.grad in the reference
            if (grad_out) *reinterpret_cast<float*>(reinterpret_cast<char*>(grad_out + base) + own) = gs;
            if (HMC) {
                // (uniform branch; a segment that starts on an odd plane draws its pair too)
                if (HMC == 1 && hm.noisy && ((z & 1) == 0 || z == b.z0)) {
                    float n[2][3];
                    sghmc_pair_draw(chain, vol.Vg, (int64_t)(z & ~1) * HW + (own >> 2), iter, hm.seed, n);
                    n_even = b.comp == 0 ? n[0][0] : (b.comp == 1 ? n[0][1] : n[0][2]);
                    n_odd = b.comp == 0 ? n[1][0] : (b.comp == 1 ? n[1][1] : n[1][2]);
                }
                float v1, m1;
                sghmc_step(cur.v, cur.m, gs, sg, HMC == 2 ? cur.e : ((z & 1) ? n_odd : n_even), lr, hm.oma, hm.amp, hm.noisy != 0, v1, m1);
                if (!frozen) {
                    *reinterpret_cast<float*>(reinterpret_cast<char*>(v + base) + own) = v1;
                    *reinterpret_cast<float*>(reinterpret_cast<char*>(hm.m + base) + own) = m1;
                }
            } else if (!frozen) *reinterpret_cast<float*>(reinterpret_cast<char*>(v + base) + own) = cur.v - lr * gs;
        });
}

template <bool SIGMA>
__global__ __launch_bounds__(kBdBlock) void sgld_update_bending_march_kernel(float* __restrict__ v, const float* __restrict__ sigma,
                                                                             const float* __restrict__ g, const float* __restrict__ v_s,
                                                                             const DevState* __restrict__ state, float lr, float s0,
                                                                             float s1, float s2, float* __restrict__ grad_out, Vol vol,
                                                                             int seg_len, int nseg, int ntx, int nty) {
    sgld_update_bending_march_body<SIGMA, 0>(v, sigma, g, v_s, state, lr, s0, s1, s2, grad_out, vol, seg_len, nseg, ntx, nty, SghmcArgs{});
}

template <bool SIGMA, int HMC>
__global__ __launch_bounds__(kBdBlock) void sghmc_update_bending_march_kernel(float* __restrict__ v, const float* __restrict__ sigma,
                                                                              const float* __restrict__ g, const float* __restrict__ v_s,
                                                                              const DevState* __restrict__ state, float lr, float s0,
                                                                              float s1, float s2, float* __restrict__ grad_out, Vol vol,
                                                                              int seg_len, int nseg, int ntx, int nty, SghmcArgs hm) {
    sgld_update_bending_march_body<SIGMA, HMC>(v, sigma, g, v_s, state, lr, s0, s1, s2, grad_out, vol, seg_len, nseg, ntx, nty, hm);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static int bend_ntx(Vol vol) { return (vol.W + BTX - 1) / BTX; }
static int bend_nty(Vol vol) { return (vol.H + BTY - 1) / BTY; }

// segment length of the gradient and of the update: the `update_seg` knob, else by launch size (run-in 4 planes)
static int bending_seg_len(Vol vol, int C) {
    const int seg_env = global_knobs().update_seg;
    const int64_t per_layer = (int64_t)bend_ntx(vol) * bend_nty(vol) * 3 * C;
    int len = pick_seg_len(vol.nz, per_layer, 4, seg_env);
    if (global_knobs().seg_fit && seg_env <= 0) {
        static int cache = 0;
        const int64_t res = resident_blocks((const void*)sgld_update_bending_march_kernel<false>, kBdBlock, &cache);
        if (res > 0) len = pick_seg_len_fit(vol.nz, 0, per_layer, 4, 4, res, 0);
    }
    return len;
}

void launch_bending_energy(const float* v, double* partials, int blocks, int C, Vol vol, hipStream_t st) {
    const int ntx = bend_ntx(vol), nty = bend_nty(vol);
    const int seg_len = pick_seg_len(vol.nz, (int64_t)ntx * nty * 3, 8, 0);
    const int nseg = (vol.nz + seg_len - 1) / seg_len;
    hipLaunchKernelGGL(bending_energy_march_kernel, dim3(blocks, C), dim3(kBdBlock), 0, st, v, partials, vol, seg_len, nseg, ntx, nty);
}

void launch_bending_grad(const float* v, const float* scale, float* out, int C, Vol vol, hipStream_t st) {
    const int ntx = bend_ntx(vol), nty = bend_nty(vol);
    const int seg_len = bending_seg_len(vol, C);
    const int nseg = (vol.nz + seg_len - 1) / seg_len;
    hipLaunchKernelGGL(bending_grad_march_kernel, dim3((unsigned)(3 * ntx * nty * nseg), C), dim3(kBdBlock), 0, st, v, scale, out, vol,
                       seg_len, nseg, ntx, nty);
}

void launch_sgld_update_bending(float* v, const float* sigma, const float* g_d0, const float* v_s, const void* dev_state, float lr,
                                float s0, float s1, float s2, float* grad_out, int C, Vol vol, hipStream_t st, const SghmcArgs* hm) {
    const int ntx = bend_ntx(vol), nty = bend_nty(vol);
    const int seg_len = bending_seg_len(vol, C);
    const int nseg = (vol.nz + seg_len - 1) / seg_len;
    const dim3 grid((unsigned)(3 * ntx * nty * nseg), C);
    if (global_knobs().launch_log) {
        static int cache_l = 0;
        log_launch("sgld_update_bending_march_kernel", BTX, BTY, (int64_t)grid.x * C, kBdBlock, seg_len, 4, vol.nz, C,
                   resident_blocks((const void*)sgld_update_bending_march_kernel<false>, kBdBlock, &cache_l));
    }
    if (hm) {  // SGHMC; injected noise only counts where noise is added at all
#define IRS_SGHMC_LAUNCH(SG, MODE)                                                                                                     \
    hipLaunchKernelGGL((sghmc_update_bending_march_kernel<SG, MODE>), grid, dim3(kBdBlock), 0, st, v, sigma, g_d0, v_s,                       \
                       (const DevState*)dev_state, lr, s0, s1, s2, grad_out, vol, seg_len, nseg, ntx, nty, *hm)
        const bool inj = hm->eps && hm->noisy;
        if (sigma && inj) IRS_SGHMC_LAUNCH(true, 2);
        else if (sigma) IRS_SGHMC_LAUNCH(true, 1);
        else if (inj) IRS_SGHMC_LAUNCH(false, 2);
        else IRS_SGHMC_LAUNCH(false, 1);
#undef IRS_SGHMC_LAUNCH
    } else if (sigma)
        hipLaunchKernelGGL(sgld_update_bending_march_kernel<true>, grid, dim3(kBdBlock), 0, st, v, sigma, g_d0, v_s,
                           (const DevState*)dev_state, lr, s0, s1, s2, grad_out, vol, seg_len, nseg, ntx, nty);
    else
        hipLaunchKernelGGL(sgld_update_bending_march_kernel<false>, grid, dim3(kBdBlock), 0, st, v, sigma, g_d0, v_s,
                           (const DevState*)dev_state, lr, s0, s1, s2, grad_out, vol, seg_len, nseg, ntx, nty);
}

}  // namespace irs
