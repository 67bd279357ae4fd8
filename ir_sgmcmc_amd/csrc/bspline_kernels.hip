// Cubic B-spline resampling of the images the package writes (absent in the reference, whose outputs are all trilinear;
// DESIGN.md section 6, "Cubic B-spline output resampling"; include/irsgmcmc.h has the definition in full): the recursive
// prefilter that turns samples into interpolation coefficients, and two gathers that evaluate the spline -- at a transformation
// on the registration grid and at the source positions of the native-resolution warp.
//
// Prefilter (irs_bspline_prefilter): three launches, x (the last axis), then y, then z, whole-sample mirror boundaries, pole
// z1 = sqrt(3) - 2, gain 6.  Per line of length n, in double with every operation rounded once:
//   c+[0]   = sum_{k < min(2n-2, 32)} z1^k (6 s[mir(k)])  (/ (1 - z1^(2n-2)) when 2n - 2 <= 32), the powers by zk *= z1 from 1;
//   c+[k]   = 6 s[k] + z1 c+[k-1];      c[n-1] = (z1 / (z1^2 - 1)) (c+[n-1] + z1 c+[n-2]);      c[k] = z1 (c[k+1] - c+[k]).
// The running values c+[k-1] and c[k+1] stay in double registers.  c+ is written to `coeff` as float32 and the anticausal
// sweep reads it back from there (coeff may be the input, and there is no workspace: float32 is the only place a line can
// rest between its two sweeps); c is rounded to float32 once when it is stored.
//   y and z: one thread per line, adjacent lanes on adjacent x, so every step of the recursion is one coalesced row access.
//   x: a line is contiguous, so one thread per line would put the lanes W floats apart.  A wavefront owns 64 lines and moves
//      them through the LDS in 64 x 64 tiles: rows are loaded with row-contiguous reads (lane = column) and stored at a pitch of
//      65 dwords, then lane l walks row l across the tile (bank (65 l + j) mod 32 = (l + j) mod 32: conflict-free in both 32-lane
//      groups) with its carry in registers, and the tile goes back out row by row.  Tiles run forward for the causal sweep and
//      backward for the anticausal one; the last tile stays in the LDS between the two; the next tile is on its way into
//      registers while the current one is walked.  Ragged tiles are masked.
//
// Evaluation at q (index coordinates, clamped to [0, n - 1] per axis), float32, every operation rounded once:
//   i0 = min(floor(q), n - 2), t = q - i0, u = 1 - t, taps i0 - 1 .. i0 + 2 mirrored once (k < 0 -> -k, k > n - 1 -> 2 (n - 1) - k);
//   w0 = u*u*u/6, w1 = (3*t*t*t - 6*t*t + 4)/6, w2 = (3*u*u*u - 6*u*u + 4)/6, w3 = t*t*t/6, each left to right as written;
//   row sums over x: acc = acc + w c from 0, taps ascending; then the four row sums over y the same way; then over z.
#include "native_device.h"

namespace irs {
namespace {

constexpr int kTile = 64;           // lines per wavefront and columns per tile of the x pass
constexpr int kPitch = kTile + 1;   // dwords between the rows of a tile in the LDS
constexpr int kSeries = 32;         // terms of the initialisation series of a long line

struct Pole {
    double z1;    // sqrt(3) - 2
    double anti;  // z1 / (z1^2 - 1)
};

// mirrored index of term k of the initialisation series (0 <= k < 2n - 2)
__device__ __forceinline__ int mirror_term(int k, int n) { return k <= n - 1 ? k : 2 * (n - 1) - k; }

// c+[0] from the series terms 6 s[mir(k)], read through `sample`
template <class F>
__device__ __forceinline__ double causal_start(int n, double z1, F sample) {
    const int T = 2 * n - 2, terms = min(T, kSeries);
    double zk = 1.0, sum = 0.0;
    for (int k = 0; k < terms; ++k) {
        sum = __dadd_rn(sum, __dmul_rn(zk, __dmul_rn(6.0, (double)sample(mirror_term(k, n)))));
        zk = __dmul_rn(zk, z1);
    }
    return T <= kSeries ? __ddiv_rn(sum, __dsub_rn(1.0, zk)) : sum;
}

// The two sweeps over the elements [lo, hi) of a line, `load(k)` / `store(k, value)` reaching element k.  They move in batches of
// kBatch elements -- all loads of a batch, then its recursion steps, then its stores -- so that a thread has kBatch independent
// loads in flight instead of one per step of a dependent chain (a batch's loads may read elements outside [lo, hi), clamped
// into it, that no step uses).
constexpr int kBatch = 16;

// causal: cp enters as c+[lo - 1] and leaves as c+[hi - 1]; last / before: the two newest c+ as stored
template <class Load, class Store>
__device__ __forceinline__ void causal_sweep(int lo, int hi, double z1, double& cp, float& last, float& before, Load load,
                                             Store store) {
    for (int k0 = lo; k0 < hi; k0 += kBatch) {
        float v[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; ++i) v[i] = load(min(k0 + i, hi - 1));
#pragma unroll
        for (int i = 0; i < kBatch; ++i)
            if (k0 + i < hi) {
                cp = __dadd_rn(__dmul_rn(6.0, (double)v[i]), __dmul_rn(z1, cp));
                before = last;
                last = v[i] = (float)cp;
            }
#pragma unroll
        for (int i = 0; i < kBatch; ++i)
            if (k0 + i < hi) store(k0 + i, v[i]);
    }
}

// anticausal, k = hi - 1 down to lo: cc enters as c[hi] and leaves as c[lo]; load(k) gives the stored c+[k]
template <class Load, class Store>
__device__ __forceinline__ void anticausal_sweep(int lo, int hi, double z1, double& cc, Load load, Store store) {
    for (int k0 = hi - 1; k0 >= lo; k0 -= kBatch) {
        float v[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; ++i) v[i] = load(max(k0 - i, lo));
#pragma unroll
        for (int i = 0; i < kBatch; ++i)
            if (k0 - i >= lo) {
                cc = __dmul_rn(z1, __dsub_rn(cc, (double)v[i]));
                v[i] = (float)cc;
            }
#pragma unroll
        for (int i = 0; i < kBatch; ++i)
            if (k0 - i >= lo) store(k0 - i, v[i]);
    }
}

__device__ __forceinline__ double anticausal_start(const Pole& pole, float last, float before) {
    return __dmul_rn(pole.anti, __dadd_rn((double)last, __dmul_rn(pole.z1, (double)before)));
}

// ---- y and z: lines of n elements `stride` apart; `stride` consecutive lines start at consecutive addresses, blockIdx.y picks
// the group of them (a plane of the y pass, a volume of the z pass).  `in` may be `out`.
__global__ __launch_bounds__(kBlock) void bspline_strided_kernel(const float* in, float* out, int n, int stride, Pole pole) {
    const int inner = blockIdx.x * kBlock + threadIdx.x;
    if (inner >= stride) return;
    const int64_t base = (int64_t)blockIdx.y * n * stride + inner;
    const float* s = in + base;
    float* c = out + base;
    const int64_t st = stride;
    auto read = [&](int k) { return s[k * st]; };
    auto back = [&](int k) { return c[k * st]; };
    auto write = [&](int k, float v) { c[k * st] = v; };
    double cp = causal_start(n, pole.z1, read);
    float last = (float)cp, before = 0.0f;
    write(0, last);
    causal_sweep(1, n, pole.z1, cp, last, before, read, write);
    double cc = anticausal_start(pole, last, before);
    write(n - 1, (float)cc);
    anticausal_sweep(0, n - 1, pole.z1, cc, back, write);
}

// ---- x: one wavefront per block, 64 lines (rows of W contiguous floats) through 64-column tiles in the LDS
__global__ __launch_bounds__(kTile) void bspline_x_kernel(const float* in, float* out, int64_t rows, int W, Pole pole) {
    __shared__ float tile[kTile * kPitch];
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kTile;
    const int nrows = (int)min((int64_t)kTile, rows - row0);
    const int ntiles = (W + kTile - 1) / kTile;
    const bool line = lane < nrows;  // this lane walks a line
    float* mine = tile + lane * kPitch;
    auto read = [&](int j) { return mine[j]; };
    auto write = [&](int j, float v) { mine[j] = v; };

    // tile t of `src` -> registers -> the LDS, lane = column: every row access is 256 contiguous bytes.  The two halves are apart
    // so that the loads of the next tile are in flight while this one is walked; rows and columns past the end repeat the last
    // valid ones (in bounds, never used)
    float pre[kTile];
    auto fetch = [&](const float* src, int t) {
        const int64_t x = min(t * kTile + lane, W - 1);
#pragma unroll
        for (int i = 0; i < kTile; ++i) pre[i] = src[(row0 + min(i, nrows - 1)) * W + x];
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < kTile; ++i) tile[i * kPitch + lane] = pre[i];
    };
    auto store = [&](int t) {
        const int x = t * kTile + lane;
        if (x < W) {
#pragma unroll 16
            for (int i = 0; i < nrows; ++i) out[(row0 + i) * W + x] = tile[i * kPitch + lane];
        }
    };

    double cp = 0.0;
    float last = 0.0f, before = 0.0f;
    fetch(in, 0);
    for (int t = 0; t < ntiles; ++t) {
        commit();
        __syncthreads();
        if (t + 1 < ntiles) fetch(in, t + 1);  // other columns than the tile stored below: safe in place
        if (line) {
            const int cols = min(kTile, W - t * kTile);
            if (t == 0) {  // the series reads at most the first 32 samples: all in this tile
                cp = causal_start(W, pole.z1, read);
                last = (float)cp;
                write(0, last);
            }
            causal_sweep(t == 0 ? 1 : 0, cols, pole.z1, cp, last, before, read, write);
        }
        __syncthreads();
        if (t < ntiles - 1) {  // the last tile stays for the anticausal sweep
            store(t);
            __syncthreads();
        }
    }
    double cc = 0.0;
    if (ntiles > 1) fetch(out, ntiles - 2);
    for (int t = ntiles - 1; t >= 0; --t) {
        if (t < ntiles - 1) {
            commit();
            __syncthreads();
            if (t > 0) fetch(out, t - 1);
        }
        if (line) {
            int cols = min(kTile, W - t * kTile);
            if (t == ntiles - 1) {
                cc = anticausal_start(pole, last, before);
                write(--cols, (float)cc);
            }
            anticausal_sweep(0, cols, pole.z1, cc, read, write);
        }
        __syncthreads();
        store(t);
        __syncthreads();
    }
}

// ---- evaluation
struct SplineAxis {
    int k[4];    // the taps, mirrored into [0, n - 1]
    float w[4];
};
// (3*t*t*t - 6*t*t + 4)/6, left to right
__device__ __forceinline__ float spline_mid(float t) {
    const float cube = __fmul_rn(__fmul_rn(__fmul_rn(3.0f, t), t), t), square = __fmul_rn(__fmul_rn(6.0f, t), t);
    return __fdiv_rn(__fadd_rn(__fsub_rn(cube, square), 4.0f), 6.0f);
}
__device__ __forceinline__ SplineAxis spline_axis(float q, int n) {
    SplineAxis a;
    q = fminf(fmaxf(q, 0.0f), (float)(n - 1));  // the border rule of every warp; a NaN position reads the first sample
    const int i0 = min((int)floorf(q), n - 2);
    const float t = __fsub_rn(q, (float)i0), u = __fsub_rn(1.0f, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = i0 - 1 + j;
        a.k[j] = k < 0 ? -k : (k > n - 1 ? 2 * (n - 1) - k : k);
    }
    const float t2 = __fmul_rn(t, t), u2 = __fmul_rn(u, u);
    a.w[0] = __fdiv_rn(__fmul_rn(u2, u), 6.0f);
    a.w[1] = spline_mid(t);
    a.w[2] = spline_mid(u);
    a.w[3] = __fdiv_rn(__fmul_rn(t2, t), 6.0f);
    return a;
}

// the spline of the coefficient volume c (D,H,W) at q = (q_z, q_y, q_x)
__device__ __forceinline__ float spline_value(const float* __restrict__ c, const float (&q)[3], int D, int H, int W) {
    const SplineAxis az = spline_axis(q[0], D), ay = spline_axis(q[1], H), ax = spline_axis(q[2], W);
    float vz = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        float vy = 0.0f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float* row = c + ((int64_t)az.k[a] * H + ay.k[b]) * W;
            float vx = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) vx = __fadd_rn(vx, __fmul_rn(ax.w[j], row[ax.k[j]]));
            vy = __fadd_rn(vy, __fmul_rn(ay.w[b], vx));
        }
        vz = __fadd_rn(vz, __fmul_rn(az.w[a], vy));
    }
    return vz;
}

__global__ __launch_bounds__(kBlock) void bspline_warp_kernel(const float* __restrict__ coeff, int64_t coeff_stride,
                                                              const float* __restrict__ tr, float* __restrict__ out, Vol vol) {
    IRS_VOXEL(vol, chain, x, y, z, vox);
    const int n[3] = {vol.D, vol.H, vol.W};
    float q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {  // component 2 - a of the transformation belongs to axis a
        const float g = tr[((int64_t)chain * 3 + (2 - a)) * vol.V + vox];
        q[a] = __fmul_rn(__fmul_rn(__fadd_rn(g, 1.0f), 0.5f), (float)(n[a] - 1));
    }
    out[(int64_t)chain * vol.V + vox] = spline_value(coeff + chain * coeff_stride, q, vol.D, vol.H, vol.W);
}

__global__ __launch_bounds__(kBlock) void native_warp_cubic_kernel(const float* __restrict__ u, const float* __restrict__ im,
                                                                   const float* __restrict__ coeff, int64_t moving_stride,
                                                                   float* __restrict__ im_out, NativeGeom gm, Vol vol) {
    IRS_VOXEL(vol, chain, x, y, z, vox);
    const int idx[3] = {z, y, x};
    float uc[3], r[3];
    native_displacement(u, chain, idx, gm, uc);  // steps 1 to 3 of native_warp_kernel
    native_source(uc, idx, gm, r);
    const NativeTaps nt = native_taps(r, gm);
    const int64_t mov = (int64_t)chain * moving_stride;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) inside = inside && nt.in[a][0] && nt.in[a][1];
    float value;
    if (inside) {  // all eight trilinear taps in the native box: the spline of the unpadded volume at r - p
        const float q[3] = {__fsub_rn(r[0], (float)gm.p[0]), __fsub_rn(r[1], (float)gm.p[1]), __fsub_rn(r[2], (float)gm.p[2])};
        value = spline_value(coeff + mov, q, gm.n[0], gm.n[1], gm.n[2]);
    } else {  // the pad or the edge ramp: what irs_native_warp writes
        value = native_trilinear(im + mov, nt, gm.fill);
    }
    im_out[(int64_t)chain * vol.V + vox] = value;
}

}  // namespace

void launch_bspline_prefilter(const float* im, float* coeff, int volumes, const Vol& vol, hipStream_t st) {
    const double z1 = sqrt(3.0) - 2.0;
    const double z1z1 = z1 * z1;
    const double denom = z1z1 - 1.0;
    const Pole pole{z1, z1 / denom};
    const int64_t rows = (int64_t)volumes * vol.D * vol.H;
    hipLaunchKernelGGL(bspline_x_kernel, dim3((unsigned)((rows + kTile - 1) / kTile)), dim3(kTile), 0, st, im, coeff, rows, vol.W,
                       pole);
    hipLaunchKernelGGL(bspline_strided_kernel, dim3((unsigned)((vol.W + kBlock - 1) / kBlock), (unsigned)(volumes * vol.D)),
                       dim3(kBlock), 0, st, coeff, coeff, vol.H, vol.W, pole);
    const int plane = vol.H * vol.W;
    hipLaunchKernelGGL(bspline_strided_kernel, dim3((unsigned)((plane + kBlock - 1) / kBlock), (unsigned)volumes), dim3(kBlock), 0,
                       st, coeff, coeff, vol.D, plane, pole);
}

void launch_bspline_warp(const float* coeff, int64_t coeff_stride, const float* transformation, float* out, int C, const Vol& vol,
                         hipStream_t st) {
    hipLaunchKernelGGL(bspline_warp_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, coeff, coeff_stride, transformation, out, vol);
}

void launch_native_warp_cubic(const float* u, const float* im, const float* coeff, int64_t moving_stride, float* im_out,
                              const NativeGeom& gm, int C, hipStream_t st) {
    const Vol vol = make_vol(gm.n[0], gm.n[1], gm.n[2]);
    hipLaunchKernelGGL(native_warp_cubic_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, u, im, coeff, moving_stride, im_out, gm, vol);
}

}  // namespace irs
