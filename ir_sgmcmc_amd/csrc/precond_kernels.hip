// Adaptive pSGLD preconditioner (absent in the reference, whose sigma field is the VI posterior's standard deviation; DESIGN.md
// section 6, "Adaptive preconditioner"): the running second moment of the gradient, and the sigma field formed from it.
//
// The arithmetic, stated once (include/irsgmcmc.h repeats it for callers; tests/_preconditioner.py restates it in numpy).  Every
// float32 step is ONE IEEE operation, rounded to nearest: add, multiply, divide, square root.  NO FMA is meant anywhere: the build
// contracts a * b + c written as one expression, so every product that feeds a sum goes through __fmul_rn / __fadd_rn, which are
// never contracted; `/` and sqrtf are the correctly rounded ones (the compiler's default for HIP).  No expf / logf.
//   accumulate, per element:  g_c = grad_v_c / (sigma_c * sigma_c)           (grad_v_c itself without a sigma field)
//                             q = g_0 * g_0;  q = q + g_c * g_c, c = 1 .. C - 1;  m = q / (float)C
//                             V = (beta * V) + ((1 - beta) * m),  1 - beta one float32 subtraction on the host
//   sigma:  vhat = V * bias;  r > 0: vhat = (float)((double sum of the (2r+1)^3 window, dz, dy, dx ascending) / (2r+1)^3)
//           s = sqrtf(vhat);  sbar = (double sum of s) / N;  lambda = (float)(damping * sbar)
//           G = 1 / (lambda + s)  (1 where sbar == 0);  Gbar = (double sum of G) / N
//           raw = sqrtf(G / (float)Gbar);  sigma = min(max(raw, sigma_min), sigma_max)
// The double sums have a fixed order: every thread sums its elements i, i + stride, ... in order, the lanes of a wavefront merge by
// the shuffle butterfly, the wavefronts of a block and then the blocks in index order (thread j of the one-block second stage
// takes blocks j, j + 256, ...).  The grids depend on N alone, so two identical call sequences are bit-identical.
//
// accumulate is pure streaming -- 12 C bytes of gradient (and as many of sigma) plus 12 of V read and 12 written per velocity
// voxel: float4 accesses, one unit per thread, nothing staged.  The box mean stages a 32 x 8 x 4 tile and its halo in LDS.
#include "kernels.h"
#include "summary_device.h"

namespace irs {
namespace {

constexpr int kPartialRows = 1024;  // rows of per-block partials in the workspace: caps the reduction grids

// ---- accumulate
__device__ __forceinline__ float precond_g(float gv, float sg, bool has_sigma, int& bad) {
    const float g = has_sigma ? gv / __fmul_rn(sg, sg) : gv;
    bad += !isfinite(g);
    return g;
}
__device__ __forceinline__ float precond_blend(float V, float q, float fC, float beta, float omb) {
    return __fadd_rn(__fmul_rn(beta, V), __fmul_rn(omb, q / fC));
}

// one block's non-finite count -> the device counter (integer atomics commute: deterministic)
__device__ __forceinline__ void precond_count(int bad, long long* nonfinite) {
    __shared__ int s_bad[kBlock / kWave];
    bad = (int)wave_sum_ll(bad);
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    if (lane == 0) s_bad[wid] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < kBlock / kWave; ++w) n += s_bad[w];
        if (n) atomicAdd((unsigned long long*)nonfinite, (unsigned long long)n);
    }
}

// units of four elements, then (C == 1 only: else N % 4 == 0) the tail of N % 4 elements, one per thread of the last block
template <bool kSigma>
__global__ __launch_bounds__(kBlock) void precond_accumulate_vec_kernel(const float* __restrict__ grad_v, const float* __restrict__ sigma,
                                                                        int C, int64_t N, float beta, float omb, float* __restrict__ V,
                                                                        long long* __restrict__ nonfinite) {
    const int64_t units = N >> 2, u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const float fC = (float)C;
    int bad = 0;
    if (u < units) {
        float q[4];
        for (int c = 0; c < C; ++c) {
            const float4 gv = ((const float4*)(grad_v + c * N))[u];
            float4 sg = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            if (kSigma) sg = ((const float4*)(sigma + c * N))[u];
            const float g[4] = {precond_g(gv.x, sg.x, kSigma, bad), precond_g(gv.y, sg.y, kSigma, bad),
                                precond_g(gv.z, sg.z, kSigma, bad), precond_g(gv.w, sg.w, kSigma, bad)};
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = c == 0 ? __fmul_rn(g[j], g[j]) : __fadd_rn(q[j], __fmul_rn(g[j], g[j]));
        }
        float4 v = ((float4*)V)[u];
        v.x = precond_blend(v.x, q[0], fC, beta, omb);
        v.y = precond_blend(v.y, q[1], fC, beta, omb);
        v.z = precond_blend(v.z, q[2], fC, beta, omb);
        v.w = precond_blend(v.w, q[3], fC, beta, omb);
        ((float4*)V)[u] = v;
    }
    const int64_t t = (units << 2) + threadIdx.x;
    if (blockIdx.x == gridDim.x - 1 && t < N) {  // C == 1 here
        const float g = precond_g(grad_v[t], kSigma ? sigma[t] : 1.0f, kSigma, bad);
        V[t] = precond_blend(V[t], __fmul_rn(g, g), fC, beta, omb);
    }
    precond_count(bad, nonfinite);
}

template <bool kSigma>
__global__ __launch_bounds__(kBlock) void precond_accumulate_kernel(const float* __restrict__ grad_v, const float* __restrict__ sigma, int C,
                                                                    int64_t N, float beta, float omb, float* __restrict__ V,
                                                                    long long* __restrict__ nonfinite) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int bad = 0;
    if (i < N) {
        float q = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float g = precond_g(grad_v[c * N + i], kSigma ? sigma[c * N + i] : 1.0f, kSigma, bad);
            q = c == 0 ? __fmul_rn(g, g) : __fadd_rn(q, __fmul_rn(g, g));
        }
        V[i] = precond_blend(V[i], q, (float)C, beta, omb);
    }
    precond_count(bad, nonfinite);
}

// ---- the box mean of vhat = V * bias: a 32 x 8 x 4 tile of outputs per block, tile + halo (clamped: replicate padding) in LDS
constexpr int kBoxX = 32, kBoxY = 8, kBoxZ = 4;

template <int R>
__global__ __launch_bounds__(kBlock) void precond_box_kernel(const float* __restrict__ V, float bias, float* __restrict__ out, Vol vol) {
    constexpr int SX = kBoxX + 2 * R, SY = kBoxY + 2 * R, SZ = kBoxZ + 2 * R;
    __shared__ float tile[SZ * SY * SX];
    const int tz = (vol.D + kBoxZ - 1) / kBoxZ;
    const int ch = blockIdx.z / tz;
    const int x0 = blockIdx.x * kBoxX, y0 = blockIdx.y * kBoxY, z0 = (blockIdx.z - ch * tz) * kBoxZ;
    const float* src = V + (int64_t)ch * vol.V;
    for (int i = threadIdx.x; i < SZ * SY * SX; i += kBlock) {
        const int sx = i % SX, sy = (i / SX) % SY, sz = i / (SX * SY);
        const int x = min(max(x0 + sx - R, 0), vol.W - 1), y = min(max(y0 + sy - R, 0), vol.H - 1);
        const int z = min(max(z0 + sz - R, 0), vol.D - 1);
        tile[i] = __fmul_rn(src[((int64_t)z * vol.H + y) * vol.W + x], bias);
    }
    __syncthreads();
    const int lx = threadIdx.x & (kBoxX - 1), ly = threadIdx.x / kBoxX;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= vol.W || y >= vol.H) return;
    constexpr double kCount = (double)((2 * R + 1) * (2 * R + 1) * (2 * R + 1));
    for (int lz = 0; lz < kBoxZ && z0 + lz < vol.D; ++lz) {
        double acc = 0.0;
        for (int dz = 0; dz <= 2 * R; ++dz)
            for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
                for (int dx = 0; dx <= 2 * R; ++dx) acc = __dadd_rn(acc, (double)tile[((lz + dz) * SY + ly + dy) * SX + lx + dx]);
        out[(int64_t)ch * vol.V + ((int64_t)(z0 + lz) * vol.H + y) * vol.W + x] = (float)(acc / kCount);
    }
}

// ---- the two means and the field
// scal (doubles in the workspace): [0] sbar, [1] Gbar
struct PrecondArgs {
    const float* src;  // V (raw: vhat = src * bias) or the smoothed vhat
    bool raw;
    float bias;
    double damping;
    int64_t N;
};
__device__ __forceinline__ float precond_s(const PrecondArgs& a, int64_t i) {
    return sqrtf(a.raw ? __fmul_rn(a.src[i], a.bias) : a.src[i]);
}
__device__ __forceinline__ float precond_G(float s, double sbar, double damping) {
    const float lambda = (float)__dmul_rn(damping, sbar);
    return sbar == 0.0 ? 1.0f : 1.0f / __fadd_rn(lambda, s);
}

// kPass 0: partial sums of s; 1: of G (reads scal[0])
template <int kPass>
__global__ __launch_bounds__(kBlock) void precond_mean_kernel(PrecondArgs a, const double* __restrict__ scal, double* __restrict__ partials) {
    __shared__ double smem[kBlock / kWave];
    const double sbar = kPass ? scal[0] : 0.0;
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.N; i += (int64_t)gridDim.x * kBlock) {
        const float s = precond_s(a, i);
        acc[0] += (double)(kPass ? precond_G(s, sbar, a.damping) : s);
    }
    block_sum<1>(acc, smem);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}
__global__ __launch_bounds__(kBlock) void precond_mean_finish_kernel(const double* __restrict__ partials, int nblocks, int64_t N,
                                                                     double* __restrict__ out) {
    __shared__ double smem[kBlock / kWave];
    double acc[1] = {0.0};
    for (int b = threadIdx.x; b < nblocks; b += kBlock) acc[0] += partials[b];
    block_sum<1>(acc, smem);
    if (threadIdx.x == 0) *out = acc[0] / (double)N;
}

// integer sums {raw < sigma_min, raw > sigma_max}; doubles {min sigma, max sigma, sum of sigma^2}
struct PrecondSummary {
    static constexpr int kInts = 2, kFloats = 3;
    static constexpr Col kind(int j) { return j == 0 ? Col::Min : j == 1 ? Col::Max : Col::Sum; }
};
using PrecondAcc = SummaryAcc<PrecondSummary>;

__global__ __launch_bounds__(kBlock) void precond_field_kernel(PrecondArgs a, const double* __restrict__ scal, float sigma_min,
                                                               float sigma_max, int C, float* __restrict__ sigma,
                                                               long long* __restrict__ ipart, double* __restrict__ fpart) {
    __shared__ PrecondAcc smem[PrecondAcc::kG];
    PrecondAcc acc = PrecondAcc::identity();
    const double sbar = scal[0];
    const float gbar = (float)scal[1];
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.N; i += (int64_t)gridDim.x * kBlock) {
        const float raw = sqrtf(precond_G(precond_s(a, i), sbar, a.damping) / gbar);
        const float sg = fminf(fmaxf(raw, sigma_min), sigma_max);
        acc.i[0] += raw < sigma_min;
        acc.i[1] += raw > sigma_max;
        acc.f[0] = fmin(acc.f[0], (double)sg);
        acc.f[1] = fmax(acc.f[1], (double)sg);
        acc.f[2] += __dmul_rn((double)sg, (double)sg);
        for (int c = 0; c < C; ++c) sigma[c * a.N + i] = sg;
    }
    acc.block_reduce(smem);
    if (threadIdx.x == 0) acc.store(ipart, fpart, blockIdx.x);
}
__global__ __launch_bounds__(kBlock) void precond_summary_kernel(const long long* __restrict__ ipart, const double* __restrict__ fpart,
                                                                 int nblocks, int64_t N, const double* __restrict__ scal,
                                                                 const long long* __restrict__ nonfinite, double* __restrict__ summary) {
    __shared__ PrecondAcc smem[PrecondAcc::kG];
    PrecondAcc acc = PrecondAcc::identity();
    for (int b = threadIdx.x; b < nblocks; b += kBlock) acc.merge(PrecondAcc::load(ipart, fpart, b));
    acc.block_reduce(smem);
    if (threadIdx.x == 0) {
        summary[0] = scal[0];
        summary[1] = scal[1];
        summary[2] = acc.f[0];
        summary[3] = acc.f[1];
        summary[4] = acc.f[2] / (double)N;
        summary[5] = (double)acc.i[0];
        summary[6] = (double)acc.i[1];
        summary[7] = nonfinite ? (double)*nonfinite : 0.0;
    }
}

int reduce_blocks(int64_t N) { return (int)std::min<int64_t>((N + kBlock - 1) / kBlock, kPartialRows); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the workspace: [scal: 2 doubles][partials: kPartialRows rows of 2 int64 + 3 doubles][r > 0: the smoothed vhat, 3 n floats]
constexpr size_t kScalBytes = 2 * sizeof(double);
constexpr size_t kPartialBytes = (size_t)kPartialRows * (PrecondSummary::kInts + PrecondSummary::kFloats) * 8;

}  // namespace

void launch_precond_accumulate(const float* grad_v, const float* sigma, int C, int64_t N, float beta, float* V, long long* nonfinite,
                               hipStream_t st) {
    const float omb = 1.0f - beta;
    const bool vec = aligned16(grad_v) && aligned16(V) && (!sigma || aligned16(sigma)) && (C == 1 || (N & 3) == 0) && N >= 4;
    if (vec) {
        const dim3 grid((unsigned)(((N >> 2) + kBlock - 1) / kBlock));
        if (sigma)
            hipLaunchKernelGGL(precond_accumulate_vec_kernel<true>, grid, dim3(kBlock), 0, st, grad_v, sigma, C, N, beta, omb, V, nonfinite);
        else
            hipLaunchKernelGGL(precond_accumulate_vec_kernel<false>, grid, dim3(kBlock), 0, st, grad_v, sigma, C, N, beta, omb, V, nonfinite);
    } else {
        const dim3 grid((unsigned)((N + kBlock - 1) / kBlock));
        if (sigma)
            hipLaunchKernelGGL(precond_accumulate_kernel<true>, grid, dim3(kBlock), 0, st, grad_v, sigma, C, N, beta, omb, V, nonfinite);
        else
            hipLaunchKernelGGL(precond_accumulate_kernel<false>, grid, dim3(kBlock), 0, st, grad_v, sigma, C, N, beta, omb, V, nonfinite);
    }
}

size_t precond_workspace_bytes(const Vol& vol, int smooth) {
    return kScalBytes + kPartialBytes + (smooth > 0 ? (size_t)3 * vol.V * sizeof(float) : 0);
}

void launch_precond_sigma(const float* V, int C, const Vol& vol, float bias, int smooth, double damping, float sigma_min,
                          float sigma_max, const long long* nonfinite, float* sigma, double* summary, void* ws, hipStream_t st) {
    double* scal = (double*)ws;
    char* rows = (char*)ws + kScalBytes;
    float* smoothed = (float*)(rows + kPartialBytes);
    const int64_t N = 3 * vol.V;
    if (smooth > 0) {
        const dim3 grid((unsigned)((vol.W + kBoxX - 1) / kBoxX), (unsigned)((vol.H + kBoxY - 1) / kBoxY),
                        (unsigned)(3 * ((vol.D + kBoxZ - 1) / kBoxZ)));
        if (smooth == 1)
            hipLaunchKernelGGL(precond_box_kernel<1>, grid, dim3(kBlock), 0, st, V, bias, smoothed, vol);
        else
            hipLaunchKernelGGL(precond_box_kernel<2>, grid, dim3(kBlock), 0, st, V, bias, smoothed, vol);
    }
    const PrecondArgs a{smooth > 0 ? smoothed : V, smooth == 0, bias, damping, N};
    const int blocks = reduce_blocks(N);
    double* partials = (double*)rows;
    hipLaunchKernelGGL(precond_mean_kernel<0>, dim3(blocks), dim3(kBlock), 0, st, a, scal, partials);
    hipLaunchKernelGGL(precond_mean_finish_kernel, dim3(1), dim3(kBlock), 0, st, partials, blocks, N, scal);
    hipLaunchKernelGGL(precond_mean_kernel<1>, dim3(blocks), dim3(kBlock), 0, st, a, scal, partials);
    hipLaunchKernelGGL(precond_mean_finish_kernel, dim3(1), dim3(kBlock), 0, st, partials, blocks, N, scal + 1);
    long long* ipart = (long long*)rows;
    double* fpart = (double*)(ipart + (size_t)PrecondSummary::kInts * blocks);
    hipLaunchKernelGGL(precond_field_kernel, dim3(blocks), dim3(kBlock), 0, st, a, scal, sigma_min, sigma_max, C, sigma, ipart, fpart);
    hipLaunchKernelGGL(precond_summary_kernel, dim3(1), dim3(kBlock), 0, st, ipart, fpart, blocks, N, scal, nonfinite, summary);
}

}  // namespace irs
