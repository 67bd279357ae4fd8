// Average surface distance of label contours (the ASD of calc_metrics, utils/util.py:152-206) with an exact separable
// Euclidean distance transform, restricted to one box per (chain, label) pair.
//
//  - boxes: the bounding box of the voxels of a label in the fixed OR the moving map.  It holds both contours, so the exact
//    transform on the box grid gives the same nearest-contour distances as the transform of the whole volume.
//  - pass W, a wavefront per line of a box, lanes on consecutive x: contour membership (neighbours read from the full
//    volume, out-of-volume neighbours do not count), one byte per voxel, and the 1-D squared distances to A and to B
//    from two sweeps (ballots carry the nearest contour voxel from chunk to chunk).
//  - passes H and D: the Felzenszwalb-Huttenlocher lower envelope of parabolas per line, one lane per x, so every step
//    of the sequential scan is one coalesced load.  The envelope of a lane lives in LDS laid out [k][lane] (lines up
//    to kSurfLdsLine) or in a global scratch slot with the same layout (longer lines).
//  - pass D writes no distance map: it adds the distances at the contour voxels into per-task partial sums (double),
//    which one block per pair reduces in fixed order.  No atomics touch a float: two calls are bit-identical.
//  - pass D with KEEP (the Hausdorff distances, hausdorff_kernels.hip) also writes the squared distances back in place and
//    keeps the largest one at the contour voxels of each direction per task, as the bits of the float.
#include <limits.h>

#include <algorithm>

#include "contour_device.h"
#include "kernels.h"

namespace irs {
namespace {

constexpr float kInf = __builtin_huge_valf();
constexpr int kNone = INT_MAX;  // 1-D distance when the line holds no contour voxel

// the pair whose task range of `pass` holds task t (empty pairs own no task)
__device__ __forceinline__ int find_pair(const SurfPair* __restrict__ plan, int P, int64_t t, int pass) {
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int64_t off = pass == 0 ? plan[mid].tw : (pass == 1 ? plan[mid].th : plan[mid].td);
        if (off <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void surf_box_init_kernel(int32_t* __restrict__ boxes, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 6 * n) boxes[i] = i % 6 < 3 ? INT_MAX : -1;
}

// a wavefront per 64-voxel row segment; lane j keeps the running box of label j (one ballot per label and segment)
__global__ __launch_bounds__(kBlock) void surf_box_kernel(const int16_t* __restrict__ F, int64_t f_stride,
                                                          const int16_t* __restrict__ M, SurfLabels lab, int L,
                                                          int32_t* __restrict__ boxes, Vol vol) {
    const int c = blockIdx.y, lane = threadIdx.x & (kWave - 1);
    const int16_t* f = F + c * f_stride;
    const int16_t* m = M + c * vol.V;
    const int segs = (vol.W + kWave - 1) / kWave;
    const int64_t tasks = (int64_t)vol.D * vol.H * segs;
    const int64_t nw = (int64_t)gridDim.x * (kBlock / kWave);
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};  // z, y, x
    for (int64_t t = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; t < tasks; t += nw) {
        const int s = (int)(t % segs);
        const int64_t row = t / segs;
        const int y = (int)(row % vol.H), z = (int)(row / vol.H), x = s * kWave + lane;
        int fv = INT_MIN, mv = INT_MIN;  // labels are int16 values: INT_MIN matches none
        if (x < vol.W) {
            fv = f[row * vol.W + x];
            mv = m[row * vol.W + x];
        }
        for (int j = 0; j < L; ++j) {
            const uint64_t b = __ballot(fv == lab.v[j] || mv == lab.v[j]);
            if (b != 0 && lane == j) {
                lo[0] = min(lo[0], z);
                hi[0] = max(hi[0], z);
                lo[1] = min(lo[1], y);
                hi[1] = max(hi[1], y);
                lo[2] = min(lo[2], s * kWave + __builtin_ctzll(b));
                hi[2] = max(hi[2], s * kWave + 63 - __builtin_clzll(b));
            }
        }
    }
    if (lane < L && hi[0] >= 0) {
        int32_t* b = boxes + ((int64_t)c * L + lane) * 6;
        for (int a = 0; a < 3; ++a) {
            atomicMin(b + a, lo[a]);
            atomicMax(b + 3 + a, hi[a]);
        }
    }
}

// pass W: a wavefront per line (pair, z, y) of a box
__global__ __launch_bounds__(kBlock) void surf_pass_w_kernel(const int16_t* __restrict__ F, int64_t f_stride,
                                                             const int16_t* __restrict__ M, SurfLabels lab, int L,
                                                             SurfPassArgs a, float s0, Vol vol) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t nw = (int64_t)gridDim.x * (kBlock / kWave);
    for (int64_t t = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; t < a.tasks[0]; t += nw) {
        const int p = find_pair(a.plan, a.P, t, 0);
        const SurfPair q = a.plan[p];
        const int label = lab.v[p % L];
        const int16_t* f = F + (p / L) * f_stride;
        const int16_t* m = M + (p / L) * vol.V;
        const int64_t r = t - q.tw;
        const int yy = (int)(r % q.ny), zz = (int)(r / q.ny);
        const int64_t base = q.vox + ((int64_t)zz * q.ny + yy) * q.nx;
        uint8_t* mb = a.memb + base;
        float* ga = a.gA + base;
        float* gb = a.gB + base;
        // sweep 1, left to right: membership, and the distance to the nearest contour voxel on the left (an int, kept in
        // the bits of the distance arrays until sweep 2)
        int carryA = -1, carryB = -1;
        for (int cx = 0; cx < q.nx; cx += kWave) {
            const int xx = cx + lane;
            const bool act = xx < q.nx;
            bool ia = false, ib = false;
            if (act) {
                ia = on_contour(f, q.z0 + zz, q.y0 + yy, q.x0 + xx, label, vol);
                ib = on_contour(m, q.z0 + zz, q.y0 + yy, q.x0 + xx, label, vol);
                mb[xx] = (uint8_t)(ia | (ib << 1));
            }
            const uint64_t bA = __ballot(ia), bB = __ballot(ib);
            const uint64_t le = lane == kWave - 1 ? ~0ull : (2ull << lane) - 1;
            const int leftA = (bA & le) ? cx + 63 - __builtin_clzll(bA & le) : carryA;
            const int leftB = (bB & le) ? cx + 63 - __builtin_clzll(bB & le) : carryB;
            if (bA) carryA = cx + 63 - __builtin_clzll(bA);
            if (bB) carryB = cx + 63 - __builtin_clzll(bB);
            if (act) {
                ga[xx] = __int_as_float(leftA >= 0 ? xx - leftA : kNone);
                gb[xx] = __int_as_float(leftB >= 0 ? xx - leftB : kNone);
            }
        }
        // sweep 2, right to left: the nearest on the right, the minimum of both, squared in spacing units
        int carryRA = kNone, carryRB = kNone;
        for (int cx = (q.nx - 1) / kWave * kWave; cx >= 0; cx -= kWave) {
            const int xx = cx + lane;
            const bool act = xx < q.nx;
            const int mm = act ? mb[xx] : 0;  // written by this lane in sweep 1
            const uint64_t bA = __ballot(mm & 1), bB = __ballot(mm & 2);
            const uint64_t ge = ~0ull << lane;
            const int rightA = (bA & ge) ? cx + __builtin_ctzll(bA & ge) : carryRA;
            const int rightB = (bB & ge) ? cx + __builtin_ctzll(bB & ge) : carryRB;
            if (bA) carryRA = cx + __builtin_ctzll(bA);
            if (bB) carryRB = cx + __builtin_ctzll(bB);
            if (act) {
                int da = __float_as_int(ga[xx]), db = __float_as_int(gb[xx]);
                if (rightA != kNone) da = min(da, rightA - xx);
                if (rightB != kNone) db = min(db, rightB - xx);
                const float ea = s0 * (float)da, eb = s0 * (float)db;
                ga[xx] = da == kNone ? kInf : ea * ea;
                gb[xx] = db == kNone ? kInf : eb * eb;
            }
        }
    }
}

// lower envelope of the parabolas w2 (i - v)^2 + g[v] over the finite g[v] of one line (Felzenszwalb & Huttenlocher 2012).
// Entry k: apex v, height g[v], left end z.  Returns the index of the last entry, -1 when no g is finite.
__device__ __forceinline__ int lower_envelope(const float* __restrict__ g, int64_t stride, int n, float w2, float* ez, float* ef,
                                              int* ev, int ls) {
    const float half_inv_w2 = 0.5f / w2;
    int k = -1;
    for (int i = 0; i < n; ++i) {
        const float fi = g[i * stride];
        if (!(fi < kInf)) continue;
        float s = -kInf;
        while (k >= 0) {
            const int vk = ev[k * ls];
            // where the parabolas of i and vk meet; the form with (i + vk) / 2 apart keeps the float cancellation small
            s = (fi - ef[k * ls]) * half_inv_w2 / (float)(i - vk) + 0.5f * (float)(i + vk);
            if (s > ez[k * ls]) break;
            --k;
        }
        ++k;
        ev[k * ls] = i;
        ef[k * ls] = fi;
        ez[k * ls] = k == 0 ? -kInf : s;
    }
    return k;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_down((int)v, off, kWave));
    return v;
}

// passes H (LAST = false: along y, in place) and D (LAST = true: along z, ends in the partial sums of the task).
// A wavefront per task (pair, plane or row, 64-wide x chunk); grid-stride over the tasks.
// KEEP (pass D only): the squared distances are also written back in place -- safe, a lane has finished lower_envelope over
// its whole column before the scan, as pass H relies on -- and the largest key of each direction goes to a.maxpart.
template <bool IN_LDS, bool LAST, bool KEEP = false>
__global__ __launch_bounds__(kWave) void surf_pass_fh_kernel(SurfPassArgs a, float w2) {
    extern __shared__ float lds[];
    constexpr int pass = LAST ? 2 : 1;
    const int lane = threadIdx.x;
    const int ncap = a.line[pass];
    const int ls = IN_LDS ? kWave : a.lanes;
    float* env = IN_LDS ? lds : a.env_scratch[pass] + (int64_t)blockIdx.x * 3 * ncap * ls;
    float* ez = env + lane;
    float* ef = env + (int64_t)ncap * ls + lane;
    int* ev = (int*)(env + 2 * (int64_t)ncap * ls) + lane;
    for (int64_t t = blockIdx.x; t < a.tasks[pass]; t += gridDim.x) {
        const int p = find_pair(a.plan, a.P, t, pass);
        const SurfPair q = a.plan[p];
        const int chunks = (q.nx + kWave - 1) / kWave;
        const int64_t r = t - (LAST ? q.td : q.th);
        const int o = (int)(r / chunks), xx = (int)(r % chunks) * kWave + lane;  // o: plane zz (pass H) or row yy (pass D)
        const bool act = xx < q.nx;
        const int n = LAST ? q.nz : q.ny;
        const int64_t stride = LAST ? (int64_t)q.ny * q.nx : q.nx;
        const int64_t base = q.vox + (LAST ? (int64_t)o * q.nx : (int64_t)o * q.ny * q.nx) + xx;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};  // |A|, |B|, sum over A of d(., B), sum over B of d(., A)
        uint32_t mx[2] = {0u, 0u};             // KEEP: max over A of d2(., B), max over B of d2(., A), as float bits
        for (int fn = 0; fn < 2 && act; ++fn) {  // fn 0: distances to A, fn 1: distances to B
            float* g = (fn == 0 ? a.gA : a.gB) + base;
            const int k = lower_envelope(g, stride, n, w2, ez, ef, ev, ls);
            int j = 0;
            for (int i = 0; i < n; ++i) {
                float d = kInf;
                if (k >= 0) {
                    while (j < k && ez[(j + 1) * ls] < (float)i) ++j;
                    const float dv = (float)(i - ev[j * ls]);
                    d = w2 * dv * dv + ef[j * ls];
                }
                if (!LAST) {
                    g[i * stride] = d;
                } else {
                    if (KEEP) g[i * stride] = d;
                    const int mm = a.memb[base + i * stride];
                    if (mm & (fn == 0 ? 2 : 1)) {
                        acc[1 - fn] += 1.0;
                        acc[3 - fn] += sqrt((double)d);
                        if (KEEP) mx[1 - fn] = max(mx[1 - fn], __float_as_uint(d));  // d >= 0: the bits order as the floats
                    }
                }
            }
        }
        if (LAST) {
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] = wave_sum(acc[v]);
            if (lane == 0)
#pragma unroll
                for (int v = 0; v < 4; ++v) a.partials[t * 4 + v] = acc[v];
            if (KEEP) {
                mx[0] = wave_max(mx[0]);
                mx[1] = wave_max(mx[1]);
                if (lane == 0) {
                    a.maxpart[t * 2] = mx[0];
                    a.maxpart[t * 2 + 1] = mx[1];
                }
            }
        }
    }
}

// one block per pair: its pass-D partials in fixed order
__global__ __launch_bounds__(kBlock) void surf_reduce_kernel(const double* __restrict__ partials, const SurfPair* __restrict__ plan,
                                                             long long* __restrict__ counts, double* __restrict__ sums) {
    __shared__ double smem[4 * (kBlock / kWave)];
    const int p = blockIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t = plan[p].td + threadIdx.x; t < plan[p + 1].td; t += kBlock)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] += partials[t * 4 + v];
    block_sum<4>(acc, smem);
    if (threadIdx.x == 0) {
        counts[2 * p] = (long long)acc[0];
        counts[2 * p + 1] = (long long)acc[1];
        sums[2 * p] = acc[2];
        sums[2 * p + 1] = acc[3];
    }
}

int grid_for(int64_t tasks, int per_block, int cap) { return (int)std::min<int64_t>((tasks + per_block - 1) / per_block, cap); }

}  // namespace

void launch_surface_boxes(const int16_t* fixed, int64_t f_stride, const int16_t* moving, const SurfLabels& lab, int L,
                          int32_t* boxes, int C, Vol vol, hipStream_t st) {
    const int n = C * L;
    hipLaunchKernelGGL(surf_box_init_kernel, dim3((6 * n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, boxes, n);
    const int64_t tasks = (int64_t)vol.D * vol.H * ((vol.W + kWave - 1) / kWave);
    // about 32 row segments per wavefront: few box atomics, enough wavefronts to fill the chip at 128^3 and above
    hipLaunchKernelGGL(surf_box_kernel, dim3(grid_for(tasks, 32 * (kBlock / kWave), 1024), C), dim3(kBlock), 0, st, fixed,
                       f_stride, moving, lab, L, boxes, vol);
}

void launch_surface_distance(const int16_t* fixed, int64_t f_stride, const int16_t* moving, const SurfLabels& lab, int L,
                             const float spacing[3], const SurfPassArgs& a, long long* counts, double* sums, Vol vol,
                             hipStream_t st) {
    if (a.tasks[0] > 0)
        hipLaunchKernelGGL(surf_pass_w_kernel, dim3(grid_for(a.tasks[0], kBlock / kWave, 65536)), dim3(kBlock), 0, st, fixed,
                           f_stride, moving, lab, L, a, spacing[0], vol);
    for (int pass = 1; pass <= 2; ++pass) {
        if (a.tasks[pass] == 0) continue;
        const float w2 = spacing[pass] * spacing[pass];
        if (!a.env_scratch[pass]) {
            const dim3 grid(grid_for(a.tasks[pass], 1, 65536));
            const size_t lds = (size_t)3 * a.line[pass] * kWave * sizeof(float);
            if (pass == 1) hipLaunchKernelGGL((surf_pass_fh_kernel<true, false>), grid, dim3(kWave), lds, st, a, w2);
            else if (a.maxpart) hipLaunchKernelGGL((surf_pass_fh_kernel<true, true, true>), grid, dim3(kWave), lds, st, a, w2);
            else hipLaunchKernelGGL((surf_pass_fh_kernel<true, true>), grid, dim3(kWave), lds, st, a, w2);
        } else {
            const dim3 grid(a.env_slots[pass]);
            if (pass == 1) hipLaunchKernelGGL((surf_pass_fh_kernel<false, false>), grid, dim3(kWave), 0, st, a, w2);
            else if (a.maxpart) hipLaunchKernelGGL((surf_pass_fh_kernel<false, true, true>), grid, dim3(kWave), 0, st, a, w2);
            else hipLaunchKernelGGL((surf_pass_fh_kernel<false, true>), grid, dim3(kWave), 0, st, a, w2);
        }
    }
    if (counts) hipLaunchKernelGGL(surf_reduce_kernel, dim3(a.P), dim3(kBlock), 0, st, a.partials, a.plan, counts, sums);
}

}  // namespace irs
