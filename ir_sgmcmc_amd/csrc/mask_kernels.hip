// Foreground masks from the image (absent in the reference, which reads every mask from a file; DESIGN.md section 6, "Automatic
// foreground masks"): an exact intensity histogram, connected-component labelling, selection of the largest components, hole
// filling and exact morphology with a Euclidean ball.  Every operator takes C volumes of (D, H, W) and treats them independently;
// nothing connects across the end of a row, a plane or a volume, because every neighbour is addressed by (x, y, z) and tested
// against the extents before it is read.
//
//  - histogram: one launch for all volumes, blockIdx.y the volume; a grid-stride stream with a per-block uint32 histogram in LDS
//    (hist_add and hist_bin of histogram_device.h), flushed to the int64 histogram with integer atomics.
//  - components: union-find on int32 parents, the parent of a voxel never larger than its own linear index, so the root of a
//    finished component is its smallest linear index.
//      1. cc_tile_kernel labels 32 x 8 x 4 tiles in LDS: every set voxel is united with its set "backward" neighbours inside the
//         tile (the 13 of the 26 offsets that come first in linear order, cut down to 3 / 9 for connectivity 6 / 18) and leaves
//         the global index of its tile root.
//      2. cc_merge_kernel unites across tile faces: the same backward neighbours, where they lie in another tile.
//      3. cc_flatten_kernel points every voxel at its root and counts the roots of every 1024 consecutive voxels.
//      4. cc_scan_kernel: one block per volume, exclusive scan of those counts -> the number of components.
//      5. cc_rank_kernel: a root's number is 1 + the roots before it in linear order (block offset + scan inside the block).
//      6. cc_relabel_kernel: every voxel takes the number of its root; background 0.
//    A union is `atomicMin(parent[larger root], smaller root)`; when the larger one was a root no longer the loop goes on from the
//    parent it had, which is smaller.  Parents only decrease, so a find walks at most V links and a union retries at most 2 V
//    times: both loops are `for` loops with that trip bound.  No workgroup waits for another and no trip count depends on another
//    workgroup's progress; what another workgroup writes in the meantime is a parent further up the same tree.
//  - keep_largest: sizes by integer atomics on the component numbers, then one block per volume picks the `keep` largest (ties: the
//    smaller number) by `keep` arg-max sweeps; fill_holes: the 6-connected components of the complement and a flag per
//    component that touches the border of the volume.
//  - morphology: the squared Euclidean distance to the nearest set voxel, capped at r2 + 1, in three separable passes with
//    |offset| <= R = floor(sqrt(r2)) each: the row pass (distance to the nearest set voxel of the row, uint8), then the lower
//    envelopes min(g^2 + dy^2) over y and min(h + dz^2) over z (uint16).  One thread per voxel, x fastest, so the lanes of a
//    wavefront read consecutive addresses in every pass.  Integers throughout: `<= r2` has no tolerance.  Voxels outside the
//    volume are never read: they are not set for a dilation and, the erosion being the dilation of the complement, not
//    background for an erosion.
// Every result is a function of the input alone: the labels are canonical (numbered by smallest linear index), the histogram, the
// sizes and the flags are integers or idempotent stores, so the order of the atomics does not show and two calls are bit-identical.
#include <algorithm>

#include "histogram_device.h"
#include "kernels.h"

namespace irs {
namespace {

// ---- histogram and threshold --------------------------------------------------------------------------------------------
// im (C,V); mask (1 or C, V) with mask_stride 0 or V, or nullptr; hist (C,bins), zero on entry.  Dynamic LDS: bins uint32.
__global__ __launch_bounds__(kBlock) void intensity_histogram_kernel(const float* __restrict__ im, const uint8_t* __restrict__ mask,
                                                                     int64_t mask_stride, int64_t V, float lo, float inv_w, int bins,
                                                                     unsigned long long* __restrict__ hist) {
    extern __shared__ uint32_t mask_hist_lds[];
    for (int i = threadIdx.x; i < bins; i += kBlock) mask_hist_lds[i] = 0;
    __syncthreads();
    const int c = blockIdx.y;
    const float* src = im + (int64_t)c * V;
    const uint8_t* m = mask ? mask + (int64_t)c * mask_stride : nullptr;
    const float last = (float)(bins - 1);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // the trip count is the wavefront's: the ballots of hist_add see every lane
    for (int64_t u0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1)); u0 < V; u0 += stride) {
        const int64_t u = u0 + (threadIdx.x & (kWave - 1));
        float x = 0.0f;
        bool take = false;
        if (u < V) {
            x = src[u];
            take = isfinite(x) && (m ? m[u] != 0 : true);
        }
        hist_add(mask_hist_lds, take, take ? hist_bin(x, lo, inv_w, last) : 0, true);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += kBlock) {
        const uint32_t n = mask_hist_lds[i];
        if (n) atomicAdd(&hist[(int64_t)c * bins + i], (unsigned long long)n);
    }
}

__global__ __launch_bounds__(kBlock) void mask_threshold_kernel(const float* __restrict__ im, float threshold, uint8_t* __restrict__ out,
                                                                Vol vol) {
    IRS_VOXEL(vol, plane, x, y, z, vox);
    const int64_t i = (int64_t)plane * vol.V + vox;
    out[i] = im[i] > threshold ? 1 : 0;  // a NaN is background
}

// ---- connected components ---------------------------------------------------------------------------------------------------
constexpr int kTx = 32, kTy = 8, kTz = 4, kTileVox = kTx * kTy * kTz;  // the tile of launch 1; kTx * kTy == kBlock
constexpr int kChunk = 4 * kBlock;                                      // consecutive voxels per block of launches 3 and 5

struct Off3 {
    int dz, dy, dx;
    bool ok;
};
// the k-th of the 13 offsets that precede a voxel in linear order; ok: within the connectivity (6 / 18 / 26: at most 1 / 2 / 3
// non-zero components)
__device__ __forceinline__ Off3 backward_offset(int k, int conn) {
    Off3 o;
    if (k < 9) {
        o.dz = -1, o.dy = k / 3 - 1, o.dx = k % 3 - 1;
    } else if (k < 12) {
        o.dz = 0, o.dy = -1, o.dx = k - 10;
    } else {
        o.dz = 0, o.dy = 0, o.dx = -1;
    }
    const int nonzero = (o.dz != 0) + (o.dy != 0) + (o.dx != 0);
    o.ok = nonzero <= (conn == 6 ? 1 : conn == 18 ? 2 : 3);
    return o;
}

__device__ __forceinline__ int uf_load(const int* L, int i) { return __atomic_load_n(L + i, __ATOMIC_RELAXED); }

// the root above x: parents strictly decrease along the walk, so it ends within `bound` (the number of elements) links
__device__ __forceinline__ int uf_find(const int* L, int x, int bound) {
    for (int it = 0; it < bound; ++it) {
        const int p = uf_load(L, x);
        if (p == x) break;
        x = p;
    }
    return x;
}

// every retry goes on from a strictly smaller a: at most 2 * bound of them
__device__ __forceinline__ void uf_union(int* L, int a, int b, int bound) {
    for (int64_t it = 0; it <= 2 * (int64_t)bound; ++it) {
        a = uf_find(L, a, bound);
        b = uf_find(L, b, bound);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;  // a was a root: it hangs under b now
        a = old;               // it had a parent already (smaller than a): unite that with b
    }
}

// launch 1: grid (tiles x, tiles y, tiles z * C); label (C,V): -1 background, else the linear index of the voxel's tile root
__global__ __launch_bounds__(kBlock) void cc_tile_kernel(const uint8_t* __restrict__ mask, int invert, int conn, Vol vol, int tiles_z,
                                                         int* __restrict__ label) {
    __shared__ int L[kTileVox];
    const int c = blockIdx.z / tiles_z, tz = blockIdx.z - c * tiles_z;
    const int x0 = blockIdx.x * kTx, y0 = blockIdx.y * kTy, z0 = tz * kTz;
    const int lx = threadIdx.x & (kTx - 1), ly = threadIdx.x / kTx;
    const int x = x0 + lx, y = y0 + ly;
    const bool in_xy = x < vol.W && y < vol.H;
    const uint8_t* m = mask + (int64_t)c * vol.V;
    int* lab = label + (int64_t)c * vol.V;
    unsigned set = 0;
#pragma unroll
    for (int lz = 0; lz < kTz; ++lz) {
        const int z = z0 + lz, li = (lz * kTy + ly) * kTx + lx;
        bool s = false;
        if (in_xy && z < vol.D) s = (m[((int64_t)z * vol.H + y) * vol.W + x] != 0) != (invert != 0);
        set |= (unsigned)s << lz;
        L[li] = s ? li : -1;
    }
    __syncthreads();
#pragma unroll
    for (int lz = 0; lz < kTz; ++lz) {
        if (!((set >> lz) & 1u)) continue;
        const int li = (lz * kTy + ly) * kTx + lx;
        for (int k = 0; k < 13; ++k) {
            const Off3 o = backward_offset(k, conn);
            const int nx = lx + o.dx, ny = ly + o.dy, nz = lz + o.dz;
            if (!o.ok || nx < 0 || nx >= kTx || ny < 0 || ny >= kTy || nz < 0) continue;
            const int ni = (nz * kTy + ny) * kTx + nx;
            if (uf_load(L, ni) >= 0) uf_union(L, li, ni, kTileVox);  // a voxel outside the volume is -1
        }
    }
    __syncthreads();
#pragma unroll
    for (int lz = 0; lz < kTz; ++lz) {
        const int z = z0 + lz;
        if (!in_xy || z >= vol.D) continue;
        int out = -1;
        if ((set >> lz) & 1u) {
            const int r = uf_find(L, (lz * kTy + ly) * kTx + lx, kTileVox);
            const int rz = r / (kTx * kTy), ry = (r / kTx) % kTy, rx = r % kTx;
            out = ((z0 + rz) * vol.H + y0 + ry) * vol.W + x0 + rx;
        }
        lab[((int64_t)z * vol.H + y) * vol.W + x] = out;
    }
}

// launch 2: one thread per voxel; the backward neighbours that lie in another tile
__global__ __launch_bounds__(kBlock) void cc_merge_kernel(int conn, Vol vol, int* __restrict__ label) {
    IRS_VOXEL(vol, c, x, y, z, vox);
    int* lab = label + (int64_t)c * vol.V;
    if (uf_load(lab, (int)vox) < 0) return;
    for (int k = 0; k < 13; ++k) {
        const Off3 o = backward_offset(k, conn);
        const int nx = x + o.dx, ny = y + o.dy, nz = z + o.dz;
        if (!o.ok || nx < 0 || nx >= vol.W || ny < 0 || ny >= vol.H || nz < 0) continue;
        if (nx / kTx == x / kTx && ny / kTy == y / kTy && nz / kTz == z / kTz) continue;  // launch 1 did it
        const int nv = (nz * vol.H + ny) * vol.W + nx;
        if (uf_load(lab, nv) >= 0) uf_union(lab, (int)vox, nv, (int)vol.V);
    }
}

// launch 3: grid (ceil(V / kChunk), C); thread t of block b owns voxels b * kChunk + 4 t .. + 3
__global__ __launch_bounds__(kBlock) void cc_flatten_kernel(int64_t V, int* __restrict__ label, int* __restrict__ block_roots) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int* lab = label + (int64_t)blockIdx.y * V;
    const int64_t v0 = (int64_t)blockIdx.x * kChunk + 4 * (int)threadIdx.x;
    int roots = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t v = v0 + j;
        if (v >= V || uf_load(lab, (int)v) < 0) continue;
        const int r = uf_find(lab, (int)v, (int)V);
        if (r == (int)v) ++roots;
        else __atomic_store_n(lab + v, r, __ATOMIC_RELAXED);
    }
    if (roots) atomicAdd(&total, roots);
    __syncthreads();
    if (threadIdx.x == 0) block_roots[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

constexpr int kScanBlock = 1024;
// launch 4: grid (C); block_roots (C, blocks) -> its exclusive scan in place; counts[c]: the sum
__global__ __launch_bounds__(kScanBlock) void cc_scan_kernel(int blocks, int* __restrict__ block_roots, int32_t* __restrict__ counts) {
    __shared__ int part[kScanBlock];
    int* br = block_roots + (int64_t)blockIdx.x * blocks;
    const int per = (blocks + kScanBlock - 1) / kScanBlock;
    const int lo = min((int)threadIdx.x * per, blocks), hi = min(lo + per, blocks);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += br[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < kScanBlock; ++i) {
            const int t = part[i];
            part[i] = run;
            run += t;
        }
        counts[blockIdx.x] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) {
        const int t = br[i];
        br[i] = run;
        run += t;
    }
}

// launch 5: the blocking of launch 3; rank[root] = its number (written at the roots only)
__global__ __launch_bounds__(kBlock) void cc_rank_kernel(int64_t V, const int* __restrict__ label, const int* __restrict__ block_offset,
                                                         int* __restrict__ rank) {
    __shared__ int scan[kBlock];
    const int* lab = label + (int64_t)blockIdx.y * V;
    int* rk = rank + (int64_t)blockIdx.y * V;
    const int64_t v0 = (int64_t)blockIdx.x * kChunk + 4 * (int)threadIdx.x;
    bool root[4];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t v = v0 + j;
        root[j] = v < V && lab[v] == (int)v;
        mine += root[j];
    }
    scan[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {  // inclusive scan over the threads of the block
        const int add = (int)threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
        __syncthreads();
        scan[threadIdx.x] += add;
        __syncthreads();
    }
    int next = block_offset[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] + scan[threadIdx.x] - mine + 1;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (root[j]) rk[v0 + j] = next++;
}

// launch 6
__global__ __launch_bounds__(kBlock) void cc_relabel_kernel(const int* __restrict__ label, const int* __restrict__ rank,
                                                            int32_t* __restrict__ out, Vol vol) {
    IRS_VOXEL(vol, c, x, y, z, vox);
    const int64_t i = (int64_t)c * vol.V + vox;
    const int r = label[i];
    out[i] = r >= 0 ? rank[(int64_t)c * vol.V + r] : 0;
}

// ---- selection and hole filling -----------------------------------------------------------------------------------------------
// sizes[c, l - 1] += 1 per voxel of component l.  The foreground is mostly ONE component and every atomic on its size hits one
// address (measured: 19 ms of the 20 ms of keep_largest at 256^3): when the voxels of a wavefront's row piece that belong to
// any component all belong to the same one, its first lane adds their number -- the rule of hist_add, on global memory
__global__ __launch_bounds__(kBlock) void component_sizes_kernel(const int32_t* __restrict__ labels, int* __restrict__ sizes, Vol vol) {
    IRS_VOXEL(vol, c, x, y, z, vox);  // (lanes past the end of the row have left: the ballots count the others)
    const int l = labels[(int64_t)c * vol.V + vox];
    const bool take = l > 0;
    const unsigned long long todo = __ballot(take);
    if (todo == 0) return;
    const int leader = __ffsll(todo) - 1;
    const int first = __builtin_amdgcn_readlane(l, leader);
    int* sz = sizes + (int64_t)c * vol.V;
    if (__ballot(take && l != first) == 0) {
        if ((int)(threadIdx.x & (kWave - 1)) == leader) atomicAdd(&sz[first - 1], (int)__popcll(todo));
        return;
    }
    if (take) atomicAdd(&sz[l - 1], 1);
}

// grid (C): `keep` arg-max sweeps over sizes[0 .. counts[c]); a picked component's size becomes -1
__global__ __launch_bounds__(kScanBlock) void select_largest_kernel(const int32_t* __restrict__ counts, int64_t V, int keep,
                                                                    int* __restrict__ sizes) {
    __shared__ int best_size[kScanBlock];
    __shared__ int best_index[kScanBlock];
    int* sz = sizes + (int64_t)blockIdx.x * V;
    const int n = counts[blockIdx.x];
    for (int k = 0; k < keep && k < n; ++k) {
        int bs = 0, bi = -1;
        for (int i = threadIdx.x; i < n; i += kScanBlock) {  // ascending i: the first of equal sizes stays
            const int s = sz[i];
            if (s > bs) bs = s, bi = i;
        }
        best_size[threadIdx.x] = bs;
        best_index[threadIdx.x] = bi;
        __syncthreads();
        for (int off = kScanBlock / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) {
                const int s = best_size[threadIdx.x + off], i = best_index[threadIdx.x + off];
                if (s > best_size[threadIdx.x] || (s == best_size[threadIdx.x] && s > 0 && i < best_index[threadIdx.x]))
                    best_size[threadIdx.x] = s, best_index[threadIdx.x] = i;
            }
            __syncthreads();
        }
        if (threadIdx.x == 0 && best_index[0] >= 0) sz[best_index[0]] = -1;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void apply_selection_kernel(const int32_t* __restrict__ labels, const int* __restrict__ sizes,
                                                                 uint8_t* __restrict__ out, Vol vol) {
    IRS_VOXEL(vol, c, x, y, z, vox);
    const int64_t i = (int64_t)c * vol.V + vox;
    const int l = labels[i];
    out[i] = l > 0 && sizes[(int64_t)c * vol.V + l - 1] < 0 ? 1 : 0;
}

// labels: the components of the complement; open_flag[c, l - 1] = 1 for one that has a voxel on the border of the volume
__global__ __launch_bounds__(kBlock) void border_flag_kernel(const int32_t* __restrict__ labels, int* __restrict__ open_flag, Vol vol) {
    IRS_VOXEL(vol, c, x, y, z, vox);
    if (x != 0 && y != 0 && z != 0 && x != vol.W - 1 && y != vol.H - 1 && z != vol.D - 1) return;
    const int l = labels[(int64_t)c * vol.V + vox];
    if (l > 0) open_flag[(int64_t)c * vol.V + l - 1] = 1;
}

__global__ __launch_bounds__(kBlock) void apply_fill_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ labels,
                                                            const int* __restrict__ open_flag, uint8_t* __restrict__ out, Vol vol) {
    IRS_VOXEL(vol, c, x, y, z, vox);
    const int64_t i = (int64_t)c * vol.V + vox;
    const int l = labels[i];
    out[i] = mask[i] != 0 || (l > 0 && open_flag[(int64_t)c * vol.V + l - 1] == 0) ? 1 : 0;
}

// ---- ball morphology ----------------------------------------------------------------------------------------------------------
constexpr int kFar = 255;  // row pass: no set voxel within R

__global__ __launch_bounds__(kBlock) void ball_row_kernel(const uint8_t* __restrict__ mask, int invert, int R, uint8_t* __restrict__ g,
                                                          Vol vol) {
    IRS_VOXEL(vol, c, x, y, z, vox);
    const uint8_t* row = mask + (int64_t)c * vol.V + vox - x;
    int best = kFar;
    for (int d = 0; d <= R; ++d) {  // ascending: the first hit is the nearest
        const bool left = x - d >= 0 && (row[x - d] != 0) != (invert != 0);
        const bool right = x + d < vol.W && (row[x + d] != 0) != (invert != 0);
        if (left || right) {
            best = d;
            break;
        }
    }
    g[(int64_t)c * vol.V + vox] = (uint8_t)best;
}

// h = min(r2 + 1, min over |dy| <= R of g(y + dy)^2 + dy^2)
__global__ __launch_bounds__(kBlock) void ball_y_kernel(const uint8_t* __restrict__ g, int R, int r2, uint16_t* __restrict__ h, Vol vol) {
    IRS_VOXEL(vol, c, x, y, z, vox);
    const uint8_t* col = g + (int64_t)c * vol.V + vox;
    int best = r2 + 1;
    const int lo = max(-R, -y), hi = min(R, vol.H - 1 - y);
    for (int d = lo; d <= hi; ++d) {
        const int a = col[(int64_t)d * vol.W];
        if (a != kFar) best = min(best, a * a + d * d);
    }
    h[(int64_t)c * vol.V + vox] = (uint16_t)best;
}

// out = (min over |dz| <= R of h(z + dz) + dz^2 <= r2), inverted for an erosion
__global__ __launch_bounds__(kBlock) void ball_z_kernel(const uint16_t* __restrict__ h, int invert, int R, int r2, uint8_t* __restrict__ out,
                                                        Vol vol) {
    IRS_VOXEL(vol, c, x, y, z, vox);
    const uint16_t* col = h + (int64_t)c * vol.V + vox;
    const int64_t plane = (int64_t)vol.H * vol.W;
    int best = r2 + 1;
    const int lo = max(-R, -z), hi = min(R, vol.D - 1 - z);
    for (int d = lo; d <= hi; ++d) best = min(best, (int)col[d * plane] + d * d);
    out[(int64_t)c * vol.V + vox] = (best <= r2) != (invert != 0) ? 1 : 0;
}

inline int cc_blocks(int64_t V) { return (int)((V + kChunk - 1) / kChunk); }
inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

void launch_intensity_histogram(const float* im, const uint8_t* mask, int64_t mask_stride, int64_t V, int C, float lo, float inv_w,
                                int bins, long long* hist, hipStream_t st) {
    (void)hipMemsetAsync(hist, 0, (size_t)C * bins * sizeof(long long), st);
    const int blocks = (int)std::min<int64_t>((V + kBlock - 1) / kBlock, 1024);
    hipLaunchKernelGGL(intensity_histogram_kernel, dim3(blocks, C), dim3(kBlock), (size_t)bins * sizeof(uint32_t), st, im, mask,
                       mask_stride, V, lo, inv_w, bins, reinterpret_cast<unsigned long long*>(hist));
}

void launch_mask_threshold(const float* im, float threshold, uint8_t* out, int C, const Vol& vol, hipStream_t st) {
    hipLaunchKernelGGL(mask_threshold_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, im, threshold, out, vol);
}

size_t connected_components_bytes(int C, int64_t V) {
    return 2 * align16((size_t)C * V * sizeof(int)) + align16((size_t)C * cc_blocks(V) * sizeof(int));
}

void launch_connected_components(const uint8_t* mask, bool invert, int conn, int32_t* labels, int32_t* counts, int C, const Vol& vol,
                                 void* ws, hipStream_t st) {
    const size_t field = align16((size_t)C * vol.V * sizeof(int));
    int* root = reinterpret_cast<int*>(ws);
    int* rank = reinterpret_cast<int*>((char*)ws + field);
    int* block_roots = reinterpret_cast<int*>((char*)ws + 2 * field);
    const int tiles_z = (vol.D + kTz - 1) / kTz, blocks = cc_blocks(vol.V);
    const dim3 tiles((vol.W + kTx - 1) / kTx, (vol.H + kTy - 1) / kTy, tiles_z * C);
    hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(kBlock), 0, st, mask, (int)invert, conn, vol, tiles_z, root);
    hipLaunchKernelGGL(cc_merge_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, conn, vol, root);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks, C), dim3(kBlock), 0, st, vol.V, root, block_roots);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(C), dim3(kScanBlock), 0, st, blocks, block_roots, counts);
    hipLaunchKernelGGL(cc_rank_kernel, dim3(blocks, C), dim3(kBlock), 0, st, vol.V, root, block_roots, rank);
    hipLaunchKernelGGL(cc_relabel_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, root, rank, labels, vol);
}

size_t mask_select_bytes(int C, int64_t V) {
    return connected_components_bytes(C, V) + align16((size_t)C * V * sizeof(int32_t)) + align16((size_t)C * sizeof(int32_t));
}

namespace {
// the components of the (inverted) mask into the tail of a mask_select_bytes workspace -> labels, counts; the first field of
// the workspace is free afterwards and comes back zeroed, one int per possible component
int* components_for_selection(const uint8_t* mask, bool invert, int conn, int C, const Vol& vol, void* ws, int32_t*& labels,
                              int32_t*& counts, hipStream_t st) {
    labels = reinterpret_cast<int32_t*>((char*)ws + connected_components_bytes(C, vol.V));
    counts = reinterpret_cast<int32_t*>((char*)labels + align16((size_t)C * vol.V * sizeof(int32_t)));
    launch_connected_components(mask, invert, conn, labels, counts, C, vol, ws, st);
    (void)hipMemsetAsync(ws, 0, (size_t)C * vol.V * sizeof(int), st);
    return reinterpret_cast<int*>(ws);
}
}  // namespace

void launch_mask_keep_largest(const uint8_t* mask, int conn, int keep, uint8_t* out, int C, const Vol& vol, void* ws, hipStream_t st) {
    int32_t *labels, *counts;
    int* sizes = components_for_selection(mask, false, conn, C, vol, ws, labels, counts, st);
    hipLaunchKernelGGL(component_sizes_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, labels, sizes, vol);
    hipLaunchKernelGGL(select_largest_kernel, dim3(C), dim3(kScanBlock), 0, st, counts, vol.V, keep, sizes);
    hipLaunchKernelGGL(apply_selection_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, labels, sizes, out, vol);
}

void launch_mask_fill_holes(const uint8_t* mask, uint8_t* out, int C, const Vol& vol, void* ws, hipStream_t st) {
    int32_t *labels, *counts;
    int* open_flag = components_for_selection(mask, true, 6, C, vol, ws, labels, counts, st);
    hipLaunchKernelGGL(border_flag_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, labels, open_flag, vol);
    hipLaunchKernelGGL(apply_fill_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, mask, labels, open_flag, out, vol);
}

size_t mask_morphology_bytes(int C, int64_t V) { return align16((size_t)C * V) + align16((size_t)C * V * sizeof(uint16_t)); }

void launch_mask_dilate(const uint8_t* mask, int r2, bool erode, uint8_t* out, int C, const Vol& vol, void* ws, hipStream_t st) {
    uint8_t* g = reinterpret_cast<uint8_t*>(ws);
    uint16_t* h = reinterpret_cast<uint16_t*>((char*)ws + align16((size_t)C * vol.V));
    int R = 0;
    while ((R + 1) * (R + 1) <= r2) ++R;  // floor(sqrt(r2)), r2 <= IRS_MASK_MAX_RADIUS^2
    const dim3 grid = vox_grid(vol, C);
    hipLaunchKernelGGL(ball_row_kernel, grid, dim3(kBlock), 0, st, mask, (int)erode, R, g, vol);
    hipLaunchKernelGGL(ball_y_kernel, grid, dim3(kBlock), 0, st, g, R, r2, h, vol);
    hipLaunchKernelGGL(ball_z_kernel, grid, dim3(kBlock), 0, st, h, (int)erode, R, r2, out, vol);
}

}  // namespace irs
