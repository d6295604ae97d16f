// Voxel-grid merge of a point cloud (include/esfm.h, "Dense-cloud merge", esfm_cloud_voxel_merge): coordinate bounds, cell keys,
// (voxel_sort.hip sorts them), run heads -> voxel ids, the per-voxel integer sums, and the filtered, key-ordered output.  Every
// sum across points is an int64 sum of quantised terms, so the result does not depend on the order the members arrive in;
// tests/merge_ref.py restates the rule and the output is compared bit for bit (-ffp-contract=off; HIP's default f32 / f64
// division and f64 sqrt are correctly rounded).
#include <cmath>

#include "block_scan.hpp"
#include "voxel_kernels.hpp"

namespace esfm {

// ---- bounds --------------------------------------------------------------------------------------------------------------
// Grid-stride over the points; each workgroup leaves the min / max of the finite points it saw and their number (min and max are
// order-free; the host folds the at most kVoxelBoundsBlocks partials).
__global__ __launch_bounds__(256) void voxel_bounds_kernel(const float *xyz, int n, VoxelBounds *partials)
{
    __shared__ float s_lo[3][256], s_hi[3][256];
    __shared__ int32_t s_n[256];
    const int tid = threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int32_t cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        const float p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) continue;
        ++cnt;
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], p[c]); hi[c] = fmaxf(hi[c], p[c]); }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { s_lo[c][tid] = lo[c]; s_hi[c][tid] = hi[c]; }
    s_n[tid] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s_lo[c][tid] = fminf(s_lo[c][tid], s_lo[c][tid + o]);
                s_hi[c][tid] = fmaxf(s_hi[c][tid], s_hi[c][tid + o]);
            }
            s_n[tid] += s_n[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        VoxelBounds b;
        for (int c = 0; c < 3; ++c) { b.lo[c] = s_lo[c][0]; b.hi[c] = s_hi[c][0]; }
        b.n_valid = s_n[0]; b.pad = 0;
        partials[blockIdx.x] = b;
    }
}

// ---- keys ----------------------------------------------------------------------------------------------------------------
// c_a = floorf((x_a - o_a) / h) in f32; the host has checked with the coordinate maximum that every index stays below 2^21.
__global__ __launch_bounds__(256) void voxel_keys_kernel(VoxelArgs a, uint64_t *keys, int32_t *index)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const float p[3] = {a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2]};
    uint64_t key = kVoxelNoKey;
    if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
        const uint64_t cx = (uint64_t)floorf((p[0] - a.o[0]) / a.h), cy = (uint64_t)floorf((p[1] - a.o[1]) / a.h),
                       cz = (uint64_t)floorf((p[2] - a.o[2]) / a.h);
        key = cz << 42 | cy << 21 | cx;
    }
    keys[i] = key;
    index[i] = (int32_t)i;
}

// ---- run heads -----------------------------------------------------------------------------------------------------------
struct VoxelIsHead {
    VoxelArgs a;
    __device__ bool operator()(int64_t i) const { return i < a.n_valid && (i == 0 || a.keys[i] != a.keys[i - 1]); }
};

// ---- accumulation --------------------------------------------------------------------------------------------------------
// One thread per sorted entry; a voxel's members are contiguous.  Each wave folds its entries by voxel with a segmented scan over
// lanes (a lane adds the partial 2^s lanes below while that lane holds the same voxel), so the last lane of every run piece holds
// the piece's sums.  A run that begins and ends inside the wave is stored; only the pieces of a run that crosses a wave or
// workgroup boundary are committed with 64-bit integer atomics -- a cloud that falls into one voxel issues one set of atomics per
// wave, not per point.
__global__ __launch_bounds__(256) void voxel_accumulate_kernel(VoxelArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < a.n_valid;
    const uint64_t key = in ? a.keys[i] : kVoxelNoKey;
    const bool head = VoxelIsHead{a}(i);
    const bool tail = in && (i + 1 == a.n_valid || a.keys[i + 1] != key);
    const int incl = block_inclusive_count(head);
    const int vid = in ? a.head_count[blockIdx.x] + incl - 1 : -1;       // (entry 0 is a head: vid >= 0 for every entry)

    int64_t v[kVoxelAccWords - 1];
#pragma unroll
    for (int w = 0; w < kVoxelAccWords - 1; ++w) v[w] = 0;
    uint64_t mask = 0;
    int has_head = head ? 1 : 0;
    if (in) {
        const int64_t p = a.order[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double cell = (double)(int64_t)((key >> (21 * c)) & 0x1FFFFFull);
            const double u = ((double)a.xyz[3 * p + c] - (double)a.o[c]) / (double)a.h - cell;
            v[c] = llrint(u * 1073741824.0);
        }
        if (a.rgb) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 + c] = a.rgb[3 * p + c];
        }
        if (a.normals) {
            const float nx = a.normals[3 * p], ny = a.normals[3 * p + 1], nz = a.normals[3 * p + 2];
            if (nx != 0.f || ny != 0.f || nz != 0.f) {
                v[6] = llrint((double)nx * 1048576.0); v[7] = llrint((double)ny * 1048576.0); v[8] = llrint((double)nz * 1048576.0);
            }
        }
        v[9] = 1;
        if (a.tags) mask = 1ull << (a.tags[p] & 63);                       // (0..63: checked on the host)
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const bool same = __shfl_up(vid, off) == vid && lane >= off;
#pragma unroll
        for (int w = 0; w < kVoxelAccWords - 1; ++w) {
            const long long t = __shfl_up((long long)v[w], off);
            if (same) v[w] += t;
        }
        const unsigned long long tm = __shfl_up((unsigned long long)mask, off);
        const int th = __shfl_up(has_head, off);
        if (same) { mask |= tm; has_head |= th; }
    }
    if (!in) return;
    if (head) a.vox_key[vid] = key;
    if (!(tail || lane == 63)) return;                                       // not the last lane of a run piece
    int64_t *dst = a.acc + (int64_t)vid * kVoxelAccWords;
    if (tail && has_head) {                                                  // the whole run is in this wave
#pragma unroll
        for (int w = 0; w < kVoxelAccWords - 1; ++w) dst[w] = v[w];
        dst[kVoxelAccWords - 1] = (int64_t)mask;
    } else {
#pragma unroll
        for (int w = 0; w < kVoxelAccWords - 1; ++w)
            if (v[w] != 0) atomicAdd(reinterpret_cast<unsigned long long *>(dst + w), (unsigned long long)v[w]);
        if (mask) atomicOr(reinterpret_cast<unsigned long long *>(dst + kVoxelAccWords - 1), (unsigned long long)mask);
    }
}

// ---- finalise, filter, ordered compaction -----------------------------------------------------------------------------------
struct VoxelIsKept {
    VoxelArgs a;
    __device__ bool operator()(int64_t v) const
    {
        if (v >= a.n_vox) return false;
        const int64_t *acc = a.acc + v * kVoxelAccWords;
        return acc[9] >= a.min_points && __popcll((unsigned long long)acc[10]) >= a.min_tags;
    }
};

// Voxel ids ascend with the key, so the block offsets plus the kept voxels before this one in the block give the key order.
__global__ __launch_bounds__(256) void voxel_write_kernel(VoxelArgs a)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = VoxelIsKept{a}(v);
    const int incl = block_inclusive_count(keep);
    if (!keep) return;
    const int64_t dst = (int64_t)a.keep_count[blockIdx.x] + incl - 1;
    const int64_t *acc = a.acc + v * kVoxelAccWords;
    const uint64_t key = a.vox_key[v];
    const int64_t k = acc[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double cell = (double)(int64_t)((key >> (21 * c)) & 0x1FFFFFull);
        a.out_xyz[3 * dst + c] = (float)((double)a.o[c] + (cell + ((double)acc[c] / (double)k) / 1073741824.0) * (double)a.h);
    }
    if (a.out_rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out_rgb[3 * dst + c] = (uint8_t)((acc[3 + c] + k / 2) / k);
    }
    if (a.out_normals) {
        const double m0 = (double)acc[6], m1 = (double)acc[7], m2 = (double)acc[8];
        const double L = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
        const bool zero = L == 0.0;
        a.out_normals[3 * dst] = zero ? 0.f : (float)(m0 / L);
        a.out_normals[3 * dst + 1] = zero ? 0.f : (float)(m1 / L);
        a.out_normals[3 * dst + 2] = zero ? 0.f : (float)(m2 / L);
    }
    if (a.out_count) a.out_count[dst] = (int32_t)k;
    if (a.out_tagmask) a.out_tagmask[dst] = (uint64_t)acc[10];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
int launch_voxel_bounds(hipStream_t st, const float *xyz, int n, VoxelBounds *partials, int *n_partials)
{
    const unsigned g = blocks_of(n) < (unsigned)kVoxelBoundsBlocks ? blocks_of(n) : (unsigned)kVoxelBoundsBlocks;
    *n_partials = (int)g;
    hipLaunchKernelGGL(voxel_bounds_kernel, dim3(g), dim3(256), 0, st, xyz, n, partials);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_voxel_keys(hipStream_t st, const VoxelArgs &a, uint64_t *keys, int32_t *index)
{
    hipLaunchKernelGGL(voxel_keys_kernel, dim3(blocks_of(a.n)), dim3(256), 0, st, a, keys, index);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_voxel_heads(hipStream_t st, const VoxelArgs &a)
{
    return launch_flag_offsets(st, a.n_valid, VoxelIsHead{a}, a.head_count);
}

int launch_voxel_accumulate(hipStream_t st, const VoxelArgs &a)
{
    hipLaunchKernelGGL(voxel_accumulate_kernel, dim3(blocks_of(a.n_valid)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_voxel_finalise(hipStream_t st, const VoxelArgs &a)
{
    if (int rc = launch_flag_offsets(st, a.n_vox, VoxelIsKept{a}, a.keep_count)) return rc;
    hipLaunchKernelGGL(voxel_write_kernel, dim3(blocks_of(a.n_vox)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
