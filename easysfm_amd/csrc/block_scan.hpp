// Device-side primitives the stages of the dense chain share (fusion, voxel merge, TSDF mesh, mesh clean-up, simplification,
// texturing, seam levelling): the launch helpers, the in-block count and the binary search, and the ordered compaction's first
// half -- flags counted per 256 indices, the counts scanned into block offsets.  Included by the .hip files; the one kernel that is
// no template lives in block_scan.hip, a code object of its own, so a stage loads no other stage's kernels to reach it.
#pragma once

#include "common.hpp"

namespace esfm {

#define LAUNCH_OK() ESFM_HIP_TRY(hipGetLastError())

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// The number of threads of the 256-thread workgroup up to and including this one for which `flag` holds (every thread calls).
// The function owns one LDS array: a kernel calls it once, or puts a barrier between two calls.
__device__ inline int block_inclusive_count(bool flag)
{
    __shared__ int32_t per_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) per_wave[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += per_wave[w];
    return before + __popcll(b & ((2ull << lane) - 1ull));        // (lane 63: 2 << 63 wraps to 0, the mask is all ones)
}

// First index in sorted[0 .. n) whose key is >= key.
__device__ inline int64_t lower_bound(const uint64_t *sorted, int64_t n, uint64_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// block_scan.hip: one workgroup's exclusive scan of per-block counts (in place) and their total
int launch_block_offsets_scan(hipStream_t st, int32_t *block_count, int n_blocks, int32_t *total);

// `flag` is a functor over a stage's argument struct, bool operator()(int64_t i) const, false at and beyond the end of the list.
template <class Flag> __global__ __launch_bounds__(256) void block_flag_count_kernel(Flag flag, int32_t *blocks)
{
    const int n = __syncthreads_count(flag((int64_t)blockIdx.x * 256 + threadIdx.x));
    if (threadIdx.x == 0) blocks[blockIdx.x] = n;
}

// The first half of an ordered compaction of n >= 1 indices (the callers return before this for an empty list: no empty grid is
// launched): blocks[b] becomes the number of flagged indices before block b, blocks[blocks_of(n)] their total.  The write kernel
// that follows calls the same functor and puts a flagged index at blocks[blockIdx.x] + block_inclusive_count(flag) - 1.
template <class Flag> int launch_flag_offsets(hipStream_t st, int64_t n, Flag flag, int32_t *blocks)
{
    const unsigned nb = blocks_of(n);
    hipLaunchKernelGGL(block_flag_count_kernel<Flag>, dim3(nb), dim3(256), 0, st, flag, blocks);
    LAUNCH_OK();
    return launch_block_offsets_scan(st, blocks, (int)nb, blocks + nb);
}

}  // namespace esfm
