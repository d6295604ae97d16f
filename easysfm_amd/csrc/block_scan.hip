// The block-offsets scan of the ordered compactions (block_scan.hpp), in a translation unit of its own: a code object is loaded
// with the first launch of any of its kernels, and every stage of the dense chain launches this one.
#include "block_scan.hpp"

namespace esfm {

// One workgroup: the exclusive scan of the block counts (in place) and the total.
__global__ __launch_bounds__(1024) void block_offsets_scan_kernel(int32_t *block_count, int n_blocks, int32_t *n_points)
{
    __shared__ int32_t part[1024];
    const int tid = threadIdx.x;
    const int per = (n_blocks + 1023) / 1024, b0 = tid * per, b1 = min(b0 + per, n_blocks);
    int32_t s = 0;
    for (int b = b0; b < b1; ++b) s += block_count[b];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int32_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int32_t run = part[tid] - s;                     // exclusive prefix of this thread's chunk
    for (int b = b0; b < b1; ++b) { const int32_t c = block_count[b]; block_count[b] = run; run += c; }
    if (tid == 1023) *n_points = part[1023];
}

int launch_block_offsets_scan(hipStream_t st, int32_t *block_count, int n_blocks, int32_t *total)
{
    hipLaunchKernelGGL(block_offsets_scan_kernel, dim3(1), dim3(1024), 0, st, block_count, n_blocks, total);
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
