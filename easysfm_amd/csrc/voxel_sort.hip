// The voxel merge's library call: rocPRIM's device radix sort (through hipCUB) of the cloud's (64-bit cell key, point index) pairs.
// A translation unit of its own for the reason cloud_sort.hip gives: the sort's kernel instantiations make a code object that is
// loaded with the first launch of any of its kernels, and only esfm_cloud_voxel_merge should pay for this one.
#include <hipcub/hipcub.hpp>

#include "voxel_kernels.hpp"

namespace esfm {

int voxel_sort_scratch_bytes(int n, size_t *bytes, hipStream_t st)
{
    *bytes = 0;
    ESFM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr, n, 0, 64, st));
    return ESFM_OK;
}

int voxel_sort_pairs(void *tmp, size_t tmp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const int32_t *idx_in, int32_t *idx_out, int n,
                     hipStream_t st)
{
    ESFM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys_in, keys_out, idx_in, idx_out, n, 0, 64, st));
    return ESFM_OK;
}

}  // namespace esfm
