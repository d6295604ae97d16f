// The mesh clean-up's library call: rocPRIM's device radix sort (through hipCUB) of 64-bit keys alone -- the directed edge keys
// and the (vertex, corner) incidence keys.  A translation unit of its own for the reason cloud_sort.hip gives: the sort's kernel
// instantiations make a code object that is loaded with the first launch of any of its kernels, and only esfm_mesh_clean should
// pay for this one.  The keys' high word is a vertex index, so the sort stops at the bit the caller names.
#include <hipcub/hipcub.hpp>

#include "mesh_kernels.hpp"

namespace esfm {

int mesh_sort_scratch_bytes(int64_t n, int end_bit, size_t *bytes, hipStream_t st)
{
    *bytes = 0;
    ESFM_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, *bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, 0, end_bit, st));
    return ESFM_OK;
}

int mesh_sort_keys(void *tmp, size_t tmp_bytes, const uint64_t *keys_in, uint64_t *keys_out, int64_t n, int end_bit, hipStream_t st)
{
    ESFM_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, keys_in, keys_out, (int)n, 0, end_bit, st));
    return ESFM_OK;
}

}  // namespace esfm
