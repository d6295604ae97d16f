// One entry of the matchers' pair table: what the host plan (match_plan.hpp) writes and every matcher kernel reads.  No HIP.
#pragma once

#include <cstdint>

namespace esfm {

// One image pair of the pair loop (cpp_code/test/sfm.cpp:140-161), rows counted in the
// concatenated descriptor buffer.
struct PairDesc {
    int32_t q_row0, nq;   // query set: first row, row count
    int32_t t_row0, nt;   // train set
    int64_t out_off;      // first output slot of this pair (exclusive prefix sum of nq)
    int32_t blk_off;      // first workgroup of this pair in the knn launch
    int32_t blk_off2;     // ... in the launch of the one-product front pass (l2_x1_query_block() queries per workgroup)
};

}  // namespace esfm
