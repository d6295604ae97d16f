// The pair plan of a matcher call (host side, no GPU): the pair table the kernels walk, its two workgroup numberings, the tables of
// the one-product front pass and the mirrored second half of the cross-check -- built once, for the plain matcher (match_api.cpp)
// and the guided one (guided_api.cpp) -- and the argument rules both share.  Pure arithmetic on the caller's set offsets and pair
// list: match_plan.cpp includes no HIP header, and tests/cpp/match_plan_check.cpp states what the kernels rely on in these tables.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#include "error.hpp"
#include "pair_desc.hpp"

namespace esfm {

// What differs between the two matchers' plans: the row limits (a set of that many rows or more is refused) with their messages.
struct PlanRules { int32_t nt_limit, nq_limit; const char *nt_msg, *nq_msg; };
// plain: a train index has 21 bits in the packed top-2 keys, a set is addressed with 32-bit byte offsets (buffer descriptors)
constexpr PlanRules kPlainPlanRules{1 << 21, 1 << 23, "train sets are limited to 2^21-1 rows", "query sets are limited to 2^23-1 rows"};
// guided: either set in the 21-bit row field of the queue entries and keys
constexpr PlanRules kGuidedPlanRules{1 << 21, 1 << 21, "sets are limited to 2^21-1 rows", "sets are limited to 2^21-1 rows"};

struct PairPlan {
    std::vector<PairDesc> tab;       // the P forward pairs; with `mirror`, followed by their P mirrors
    std::vector<int32_t> blk_pair;   // the pair of every block of the second numbering (the front pass's workgroups look their work up here)
    std::vector<int32_t> by_train;   // pair indices sorted by train set (l2_finish_kernel walks the pairs in this order: the workgroups that
                                     // fetch rows of one train set run next to each other, on one XCD, and find them in its L2)
    int n_fwd = 0;
    int n_blocks = 0, n_blocks2 = 0;   // workgroups of the two numberings
    int max_nt = 0;
    int64_t fwd_queries = 0, total_queries = 0;   // sum of nq over the forward pairs / over the whole table
    int64_t total_rows = 0;
};

// query_block: queries per workgroup of the knn launch (blk_off); query_block2: ... of the front pass (blk_off2) -- 0: no second
// numbering and no blk_pair / by_train tables; mirror: entry P + p is pair p with query and train swapped (the cross-check: one pass,
// both directions).  out_offset (may be NULL): P + 1 entries, the forward pairs' exclusive prefix sum of nq and its total -- of a
// mirrored plan too, whose second half continues the numbering behind it.  *plan is overwritten as a whole.
int make_plan(const int32_t *set_row_offset, int n_sets, const int32_t *pairs, int n_pairs, int query_block, int query_block2, bool mirror,
              const PlanRules &rules, int64_t *out_offset, PairPlan *plan);

// The grid of the fused L2 launch (l2_fused_kernel, match_kernels.hip): the front pass's n_blocks2 blocks, one workgroup each, padded
// to a multiple of 8 -- workgroups are dealt round-robin over the 8 XCDs, so the finish role's workgroup k lands on XCD k % 8 as in a
// launch of its own -- then `slices` finish workgroups per pair.  Workgroup w: w < n_pass a pass block, w < n_pad padding (returns at
// once), else finish workgroup w - n_pad.  A pair's finish workgroups wait until pair_blocks2() pass blocks have counted themselves:
// that is the number of entries of blk_pair that name the pair, blk_off2[p + 1] - blk_off2[p] (tests/cpp/match_fused_grid_check.cpp).
struct FusedGrid { int n_pass = 0, slices = 0; int64_t n_pad = 0, total = 0; };
inline FusedGrid fused_grid_of(int n_blocks2, int n_pairs, int slices)
{
    FusedGrid g;
    g.n_pass = n_blocks2;
    g.n_pad = ((int64_t)n_blocks2 + 7) / 8 * 8;
    g.slices = slices;
    g.total = g.n_pad + (int64_t)n_pairs * slices;      // (the launcher refuses 2^31 and more)
    return g;
}
// finish workgroups per pair of the fused launch: about two rounds of its 2 x 256 slots (measured on 300 pairs of 4096 x 4096: 1 slice
// 0.530 ms per step, 2: 0.517, 3: 0.512, 4: 0.516, 7 -- the two-launch default -- 0.524: a finish workgroup's fixed costs weigh more at
// two per CU, beside pass blocks, than at three per CU with the chip to itself)
inline int fused_slices_default(int n_pairs) { return std::max(1, std::min(8, 1024 / std::max(n_pairs, 1))); }
inline int pair_blocks2(const PairDesc &d, int query_block2) { return (int)(((int64_t)d.nq + query_block2 - 1) / query_block2); }

// ctx, metric and width as every matcher entry point checks them, in this order (width_msg: the text of a width <= 0)
int check_metric_width(const esfm_ctx *ctx, esfm_metric metric, int width, const char *width_msg);

// the descriptor widths the Hamming kernels are built for, and what every entry point says about another one
inline bool hamming_supported(int nbytes) { return nbytes == 16 || nbytes == 32 || nbytes == 64; }
int check_hamming_width(esfm_metric metric, int width);

inline size_t match_row_bytes(esfm_metric metric, int width) { return metric == ESFM_L2_F32 ? sizeof(float) * (size_t)width : (size_t)width; }

}  // namespace esfm
