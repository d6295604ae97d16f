// The pair plan of a matcher call (host side, no GPU): the pair table the kernels walk, its two workgroup numberings, the tables of
// the one-product front pass and the mirrored second half of the cross-check -- built once, for the plain matcher (match_api.cpp)
// and the guided one (guided_api.cpp) -- and the argument rules both share.  Pure arithmetic on the caller's set offsets and pair
// list: match_plan.cpp includes no HIP header, and tests/cpp/match_plan_check.cpp states what the kernels rely on in these tables.
#pragma once

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

// ctx, metric and width as every matcher entry point checks them, in this order (width_msg: the text of a width <= 0)
int check_metric_width(const esfm_ctx *ctx, esfm_metric metric, int width, const char *width_msg);

// the descriptor widths the Hamming kernels are built for, and what every entry point says about another one
inline bool hamming_supported(int nbytes) { return nbytes == 16 || nbytes == 32 || nbytes == 64; }
int check_hamming_width(esfm_metric metric, int width);

inline size_t match_row_bytes(esfm_metric metric, int width) { return metric == ESFM_L2_F32 ? sizeof(float) * (size_t)width : (size_t)width; }

}  // namespace esfm
