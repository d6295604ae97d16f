// The pair plan and the shared argument rules of the matcher entry points (match_plan.hpp).  Host only: no HIP header.
#include "match_plan.hpp"

#include <algorithm>

namespace esfm {

int make_plan(const int32_t *set_row_offset, int n_sets, const int32_t *pairs, int n_pairs, int query_block, int query_block2, bool mirror,
              const PlanRules &rules, int64_t *out_offset, PairPlan *plan)
{
    ESFM_REQUIRE(set_row_offset != nullptr && n_sets >= 1, "set_row_offset/n_sets");
    ESFM_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || pairs != nullptr), "pairs/n_pairs");
    ESFM_REQUIRE(set_row_offset[0] == 0, "set_row_offset[0] must be 0");
    for (int s = 0; s < n_sets; ++s) ESFM_REQUIRE(set_row_offset[s + 1] >= set_row_offset[s], "set_row_offset must be non-decreasing");
    const bool tables = query_block2 > 0;
    *plan = PairPlan{};
    plan->total_rows = set_row_offset[n_sets];
    plan->n_fwd = n_pairs;
    plan->tab.resize((size_t)n_pairs * (mirror ? 2 : 1));
    int64_t off = 0, blk = 0, blk2 = 0;
    for (size_t g = 0; g < plan->tab.size(); ++g) {
        const int p = (int)(g % (size_t)n_pairs);
        const bool rev = g >= (size_t)n_pairs;      // the mirror of pair p: the roles swapped
        const int qs = pairs[2 * p + (rev ? 1 : 0)], ts = pairs[2 * p + (rev ? 0 : 1)];
        ESFM_REQUIRE(qs >= 0 && qs < n_sets && ts >= 0 && ts < n_sets, "pair refers to a set out of range");
        PairDesc &d = plan->tab[g];
        d.q_row0 = set_row_offset[qs]; d.nq = set_row_offset[qs + 1] - set_row_offset[qs];
        d.t_row0 = set_row_offset[ts]; d.nt = set_row_offset[ts + 1] - set_row_offset[ts];
        ESFM_REQUIRE(d.nt < rules.nt_limit, rules.nt_msg);
        ESFM_REQUIRE(d.nq < rules.nq_limit, rules.nq_msg);
        d.out_off = off; d.blk_off = (int32_t)blk; d.blk_off2 = (int32_t)blk2;
        plan->max_nt = std::max(plan->max_nt, (int)d.nt);
        if (!rev && out_offset) out_offset[p] = off;
        off += d.nq;
        blk += (d.nq + query_block - 1) / query_block;
        if (tables) blk2 += (d.nq + query_block2 - 1) / query_block2;
        ESFM_REQUIRE(blk < (int64_t)1 << 31, "too many workgroups for one launch; split the pair list");
        plan->blk_pair.resize((size_t)blk2, (int32_t)g);
        if (g + 1 == (size_t)n_pairs) plan->fwd_queries = off;
    }
    if (out_offset) out_offset[n_pairs] = plan->fwd_queries;
    plan->by_train.resize(tables ? plan->tab.size() : 0);
    for (size_t g = 0; g < plan->by_train.size(); ++g) plan->by_train[g] = (int32_t)g;
    std::stable_sort(plan->by_train.begin(), plan->by_train.end(),
                     [&](int32_t a, int32_t b) { return plan->tab[(size_t)a].t_row0 < plan->tab[(size_t)b].t_row0; });
    plan->n_blocks = (int)blk;
    plan->n_blocks2 = (int)blk2;
    plan->total_queries = off;
    return ESFM_OK;
}

int check_metric_width(const esfm_ctx *ctx, esfm_metric metric, int width, const char *width_msg)
{
    if (!ctx) { set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (metric != ESFM_L2_F32 && metric != ESFM_HAMMING) { set_error("unknown metric %d", (int)metric); return ESFM_ERR_INVALID_ARG; }
    if (width <= 0) { set_error("%s", width_msg); return ESFM_ERR_INVALID_ARG; }
    return ESFM_OK;
}

int check_hamming_width(esfm_metric metric, int width)
{
    if (metric != ESFM_HAMMING || hamming_supported(width)) return ESFM_OK;
    set_error("hamming descriptors must be 16, 32 or 64 bytes (got %d)", width); return ESFM_ERR_UNSUPPORTED;
}

}  // namespace esfm
