// C-ABI entry points of epipolar-guided matching (include/esfm.h "Epipolar-guided matching").
// Host logic only: argument checks, the pair and geometry tables, scratch, kernel sequencing.  Nothing of the plain matcher's
// context state (esfm::MatchState) is touched: a buffer prepared with esfm_match_prepare_dev stays prepared across these calls.
#include <algorithm>
#include <cmath>
#include <vector>

#include "guided_kernels.hpp"
#include "match_plan.hpp"

using esfm::GuidedGeom;
using esfm::PairDesc;

namespace {

// What is guided in a guided call's plan: every forward pair's geometry.
struct GuidedPlan : esfm::PairPlan {
    std::vector<GuidedGeom> geom;   // one per forward pair
};

int check_filters(int use_ratio, double ratio, int cross_check)
{
    ESFM_REQUIRE(use_ratio == 0 || use_ratio == 1, "use_ratio must be 0 or 1");
    ESFM_REQUIRE(cross_check == 0 || cross_check == 1, "cross_check must be 0 or 1");
    ESFM_REQUIRE(use_ratio == 1 || cross_check == 1, "at least one of use_ratio and cross_check must be on");
    ESFM_REQUIRE(use_ratio == 0 || ratio == ratio, "ratio is NaN");
    return ESFM_OK;
}

int check_guided(esfm_ctx *ctx, esfm_metric metric, int width, double max_epipolar_px)
{
    if (int rc = esfm::check_metric_width(ctx, metric, width, "check_guided: descriptor width must be positive")) return rc;
    ESFM_REQUIRE(max_epipolar_px > 0.0, "max_epipolar_px must be positive (+inf allowed) and not NaN");
    if (int rc = esfm::check_hamming_width(metric, width)) return rc;
    return esfm::set_device(ctx);
}

// The pair table (out_offset: the forward pairs' prefix sum of nq) and every forward pair's geometry.
int make_plan(const int32_t *set_row_offset, int n_sets, const int32_t *pairs, int n_pairs, const double *E, const float *K4,
              double max_epipolar_px, bool mirror, int64_t *out_offset, GuidedPlan *plan)
{
    ESFM_REQUIRE(out_offset != nullptr, "out_offset is NULL");
    ESFM_REQUIRE(set_row_offset != nullptr && n_sets >= 1, "set_row_offset/n_sets");      // (first, as ever; make_plan looks again)
    ESFM_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || (pairs != nullptr && E != nullptr && K4 != nullptr)), "pairs/E/K4_per_pair/n_pairs");
    if (int rc = esfm::make_plan(set_row_offset, n_sets, pairs, n_pairs, esfm::kGuidedQueryBlock, 0, mirror, esfm::kGuidedPlanRules, out_offset, plan)) return rc;
    plan->geom.resize((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        GuidedGeom &gm = plan->geom[(size_t)p];
        for (int k = 0; k < 9; ++k) gm.E[k] = E[9 * (size_t)p + k];
        gm.fx = (double)K4[4 * p]; gm.cx = (double)K4[4 * p + 1]; gm.fy = (double)K4[4 * p + 2]; gm.cy = (double)K4[4 * p + 3];
        if (!(std::isfinite(gm.fx) && std::isfinite(gm.fy) && std::isfinite(gm.cx) && std::isfinite(gm.cy)) || gm.fx == 0.0 || gm.fy == 0.0) {
            esfm::set_error("bad camera intrinsics for pair %d", p);
            return ESFM_ERR_NUMERIC;
        }
        esfm::guided_set_threshold(gm, max_epipolar_px);
    }
    return ESFM_OK;
}

// Tables up, one launch: the guided 2-NN tables of every entry of the plan.
int knn2_core(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const float *kp_dev, int width, const GuidedPlan &plan,
              int32_t *knn_idx, float *knn_dist, int32_t *n_adm, const PairDesc **dev_tab_out)
{
    const size_t tab_bytes = plan.tab.size() * sizeof(PairDesc), geom_bytes = plan.geom.size() * sizeof(GuidedGeom);
    static_assert(sizeof(PairDesc) % 8 == 0, "the geometry table follows the pair table, 8-byte aligned");
    if (int rc = ctx->guided_tab.reserve(tab_bytes + geom_bytes)) return rc;
    char *base = ctx->guided_tab.as<char>();
    ESFM_HIP_TRY(esfm::copy_h2d(base, plan.tab.data(), tab_bytes, ctx->stream));
    ESFM_HIP_TRY(esfm::copy_h2d(base + tab_bytes, plan.geom.data(), geom_bytes, ctx->stream));
    // (the tables are pageable host memory: the copies have consumed them when they return)
    const PairDesc *dev_tab = reinterpret_cast<const PairDesc *>(base);
    if (dev_tab_out) *dev_tab_out = dev_tab;
    return esfm::launch_guided_knn2(ctx->stream, metric, width, desc_dev, kp_dev, dev_tab, (int)plan.tab.size(), plan.n_fwd,
                                    reinterpret_cast<const GuidedGeom *>(base + tab_bytes), plan.n_blocks, knn_idx, knn_dist, n_adm);
}

int match_lists_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const float *kp_dev, const int32_t *set_row_offset, int n_sets,
                    int width, const int32_t *pairs, int n_pairs, const double *E, const float *K4, double max_epipolar_px, int use_ratio,
                    double ratio, int cross_check, int32_t *query_idx_dev, int32_t *train_idx_dev, float *distance_dev, int32_t *n_out_dev,
                    int64_t *out_offset)
{
    if (int rc = check_guided(ctx, metric, width, max_epipolar_px)) return rc;
    if (int rc = check_filters(use_ratio, ratio, cross_check)) return rc;
    GuidedPlan plan;
    if (int rc = make_plan(set_row_offset, n_sets, pairs, n_pairs, E, K4, max_epipolar_px, cross_check != 0, out_offset, &plan)) return rc;
    if (n_pairs == 0) return ESFM_OK;
    ESFM_REQUIRE(n_out_dev != nullptr, "n_out_dev is NULL");
    if (plan.fwd_queries == 0) {
        ESFM_HIP_TRY(hipMemsetAsync(n_out_dev, 0, sizeof(int32_t) * (size_t)n_pairs, ctx->stream));
        return ESFM_OK;
    }
    ESFM_REQUIRE(desc_dev && kp_dev && query_idx_dev && train_idx_dev && distance_dev, "device pointer is NULL");
    if (int rc = ctx->guided_idx.reserve(sizeof(int32_t) * 2 * (size_t)plan.total_queries)) return rc;
    if (int rc = ctx->guided_dist.reserve(sizeof(float) * 2 * (size_t)plan.total_queries)) return rc;
    int32_t *knn_idx = ctx->guided_idx.as<int32_t>();
    float *knn_dist = ctx->guided_dist.as<float>();
    const PairDesc *dev_tab = nullptr;
    if (int rc = knn2_core(ctx, metric, desc_dev, kp_dev, width, plan, knn_idx, knn_dist, nullptr, &dev_tab)) return rc;
    // the filters are the plain matcher's, on the guided tables: a missing second neighbour (-1) fails the ratio test
    if (cross_check)
        return esfm::launch_cross_check_compact(ctx->stream, dev_tab, n_pairs, knn_idx, knn_dist, use_ratio, ratio, query_idx_dev, train_idx_dev,
                                                distance_dev, n_out_dev);
    return esfm::launch_ratio_compact(ctx->stream, dev_tab, n_pairs, knn_idx, knn_dist, ratio, query_idx_dev, train_idx_dev, distance_dev, n_out_dev);
}

// Host pointers in and out: upload once, one launch sequence, the lists packed on the device before the read-back.
int match_pairs_host(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const float *kp_host, const int32_t *set_row_offset, int n_sets,
                     int width, const int32_t *pairs, int n_pairs, const double *E, const float *K4, double max_epipolar_px, int use_ratio,
                     double ratio, int cross_check, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out, int64_t *out_offset)
{
    if (int rc = check_guided(ctx, metric, width, max_epipolar_px)) return rc;
    if (int rc = check_filters(use_ratio, ratio, cross_check)) return rc;
    {
        GuidedPlan plan;      // (argument checks and out_offset before anything is uploaded)
        if (int rc = make_plan(set_row_offset, n_sets, pairs, n_pairs, E, K4, max_epipolar_px, false, out_offset, &plan)) return rc;
    }
    if (n_pairs == 0) return ESFM_OK;
    ESFM_REQUIRE(n_out != nullptr, "n_out is NULL");
    for (int p = 0; p < n_pairs; ++p) n_out[p] = 0;
    const size_t nq = (size_t)out_offset[n_pairs];
    if (nq == 0) return ESFM_OK;
    ESFM_REQUIRE(desc_host && kp_host && query_idx && train_idx && distance, "host pointer is NULL");
    hipStream_t st = ctx->stream;
    const size_t rows = (size_t)set_row_offset[n_sets];
    if (int rc = ctx->guided_bank.reserve(esfm::match_row_bytes(metric, width) * rows + 16)) return rc;
    if (int rc = ctx->guided_kp.reserve(sizeof(float) * 2 * rows + 16)) return rc;
    ESFM_HIP_TRY(esfm::copy_h2d(ctx->guided_bank.ptr, desc_host, esfm::match_row_bytes(metric, width) * rows, st));
    ESFM_HIP_TRY(esfm::copy_h2d(ctx->guided_kp.ptr, kp_host, sizeof(float) * 2 * rows, st));
    if (int rc = esfm::reserve_match_list_stage(ctx, nq, n_pairs)) return rc;
    std::vector<int64_t> off2((size_t)n_pairs + 1);
    if (int rc = match_lists_dev(ctx, metric, ctx->guided_bank.ptr, ctx->guided_kp.as<float>(), set_row_offset, n_sets, width, pairs, n_pairs, E, K4,
                                 max_epipolar_px, use_ratio, ratio, cross_check, ctx->stage_b.as<int32_t>(), ctx->stage_c.as<int32_t>(),
                                 ctx->stage_d.as<float>(), ctx->stage_e.as<int32_t>(), off2.data()))
        return rc;
    // packed read-back (as esfm_match_pairs, always packed): the transfer is proportional to the matches, not to the queries
    return esfm::read_back_match_lists(ctx, n_pairs, off2.data(), nq, false, query_idx, train_idx, distance, n_out);
}

// One pair through the host-pointer form: sets [train rows | query rows], the pair (1, 0).
int single_pair(esfm_ctx *ctx, esfm_metric metric, const void *q, const float *kp_q, int nq, const void *t, const float *kp_t, int nt, int width,
                const double *E, const float *K4, double max_epipolar_px, int use_ratio, double ratio, int cross_check, int32_t *query_idx,
                int32_t *train_idx, float *distance, int32_t *n_out)
{
    if (int rc = check_guided(ctx, metric, width, max_epipolar_px)) return rc;
    ESFM_REQUIRE(n_out != nullptr, "n_out is NULL");
    ESFM_REQUIRE(nq >= 0 && nt >= 0, "negative row count");
    ESFM_REQUIRE(nq == 0 || (q && kp_q), "q / kp_q is NULL");
    ESFM_REQUIRE(nt == 0 || (t && kp_t), "t / kp_t is NULL");
    ESFM_REQUIRE(nq == 0 || (query_idx && train_idx && distance), "output pointer is NULL");
    *n_out = 0;
    const size_t rb = esfm::match_row_bytes(metric, width);
    std::vector<char> bank(rb * ((size_t)nt + (size_t)nq) + 1);
    std::vector<float> kps(2 * ((size_t)nt + (size_t)nq) + 1);
    if (nt) { memcpy(bank.data(), t, rb * (size_t)nt); memcpy(kps.data(), kp_t, sizeof(float) * 2 * (size_t)nt); }
    if (nq) { memcpy(bank.data() + rb * (size_t)nt, q, rb * (size_t)nq); memcpy(kps.data() + 2 * (size_t)nt, kp_q, sizeof(float) * 2 * (size_t)nq); }
    const int32_t offs[3] = {0, nt, nt + nq};
    const int32_t pr[2] = {1, 0};
    int64_t out_off[2];
    return match_pairs_host(ctx, metric, bank.data(), kps.data(), offs, 2, width, pr, 1, E, K4, max_epipolar_px, use_ratio, ratio, cross_check, query_idx,
                            train_idx, distance, n_out, out_off);
}

}  // namespace

extern "C" {

int esfm_match_guided_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const float *kp_dev, const int32_t *set_row_offset,
                                int n_sets, int width, const int32_t *pairs, int n_pairs, const double *E, const float *K4_per_pair,
                                double max_epipolar_px, int use_ratio, double ratio, int cross_check, int32_t *query_idx_dev,
                                int32_t *train_idx_dev, float *distance_dev, int32_t *n_out_dev, int64_t *out_offset)
{
    return match_lists_dev(ctx, metric, desc_dev, kp_dev, set_row_offset, n_sets, width, pairs, n_pairs, E, K4_per_pair, max_epipolar_px, use_ratio,
                           ratio, cross_check, query_idx_dev, train_idx_dev, distance_dev, n_out_dev, out_offset);
}

int esfm_match_guided_pairs(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const float *kp_host, const int32_t *set_row_offset,
                            int n_sets, int width, const int32_t *pairs, int n_pairs, const double *E, const float *K4_per_pair,
                            double max_epipolar_px, int use_ratio, double ratio, int cross_check, int32_t *query_idx, int32_t *train_idx,
                            float *distance, int32_t *n_out, int64_t *out_offset)
{
    return match_pairs_host(ctx, metric, desc_host, kp_host, set_row_offset, n_sets, width, pairs, n_pairs, E, K4_per_pair, max_epipolar_px, use_ratio,
                            ratio, cross_check, query_idx, train_idx, distance, n_out, out_offset);
}

int esfm_knn2_guided_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const float *kp_dev, const int32_t *set_row_offset,
                               int n_sets, int width, const int32_t *pairs, int n_pairs, const double *E, const float *K4_per_pair,
                               double max_epipolar_px, int32_t *knn_idx_dev, float *knn_dist_dev, int32_t *n_adm_dev, int64_t *out_offset)
{
    if (int rc = check_guided(ctx, metric, width, max_epipolar_px)) return rc;
    GuidedPlan plan;
    if (int rc = make_plan(set_row_offset, n_sets, pairs, n_pairs, E, K4_per_pair, max_epipolar_px, false, out_offset, &plan)) return rc;
    if (plan.total_queries == 0) return ESFM_OK;
    ESFM_REQUIRE(desc_dev && kp_dev && knn_idx_dev && knn_dist_dev, "device pointer is NULL");
    return knn2_core(ctx, metric, desc_dev, kp_dev, width, plan, knn_idx_dev, knn_dist_dev, n_adm_dev, nullptr);
}

int esfm_match_guided_l2_f32(esfm_ctx *ctx, const float *q, const float *kp_q, int nq, const float *t, const float *kp_t, int nt, int dim,
                             const double *E, const float *K4, double max_epipolar_px, int use_ratio, double ratio, int cross_check,
                             int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    return single_pair(ctx, ESFM_L2_F32, q, kp_q, nq, t, kp_t, nt, dim, E, K4, max_epipolar_px, use_ratio, ratio, cross_check, query_idx, train_idx,
                       distance, n_out);
}

int esfm_match_guided_hamming(esfm_ctx *ctx, const uint8_t *q, const float *kp_q, int nq, const uint8_t *t, const float *kp_t, int nt, int nbytes,
                              const double *E, const float *K4, double max_epipolar_px, int use_ratio, double ratio, int cross_check,
                              int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    return single_pair(ctx, ESFM_HAMMING, q, kp_q, nq, t, kp_t, nt, nbytes, E, K4, max_epipolar_px, use_ratio, ratio, cross_check, query_idx,
                       train_idx, distance, n_out);
}

}  // extern "C"
