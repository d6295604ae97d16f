// C-ABI entry points of the uncalibrated start (include/esfm.h "Fundamental-matrix RANSAC"): 7-point RANSAC with the semantics of
// cv::findFundamentalMat(pts1, pts2, FM_RANSAC, threshold, confidence) where the rule list of esfm.h does not say otherwise, and the
// focal-length cost over fundamental matrices.
//
// Host side: the cv::RNG sample stream (no subset check) and the registrator's replay over the inlier counts the GPU produced for a
// chunk of iterations of every pair at once, both ransac_host.hpp's (fill_round / replay_round).  Everything that touches the
// correspondences -- the 7-point solve, the float epipolar error, masks, the re-fit's sums, its eigenvector and the rank-2 step --
// runs in fundamental_kernels.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "fundamental_core.hpp"
#include "fundamental_kernels.hpp"
#include "ransac_host.hpp"
#include "ransac_kernels.hpp"   // check_pair_args, launch_ransac_take_best
#include "scratch_layout.hpp"

using esfm::FundPair;
using namespace esfm::ransac;   // CvRng, draw_distinct, Registrator, fill_round, replay_round, RoundTables, the constants

namespace {

constexpr int kChunk = 64;            // iterations of every active pair evaluated per round
constexpr int kModels = 3;            // models per sample at most

// Scratch of esfm_find_fundamental_pairs, laid out like the homography's: t = the rounds' int32 tables (three models per slot); behind
// them, on the device only, `ok` (the re-fit's flags, one per pair; in the last scoring pass the model counts) and three counts per
// pair for that pass.  The rest: byte offsets into stage_e; best | refit is one array.
struct FundLayout {
    RoundTables t;
    size_t ok, ints;
    size_t models, best_refit, mask, bytes_e;
    FundLayout(int n_pairs, int chunk, int n_total) : t(n_pairs, chunk, kSevenPoints, kModels), ok(t.end), ints(t.end + 4 * (size_t)n_pairs)
    {
        esfm::ScratchCarver c;
        models = c.take(sizeof(double) * 27 * std::max(t.n_slots, (size_t)n_pairs)); best_refit = c.take(sizeof(double) * 18 * (size_t)n_pairs);
        mask = c.take((size_t)std::max(n_total, 1)); bytes_e = c.at;
    }
};

}  // namespace

extern "C" {

int esfm_find_fundamental_pairs(esfm_ctx *ctx, int n_pairs, const int32_t *point_offset, const float *pts1, const float *pts2, double threshold,
                                double confidence, double *F_out, uint8_t *mask, int32_t *status, int32_t *iterations, int32_t *n_inliers)
{
    if (int rc = esfm::check_pair_args(ctx, n_pairs, point_offset, pts1, pts2)) return rc;
    if (n_pairs == 0) return ESFM_OK;
    ESFM_REQUIRE(F_out && status, "NULL argument");
    const int n_total = point_offset[n_pairs];
    ESFM_REQUIRE(n_total == 0 || mask, "mask is NULL");
    ESFM_REQUIRE(confidence > 0.0 && confidence < 1.0, "confidence must be in (0, 1)");
    ESFM_REQUIRE(threshold >= 0.0 && std::isfinite(threshold), "threshold must be finite and not negative");
    hipStream_t st = ctx->stream;

    std::vector<Registrator> S;
    S.reserve((size_t)n_pairs);
    std::vector<FundPair> tab((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        FundPair &r = tab[(size_t)p];
        r.first = point_offset[p]; r.count = point_offset[p + 1] - point_offset[p]; r.active = 1;
        r.thresh_sq = (float)(threshold * threshold);
        status[p] = 0;
        if (iterations) iterations[p] = 0;
        if (n_inliers) n_inliers[p] = 0;
        for (int k = 0; k < 9; ++k) F_out[9 * (size_t)p + k] = 0.0;
        S.emplace_back(kSevenPoints, kFundamentalMaxIters, r.count);
    }
    if (n_total > 0) memset(mask, 0, (size_t)n_total);

    const FundLayout L(n_pairs, kChunk, n_total);
    const size_t np = (size_t)n_pairs, nt = (size_t)std::max(n_total, 1);
    if (int rc = ctx->stage_a.reserve(sizeof(float) * 2 * nt)) return rc;
    if (int rc = ctx->stage_b.reserve(sizeof(float) * 2 * nt)) return rc;
    if (int rc = ctx->stage_c.reserve(sizeof(FundPair) * np)) return rc;
    if (int rc = ctx->stage_d.reserve(sizeof(int32_t) * L.ints)) return rc;
    if (int rc = ctx->stage_e.reserve(L.bytes_e)) return rc;
    if (int rc = ctx->pin_rounds(sizeof(int32_t) * L.t.end)) return rc;
    float *d_p1 = ctx->stage_a.as<float>(), *d_p2 = ctx->stage_b.as<float>();
    FundPair *d_tab = ctx->stage_c.as<FundPair>();
    int32_t *d_t = ctx->stage_d.as<int32_t>(), *h_t = static_cast<int32_t *>(ctx->pinned_rounds);   // the same offsets L.t on both sides
    int32_t *d_counts = d_t + L.t.counts, *d_ok = d_t + L.ok;
    uint8_t *d_e = ctx->stage_e.as<uint8_t>();
    double *d_models = reinterpret_cast<double *>(d_e + L.models), *d_best = reinterpret_cast<double *>(d_e + L.best_refit), *d_refit = d_best + 9 * np;
    uint8_t *d_mask = d_e + L.mask;
    if (n_total > 0) {
        ESFM_HIP_TRY(esfm::copy_h2d(d_p1, pts1, sizeof(float) * 2 * (size_t)n_total, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d_p2, pts2, sizeof(float) * 2 * (size_t)n_total, st));
    }
    ESFM_HIP_TRY(hipMemsetAsync(d_best, 0, sizeof(double) * 18 * np, st));   // best | refit
    ESFM_HIP_TRY(hipMemsetAsync(d_ok, 0, sizeof(int32_t) * np, st));

    const auto draw = [&](int p) {
        const int n = tab[(size_t)p].count;
        return [=](CvRng &rng, int32_t *idx) { draw_distinct(rng, n, kSevenPoints, idx); return true; };
    };
    std::vector<int32_t> exact_take;
    while (fill_round(S.data(), n_pairs, kChunk, h_t + L.t.samples, draw)) {
        for (int p = 0; p < n_pairs; ++p) tab[(size_t)p].active = S[(size_t)p].done ? 0 : 1;
        ESFM_HIP_TRY(esfm::copy_h2d(d_tab, tab.data(), sizeof(FundPair) * np, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d_t + L.t.samples, h_t + L.t.samples, sizeof(int32_t) * kSevenPoints * L.t.n_slots, st));
        if (int rc = esfm::launch_fundamental_chunk(st, d_tab, n_pairs, d_p1, d_p2, d_t + L.t.samples, kChunk, d_models, d_t + L.t.n_models, d_counts, ctx)) return rc;
        ESFM_HIP_TRY(esfm::copy_d2h(h_t + L.t.down, d_t + L.t.down, sizeof(int32_t) * L.t.down_len, st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
        // n == 7: the seven points' model with the most inliers, the first in model order on ties (the registrator would take model 0)
        exact_take.clear();
        for (int p = 0; p < n_pairs; ++p) {
            Registrator &s = S[(size_t)p];
            if (s.done || !s.exact) continue;
            const size_t g0 = (size_t)kChunk * p;
            const int nm = h_t[L.t.n_models + g0];
            int best_m = -1, best_c = -1;
            for (int m = 0; m < nm; ++m) { const int c = h_t[L.t.counts + kModels * g0 + m]; if (c > best_c) { best_c = c; best_m = m; } }
            if (best_m >= 0) { s.max_good = tab[(size_t)p].count; exact_take.push_back(p); exact_take.push_back((int32_t)g0); exact_take.push_back(best_m); }
            s.done = true;
        }
        int n_take = replay_round(S.data(), n_pairs, point_offset, kChunk, h_t + L.t.n_models, h_t + L.t.counts, kModels, confidence, h_t + L.t.take);
        for (size_t e = 0; e < exact_take.size(); ++e) h_t[L.t.take + 3 * (size_t)n_take + e] = exact_take[e];
        n_take += (int)(exact_take.size() / 3);
        if (n_take > 0) {
            ESFM_HIP_TRY(esfm::copy_h2d(d_t + L.t.take, h_t + L.t.take, sizeof(int32_t) * 3 * (size_t)n_take, st));
            if (int rc = esfm::launch_ransac_take_best(st, d_t + L.t.take, n_take, d_models, 27, d_best)) return rc;
        }
    }
    // masks of the winners, then the re-fit on them
    std::vector<int32_t> ok((size_t)n_pairs, 0);
    std::vector<double> refit(9 * (size_t)n_pairs, 0.0);
    for (int p = 0; p < n_pairs; ++p) {
        status[p] = S[(size_t)p].max_good > 0 ? 1 : 0;
        if (iterations) iterations[p] = S[(size_t)p].iter;
        tab[(size_t)p].active = 1;
    }
    ESFM_HIP_TRY(esfm::copy_h2d(d_tab, tab.data(), sizeof(FundPair) * (size_t)n_pairs, st));
    if (n_total > 0) {
        if (int rc = esfm::launch_fundamental_mask(st, d_tab, n_pairs, d_p1, d_p2, d_best, d_mask)) return rc;
        ESFM_HIP_TRY(esfm::copy_d2h(mask, d_mask, (size_t)n_total, st));
        for (int p = 0; p < n_pairs; ++p) tab[(size_t)p].active = (status[p] && !S[(size_t)p].exact) ? 1 : 0;
        ESFM_HIP_TRY(esfm::copy_h2d(d_tab, tab.data(), sizeof(FundPair) * (size_t)n_pairs, st));   // (stream-ordered behind the mask kernel's read)
        if (int rc = esfm::launch_fundamental_refit(st, d_tab, n_pairs, d_p1, d_p2, d_mask, d_refit, d_ok)) return rc;
        ESFM_HIP_TRY(esfm::copy_d2h(refit.data(), d_refit, sizeof(double) * 9 * (size_t)n_pairs, st));
        ESFM_HIP_TRY(esfm::copy_d2h(ok.data(), d_ok, sizeof(int32_t) * (size_t)n_pairs, st));
    }
    ESFM_HIP_TRY(esfm::copy_d2h(F_out, d_best, sizeof(double) * 9 * (size_t)n_pairs, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    for (int p = 0; p < n_pairs; ++p) {
        const int n = tab[(size_t)p].count;
        uint8_t *m = mask + point_offset[p];
        if (!status[p]) {
            if (n > 0) memset(m, 0, (size_t)n);
            for (int k = 0; k < 9; ++k) F_out[9 * (size_t)p + k] = 0.0;
            continue;
        }
        if (S[(size_t)p].exact) memset(m, 1, (size_t)n);
        else if (ok[(size_t)p]) for (int k = 0; k < 9; ++k) F_out[9 * (size_t)p + k] = refit[9 * (size_t)p + k];   // (else: the RANSAC winner stays)
    }
    if (n_inliers && n_total > 0) {
        // the correspondences within the threshold of the RETURNED model: the scoring kernel once more, one "iteration" per pair.  Its
        // model table has 27 doubles and its counts three ints per slot: model 0 of slot p = the returned F.
        std::vector<double> slot(27 * np, 0.0);
        std::vector<int32_t> cnt3(3 * np, 0);
        for (int p = 0; p < n_pairs; ++p) { tab[(size_t)p].active = 1; for (int k = 0; k < 9; ++k) slot[27 * (size_t)p + k] = F_out[9 * (size_t)p + k]; }
        ESFM_HIP_TRY(esfm::copy_h2d(d_tab, tab.data(), sizeof(FundPair) * (size_t)n_pairs, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d_models, slot.data(), sizeof(double) * 27 * np, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d_ok, status, sizeof(int32_t) * np, st));
        if (int rc = esfm::launch_fundamental_score(st, d_tab, n_pairs, d_p1, d_p2, 1, d_models, d_ok, d_ok + np)) return rc;
        ESFM_HIP_TRY(esfm::copy_d2h(cnt3.data(), d_ok + np, sizeof(int32_t) * 3 * np, st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
        for (int p = 0; p < n_pairs; ++p) n_inliers[p] = status[p] ? cnt3[3 * (size_t)p] : 0;
    }
    return ESFM_OK;
}

int esfm_find_fundamental(esfm_ctx *ctx, const float *pts1, const float *pts2, int n, double threshold, double confidence, double *F, uint8_t *mask,
                          int32_t *iterations)
{
    if (n < 0) { esfm::set_error("negative point count"); return ESFM_ERR_INVALID_ARG; }
    if (n < kSevenPoints) { esfm::set_error("a fundamental matrix needs at least 7 correspondences"); return ESFM_ERR_UNSUPPORTED; }
    const int32_t off[2] = {0, n};
    int32_t status = 0;
    if (int rc = esfm_find_fundamental_pairs(ctx, 1, off, pts1, pts2, threshold, confidence, F, mask, &status, iterations, nullptr)) return rc;
    if (!status) { esfm::set_error("no fundamental matrix found (no model with 7 inliers)"); return ESFM_ERR_NUMERIC; }
    return ESFM_OK;
}

// The minimal solver alone on the GPU: n_samples samples of seven correspondences in pixels.
int esfm_fundamental_models(esfm_ctx *ctx, const double *q1, const double *q2, int n_samples, double *F_out, int32_t *n_models)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(n_samples >= 0, "negative sample count");
    if (n_samples == 0) return ESFM_OK;
    ESFM_REQUIRE(q1 && q2 && F_out && n_models, "NULL argument");
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)n_samples;
    std::vector<double> q(28 * n);
    for (size_t g = 0; g < n; ++g) for (int k = 0; k < 14; ++k) { q[28 * g + k] = q1[14 * g + k]; q[28 * g + 14 + k] = q2[14 * g + k]; }
    if (int rc = ctx->stage_e.reserve(sizeof(double) * (28 + 27) * n)) return rc;
    if (int rc = ctx->stage_d.reserve(sizeof(int32_t) * n)) return rc;
    double *d_q = ctx->stage_e.as<double>(), *d_models = d_q + 28 * n;
    int32_t *d_nm = ctx->stage_d.as<int32_t>();
    ESFM_HIP_TRY(esfm::copy_h2d(d_q, q.data(), sizeof(double) * 28 * n, st));
    if (int rc = esfm::launch_fundamental_solve_samples(st, d_q, n_samples, d_models, d_nm)) return rc;
    ESFM_HIP_TRY(esfm::copy_d2h(F_out, d_models, sizeof(double) * 27 * n, st));
    ESFM_HIP_TRY(esfm::copy_d2h(n_models, d_nm, sizeof(int32_t) * n, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

// ... and the host build of the same header (no GPU)
int esfm_fundamental_models_host(const double *q1, const double *q2, int n_samples, double *F_out, int32_t *n_models)
{
    if (n_samples < 0 || (n_samples && !(q1 && q2 && F_out && n_models))) { esfm::set_error("esfm_fundamental_models_host: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    for (size_t g = 0; g < (size_t)n_samples; ++g) n_models[g] = esfm::fundm::fundamental_from_7(q1 + 14 * g, q2 + 14 * g, F_out + 27 * g);
    return ESFM_OK;
}

// Host-only: the 8-point re-fit on the masked points in the refit kernel's summation order.
int esfm_fundamental_refit_host(const float *pts1, const float *pts2, int n, const uint8_t *mask, double *F)
{
    if (n < 0 || !F || (n && !(pts1 && pts2))) { esfm::set_error("esfm_fundamental_refit_host: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    if (!esfm::fundm::fundamental_refit_host(pts1, pts2, n, mask, F)) { esfm::set_error("no fundamental matrix (fewer than 8 inliers or a degenerate system)"); return ESFM_ERR_NUMERIC; }
    return ESFM_OK;
}

// Host-only: the first n_samples 7-subsets the RANSAC draws for `count` points.
int esfm_fundamental_sample_stream(int count, int n_samples, int32_t *idx)
{
    if (count < kSevenPoints || n_samples < 0 || (n_samples && !idx)) { esfm::set_error("esfm_fundamental_sample_stream: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    CvRng rng;
    for (int s = 0; s < n_samples; ++s) draw_distinct(rng, count, kSevenPoints, idx + 7 * (size_t)s);
    return ESFM_OK;
}

static int focal_cost_args(int n_pairs, const double *F, const double *weight, int n_cand, const double *cand, double *cost)
{
    ESFM_REQUIRE(n_pairs >= 1 && n_cand >= 0, "esfm_focal_cost: needs at least one pair and a non-negative candidate count");
    ESFM_REQUIRE(F && weight && (n_cand == 0 || (cand && cost)), "NULL argument");
    return ESFM_OK;
}

// cost[k] of the Mendonca-Cipolla measure over the pairs' fundamental matrices, one thread per (candidate, pair)
int esfm_focal_cost(esfm_ctx *ctx, int n_pairs, const double *F, const double *weight, double cx, double cy, int n_cand, const double *candidates,
                    double *cost_out)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = focal_cost_args(n_pairs, F, weight, n_cand, candidates, cost_out)) return rc;
    if (n_cand == 0) return ESFM_OK;
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const size_t np = (size_t)n_pairs, nc = (size_t)n_cand;
    if (int rc = ctx->stage_e.reserve(sizeof(double) * (10 * np + 2 * nc + np * nc))) return rc;
    double *d_F = ctx->stage_e.as<double>(), *d_w = d_F + 9 * np, *d_cand = d_w + np, *d_cost = d_cand + nc, *d_terms = d_cost + nc;
    ESFM_HIP_TRY(esfm::copy_h2d(d_F, F, sizeof(double) * 9 * np, st));
    ESFM_HIP_TRY(esfm::copy_h2d(d_w, weight, sizeof(double) * np, st));
    ESFM_HIP_TRY(esfm::copy_h2d(d_cand, candidates, sizeof(double) * nc, st));
    if (int rc = esfm::launch_focal_cost(st, n_pairs, d_F, d_w, cx, cy, n_cand, d_cand, d_terms, d_cost)) return rc;
    ESFM_HIP_TRY(esfm::copy_d2h(cost_out, d_cost, sizeof(double) * nc, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

int esfm_focal_cost_host(int n_pairs, const double *F, const double *weight, double cx, double cy, int n_cand, const double *candidates, double *cost_out)
{
    if (int rc = focal_cost_args(n_pairs, F, weight, n_cand, candidates, cost_out)) return rc;
    esfm::fundm::focal_cost_host(n_pairs, F, weight, cx, cy, n_cand, candidates, cost_out);
    return ESFM_OK;
}

}  // extern "C"
