// C-ABI entry points of the homography model of two-view verification (include/esfm.h "Homography RANSAC"): RANSAC with the semantics
// of cv::findHomography(pts1, pts2, RANSAC, threshold, mask, 2000, confidence) without its final Levenberg-Marquardt polish.
//
// Host side: the cv::RNG sample stream with getSubset's subset check and the registrator's replay over the inlier counts the GPU produced
// for a chunk of iterations of every pair at once, both ransac_host.hpp's (fill_round / replay_round).  Everything that touches the
// correspondences -- the 4-point solve, the float transfer error, masks, the re-fit's sums and its eigenvector -- runs in
// homography_kernels.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "homography_core.hpp"
#include "homography_kernels.hpp"
#include "ransac_host.hpp"
#include "ransac_kernels.hpp"   // check_pair_args, launch_ransac_take_best
#include "scratch_layout.hpp"

using esfm::HomogPair;
using namespace esfm::ransac;   // CvRng, draw_subset, Registrator, fill_round, replay_round, RoundTables, the constants

namespace {

constexpr int kChunk = 64;            // iterations of every active pair evaluated per round

// Scratch of esfm_find_homography_pairs.  t: the rounds' int32 tables (one model per slot, n_models = the kernels' has_model), element
// offsets into stage_d and into its pinned mirror alike; `ok` (the re-fit's flags) follows them on the device only.  The rest: byte
// offsets into stage_e on 256-byte boundaries; best | refit is one array because one memset clears both.
struct HomogLayout {
    RoundTables t;
    size_t ok, ints;
    size_t models, best_refit, mask, bytes_e;
    HomogLayout(int n_pairs, int chunk, int n_total) : t(n_pairs, chunk, kFourPoints, 1), ok(t.end), ints(t.end + (size_t)n_pairs)
    {
        esfm::ScratchCarver c;
        models = c.take(sizeof(double) * 9 * t.n_slots); best_refit = c.take(sizeof(double) * 18 * (size_t)n_pairs);
        mask = c.take((size_t)std::max(n_total, 1)); bytes_e = c.at;
    }
};

}  // namespace

extern "C" {

int esfm_find_homography_pairs(esfm_ctx *ctx, int n_pairs, const int32_t *point_offset, const float *pts1, const float *pts2, double threshold,
                               double confidence, double *H_out, uint8_t *mask, int32_t *status, int32_t *iterations, int32_t *n_inliers)
{
    if (int rc = esfm::check_pair_args(ctx, n_pairs, point_offset, pts1, pts2)) return rc;
    if (n_pairs == 0) return ESFM_OK;
    ESFM_REQUIRE(H_out && status, "NULL argument");
    const int n_total = point_offset[n_pairs];
    ESFM_REQUIRE(n_total == 0 || mask, "mask is NULL");
    ESFM_REQUIRE(confidence > 0.0 && confidence < 1.0, "confidence must be in (0, 1)");
    ESFM_REQUIRE(threshold >= 0.0 && std::isfinite(threshold), "threshold must be finite and not negative");
    hipStream_t st = ctx->stream;

    std::vector<Registrator> S;
    S.reserve((size_t)n_pairs);
    std::vector<HomogPair> tab((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        HomogPair &r = tab[(size_t)p];
        r.first = point_offset[p]; r.count = point_offset[p + 1] - point_offset[p]; r.active = 1;
        r.thresh_sq = (float)(threshold * threshold);
        status[p] = 0;
        if (iterations) iterations[p] = 0;
        if (n_inliers) n_inliers[p] = 0;
        for (int k = 0; k < 9; ++k) H_out[9 * (size_t)p + k] = 0.0;
        S.emplace_back(kFourPoints, kHomogMaxIters, r.count);
    }
    if (n_total > 0) memset(mask, 0, (size_t)n_total);

    const HomogLayout L(n_pairs, kChunk, n_total);
    const size_t np = (size_t)n_pairs, nt = (size_t)std::max(n_total, 1);
    if (int rc = ctx->stage_a.reserve(sizeof(float) * 2 * nt)) return rc;
    if (int rc = ctx->stage_b.reserve(sizeof(float) * 2 * nt)) return rc;
    if (int rc = ctx->stage_c.reserve(sizeof(HomogPair) * np)) return rc;
    if (int rc = ctx->stage_d.reserve(sizeof(int32_t) * L.ints)) return rc;
    if (int rc = ctx->stage_e.reserve(L.bytes_e)) return rc;
    if (int rc = ctx->pin_rounds(sizeof(int32_t) * L.t.end)) return rc;
    float *d_p1 = ctx->stage_a.as<float>(), *d_p2 = ctx->stage_b.as<float>();
    HomogPair *d_tab = ctx->stage_c.as<HomogPair>();
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

    const auto draw = [&](int p) {   // (the subset check needs the points, which the host has anyway)
        const int n = tab[(size_t)p].count;
        const float *a = pts1 + 2 * (size_t)tab[(size_t)p].first, *b = pts2 + 2 * (size_t)tab[(size_t)p].first;
        return [=](CvRng &rng, int32_t *idx) { return draw_subset(rng, n, a, b, idx); };
    };
    while (fill_round(S.data(), n_pairs, kChunk, h_t + L.t.samples, draw)) {
        for (int p = 0; p < n_pairs; ++p) tab[(size_t)p].active = S[(size_t)p].done ? 0 : 1;
        ESFM_HIP_TRY(esfm::copy_h2d(d_tab, tab.data(), sizeof(HomogPair) * np, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d_t + L.t.samples, h_t + L.t.samples, sizeof(int32_t) * kFourPoints * L.t.n_slots, st));
        if (int rc = esfm::launch_homography_chunk(st, d_tab, n_pairs, d_p1, d_p2, d_t + L.t.samples, kChunk, d_models, d_t + L.t.n_models, d_counts, ctx)) return rc;
        ESFM_HIP_TRY(esfm::copy_d2h(h_t + L.t.down, d_t + L.t.down, sizeof(int32_t) * L.t.down_len, st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
        const int n_take = replay_round(S.data(), n_pairs, point_offset, kChunk, h_t + L.t.n_models, h_t + L.t.counts, 1, confidence, h_t + L.t.take);
        if (n_take > 0) {
            ESFM_HIP_TRY(esfm::copy_h2d(d_t + L.t.take, h_t + L.t.take, sizeof(int32_t) * 3 * (size_t)n_take, st));
            if (int rc = esfm::launch_ransac_take_best(st, d_t + L.t.take, n_take, d_models, 9, d_best)) return rc;
        }
    }
    // masks of the winners, then the re-fit on them (pairs with a model and more than four points)
    std::vector<int32_t> ok((size_t)n_pairs, 0);
    std::vector<double> refit(9 * (size_t)n_pairs, 0.0);
    for (int p = 0; p < n_pairs; ++p) {
        status[p] = S[(size_t)p].max_good > 0 ? 1 : 0;
        if (iterations) iterations[p] = S[(size_t)p].iter;
        tab[(size_t)p].active = 1;
    }
    ESFM_HIP_TRY(esfm::copy_h2d(d_tab, tab.data(), sizeof(HomogPair) * (size_t)n_pairs, st));
    if (n_total > 0) {
        if (int rc = esfm::launch_homography_mask(st, d_tab, n_pairs, d_p1, d_p2, d_best, d_mask)) return rc;
        ESFM_HIP_TRY(esfm::copy_d2h(mask, d_mask, (size_t)n_total, st));
        for (int p = 0; p < n_pairs; ++p) tab[(size_t)p].active = (status[p] && !S[(size_t)p].exact) ? 1 : 0;
        ESFM_HIP_TRY(esfm::copy_h2d(d_tab, tab.data(), sizeof(HomogPair) * (size_t)n_pairs, st));   // (stream-ordered behind the mask kernel's read)
        if (int rc = esfm::launch_homography_refit(st, d_tab, n_pairs, d_p1, d_p2, d_mask, d_refit, d_ok)) return rc;
        ESFM_HIP_TRY(esfm::copy_d2h(refit.data(), d_refit, sizeof(double) * 9 * (size_t)n_pairs, st));
        ESFM_HIP_TRY(esfm::copy_d2h(ok.data(), d_ok, sizeof(int32_t) * (size_t)n_pairs, st));
    }
    ESFM_HIP_TRY(esfm::copy_d2h(H_out, d_best, sizeof(double) * 9 * (size_t)n_pairs, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    for (int p = 0; p < n_pairs; ++p) {
        const int n = tab[(size_t)p].count;
        uint8_t *m = mask + point_offset[p];
        if (!status[p]) {
            if (n > 0) memset(m, 0, (size_t)n);
            for (int k = 0; k < 9; ++k) H_out[9 * (size_t)p + k] = 0.0;
            continue;
        }
        if (S[(size_t)p].exact) memset(m, 1, (size_t)n);   // bestMask.setTo(1)
        else if (ok[(size_t)p]) for (int k = 0; k < 9; ++k) H_out[9 * (size_t)p + k] = refit[9 * (size_t)p + k];   // (else: the RANSAC winner stays)
    }
    if (n_inliers && n_total > 0) {
        // the correspondences within the threshold of the RETURNED model: the scoring kernel once more, one "iteration" per pair
        for (int p = 0; p < n_pairs; ++p) tab[(size_t)p].active = 1;
        ESFM_HIP_TRY(esfm::copy_h2d(d_tab, tab.data(), sizeof(HomogPair) * (size_t)n_pairs, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d_refit, H_out, sizeof(double) * 9 * (size_t)n_pairs, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d_ok, status, sizeof(int32_t) * (size_t)n_pairs, st));
        if (int rc = esfm::launch_homography_score(st, d_tab, n_pairs, d_p1, d_p2, 1, d_refit, d_ok, d_counts)) return rc;
        ESFM_HIP_TRY(esfm::copy_d2h(n_inliers, d_counts, sizeof(int32_t) * (size_t)n_pairs, st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
    }
    return ESFM_OK;
}

int esfm_find_homography(esfm_ctx *ctx, const float *pts1, const float *pts2, int n, double threshold, double confidence, double *H, uint8_t *mask,
                         int32_t *iterations)
{
    if (n < 0) { esfm::set_error("negative point count"); return ESFM_ERR_INVALID_ARG; }
    if (n < kFourPoints) { esfm::set_error("a homography needs at least 4 correspondences"); return ESFM_ERR_UNSUPPORTED; }
    const int32_t off[2] = {0, n};
    int32_t status = 0;
    if (int rc = esfm_find_homography_pairs(ctx, 1, off, pts1, pts2, threshold, confidence, H, mask, &status, iterations, nullptr)) return rc;
    if (!status) { esfm::set_error("no homography found (no sample passed the subset check, or no model with 4 inliers)"); return ESFM_ERR_NUMERIC; }
    return ESFM_OK;
}

// The minimal solver alone on the GPU: n_samples samples of four correspondences in pixels.
int esfm_homography_models(esfm_ctx *ctx, const double *q1, const double *q2, int n_samples, double *H_out, int32_t *has_model)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(n_samples >= 0, "negative sample count");
    if (n_samples == 0) return ESFM_OK;
    ESFM_REQUIRE(q1 && q2 && H_out && has_model, "NULL argument");
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)n_samples;
    std::vector<double> q(16 * n);
    for (size_t g = 0; g < n; ++g) for (int k = 0; k < 8; ++k) { q[16 * g + k] = q1[8 * g + k]; q[16 * g + 8 + k] = q2[8 * g + k]; }
    if (int rc = ctx->stage_e.reserve(sizeof(double) * (16 + 9) * n)) return rc;
    if (int rc = ctx->stage_d.reserve(sizeof(int32_t) * n)) return rc;
    double *d_q = ctx->stage_e.as<double>(), *d_models = d_q + 16 * n;
    int32_t *d_has = ctx->stage_d.as<int32_t>();
    ESFM_HIP_TRY(esfm::copy_h2d(d_q, q.data(), sizeof(double) * 16 * n, st));
    if (int rc = esfm::launch_homography_solve_samples(st, d_q, n_samples, d_models, d_has)) return rc;
    ESFM_HIP_TRY(esfm::copy_d2h(H_out, d_models, sizeof(double) * 9 * n, st));
    ESFM_HIP_TRY(esfm::copy_d2h(has_model, d_has, sizeof(int32_t) * n, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

// ... and the host build of the same header (no GPU)
int esfm_homography_models_host(const double *q1, const double *q2, int n_samples, double *H_out, int32_t *has_model)
{
    if (n_samples < 0 || (n_samples && !(q1 && q2 && H_out && has_model))) { esfm::set_error("esfm_homography_models_host: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    for (size_t g = 0; g < (size_t)n_samples; ++g) has_model[g] = esfm::homog::homography_from_4(q1 + 8 * g, q2 + 8 * g, H_out + 9 * g) ? 1 : 0;
    return ESFM_OK;
}

// Host-only: the re-fit on the masked points in the refit kernel's summation order.
int esfm_homography_refit_host(const float *pts1, const float *pts2, int n, const uint8_t *mask, double *H)
{
    if (n < 0 || !H || (n && !(pts1 && pts2))) { esfm::set_error("esfm_homography_refit_host: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    if (!esfm::homog::homography_refit_host(pts1, pts2, n, mask, H)) { esfm::set_error("no homography (fewer than 4 inliers or a degenerate system)"); return ESFM_ERR_NUMERIC; }
    return ESFM_OK;
}

// Host-only: the first n_samples 4-subsets getSubset emits for these correspondences, the subset check included.
int esfm_homography_sample_stream(const float *pts1, const float *pts2, int count, int n_samples, int32_t *idx, int64_t *redraws)
{
    if (count < kFourPoints || n_samples < 0 || !pts1 || !pts2 || (n_samples && !idx)) { esfm::set_error("esfm_homography_sample_stream: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    CvRng rng;
    if (redraws) *redraws = 0;
    for (int s = 0; s < n_samples; ++s)
        if (!draw_subset(rng, count, pts1, pts2, idx + 4 * (size_t)s, redraws)) { esfm::set_error("no subset passed the check in 1000 attempts (sample %d)", s); return ESFM_ERR_NUMERIC; }
    return ESFM_OK;
}

}  // extern "C"
