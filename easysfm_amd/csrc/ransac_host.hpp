// Host side of OpenCV's RANSAC point-set registrator, shared by the essential-matrix, the homography and the PnP entry points
// [upstream opencv/modules/calib3d/src/ptsetreg.cpp, modules/core/include/opencv2/core/operations.hpp]: the cv::RNG recurrence,
// getSubset's sampling rules, RANSACUpdateNumIters, and RANSACPointSetRegistrator::run replayed over rounds of `chunk` iterations whose
// inlier counts come from elsewhere (the GPU; a table in tests/cpp/ransac_rounds_check_main.cpp).  Pure host arithmetic over plain
// arrays: no HIP call, no esfm_ctx.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace esfm {
namespace ransac {

constexpr int kFivePoints = 5;           // the 5-point essential kernel and solvePnPRansac's EPnP kernel draw 5
constexpr int kFourPoints = 4;           // the homography model (esfm.h "Homography RANSAC") draws 4
constexpr int kSevenPoints = 7;          // the fundamental matrix (esfm.h "Fundamental-matrix RANSAC") draws 7
constexpr int kEssentialMaxIters = 1000; // RANSACPointSetRegistrator default (findEssentialMat does not override it)
constexpr int kHomogMaxIters = 2000;     // cv::findHomography's maxIters default
constexpr int kFundamentalMaxIters = 1000; // the registrator's default, as for the essential matrix
constexpr int kSubsetAttempts = 1000;    // getSubset's maxAttempts

struct CvRng {                        // cv::RNG((uint64)-1)
    uint64_t state = 0xFFFFFFFFFFFFFFFFull;
    unsigned next() { state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32); return (unsigned)state; }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

// getSubset's inner loop: m distinct indices below count, a repeat is redrawn
inline void draw_distinct(CvRng &rng, int count, int m, int32_t *idx)
{
    for (int i = 0; i < m;) {
        int v;
        for (;;) {
            v = idx[i] = rng.uniform(0, count);
            int j = 0;
            for (; j < i; ++j) if (v == idx[j]) break;
            if (j == i) break;
        }
        ++i;
    }
}

// RANSACPointSetRegistrator::getSubset for a model without checkSubset
inline void draw_subset(CvRng &rng, int count, int32_t idx[kFivePoints]) { draw_distinct(rng, count, kFivePoints, idx); }

// twice the signed area of the triangle (a, b, c), in double on the float coordinates
inline double tri_cross(const float *p, int a, int b, int c)
{
    const double dx1 = (double)p[2 * b] - (double)p[2 * a], dy1 = (double)p[2 * b + 1] - (double)p[2 * a + 1];
    const double dx2 = (double)p[2 * c] - (double)p[2 * a], dy2 = (double)p[2 * c + 1] - (double)p[2 * a + 1];
    return dx1 * dy2 - dy1 * dx2;
}
inline bool tri_collinear(const float *p, int a, int b, int c)
{
    const double dx1 = (double)p[2 * b] - (double)p[2 * a], dy1 = (double)p[2 * b + 1] - (double)p[2 * a + 1];
    const double dx2 = (double)p[2 * c] - (double)p[2 * a], dy2 = (double)p[2 * c + 1] - (double)p[2 * a + 1];
    return std::fabs(dx1 * dy2 - dy1 * dx2) <= (double)FLT_EPSILON * (std::fabs(dx1) + std::fabs(dy1) + std::fabs(dx2) + std::fabs(dy2));
}

// HomographyEstimatorCallback::checkSubset on the four correspondences idx[0..3] of pts1 -> pts2 (float pairs): false when one of the
// four triples (0,1,2), (1,2,3), (0,2,3), (0,1,3) is collinear (or two of its points coincide) in either image, or when the triples do
// not keep one orientation -- the product of the two images' signed areas is negative for some but not for all four.
inline bool check_subset4(const float *pts1, const float *pts2, const int32_t idx[kFourPoints])
{
    static const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    for (int k = 0; k < 4; ++k) if (tri_collinear(pts1, idx[tt[k][0]], idx[tt[k][1]], idx[tt[k][2]])) return false;
    for (int k = 0; k < 4; ++k) if (tri_collinear(pts2, idx[tt[k][0]], idx[tt[k][1]], idx[tt[k][2]])) return false;
    int negative = 0;
    for (int k = 0; k < 4; ++k)
        negative += tri_cross(pts1, idx[tt[k][0]], idx[tt[k][1]], idx[tt[k][2]]) * tri_cross(pts2, idx[tt[k][0]], idx[tt[k][1]], idx[tt[k][2]]) < 0.0 ? 1 : 0;
    return negative == 0 || negative == 4;
}

// getSubset for the model with checkSubset: four distinct indices, then the subset check; a rejected subset is redrawn whole, up to
// kSubsetAttempts attempts.  false: no subset passed (the stream has advanced by all attempts).  *redraws (or NULL) is increased by
// the number of rejected subsets.
inline bool draw_subset(CvRng &rng, int count, const float *pts1, const float *pts2, int32_t idx[kFourPoints], int64_t *redraws = nullptr)
{
    for (int attempt = 0; attempt < kSubsetAttempts; ++attempt) {
        draw_distinct(rng, count, kFourPoints, idx);
        if (check_subset4(pts1, pts2, idx)) return true;
        if (redraws) ++*redraws;
    }
    return false;
}

inline int update_num_iters(double p, double ep, int model_points, int max_iters)   // cv::RANSACUpdateNumIters
{
    p = std::max(p, 0.0); p = std::min(p, 1.0);
    ep = std::max(ep, 0.0); ep = std::min(ep, 1.0);
    double num = std::max(1.0 - p, DBL_MIN);
    double denom = 1.0 - std::pow(1.0 - ep, model_points);
    if (denom < DBL_MIN) return 0;
    num = std::log(num); denom = std::log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::lrint(num / denom);
}

// ---- RANSACPointSetRegistrator::run, one problem's state -----------------------------------------------------------------------------
struct Registrator {
    CvRng rng;
    int model_points, niters, max_good = 0, iter = 0;
    int valid = 0;         // slots of the current round that may count (fill_round)
    bool done, exact;      // exact: count == model_points -- the model of all points, every point an inlier, no iteration
    bool failed = false;   // the sampler gave up: the loop ends before that iteration
    Registrator(int model_points, int max_iters, int count)
        : model_points(model_points), niters(max_iters), done(count < model_points /* run() returns false */), exact(count == model_points) {}
    // a hypothesis with `good` inliers among `count` points, in iteration order: true when it is the new best
    bool offer(int good, int count, double confidence)
    {
        if (!(good > std::max(max_good, model_points - 1))) return false;
        max_good = good;
        niters = update_num_iters(confidence, (double)(count - good) / count, model_points, niters);
        return true;
    }
};

// The int32 tables of one round of n_pairs problems x chunk slots, as element offsets into ONE array: samples | n_models | counts |
// take.  n_models | counts is contiguous on purpose -- it comes down in one copy (`down`).
struct RoundTables {
    size_t n_slots, samples = 0, n_models, counts, take, end;
    size_t down, down_len;   // the span n_models | counts
    RoundTables(int n_pairs, int chunk, int model_points, int models_per_slot)
        : n_slots((size_t)n_pairs * (size_t)chunk), n_models((size_t)model_points * n_slots), counts(n_models + n_slots),
          take(counts + (size_t)models_per_slot * n_slots), end(take + 3 * (size_t)n_pairs), down(n_models), down_len(take - n_models) {}
};

// Writes the next round's samples[model_points * (chunk * p + k) ..], first index -1 for an idle slot, and every state's `valid`.
// draw_of(p) gives pair p's getSubset as draw(rng, idx) -> bool (false: it gave up), so that what a pair's draws share is looked up
// once per round and not once per draw.  Returns whether any pair is still active.
// A pair draws valid = min(chunk, niters - iter) samples, not chunk: niters never grows, so later slots could never be replayed, and
// a pair that needs another round had valid == chunk (with valid < chunk its replay ends at iter == the old niters >= niters: done) --
// the generator therefore stands where the one-iteration-at-a-time loop has it, whatever the chunk size.
template <class DrawOf>
inline bool fill_round(Registrator *S, int n_pairs, int chunk, int32_t *samples, DrawOf draw_of)
{
    bool any = false;
    for (int p = 0; p < n_pairs; ++p) {
        Registrator &s = S[p];
        const int m = s.model_points;
        s.valid = s.done ? 0 : (s.exact ? 1 : std::min(chunk, s.niters - s.iter));
        int32_t *dst = samples + (size_t)m * chunk * p;
        int k = 0;
        if (s.valid > 0 && s.exact) { for (int j = 0; j < m; ++j) dst[j] = j; k = 1; }
        else if (s.valid > 0) {
            const auto draw = draw_of(p);
            for (const int valid = s.valid; k < valid; ++k) if (!draw(s.rng, dst + (size_t)m * k)) { s.valid = k; s.failed = true; break; }
        }
        for (; k < chunk; ++k) dst[(size_t)m * k] = -1;
        any = any || !s.done;
    }
    return any;
}

// Replays run() over the round fill_round set up: per live pair its valid slots in order, slot g = chunk * p + k holding n_models[g]
// models with counts[models_per_slot * g + m] inliers among the pair's point_offset[p + 1] - point_offset[p] points.  A pair ends
// at iter >= niters or after a failed draw.  Appends (pair, slot, model) of every pair's new best to `take`; returns their number.
inline int replay_round(Registrator *S, int n_pairs, const int32_t *point_offset, int chunk, const int32_t *n_models, const int32_t *counts,
                        int models_per_slot, double confidence, int32_t *take)
{
    int n_take = 0;
    for (int p = 0; p < n_pairs; ++p) {
        Registrator &s = S[p];
        if (s.done) continue;
        const int n = point_offset[p + 1] - point_offset[p];
        const size_t g0 = (size_t)chunk * p;
        long best_slot = -1; int best_m = -1;
        if (s.exact) {
            if (n_models[g0] > 0) { best_slot = (long)g0; best_m = 0; s.max_good = n; }
            s.done = true;
        } else {
            for (int k = 0; k < s.valid && s.iter < s.niters; ++k, ++s.iter)
                for (int m = 0; m < n_models[g0 + k]; ++m)
                    if (s.offer(counts[(size_t)models_per_slot * (g0 + k) + m], n, confidence)) { best_slot = (long)(g0 + k); best_m = m; }
            if (s.iter >= s.niters || s.failed) s.done = true;
        }
        if (best_slot >= 0) { take[3 * n_take] = p; take[3 * n_take + 1] = (int32_t)best_slot; take[3 * n_take + 2] = best_m; ++n_take; }
    }
    return n_take;
}

}  // namespace ransac
}  // namespace esfm
