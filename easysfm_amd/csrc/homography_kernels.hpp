// Launch interface between homography_api.cpp (cv::RNG replay with the subset check, RANSAC bookkeeping on the host) and
// homography_kernels.hip.
#pragma once

#include "common.hpp"

namespace esfm {

struct HomogPair {        // one image pair's correspondences inside the concatenated point arrays
    int32_t first, count;
    int32_t active;       // still iterating in this round
    float thresh_sq;      // (float)(threshold * threshold): the cut on the float transfer error
};

// one chunk of iterations of every pair: samples[4 g ..] (first index < 0: idle slot) -> models[9 g ..], has_model[g], counts[g]
int launch_homography_chunk(hipStream_t st, const HomogPair *pairs, int n_pairs, const float *p1, const float *p2, const int32_t *samples, int chunk,
                            double *models, int32_t *has_model, int32_t *counts, esfm_ctx *timing_ctx);
// the scoring kernel alone: counts[g] = inliers of models[9 g ..] among the points of pair g / chunk (0 where has_model[g] <= 0)
int launch_homography_score(hipStream_t st, const HomogPair *pairs, int n_pairs, const float *p1, const float *p2, int chunk, const double *models,
                            const int32_t *has_model, int32_t *counts);
// the minimal solver alone on samples given as pixel coordinates (q[16 g ..] = q1[8], q2[8])
int launch_homography_solve_samples(hipStream_t st, const double *q, int n, double *models, int32_t *has_model);
int launch_homography_mask(hipStream_t st, const HomogPair *pairs, int n_pairs, const float *p1, const float *p2, const double *best, uint8_t *mask);
// per pair with `active` set: the re-fit on the points whose mask is set -> refit[9 p ..], ok[p] (0: fewer than 4 inliers or no model)
int launch_homography_refit(hipStream_t st, const HomogPair *pairs, int n_pairs, const float *p1, const float *p2, const uint8_t *mask, double *refit,
                            int32_t *ok);

}  // namespace esfm
