// Launch interface between fundamental_api.cpp (cv::RNG replay, RANSAC bookkeeping on the host) and fundamental_kernels.hip.
#pragma once

#include "common.hpp"
#include "homography_kernels.hpp"

namespace esfm {

using FundPair = HomogPair;   // first, count, active, thresh_sq: (float)(threshold * threshold), the cut on the float epipolar error

// one chunk of iterations of every pair: samples[7 g ..] (first index < 0: idle slot) -> models[27 g ..] (up to three, in root order),
// n_models[g], counts[3 g + m]
int launch_fundamental_chunk(hipStream_t st, const FundPair *pairs, int n_pairs, const float *p1, const float *p2, const int32_t *samples, int chunk,
                             double *models, int32_t *n_models, int32_t *counts, esfm_ctx *timing_ctx);
// the scoring kernel alone: counts[3 g + m] = inliers of models[27 g + 9 m ..] among the points of pair g / chunk, m < n_models[g] (else 0)
int launch_fundamental_score(hipStream_t st, const FundPair *pairs, int n_pairs, const float *p1, const float *p2, int chunk, const double *models,
                             const int32_t *n_models, int32_t *counts);
// the minimal solver alone on samples given as pixel coordinates (q[28 g ..] = q1[14], q2[14])
int launch_fundamental_solve_samples(hipStream_t st, const double *q, int n, double *models, int32_t *n_models);
int launch_fundamental_mask(hipStream_t st, const FundPair *pairs, int n_pairs, const float *p1, const float *p2, const double *best, uint8_t *mask);
// per pair with `active` set: the 8-point re-fit on the points whose mask is set -> refit[9 p ..], ok[p] (0: fewer than 8 inliers or no model)
int launch_fundamental_refit(hipStream_t st, const FundPair *pairs, int n_pairs, const float *p1, const float *p2, const uint8_t *mask, double *refit,
                             int32_t *ok);
// cost[k] = sum_p w_p term(F_p, cand[k]) / sum_p w_p; terms: n_cand * n_pairs doubles of work space
int launch_focal_cost(hipStream_t st, int n_pairs, const double *F, const double *weight, double cx, double cy, int n_cand, const double *cand,
                      double *terms, double *cost);

}  // namespace esfm
