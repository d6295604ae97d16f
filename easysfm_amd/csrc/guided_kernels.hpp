// Launch interface between guided_api.cpp (host logic) and guided_kernels.hip (gfx950 kernels): epipolar-guided matching
// (include/esfm.h "Epipolar-guided matching").
// The guided pass reads the raw descriptor rows and the keypoints only.  It neither needs nor disturbs esfm_match_prepare_dev's
// state: no operand image, norm, counter or table of the plain matcher (esfm::MatchState) is read or written here, so a guided call
// between two plain calls on a prepared buffer leaves the buffer prepared and the plain results as they were.
#pragma once

#include "match_lists.hpp"   // PairDesc; the filters behind the guided tables are the plain matcher's list kernels

namespace esfm {

// The verified geometry of one image pair: E row-major, the query frame's intrinsics, tsq = (float)((max_epipolar_px / ((fx + fy) / 2))^2),
// and the two cuts of the division-free verdict (guided_kernels.hip guided_admissible): t_in just below tsq, t_out just above the
// next float after tsq.
struct GuidedGeom {
    double E[9];
    double fx, cx, fy, cy;
    double t_in, t_out;
    float tsq;
    int32_t pad;
};
void guided_set_threshold(GuidedGeom &g, double max_epipolar_px);

constexpr int kGuidedQueryBlock = 256;   // queries per workgroup (PairDesc::blk_off counts these blocks)

// The guided 2-NN table of every pair of `pairs` (n_tab entries; entry g >= n_fwd is forward pair g - n_fwd with query and train
// swapped: its lanes own rows of the forward TRAIN set and the predicate keeps its operand roles).  geom: one entry per forward pair.
// knn_idx / knn_dist: 2 per query at 2 * (out_off + q), missing neighbours -1 / FLT_MAX; n_adm (may be NULL): admissible rows per query.
int launch_guided_knn2(hipStream_t st, esfm_metric metric, int width, const void *desc, const float *kp, const PairDesc *pairs, int n_tab,
                       int n_fwd, const GuidedGeom *geom, int n_blocks, int32_t *knn_idx, float *knn_dist, int32_t *n_adm);

}  // namespace esfm
