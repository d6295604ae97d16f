// Launch interface between track_api.cpp and track_kernels.hip (esfm_track_triangulate, esfm_track_evaluate).
#pragma once

#include "common.hpp"
#include "scratch_layout.hpp"
#include "track_core.hpp"

namespace esfm {

struct TrackArgs {
    int32_t n_cam, n_pt, n_obs;
    int32_t evaluate;              // 1: judge xyz_in, no hypotheses and no refit
    track::Options opt;
    // inputs (device)
    const int32_t *cam_idx, *pt_idx;
    const float *uv, *K4;
    const double *Rt, *xyz_in;     // xyz_in may be NULL for triangulate
    // grouping
    uint64_t *keys;                // pt_idx << 32 | input index, before the sort
    const uint64_t *sorted;        // ... and after it
    int32_t *head_blocks;          // per 256 sorted keys: run heads, then their exclusive offset; the total behind them
    int32_t *track_first;          // n_tracks + 1: the sorted position of each track's first observation; n_obs behind the last
    track::Obs *long_rec;          // n_obs records for the tracks above track::kStageCap, or NULL when there is none
    // outputs (device)
    double *xyz_out;               // NULL for evaluate
    uint8_t *obs_inlier;
    float *obs_err2;
    int32_t *pt_status, *pt_n_inliers;
    double *pt_min_cos, *pt_mse;
};

// the key width of the sort: the high word is a point index below n_pt
inline int track_key_bits(int32_t n_pt) { return 32 + bit_width((uint64_t)n_pt); }

// keys, sort, run heads, the per-point defaults, one wave per track.  n_pt >= 1, n_obs >= 1.
int launch_track_solve(hipStream_t st, const TrackArgs &a, void *sort_tmp, size_t sort_bytes);
// n_obs = 0: the per-point defaults alone
int launch_track_defaults(hipStream_t st, const TrackArgs &a);

}  // namespace esfm
