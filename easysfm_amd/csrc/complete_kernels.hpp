// Launch interface between complete_api.cpp and complete_kernels.hip (esfm_track_complete, esfm_track_complete_dev).
#pragma once

#include "common.hpp"
#include "complete_core.hpp"
#include "scratch_layout.hpp"

namespace esfm {

struct CompleteArgs {
    int32_t n_cam, n_pt, n_obs, n_rows;
    int32_t metric, width;             // esfm_metric; floats (L2) or bytes (Hamming) per descriptor row
    complete::Options opt;
    // inputs (device)
    const void *desc;                  // n_rows descriptor rows
    const float *kp;                   // 2 per row
    const uint8_t *kp_free;            // 1 per row
    const int32_t *row_off;            // n_cam + 1
    const float *K4;
    const double *Rt, *xyz;
    // the observations grouped by point, each point's in input order (the host's stable counting sort)
    const int32_t *pt_first;           // n_pt + 1
    const int32_t *obs_cam, *obs_row;  // n_obs: camera, and descriptor row (row_off[cam] + obs_kp)
    // grid
    complete::CamGrid *grid;           // n_cam
    uint64_t *keys;                    // per row: complete::grid_key, camera field n_cam for a row that takes no part
    const uint64_t *sorted;            // ... sorted
    // jobs
    int32_t *job_blocks;               // per 256 (point, camera) combinations: jobs, then their exclusive offset; the total behind them
    uint64_t *jobs;                    // point << 32 | camera, in (point, camera) order
    // results
    unsigned long long *claim;         // per row: complete::claim_key of the best proposal, complete::kNoClaim without one
    unsigned long long *counters;      // [4] as esfm_track_complete's stats ([2] is filled by the last kernel)
    int32_t *kp_point;
    float *kp_dist;
    int64_t *stats;                    // may be NULL
};

__host__ __device__ inline int64_t complete_combinations(const CompleteArgs &a) { return (int64_t)a.n_pt * a.n_cam; }
// the key width of the grid sort: the camera field holds 0 .. n_cam
inline int complete_key_bits(int32_t n_cam) { return complete::kCellBits + complete::kRowBits + bit_width((uint64_t)n_cam); }

// boxes and grids, keys, the sort.  n_rows >= 1, n_cam >= 1.
int launch_complete_grid(hipStream_t st, const CompleteArgs &a, void *sort_tmp, size_t sort_bytes);
// the count of the jobs per 256 combinations and its scan: n_jobs = job_blocks[blocks_of(combinations)].  n_pt >= 1, n_cam >= 1.
int launch_complete_job_count(hipStream_t st, const CompleteArgs &a);
// the ordered job list (n_jobs >= 1, read back by the caller: `jobs` has that many entries)
int launch_complete_jobs(hipStream_t st, const CompleteArgs &a);
// the search with its claims (n_jobs >= 1)
int launch_complete_search(hipStream_t st, const CompleteArgs &a, int32_t n_jobs);
// claims -> kp_point / kp_dist, the counters -> stats.  Also the whole answer of a call without jobs.
int launch_complete_decode(hipStream_t st, const CompleteArgs &a);

}  // namespace esfm
