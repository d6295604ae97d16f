// The bundle-adjustment problem object behind the C ABI: what ba_api.cpp (create / set / get / destroy) and ba_solve.cpp (the
// Levenberg-Marquardt solve) share.
#pragma once

#include <algorithm>
#include <vector>

#include "ba_kernels.hpp"
#include "ba_chol_sparse.hpp"

struct esfm_ba_problem {
    esfm_ctx *ctx = nullptr;
    esfm::BADev d;
    std::vector<esfm_ctx::BaChunk> allocs;   // the chunks dev_alloc carves the problem's arrays from
    char *arena_cur = nullptr;            // free space of the newest chunk
    size_t arena_left = 0;
    std::vector<double> cam_nobs_local;  // this rank's observation count per camera-side block
    // box bounds (reference ba.cpp:155-162 reference camera, ba.cpp:190-194 intrinsics); +-inf where there is none
    int ref_cam = -1;
    double ref_threshold = 0.0;
    std::vector<double> calib_center, calib_tol;   // per free intrinsics block: [4 G] box centres, [G] half widths
    std::vector<double> radial_center, radial_tol; // radial problems (BADev::radial): [2 G] box centres of k1, k2, [G] half widths
    esfm::ScalParts parts{};    // the kernel forms of this problem and the per-workgroup scalar partials pending on the device (BADev::parts points here)
    double *h_scal = nullptr;   // pinned host copy of the scalar slots: the LM loop reads them back twice per iteration
    unsigned long long seq = 0; // sequence number of the last publication (the flag sits behind the scalars)
    // structure of the reduced camera system (ba_sparse_plan.hpp): this rank's co-visible camera pairs, from the observation list at
    // creation; the plan and its device tables are built by the first solve that can use them (several ranks: from the union of
    // the ranks' pairs) and kept
    std::vector<uint8_t> pair_flags;
    std::vector<int32_t> h_pt_start, h_obs_cam;
    esfm::SparseSolve *sparse = nullptr;
    int sparse_key = -1;        // what `sparse` was planned for: 0 one rank, 1 several ranks; -1 not planned yet
    int sparse_leaf_max = 0;
    bool sparse_worthwhile = false;
};

namespace esfm {

void ba_options_default(esfm_ba_options *o);

// A problem's ~45 device arrays are carved from a few chunks (256-byte aligned, 256 spare bytes behind each array) instead of one
// hipMalloc each: the small problems of an incremental reconstruction -- a BA call every ba_frequency frames, a dozen cameras and a
// few thousand observations -- are set up and torn down once per call (profiles/r05_driver_surf_undistort_pnp.txt: set-up 0.3 - 0.9 ms, tear-down 0.4 -
// 0.9 ms with one or two chunks; 0.14 / 0.0 ms once the chunks come from and go back to the context, below; the call's 4 - 5 ms are
// its up to 50 LM iterations of 0.075 - 0.087 ms, a launch-latency chain).  An
// array that does not fit the current chunk's rest opens a chunk of its own size (at least kArenaChunk): the large arrays of BA-512
// still get one allocation each.
int ba_dev_alloc_bytes(esfm_ba_problem *p, void **out, size_t bytes);
template <class T> int ba_dev_alloc(esfm_ba_problem *p, T **out, size_t count)
{
    return ba_dev_alloc_bytes(p, reinterpret_cast<void **>(out), sizeof(T) * count);
}

}  // namespace esfm
