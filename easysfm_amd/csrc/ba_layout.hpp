// Index tables of one bundle-adjustment problem (host side, no GPU): the observations sorted by point, the per-camera chunks of the
// atomic-free camera sums, the three families of Schur tables (matrix-core, windowed, wide) and the point chunks.  Pure arithmetic on
// the caller's (camera, point) index lists; ba_api.cpp uploads the vectors as they stand and the BA kernel files read them (BADev names
// the consumers).  The solver is bit-reproducible BECAUSE the order inside these tables is fixed: tests/cpp/ba_layout_check.cpp states
// what the kernels rely on.
#pragma once

#include <cstdint>
#include <vector>

namespace esfm {

constexpr int kCamChunk = 256, kCamPart = 37;  // observations per camera chunk; doubles of one chunk's partial sums (BADev::cam_part)
constexpr int kRadialPart = 27;                // radial problems: a chunk's sums of its group's block, G'G (21, upper triangle) and G'r (6) (BADev::cam_part_k)
constexpr int kPtChunkObs = 256;               // observations per point chunk (back-substitution, per-point normal blocks)
constexpr int kSchurWinCams = 28;              // cameras in the windowed Schur kernel's LDS window
constexpr int kSchurMfCams = 13;               // cameras in the matrix-core Schur kernel's window (80 rows = 5 MFMA block rows)

// observations grouped by point (counting sort, stable: keeps the caller's order inside a point)
struct BaPointSort {
    std::vector<int32_t> order;     // [n_obs] caller's index of sorted observation t
    std::vector<int32_t> cam, pt;   // [n_obs] camera / point of sorted observation t
    std::vector<int32_t> pt_start;  // [n_pt + 1] CSR over the sorted observations
};
BaPointSort ba_sort_by_point(int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx);

struct BaLayout : BaPointSort {
    std::vector<int32_t> cam_nobs;  // [n_real] this rank's observations per camera
    // camera CSR of the sorted observations, cut into chunks of kCamChunk (one camera per chunk)
    std::vector<int32_t> cam_obs, cchunk_cam, cchunk_beg, cchunk_end, cam_chunk0;
    // Schur tables (only with schur_tables; empty otherwise, and a table without chunks is empty throughout).  [0]: plain camera
    // indices, [1] / _b: indices rotated by n_real / 2 (the seam of a closed camera loop)
    std::vector<int32_t> mslot_obs[2], mslot_pc[2], mbatch_slot[2], mchunk_batch0[2], mchunk_cam0[2];
    std::vector<int32_t> slot_obs, chunk_slot, chunk_cam0, slot_obs_b, chunk_slot_b, chunk_cam0_b;
    std::vector<int32_t> wide_obs;
    // point chunks: consecutive points with at most kPtChunkObs observations (and points) per chunk; a longer track stands alone
    std::vector<int32_t> pchunk_pt0;   // [n_pchunks + 1]
    std::vector<int32_t> pchunk_info;  // [4 max(n_pchunks, 1)] {first point, end point, first observation, end observation}
};

// cam_idx in [0, n_real), pt_idx in [0, n_pt) (the caller has checked).  schur_tables: the LDS-slab Schur does not apply to this
// problem (BaForms::schur, ba_forms.hpp); num_cu sizes the Schur chunks (about two per compute unit).
BaLayout make_ba_layout(int n_real, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, int num_cu, bool schur_tables);

}  // namespace esfm
