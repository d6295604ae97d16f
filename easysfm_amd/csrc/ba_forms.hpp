// Which form of the size-dependent bundle-adjustment kernels a problem takes (host side, no GPU), and every size that both this rule
// and a kernel or its launcher read: each number is written once, here.  tests/cpp/ba_forms_check.cpp pins the table of DESIGN.md
// section 5.1a.
#pragma once

#include <cstddef>

namespace esfm {

// A function of the problem's sizes alone (ba_forms): evaluated once at creation, sizes the buffers each form needs and is what every
// launcher reads (BADev::parts->forms); conditions of the running solve (one rank or several, bounds, the structure-aware plan)
// combine with it at the launch sites.  DESIGN.md section 5 has the table.
struct BaForms {
    enum Schur { SCHUR_LDS_SLABS,   // all camera blocks of S in every workgroup's LDS, summed over per-workgroup slabs (ba_schur_lds_kernel)
                 SCHUR_TABLES };    // matrix-core / windowed / wide tables of BaLayout
    enum Solve { SOLVE_SMALL_ONE_WG,   // one-workgroup MFMA solve, the camera step included (ba_chol_small_kernel)
                 SOLVE_LDS,            // one workgroup, packed factor in LDS (ba_chol_solve_kernel)
                 SOLVE_TILED };        // multi-workgroup tiled solve, dense or structure-aware (ba_chol_large.hip, ba_chol_sparse.hip)
    Schur schur = SCHUR_LDS_SLABS;
    Solve solve = SOLVE_SMALL_ONE_WG;
    bool sweep_sums_in_lds = false;    // the Jacobian sweep keeps the per-camera sums in LDS (else: camera chunks, BaLayout::cchunk_*)
    bool large = false;                // >= 2^20 observations: 512-thread sweep, chunked per-point blocks, candidate cost in a pass of its own
};
// n_groups: the free intrinsics blocks (one per camera group; read only with has_calib).  The rule is the one of a single block with
// n_cam = n_real_cam + n_groups, except that with several groups the sweep never keeps the per-camera sums in LDS: a group's ten
// sums G'G / G'r are its cameras' chunk sums added in chunk order (ba_camacc_groups_kernel), so every size takes the camera chunks.
// radial: the blocks also carry k1, k2; such a problem takes the grouped path even with one group.
BaForms ba_forms(int n_real_cam, bool has_calib, int n_obs, int n_groups = 1, bool radial = false);

// dynamic LDS of the three kernels that have an in-LDS form
constexpr int kLinLdsPerCam = 27 * 8 + 7 * 8 + 4 + 7 * 4;   // ba_linearize_kernel: acc, maxima, count, exponents
// (ALL of the sweep's LDS: at 538 cameras 144 bytes short of a compute unit's 160 KiB, so the kernel keeps no static __shared__ object)
constexpr size_t lin_lds_bytes(int n_real_cam) { return 18 * sizeof(double) + (size_t)n_real_cam * kLinLdsPerCam; }
// LDS pitch of a 6 x 6 block: 37 doubles, not 36.  The lanes of a wave add the same entry of DIFFERENT blocks; at pitch 36 (288 B)
// those addresses fall on 8 of the 64 banks (SQ_LDS_BANK_CONFLICT was two thirds of SQ_LDS_IDX_ACTIVE), at 37 on all of them.
constexpr int kSchurPitch = 37;
constexpr size_t schur_lds_bytes(int n_cam)     // ba_schur_lds_kernel: [nblk * kSchurPitch] blocks, [6 n_cam] right-hand side, then [6 n_cam] ints: qexp
{
    return sizeof(double) * ((size_t)n_cam * (n_cam + 1) / 2 * kSchurPitch + 6 * (size_t)n_cam) + sizeof(int) * 6 * (size_t)n_cam;
}
constexpr size_t chol_lds_bytes(int n_cam)      // ba_chol_solve_kernel: packed lower factor with the right-hand side row, reciprocal diagonal, flag
{
    const size_t n = 6 * (size_t)n_cam;
    return sizeof(double) * ((n + 1) * (n + 2) / 2 + n + 2);
}
// ba_schur_calib_kernel (free intrinsics): 8 doubles of reduction scratch, then -- while it fits the 64 KiB a workgroup may always take --
// an LDS copy of the intrinsics block row, 4 x 6 n_real_cam; beyond (n_real_cam >= 342) the row's addends go to d.red directly
constexpr size_t kCalibRowLdsBudget = 64 * 1024;
constexpr size_t calib_row_lds_bytes(int n_real_cam) { return sizeof(double) * (8 + (size_t)4 * 6 * n_real_cam); }
constexpr bool ba_calib_row_in_lds(int n_real_cam) { return calib_row_lds_bytes(n_real_cam) <= kCalibRowLdsBudget; }
// ba_schur_groups_kernel (several free intrinsics blocks): the block rows of ALL groups, 4 n_groups rows of 6 (n_real_cam + n_groups)
// fixed-point entries -- the camera columns and the group-by-group cross blocks -- under the same budget (two groups: up to 168
// cameras); beyond, every addend goes to d.red directly
// radial problems (k1, k2 free in slots 4 and 5 of every block, one group or several): 6 n_groups rows, 8 * 6 G * 6 (n_real_cam + G)
// bytes (two groups: up to 111 cameras)
constexpr size_t calib_groups_lds_bytes(int n_real_cam, int n_groups, bool radial = false)
{
    return sizeof(double) * ((size_t)(radial ? 6 : 4) * n_groups * 6 * ((size_t)n_real_cam + n_groups));
}
constexpr bool ba_calib_groups_in_lds(int n_real_cam, int n_groups, bool radial = false)
{
    return calib_groups_lds_bytes(n_real_cam, n_groups, radial) <= kCalibRowLdsBudget;
}
// the one-workgroup MFMA solve (ba_chol_small_kernel) holds at most kSmallMaxNb block rows of kSmallTile (= SB, ba_chol_tile.hpp)
// unknowns: n = 6 n_cam <= 176
constexpr int kSmallTile = 16, kSmallMaxNb = 11;
constexpr bool ba_chol_small_fits(int n_cam) { return (6 * n_cam + kSmallTile - 1) / kSmallTile <= kSmallMaxNb; }

}  // namespace esfm
