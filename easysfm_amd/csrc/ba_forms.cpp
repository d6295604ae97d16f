// The size-dependent kernel forms (BaForms, ba_forms.hpp): the one place their thresholds are written.
#include "ba_forms.hpp"

namespace esfm {

constexpr int kLinSmallObs = 1 << 20;              // observations from which a problem is `large`
constexpr size_t kLinLdsBudget = 160 * 1024;       // the sweep: one workgroup per CU may take all of a CU's LDS
constexpr size_t kSchurLdsBudget = 156 * 1024;     // the LDS-slab Schur kernel
constexpr size_t kCholLdsBudget = 150 * 1024;      // the one-workgroup reduced solve with its packed factor in LDS

BaForms ba_forms(int n_real_cam, bool has_calib, int n_obs, int n_groups, bool radial)
{
    const int n_cam = n_real_cam + (has_calib ? n_groups : 0);
    BaForms f;
    f.schur = schur_lds_bytes(n_cam) <= kSchurLdsBudget ? BaForms::SCHUR_LDS_SLABS : BaForms::SCHUR_TABLES;
    f.sweep_sums_in_lds = lin_lds_bytes(n_real_cam) <= kLinLdsBudget && !(has_calib && (n_groups > 1 || radial));
    f.large = n_obs >= kLinSmallObs;
    f.solve = ba_chol_small_fits(n_cam) ? BaForms::SOLVE_SMALL_ONE_WG : chol_lds_bytes(n_cam) <= kCholLdsBudget ? BaForms::SOLVE_LDS : BaForms::SOLVE_TILED;
    return f;
}

}  // namespace esfm
