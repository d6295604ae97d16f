// Prints which kernel forms ba_forms (easysfm_amd/csrc/ba_forms.cpp) gives a RADIAL problem (free k1, k2 per camera group):
// `schur solve sweep_sums_in_lds large group_rows_in_lds` per "n_real n_groups n_obs" triple on the command line
// (tests/test_ba_radial_gpu.py asserts each of its sizes takes the form it is about).
#include <cstdio>
#include <cstdlib>

#include "ba_forms.hpp"

using namespace esfm;

int main(int argc, char **argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) { fprintf(stderr, "usage: %s n_real n_groups n_obs [n_real n_groups n_obs ...]\n", argv[0]); return 2; }
    static const char *const schur[] = {"SCHUR_LDS_SLABS", "SCHUR_TABLES"};
    static const char *const solve[] = {"SOLVE_SMALL_ONE_WG", "SOLVE_LDS", "SOLVE_TILED"};
    for (int a = 1; a + 2 < argc; a += 3) {
        const int n_real = atoi(argv[a]), groups = atoi(argv[a + 1]), n_obs = atoi(argv[a + 2]);
        const BaForms f = ba_forms(n_real, true, n_obs, groups, true);
        // the last column: the 6 G block rows of ba_schur_groups_kernel<true> in LDS
        printf("%s %s %d %d %d\n", schur[f.schur], solve[f.solve], f.sweep_sums_in_lds ? 1 : 0, f.large ? 1 : 0, ba_calib_groups_in_lds(n_real, groups, true) ? 1 : 0);
    }
    return 0;
}
