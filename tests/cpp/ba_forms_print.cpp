// Prints which kernel forms ba_forms (easysfm_amd/csrc/ba_forms.cpp) gives a problem: `schur solve sweep_sums_in_lds large calib_row_in_lds`
// per "n_real calib n_obs" triple on the command line (tests/test_ba_forms_gpu.py asserts each of its sizes takes the form it is about).
#include <cstdio>
#include <cstdlib>

#include "ba_forms.hpp"

using namespace esfm;

int main(int argc, char **argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) { fprintf(stderr, "usage: %s n_real calib n_obs [n_real calib n_obs ...]\n", argv[0]); return 2; }
    static const char *const schur[] = {"SCHUR_LDS_SLABS", "SCHUR_TABLES"};
    static const char *const solve[] = {"SOLVE_SMALL_ONE_WG", "SOLVE_LDS", "SOLVE_TILED"};
    for (int a = 1; a + 2 < argc; a += 3) {
        const int n_real = atoi(argv[a]), calib = atoi(argv[a + 1]), n_obs = atoi(argv[a + 2]);
        const BaForms f = ba_forms(n_real, calib != 0, n_obs);
        // the last column is ba_schur_calib's own threshold: the kernel runs with free intrinsics only, "-" without
        printf("%s %s %d %d %s\n", schur[f.schur], solve[f.solve], f.sweep_sums_in_lds ? 1 : 0, f.large ? 1 : 0,
               calib ? (ba_calib_row_in_lds(n_real) ? "1" : "0") : "-");
    }
    return 0;
}
