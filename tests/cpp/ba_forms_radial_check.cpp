// The rows of DESIGN.md section 5.1a for radial problems (free k1, k2 per camera group): the LDS rule of the grouped block-row kernel
// with 6-wide blocks -- 8 * 6 G * 6 (n_real + G) bytes within 64 KiB -- asserted on both sides of its boundary, and ba_forms with the
// radial flag against easysfm_amd/csrc/ba_forms.cpp (tests/test_ba_radial_cpu.py builds this against ba_forms.cpp alone, no GPU).
// A radial problem takes the grouped rule with any group count, one included: the sweep never keeps the per-camera sums in LDS.
#include <cstddef>
#include <cstdio>
#include <initializer_list>

#include "ba_forms.hpp"

using namespace esfm;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                                                                  \
    do {                                                                                                  \
        if (!(cond) && g_failed++ < 40) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

// two groups: 576 (n_real + 2) bytes, n_real <= 111
static_assert(calib_groups_lds_bytes(111, 2, true) == 65088 && calib_groups_lds_bytes(112, 2, true) == 65664, "two radial groups: n_real <= 111");
static_assert(ba_calib_groups_in_lds(111, 2, true) && !ba_calib_groups_in_lds(112, 2, true), "two radial groups: n_real <= 111");
// one group: 288 (n_real + 1) bytes, n_real <= 226
static_assert(ba_calib_groups_in_lds(226, 1, true) && !ba_calib_groups_in_lds(227, 1, true), "one radial group: n_real <= 226");
// the pinhole rule is where it was
static_assert(calib_groups_lds_bytes(168, 2) == 65280 && calib_groups_lds_bytes(168, 2, false) == 65280, "the defaulted flag is the pinhole rule");
static_assert(ba_calib_groups_in_lds(168, 2) && !ba_calib_groups_in_lds(169, 2), "two pinhole groups: n_real <= 168");
static_assert(2 * calib_groups_lds_bytes(50, 3, true) == 3 * calib_groups_lds_bytes(50, 3), "6 rows per block against 4");
static_assert(ba_calib_groups_in_lds(3, 1, true) && ba_calib_groups_in_lds(6, 2, true) && ba_calib_groups_in_lds(5, 5, true), "the small cases keep their rows in LDS");

constexpr int kObs = 1000;
constexpr int kMaxBlocks = 45999 / 6;

bool same(const BaForms &a, const BaForms &b)
{
    return a.schur == b.schur && a.solve == b.solve && a.sweep_sums_in_lds == b.sweep_sums_in_lds && a.large == b.large;
}

void forms()
{
    for (int n_real : {1, 3, 27, 28, 30, 31, 111, 112, 538, 539, 4000})
        for (int n_obs : {kObs, (1 << 20) - 1, 1 << 20}) {
            // without the flag, and with it but without free intrinsics: the rule as it was
            CHECK(same(ba_forms(n_real, true, n_obs, 2), ba_forms(n_real, true, n_obs, 2, false)), "n_real %d", n_real);
            CHECK(same(ba_forms(n_real, false, n_obs, 1, true), ba_forms(n_real, false, n_obs)), "n_real %d", n_real);
            // several groups: the flag changes nothing; one group: only the sweep's sums move to the camera chunks
            CHECK(same(ba_forms(n_real, true, n_obs, 2, true), ba_forms(n_real, true, n_obs, 2)), "n_real %d", n_real);
            BaForms one = ba_forms(n_real, true, n_obs, 1);
            one.sweep_sums_in_lds = false;
            CHECK(same(ba_forms(n_real, true, n_obs, 1, true), one), "n_real %d", n_real);
        }
    // two radial groups, the sizes the GPU tests solve at
    CHECK(ba_forms(27, true, kObs, 2, true).solve == BaForms::SOLVE_SMALL_ONE_WG && ba_forms(28, true, kObs, 2, true).solve == BaForms::SOLVE_LDS, "27 | 28");
    CHECK(ba_forms(30, true, kObs, 2, true).schur == BaForms::SCHUR_LDS_SLABS && ba_forms(31, true, kObs, 2, true).schur == BaForms::SCHUR_TABLES, "30 | 31");
    CHECK(ba_forms(30, true, kObs, 2, true).solve == BaForms::SOLVE_LDS && ba_forms(31, true, kObs, 2, true).solve == BaForms::SOLVE_TILED, "30 | 31");
}

void sweep()
{
    for (int G : {1, 2, 5, 40}) {
        int row_switches = 0;
        for (int n_real = 1; n_real + G <= kMaxBlocks; ++n_real) {
            CHECK(!ba_forms(n_real, true, kObs, G, true).sweep_sums_in_lds, "G %d n_real %d", G, n_real);
            // one way only, never more than the budget, and never in LDS where the pinhole rows are not
            CHECK(ba_calib_groups_in_lds(n_real + 1, G, true) <= ba_calib_groups_in_lds(n_real, G, true), "G %d n_real %d", G, n_real);
            row_switches += ba_calib_groups_in_lds(n_real + 1, G, true) != ba_calib_groups_in_lds(n_real, G, true);
            CHECK((ba_calib_groups_in_lds(n_real, G, true) ? calib_groups_lds_bytes(n_real, G, true) : 0) <= kCalibRowLdsBudget, "G %d n_real %d", G, n_real);
            CHECK(ba_calib_groups_in_lds(n_real, G, true) <= ba_calib_groups_in_lds(n_real, G), "G %d n_real %d", G, n_real);
            // the formula of the issue, written out
            CHECK(calib_groups_lds_bytes(n_real, G, true) == (size_t)8 * 6 * G * 6 * (n_real + G), "G %d n_real %d", G, n_real);
        }
        CHECK(row_switches == (G < 40 ? 1 : 0), "G %d: %d", G, row_switches);
    }
}

}  // namespace

int main()
{
    forms();
    sweep();
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("ba forms (radial) ok\n");
    return 0;
}
