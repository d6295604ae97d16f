// The rows of DESIGN.md section 5.1a for several free intrinsics blocks (multiple-camera mode): ba_forms with a group count, asserted
// against easysfm_amd/csrc/ba_forms.cpp at each boundary and its neighbour (tests/test_ba_groups_cpu.py builds this against
// ba_forms.cpp alone, no GPU).  The rule is the one-block rule with n_cam = n_real + G, except that with G > 1 the sweep never keeps
// the per-camera sums in LDS; the grouped block-row kernel has its own LDS rule.
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

// the byte counts the grouped block rows' boundary follows from: 4 G rows of 6 (n_real + G) 8-byte entries within 64 KiB
static_assert(calib_groups_lds_bytes(168, 2) == 65280 && calib_groups_lds_bytes(169, 2) == 65664, "two groups: n_real <= 168");
static_assert(ba_calib_groups_in_lds(168, 2) && !ba_calib_groups_in_lds(169, 2), "two groups: n_real <= 168");
static_assert(calib_groups_lds_bytes(25, 25) == 240000 && !ba_calib_groups_in_lds(25, 25), "25 cameras, one group each: global atomics");
static_assert(ba_calib_groups_in_lds(6, 6) && ba_calib_groups_in_lds(4, 2), "the small cases keep their rows in LDS");

constexpr int kObs = 1000;              // any count below 2^20
constexpr int kMaxBlocks = 45999 / 6;   // the library accepts 6 (n_real + G) < 46 000

bool same(const BaForms &a, const BaForms &b)
{
    return a.schur == b.schur && a.solve == b.solve && a.sweep_sums_in_lds == b.sweep_sums_in_lds && a.large == b.large;
}

void one_group_is_the_old_rule()
{
    // the defaulted argument, an explicit 1, and any group count without free intrinsics
    for (int n_real : {0, 1, 6, 27, 28, 29, 31, 32, 33, 341, 342, 538, 539, 4000})
        for (int n_obs : {0, kObs, (1 << 20) - 1, 1 << 20}) {
            CHECK(same(ba_forms(n_real, true, n_obs), ba_forms(n_real, true, n_obs, 1)), "n_real %d n_obs %d", n_real, n_obs);
            CHECK(same(ba_forms(n_real, false, n_obs), ba_forms(n_real, false, n_obs, 1)), "n_real %d n_obs %d", n_real, n_obs);
            CHECK(same(ba_forms(n_real, false, n_obs), ba_forms(n_real, false, n_obs, 7)), "n_real %d n_obs %d", n_real, n_obs);
        }
}

void boundaries()
{
    for (int G : {2, 3, 6, 25}) {
        // a camera boundary at n_cam is at n_real = n_cam - G
        auto at_cam = [&](int n_cam) { return ba_forms(n_cam - G, true, kObs, G); };
        CHECK(at_cam(32).schur == BaForms::SCHUR_LDS_SLABS, "G %d", G);
        CHECK(at_cam(33).schur == BaForms::SCHUR_TABLES, "G %d", G);
        if (G <= 29) CHECK(at_cam(29).solve == BaForms::SOLVE_SMALL_ONE_WG, "G %d", G);
        CHECK(at_cam(30).solve == BaForms::SOLVE_LDS, "G %d", G);
        CHECK(at_cam(32).solve == BaForms::SOLVE_LDS, "G %d", G);
        CHECK(at_cam(33).solve == BaForms::SOLVE_TILED, "G %d", G);
        // several groups: the camera-chunk sums at every size
        for (int n_real : {1, 4, 27, 538, 539}) CHECK(!ba_forms(n_real, true, kObs, G).sweep_sums_in_lds, "G %d n_real %d", G, n_real);
        for (int n_real : {6, 32, 539}) {
            CHECK(!ba_forms(n_real, true, (1 << 20) - 1, G).large, "G %d n_real %d", G, n_real);
            CHECK(ba_forms(n_real, true, 1 << 20, G).large, "G %d n_real %d", G, n_real);
        }
    }
    // two groups, the sizes the GPU tests solve at
    CHECK(ba_forms(27, true, kObs, 2).solve == BaForms::SOLVE_SMALL_ONE_WG && ba_forms(28, true, kObs, 2).solve == BaForms::SOLVE_LDS, "27 | 28");
    CHECK(ba_forms(30, true, kObs, 2).schur == BaForms::SCHUR_LDS_SLABS && ba_forms(31, true, kObs, 2).schur == BaForms::SCHUR_TABLES, "30 | 31");
    CHECK(ba_forms(30, true, kObs, 2).solve == BaForms::SOLVE_LDS && ba_forms(31, true, kObs, 2).solve == BaForms::SOLVE_TILED, "30 | 31");
}

void sweep()
{
    for (int G : {2, 5, 40}) {
        int schur_switches = 0, solve_switches = 0, row_switches = 0;
        BaForms prev = ba_forms(1, true, kObs, G);
        for (int n_real = 1; n_real + G <= kMaxBlocks; ++n_real) {
            const BaForms f = ba_forms(n_real, true, kObs, G);
            CHECK(f.schur >= prev.schur && f.solve >= prev.solve && f.solve - prev.solve <= 1 && !f.sweep_sums_in_lds, "G %d n_real %d", G, n_real);
            schur_switches += f.schur != prev.schur; solve_switches += f.solve != prev.solve;
            if (f.solve == BaForms::SOLVE_TILED) CHECK(f.schur == BaForms::SCHUR_TABLES, "G %d n_real %d", G, n_real);
            // the grouped block rows: one way only, and the launch never asks for more than the budget
            CHECK(ba_calib_groups_in_lds(n_real + 1, G) <= ba_calib_groups_in_lds(n_real, G), "G %d n_real %d", G, n_real);
            row_switches += ba_calib_groups_in_lds(n_real + 1, G) != ba_calib_groups_in_lds(n_real, G);
            CHECK((ba_calib_groups_in_lds(n_real, G) ? calib_groups_lds_bytes(n_real, G) : 0) <= kCalibRowLdsBudget, "G %d n_real %d", G, n_real);
            prev = f;
        }
        // (G = 40: n_cam starts beyond both camera boundaries and the rows never fit)
        CHECK(schur_switches == (G < 32 ? 1 : 0) && solve_switches == (G < 29 ? 2 : G < 32 ? 1 : 0) && row_switches == (G < 40 ? 1 : 0), "G %d: %d %d %d", G,
              schur_switches, solve_switches, row_switches);
    }
}

}  // namespace

int main()
{
    one_group_is_the_old_rule();
    boundaries();
    sweep();
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("ba forms (groups) ok\n");
    return 0;
}
