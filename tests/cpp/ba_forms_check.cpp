// The table of DESIGN.md section 5.1a -- which form of the size-dependent bundle-adjustment kernels a problem takes -- asserted
// against easysfm_amd/csrc/ba_forms.cpp at each boundary and its neighbour, with and without free intrinsics
// (tests/test_ba_forms.py builds this against ba_forms.cpp alone, no GPU).
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

// the byte counts the boundaries follow from
static_assert(schur_lds_bytes(32) == 158592 && schur_lds_bytes(32) <= 156 * 1024 && schur_lds_bytes(33) > 156 * 1024, "LDS-slab Schur: n_cam <= 32");
static_assert(lin_lds_bytes(0) == 144 && kLinLdsPerCam == 304 && lin_lds_bytes(538) <= 160 * 1024 && lin_lds_bytes(539) > 160 * 1024, "sweep sums: n_real <= 538");
static_assert(chol_lds_bytes(32) == 151320 && chol_lds_bytes(32) <= 150 * 1024 && chol_lds_bytes(33) == 160800, "packed factor in LDS: n_cam <= 32");
static_assert(calib_row_lds_bytes(0) == 64 && calib_row_lds_bytes(341) == 65536 && calib_row_lds_bytes(341) <= 64 * 1024 && calib_row_lds_bytes(342) == 65728,
              "intrinsics block row in LDS: n_real <= 341");
static_assert(ba_chol_small_fits(29) && !ba_chol_small_fits(30) && kSmallTile * kSmallMaxNb == 176, "one-workgroup solve: 6 n_cam <= 176");

constexpr int kObs = 1000;              // any count below 2^20
constexpr int kMaxCam = 45999 / 6;      // the library accepts 6 n_cam < 46 000

void boundaries()
{
    for (int calib = 0; calib < 2; ++calib) {
        // a camera boundary at n_cam is at n_real = n_cam - 1 with free intrinsics (n_cam = n_real + 1)
        auto at_cam = [&](int n_cam) { return ba_forms(n_cam - calib, calib != 0, kObs); };
        CHECK(at_cam(32).schur == BaForms::SCHUR_LDS_SLABS, "calib %d", calib);
        CHECK(at_cam(33).schur == BaForms::SCHUR_TABLES, "calib %d", calib);
        CHECK(at_cam(29).solve == BaForms::SOLVE_SMALL_ONE_WG, "calib %d", calib);
        CHECK(at_cam(30).solve == BaForms::SOLVE_LDS, "calib %d", calib);
        CHECK(at_cam(32).solve == BaForms::SOLVE_LDS, "calib %d", calib);
        CHECK(at_cam(33).solve == BaForms::SOLVE_TILED, "calib %d", calib);
        // the sweep's sums are per REAL camera: independent of the intrinsics block
        CHECK(ba_forms(538, calib != 0, kObs).sweep_sums_in_lds, "calib %d", calib);
        CHECK(!ba_forms(539, calib != 0, kObs).sweep_sums_in_lds, "calib %d", calib);
        for (int n_real : {6, 32, 33, 539}) {
            CHECK(!ba_forms(n_real, calib != 0, (1 << 20) - 1).large, "calib %d n_real %d", calib, n_real);
            CHECK(ba_forms(n_real, calib != 0, 1 << 20).large, "calib %d n_real %d", calib, n_real);
        }
        CHECK(!at_cam(32).large && !ba_forms(6, calib != 0, 0).large, "calib %d", calib);
    }
    // ba_schur_calib's LDS copy of the intrinsics block row: per REAL camera, and independent of every BaForms value
    CHECK(ba_calib_row_in_lds(1) && ba_calib_row_in_lds(341) && !ba_calib_row_in_lds(342) && !ba_calib_row_in_lds(kMaxCam - 1), "calib row");
    int row_switches = 0;
    for (int n_real = 1; n_real < kMaxCam; ++n_real) {
        CHECK(ba_calib_row_in_lds(n_real + 1) <= ba_calib_row_in_lds(n_real), "n_real %d", n_real);
        row_switches += ba_calib_row_in_lds(n_real + 1) != ba_calib_row_in_lds(n_real);
        // the launch never asks for more than the budget, whichever branch it takes
        CHECK((ba_calib_row_in_lds(n_real) ? calib_row_lds_bytes(n_real) : calib_row_lds_bytes(0)) <= kCalibRowLdsBudget, "n_real %d", n_real);
    }
    CHECK(row_switches == 1, "%d", row_switches);
}

void sweep()
{
    for (int calib = 0; calib < 2; ++calib) {
        int schur_switches = 0, sweep_switches = 0, solve_switches = 0;
        BaForms prev = ba_forms(1 - calib, calib != 0, kObs);
        for (int n_cam = 1; n_cam <= kMaxCam; ++n_cam) {
            const BaForms f = ba_forms(n_cam - calib, calib != 0, kObs);
            // every rule moves one way only, once per boundary
            CHECK(f.schur >= prev.schur && f.solve >= prev.solve && f.solve - prev.solve <= 1 && f.sweep_sums_in_lds <= prev.sweep_sums_in_lds,
                  "calib %d n_cam %d", calib, n_cam);
            schur_switches += f.schur != prev.schur; sweep_switches += f.sweep_sums_in_lds != prev.sweep_sums_in_lds; solve_switches += f.solve != prev.solve;
            // ba_schur hands red to the tiled solve in fixed point only on its SCHUR_TABLES path
            if (f.solve == BaForms::SOLVE_TILED) CHECK(f.schur == BaForms::SCHUR_TABLES, "calib %d n_cam %d", calib, n_cam);
            // the LDS-slab Schur: the rule the slab buffer used to be allocated by (ba_schur_slab_doubles -- 36 doubles per block and the
            // right-hand side -- at most 156 KiB) and the launch's real LDS need (schur_lds_bytes: pitch 37 and the exponents) agree
            const size_t slab_doubles = (size_t)n_cam * (n_cam + 1) / 2 * 36 + 6 * (size_t)n_cam;
            const bool by_slab = sizeof(double) * slab_doubles <= 156 * 1024, by_launch = schur_lds_bytes(n_cam) <= 156 * 1024;
            CHECK(by_slab == by_launch && by_launch == (f.schur == BaForms::SCHUR_LDS_SLABS), "calib %d n_cam %d", calib, n_cam);
            prev = f;
        }
        CHECK(schur_switches == 1 && sweep_switches == 1 && solve_switches == 2, "calib %d: %d %d %d", calib, schur_switches, sweep_switches, solve_switches);
    }
}

}  // namespace

int main()
{
    boundaries();
    sweep();
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("ba forms ok\n");
    return 0;
}
