// Stand-alone host program: the host build of easysfm_amd/csrc/fundamental_core.hpp on degenerate samples -- identical points, repeated
// points, exactly collinear sevens, non-finite and huge coordinates, an affine map, cubics with vanishing coefficients -- and on the
// re-fit and the focal cost at their edges.  Built plainly and with -fsanitize=address,undefined by tests/test_fundamental_cpu.py: every
// call must return, the model count must be 0 .. 3, every counted model finite, of unit norm and of canonical sign, the slots behind zero.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../easysfm_amd/csrc/fundamental_core.hpp"

using namespace esfm::fundm;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static void check_models(const double *q1, const double *q2)
{
    double F[27];
    const int n = fundamental_from_7(q1, q2, F);
    CHECK(n >= 0 && n <= 3);
    for (int m = 0; m < 3; ++m) {
        double ss = 0.0, big = 0.0, at = 0.0;
        bool zero = true;
        for (int i = 0; i < 9; ++i) {
            const double v = F[9 * m + i];
            CHECK(std::isfinite(v));
            ss += v * v; zero = zero && v == 0.0;
            if (std::fabs(v) > big) { big = std::fabs(v); at = v; }
        }
        if (m >= n) CHECK(zero);
        else if (!zero) { CHECK(std::fabs(std::sqrt(ss) - 1.0) < 1e-12); CHECK(at > 0.0); }
    }
}

int main()
{
    const double gen1[14] = {120.5, 80.25, 610, 95, 333, 401.5, 87, 300, 512, 256, 699, 470, 250, 130};
    const double gen2[14] = {131, 70, 590, 110, 350, 380, 99, 310, 500, 270, 680, 455, 262, 118};
    check_models(gen1, gen2);
    std::vector<double> a(gen1, gen1 + 14), b(gen2, gen2 + 14);
    for (int k = 0; k < 7; ++k) { a[2 * k] = 37.5; a[2 * k + 1] = 91.25; }                     // seven identical points in image 1
    check_models(a.data(), gen2); check_models(a.data(), a.data()); check_models(gen1, a.data());
    a.assign(gen1, gen1 + 14); b.assign(gen2, gen2 + 14);
    for (int k = 1; k < 4; ++k) { a[2 * k] = a[0]; a[2 * k + 1] = a[1]; b[2 * k] = b[0]; b[2 * k + 1] = b[1]; }   // a point four times
    check_models(a.data(), b.data());
    for (int k = 0; k < 7; ++k) { a[2 * k] = 10.0 + 40.0 * k; a[2 * k + 1] = 30.0 + 20.0 * k; }  // exactly collinear
    check_models(a.data(), gen2); check_models(a.data(), a.data());
    a.assign(gen1, gen1 + 14); a[6] = INFINITY; check_models(a.data(), gen2);
    a.assign(gen1, gen1 + 14); a[3] = NAN; check_models(gen1, a.data());
    for (int k = 0; k < 14; ++k) { a[k] = gen1[k] * 1e3 + 1e6; b[k] = gen2[k] * 1e3 + 1e6; }
    check_models(a.data(), b.data());
    for (int k = 0; k < 14; ++k) { a[k] = gen1[k] * 1e150; b[k] = gen2[k] * 1e-150; }           // overflow and underflow inside the solve
    check_models(a.data(), b.data());
    for (int k = 0; k < 7; ++k) { b[2 * k] = 1.1 * gen1[2 * k] - 0.1 * gen1[2 * k + 1] + 12.0; b[2 * k + 1] = 0.2 * gen1[2 * k] + 0.9 * gen1[2 * k + 1] - 7.0; }
    check_models(gen1, b.data());                                                                // an exact affine map
    for (int k = 0; k < 14; ++k) a[k] = 0.0;
    check_models(a.data(), a.data());

    // the cubic rule at its edges
    double x[3];
    const double c0[4] = {0, 0, 0, 0}, c1[4] = {-2, 4, 0, 0}, c2[4] = {2, -3, 1, 0}, c3[4] = {-6, 11, -6, 1}, c4[4] = {1, 1, 1, 1}, c5[4] = {NAN, 1, 1, 1},
                 c6[4] = {1, 0, 1, 0}, c7[4] = {0, 0, 0, 1}, c8[4] = {1e300, -1e300, 1e300, 1e-300}, c9[4] = {INFINITY, 1, 1, 1};
    CHECK(cubic_roots(c0, x) == 0);
    CHECK(cubic_roots(c1, x) == 1 && x[0] == 0.5);
    CHECK(cubic_roots(c2, x) == 2 && x[0] == 1.0 && x[1] == 2.0);
    CHECK(cubic_roots(c3, x) == 3 && std::fabs(x[0] - 1.0) < 1e-14 && std::fabs(x[1] - 2.0) < 1e-14 && std::fabs(x[2] - 3.0) < 1e-14);
    CHECK(cubic_roots(c4, x) == 1 && x[0] == -1.0);
    CHECK(cubic_roots(c5, x) == 0);
    CHECK(cubic_roots(c6, x) == 0);
    CHECK(cubic_roots(c7, x) >= 1 && x[0] == 0.0);
    CHECK(cubic_roots(c8, x) <= 3);
    CHECK(cubic_roots(c9, x) == 0);

    // the re-fit: fewer than 8 points, a mask that leaves fewer than 8, identical points, more points than lanes
    std::vector<float> p1(2 * 600), p2(2 * 600);
    std::vector<unsigned char> mask(600, 0);
    for (int i = 0; i < 600; ++i) { p1[2 * i] = 5.f + (float)((i * 37) % 751); p1[2 * i + 1] = 7.f + (float)((i * 91) % 499); p2[2 * i] = p1[2 * i] + (float)(i % 13) - 6.f; p2[2 * i + 1] = p1[2 * i + 1] + 0.01f * p1[2 * i]; }
    double F[9];
    CHECK(!fundamental_refit_host(p1.data(), p2.data(), 7, nullptr, F));
    CHECK(!fundamental_refit_host(p1.data(), p2.data(), 0, nullptr, F));
    for (int i = 0; i < 7; ++i) mask[50 * i] = 1;
    CHECK(!fundamental_refit_host(p1.data(), p2.data(), 600, mask.data(), F));
    CHECK(fundamental_refit_host(p1.data(), p2.data(), 600, nullptr, F));
    CHECK(fundamental_refit_host(p1.data(), p2.data(), 8, nullptr, F) || F[0] == 0.0);
    std::vector<float> same(2 * 20, 3.5f);
    CHECK(!fundamental_refit_host(same.data(), same.data(), 20, nullptr, F));
    for (int i = 0; i < 9; ++i) CHECK(F[i] == 0.0);

    // the focal cost: one pair, more pairs than lanes, a zero matrix (NaN cost, no fault)
    std::vector<double> Fs(9 * 300), w(300, 1.0), cost(3);
    CHECK(fundamental_refit_host(p1.data(), p2.data(), 600, nullptr, F));
    for (int p = 0; p < 300; ++p) for (int i = 0; i < 9; ++i) Fs[9 * p + i] = F[i];
    const double cand[3] = {230.4, 620.0, 2304.0};
    focal_cost_host(1, Fs.data(), w.data(), 384.0, 256.0, 3, cand, cost.data());
    for (int k = 0; k < 3; ++k) CHECK(cost[k] >= 0.0 && cost[k] <= 1.0);
    const double one = cost[1];
    focal_cost_host(300, Fs.data(), w.data(), 384.0, 256.0, 3, cand, cost.data());
    CHECK(std::fabs(cost[1] - one) < 1e-12);
    for (int i = 0; i < 9; ++i) Fs[i] = 0.0;
    focal_cost_host(1, Fs.data(), w.data(), 384.0, 256.0, 3, cand, cost.data());
    CHECK(std::isnan(cost[0]));

    // the float score: a zero model and a NaN model admit nothing
    const float Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, N[9] = {NAN, 0, 0, 0, 1, 0, 0, 0, 1};
    CHECK(!epipolar_inlier(Z, 1.f, 2.f, 3.f, 4.f, 1.f));
    CHECK(!epipolar_inlier(N, 1.f, 2.f, 3.f, 4.f, 1.f));

    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("fundamental degenerate check ok\n");
    return 0;
}
