// Stand-alone host check of the homography model's host pieces (no GPU call is made):
//   1  p3dv::FeatureMatching::findInitializeFramePair's max_h_inlier_ratio on the hand-made 4-frame table of
//      tests/test_homography_cpu.py (the C++ mirror must choose what the Python member chooses);
//   2  homography_core.hpp's host build -- the minimal solve and the re-fit in the refit kernel's summation order -- on a fixed sample,
//      against constants printed by the Python restatement (tests/homography_ref.py, route (a)), bit for bit;
//   3  ransac_host.hpp's subset check and 4-point sampler on hand-made point sets.
// Built by tests/test_homography_cpu.py, once plainly and once with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>

#include "../../easysfm_amd/host/esfm_host.hpp"
#include "../../easysfm_amd/csrc/homography_core.hpp"
#include "../../easysfm_amd/csrc/ransac_host.hpp"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static bool same_bits(const double *a, const double *b, int n) { return std::memcmp(a, b, sizeof(double) * size_t(n)) == 0; }

static int check_init_pair()
{
    using namespace p3dv;
    // tracks 0-9: frames 2, 3; tracks 10-15: frames 1, 2; tracks 16-21: frames 0, 1.  Scores: (3,2) = 20, (2,1) = 12, (1,0) = 12, others 0.
    std::vector<std::vector<bool>> track(4, std::vector<bool>(22, false));
    for (int t = 0; t < 10; ++t) track[2][size_t(t)] = track[3][size_t(t)] = true;
    for (int t = 10; t < 16; ++t) track[1][size_t(t)] = track[2][size_t(t)] = true;
    for (int t = 16; t < 22; ++t) track[0][size_t(t)] = track[1][size_t(t)] = true;
    std::vector<frame_t> frames(4);
    std::vector<std::vector<double>> depth(4, std::vector<double>(4, 5.0)), ratio(4, std::vector<double>(4, 0.05));
    ratio[3][2] = 0.95;
    FeatureMatching fm;
    fm.quiet = true;
    int a = -1, b = -1, cand = -1, skip = -1;
    double d = 0.0;
    CHECK(fm.findInitializeFramePair(track, frames, depth, a, b, d, 5, 50.0) && a == 3 && b == 2);                      // no limit: the best score
    CHECK(fm.findInitializeFramePair(track, frames, depth, a, b, d, 5, 50.0, -1.0, &ratio) && a == 3 && b == 2);        // limit off: the table is not looked at
    CHECK(fm.findInitializeFramePair(track, frames, depth, a, b, d, 5, 50.0, 0.8, &ratio, &cand, &skip) && a == 2 && b == 1);   // skipped; the tie goes to the later pair
    CHECK(cand == 6 && skip == 1);
    CHECK(fm.findInitializeFramePair(track, frames, depth, a, b, d, 5, 50.0, 0.95, &ratio) && a == 3 && b == 2);        // `>`: a ratio AT the limit stays
    depth[2][1] = 60.0;                                                                                                 // the depth guard comes first
    CHECK(fm.findInitializeFramePair(track, frames, depth, a, b, d, 5, 50.0, 0.8, &ratio, &cand, &skip) && a == 1 && b == 0);
    CHECK(cand == 5 && skip == 1);
    ratio[1][0] = 0.9; ratio[2][1] = 0.9;
    depth[2][1] = 5.0;
    CHECK(!fm.findInitializeFramePair(track, frames, depth, a, b, d, 5, 50.0, 0.8, &ratio, &cand, &skip) && a == 1 && b == 0);   // every scoring pair skipped: the default pair
    CHECK(skip == 3);
    // the member exists with the documented signature (it needs a GPU to run)
    bool (MotionEstimator::*member)(frame_t &, frame_t &, std::vector<DMatch> &, std::vector<DMatch> &, double *, double, double, int *) = &MotionEstimator::estimate2D2D_H4P_RANSAC;
    CHECK(member != nullptr);
    return 0;
}

static int check_core()
{
    using namespace esfm::homog;
    const double p1[8] = {12.5, 20.25, 300.75, 41.5, 280.0, 330.125, 25.5, 310.0};
    const double p2[8] = {15.0, 18.5, 310.25, 52.0, 275.5, 345.75, 18.25, 298.5};
    const double want[9] = {0x1.e936f95c411e0p-1, -0x1.00aec0dce3cf5p-5, 0x1.d42b479077156p+1, 0x1.0ea2a142af799p-5, 0x1.efcd67edea951p-1,
                            -0x1.903389a7dfff4p+0, -0x1.d5b9fb07c2aeep-13, 0x1.e5567108f47f2p-16, 0x1.0000000000000p+0};
    double H[9];
    CHECK(homography_from_4(p1, p2, H));
    CHECK(same_bits(H, want, 9));
    // four identical points: no model, zeros
    const double same[8] = {37.5, 91.25, 37.5, 91.25, 37.5, 91.25, 37.5, 91.25};
    CHECK(!homography_from_4(same, same, H));
    for (int k = 0; k < 9; ++k) CHECK(H[k] == 0.0);
    // the re-fit on seven points, the sixth masked out
    const float a[14] = {12.5f, 20.25f, 300.75f, 41.5f, 280.0f, 330.125f, 25.5f, 310.0f, 150.5f, 160.25f, 90.0f, 250.5f, 220.25f, 80.0f};
    const float b[14] = {0x1.e000000000000p+3f, 0x1.2800000000000p+4f, 0x1.3640000000000p+8f, 0x1.a000000000000p+5f, 0x1.1380000000000p+8f,
                         0x1.59c0000000000p+8f, 0x1.2400000000000p+4f, 0x1.2a80000000000p+8f, 0x1.25e8740000000p+7f, 0x1.472cfe0000000p+7f,
                         0x1.4b7e5e0000000p+6f, 0x1.ee5a7a0000000p+7f, 0x1.bc14020000000p+7f, 0x1.5d25040000000p+6f};
    const unsigned char mask[7] = {1, 1, 1, 1, 1, 0, 1};
    const double want_refit[9] = {0x1.e987d42a9a059p-1, -0x1.fdc5762abb419p-6, 0x1.d3ee7a879d33cp+1, 0x1.104ab2b7286f3p-5, 0x1.f032b8e366465p-1,
                                  -0x1.94519d5f39a52p+0, -0x1.d2c960775e5a7p-13, 0x1.fe2f542ddf779p-16, 0x1.0000000000000p+0};
    CHECK(homography_refit_host(a, b, 7, mask, H));
    CHECK(same_bits(H, want_refit, 9));
    const unsigned char three[7] = {1, 0, 1, 0, 0, 0, 1};
    CHECK(!homography_refit_host(a, b, 7, three, H));            // fewer than four inliers
    // the float transfer error: a point the model maps exactly is an inlier at threshold 0
    float Hf[9] = {1.f, 0.f, 2.f, 0.f, 1.f, -3.f, 0.f, 0.f, 1.f};
    CHECK(transfer_inlier(Hf, 10.f, 20.f, 12.f, 17.f, 0.f));
    CHECK(!transfer_inlier(Hf, 10.f, 20.f, 13.f, 17.f, 0.99f) && transfer_inlier(Hf, 10.f, 20.f, 13.f, 17.f, 1.f));   // err = 1: `<=`
    return 0;
}

static int check_sampler()
{
    using namespace esfm::ransac;
    const float sq[8] = {0.f, 0.f, 100.f, 0.f, 100.f, 100.f, 0.f, 100.f};
    const float flipped[8] = {0.f, 0.f, 100.f, 0.f, 0.f, 100.f, 100.f, 100.f};       // corners 2 and 3 swapped: orientation of two triples flips
    const float mirrored[8] = {100.f, 0.f, 0.f, 0.f, 0.f, 100.f, 100.f, 100.f};      // a reflection: all four flip, which is consistent
    const float line[8] = {0.f, 0.f, 50.f, 50.f, 100.f, 100.f, 0.f, 100.f};          // points 0, 1, 2 collinear
    const float twice[8] = {0.f, 0.f, 0.f, 0.f, 100.f, 100.f, 0.f, 100.f};           // points 0 and 1 coincide
    const int32_t id[4] = {0, 1, 2, 3};
    CHECK(check_subset4(sq, sq, id));
    CHECK(!check_subset4(sq, flipped, id));
    CHECK(check_subset4(sq, mirrored, id));
    CHECK(!check_subset4(line, sq, id) && !check_subset4(sq, line, id));
    CHECK(!check_subset4(twice, sq, id));
    // on four usable points every draw is a permutation of them; on a collinear set the sampler gives up after its 1000 attempts
    CvRng rng;
    int32_t idx[4];
    int64_t redraws = 0;
    CHECK(draw_subset(rng, 4, sq, sq, idx, &redraws) && redraws == 0);
    CHECK((1 << idx[0] | 1 << idx[1] | 1 << idx[2] | 1 << idx[3]) == 15);
    CvRng rng2;
    CHECK(!draw_subset(rng2, 4, line, sq, idx, &redraws) && redraws == kSubsetAttempts);
    // the 5-point form is untouched: same stream as before from a fresh generator
    CvRng r5;
    int32_t i5[5];
    draw_subset(r5, 100, i5);
    for (int k = 0; k < 5; ++k) CHECK(i5[k] >= 0 && i5[k] < 100);
    CHECK(update_num_iters(0.995, 0.5, 4, 2000) == 82);          // log(0.005) / log(1 - 0.5^4) = 82.1
    return 0;
}

int main()
{
    if (check_init_pair() || check_core() || check_sampler()) return 1;
    std::printf("homography check ok\n");
    return 0;
}
