// GPU program: the two ways the native driver reaches the homography statistic -- the per-pair member
// MotionEstimator::estimate2D2D_H4P_RANSAC (ESFM_PAIR_BY_PAIR=1) and the batch estimate2D2D_H4P_RANSAC_pairs -- on correspondence sets
// handed in by tests/test_init_degeneracy_gpu.py.  Input file: int32 n_jobs, then per job int32 n, n x 2 floats (image 1), n x 2 floats
// (image 2).  One line per job: "job p per_pair <n_inliers> mask <matches appended> batch <n_inliers>"; the test compares them with each
// other and with the Python pipeline's h_inliers.
#include <cstdio>
#include <fstream>

#include "../../easysfm_amd/host/esfm_host.hpp"

using namespace p3dv;

int main(int argc, char **argv)
{
    if (argc != 3) { std::printf("usage: homography_paths input.bin threshold\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const double threshold = std::atof(argv[2]);
    int32_t n_jobs = 0;
    in.read(reinterpret_cast<char *>(&n_jobs), 4);
    if (!in || n_jobs < 0 || n_jobs > 4096) { std::printf("bad input\n"); return 2; }
    std::vector<frame_t> frames(size_t(2 * n_jobs));
    std::vector<std::pair<int, int>> jobs;
    std::vector<std::vector<DMatch>> matches(static_cast<size_t>(n_jobs));
    for (int p = 0; p < n_jobs; ++p) {
        int32_t n = 0;
        in.read(reinterpret_cast<char *>(&n), 4);
        if (!in || n < 0 || n > (1 << 20)) { std::printf("bad input\n"); return 2; }
        std::vector<float> a(size_t(2 * n)), b(size_t(2 * n));
        in.read(reinterpret_cast<char *>(a.data()), std::streamsize(sizeof(float) * a.size()));
        in.read(reinterpret_cast<char *>(b.data()), std::streamsize(sizeof(float) * b.size()));
        if (!in) { std::printf("short input\n"); return 2; }
        frame_t &f1 = frames[size_t(2 * p)], &f2 = frames[size_t(2 * p + 1)];
        f1.keypoints.resize(size_t(n)); f2.keypoints.resize(size_t(n));
        for (int i = 0; i < n; ++i) {
            f1.keypoints[size_t(i)].pt.x = a[size_t(2 * i)]; f1.keypoints[size_t(i)].pt.y = a[size_t(2 * i + 1)];
            f2.keypoints[size_t(i)].pt.x = b[size_t(2 * i)]; f2.keypoints[size_t(i)].pt.y = b[size_t(2 * i + 1)];
            matches[size_t(p)].emplace_back(i, i, 0, 0.f);
        }
        jobs.emplace_back(2 * p, 2 * p + 1);
    }
    MotionEstimator ee;
    std::vector<int> batch;
    if (!ee.estimate2D2D_H4P_RANSAC_pairs(frames, jobs, matches, batch, threshold)) { std::printf("batch failed: %s\n", esfm_last_error()); return 1; }
    for (int p = 0; p < n_jobs; ++p) {
        std::vector<DMatch> appended;
        int count = -1;
        double H[9];
        const bool found = ee.estimate2D2D_H4P_RANSAC(frames[size_t(2 * p)], frames[size_t(2 * p + 1)], matches[size_t(p)], appended, H, threshold, 0.995, &count);
        std::printf("job %d per_pair %d mask %d batch %d found %d\n", p, count, int(appended.size()), batch[size_t(p)], found ? 1 : 0);
    }
    return 0;
}
