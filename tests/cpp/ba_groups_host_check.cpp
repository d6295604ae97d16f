// The packing of the C++ BundleAdjustment mirror (easysfm_amd/host/esfm_host.hpp) in multiple-camera mode: one intrinsics block per
// distinct camera_id of the processed frames, in order of first appearance, started from that group's first frame's K_cam; one
// distinct id is the shared block exactly as before.  Host only: setBAProblem launches nothing (tests/test_ba_groups_cpu.py builds it).
#include <cstdio>

#include "../../easysfm_amd/host/esfm_host.hpp"

using namespace p3dv;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond) && g_failed++ < 40) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);    \
    } while (0)

void make(const std::vector<int> &ids, std::vector<frame_t> &frames, pointcloud_sparse_t &cloud)
{
    const int n_pt = 40;
    frames.clear();
    cloud = pointcloud_sparse_t();
    for (int p = 0; p < n_pt; ++p) {
        PointXYZRGB q; q.x = float(0.1 * p); q.y = float(1.0 - 0.05 * p); q.z = float(5.0 + 0.01 * p);
        cloud.points.push_back(q);
        cloud.unique_point_ids.push_back(100 + p);
    }
    for (size_t c = 0; c < ids.size(); ++c) {
        frame_t fr((unsigned)c, "");
        for (int p = 0; p < n_pt; ++p) {
            KeyPoint kp; kp.pt.x = float(10 * c + p); kp.pt.y = float(3 * p);
            fr.keypoints.push_back(kp);
        }
        fr.init_pixel_ids();
        for (int p = 0; p < n_pt; ++p) { fr.unique_pixel_ids[size_t(p)] = 100 + p; fr.unique_pixel_has_match[size_t(p)] = true; }
        fr.K_cam(0, 0) = float(2000 + c); fr.K_cam(0, 2) = float(700 + c); fr.K_cam(1, 1) = float(2100 + c); fr.K_cam(1, 2) = float(500 + c);
        fr.camera_id = ids[c];
        frames.push_back(fr);
    }
}

}  // namespace

int main()
{
    std::vector<frame_t> frames;
    pointcloud_sparse_t cloud;
    std::vector<bool> process = {false, true, false, false, false, false};   // frame 1 is not processed
    {
        make({7, 3, 7, 3, 5, 7}, frames, cloud);
        CHECK(frame_t().camera_id == 0);
        BundleAdjustment ba;
        ba.setBAProblem(frames, process, cloud, 25.0, 0);
        CHECK(ba.group_camera_ids_ == std::vector<int>({7, 3, 5}));
        CHECK(ba.camera_group_ == std::vector<int>({0, 0, 1, 2, 0}));
        CHECK(ba.num_cameras_ == 5 && ba.num_parameters_ == 6 * 5 + 3 * 40 + 4 * 3 && (int)ba.parameters_.size() == ba.num_parameters_);
        const int first[3] = {0, 3, 4};
        for (int g = 0; g < 3; ++g) {
            const Matrix3f &K = frames[size_t(first[g])].K_cam;
            const double *k4 = ba.mutable_calib() + 4 * g;
            CHECK(k4[0] == K(0, 0) && k4[1] == K(0, 2) && k4[2] == K(1, 1) && k4[3] == K(1, 2));
        }
        // fixed intrinsics: camera ids play no part
        ba.initBA();
        ba.setBAProblem(frames, process, cloud, 0.0, 0);
        CHECK(ba.group_camera_ids_.empty() && ba.camera_group_.empty() && ba.num_parameters_ == 6 * 5 + 3 * 40);
    }
    {
        // one distinct id among the processed frames: the shared block of calibs_[0], the same parameters whatever the id is called
        std::vector<frame_t> other;
        pointcloud_sparse_t cloud2;
        make({4, 9, 4, 4, 4, 4}, frames, cloud);
        make({0, 0, 0, 0, 0, 0}, other, cloud2);
        BundleAdjustment a, b;
        a.setBAProblem(frames, process, cloud, 25.0, 0);
        b.setBAProblem(other, process, cloud2, 25.0, 0);
        CHECK(a.group_camera_ids_.empty() && a.camera_group_.empty() && a.num_parameters_ == 6 * 5 + 3 * 40 + 4);
        CHECK(a.parameters_ == b.parameters_);
        const Matrix3f &K = frames[0].K_cam;
        const double *k4 = a.mutable_calib();
        CHECK(k4[0] == K(0, 0) && k4[1] == K(0, 2) && k4[2] == K(1, 1) && k4[3] == K(1, 2));
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("ba groups host check ok\n");
    return 0;
}
