// The packing of the C++ BundleAdjustment mirror (easysfm_amd/host/esfm_host.hpp) with free radial distortion: a positive
// radial_tolerance opens one block fx, cx, fy, cy, k1, k2 per distinct camera_id of the processed frames -- ONE id included --, in order
// of first appearance, started from that group's first frame's K_cam and radial_cam; keypoints_raw are observed where a frame has them;
// a tolerance of 0, or the argument left out, is the packing as before.  Host only: setBAProblem launches nothing
// (tests/test_radial_host_cpu.py builds it).
#include <cstdio>

#include "../../easysfm_amd/host/esfm_host.hpp"

using namespace p3dv;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond) && g_failed++ < 40) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);    \
    } while (0)

void make(const std::vector<int> &ids, std::vector<frame_t> &frames, pointcloud_sparse_t &cloud, bool with_radial)
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
        if (with_radial) { fr.radial_cam[0] = -0.01 * double(c + 1); fr.radial_cam[1] = 0.001 * double(c + 1); }
        frames.push_back(fr);
    }
}

}  // namespace

int main()
{
    std::vector<frame_t> frames;
    pointcloud_sparse_t cloud;
    std::vector<bool> process = {false, true, false, false, false, false};   // frame 1 is not processed
    const int n0 = 6 * 5 + 3 * 40;
    {
        make({7, 3, 7, 3, 5, 7}, frames, cloud, true);
        CHECK(frame_t().radial_cam[0] == 0.0 && frame_t().radial_cam[1] == 0.0 && frame_t().keypoints_raw.empty());
        // frame 2 (processed camera 1) carries raw pixels: those are observed
        for (const KeyPoint &kp : frames[2].keypoints) { Point2f q = kp.pt; q.x += 1.0f; q.y += 1.0f; frames[2].keypoints_raw.push_back(q); }
        BundleAdjustment ba;
        ba.setBAProblem(frames, process, cloud, 25.0, 0, 0.5);
        CHECK(ba.radial_tolerance_ == 0.5);
        CHECK(ba.group_camera_ids_ == std::vector<int>({7, 3, 5}));
        CHECK(ba.camera_group_ == std::vector<int>({0, 0, 1, 2, 0}));
        CHECK(ba.num_cameras_ == 5 && ba.num_parameters_ == n0 + 4 * 3 + 2 * 3 && (int)ba.parameters_.size() == ba.num_parameters_);
        CHECK(ba.mutable_radial() == ba.mutable_calib() + 12);
        // solveBA takes the tolerance too, positive exactly when the problem was set up with radial blocks: refused before any GPU work
        CHECK(!ba.solveBA(25.0) && !ba.solveBA(25.0, 0.0));
        const int first[3] = {0, 3, 4};
        for (int g = 0; g < 3; ++g) {
            const frame_t &fr = frames[size_t(first[g])];
            const double *k4 = ba.mutable_calib() + 4 * g, *k2 = ba.mutable_radial() + 2 * g;
            CHECK(k4[0] == fr.K_cam(0, 0) && k4[1] == fr.K_cam(0, 2) && k4[2] == fr.K_cam(1, 1) && k4[3] == fr.K_cam(1, 2));
            CHECK(k2[0] == fr.radial_cam[0] && k2[1] == fr.radial_cam[1]);
        }
        for (int k = 0; k < ba.num_observations_; ++k) {
            const int p = ba.point_index_[size_t(k)];
            const frame_t &fr = frames[ba.camera_index_[size_t(k)] == 0 ? 0 : size_t(ba.camera_index_[size_t(k)] + 1)];
            const Point2f want = ba.camera_index_[size_t(k)] == 1 ? fr.keypoints_raw[size_t(p)] : fr.keypoints[size_t(p)].pt;
            CHECK(ba.points_2d_[size_t(k)].x == want.x && ba.points_2d_[size_t(k)].y == want.y);
        }
        // a tolerance of 0, and the argument left out: the packing as before -- radial_cam and keypoints_raw play no part
        std::vector<frame_t> plain;
        pointcloud_sparse_t cloud2;
        make({7, 3, 7, 3, 5, 7}, plain, cloud2, false);
        BundleAdjustment a, b, c;
        a.setBAProblem(frames, process, cloud, 25.0, 0, 0.0);
        b.setBAProblem(frames, process, cloud, 25.0, 0);
        c.setBAProblem(plain, process, cloud2, 25.0, 0);
        CHECK(a.radial_tolerance_ == 0.0 && a.num_parameters_ == n0 + 4 * 3);
        CHECK(!a.solveBA(25.0, 0.5));
        CHECK(a.parameters_ == b.parameters_ && a.parameters_ == c.parameters_);
        for (int k = 0; k < a.num_observations_; ++k) CHECK(a.points_2d_[size_t(k)].x == c.points_2d_[size_t(k)].x && a.points_2d_[size_t(k)].y == c.points_2d_[size_t(k)].y);
    }
    {
        // ONE camera id still opens a radial block, with fixed pinhole intrinsics too
        make({4, 4, 4, 4, 4, 4}, frames, cloud, true);
        BundleAdjustment ba;
        ba.setBAProblem(frames, process, cloud, 0.0, 0, 0.5);
        CHECK(ba.group_camera_ids_ == std::vector<int>({4}) && ba.camera_group_ == std::vector<int>({0, 0, 0, 0, 0}));
        CHECK(ba.num_parameters_ == n0 + 4 + 2);
        CHECK(ba.mutable_calib()[0] == frames[0].K_cam(0, 0) && ba.mutable_radial()[0] == frames[0].radial_cam[0] && ba.mutable_radial()[1] == frames[0].radial_cam[1]);
        // ... and without the tolerance the fixed-intrinsics packing
        ba.initBA();
        ba.setBAProblem(frames, process, cloud, 0.0, 0);
        CHECK(ba.group_camera_ids_.empty() && ba.num_parameters_ == n0 && ba.radial_tolerance_ == 0.0);
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("ba radial host check ok\n");
    return 0;
}
