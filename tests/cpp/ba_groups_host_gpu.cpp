// GPU test of the C++ BundleAdjustment mirror (easysfm_amd/host/esfm_host.hpp) in multiple-camera mode: doSFMBA over frames of two
// cameras, the assertions of tests/test_ba_groups_gpu.py::test_mirror_doSFMBA_writes_each_group_its_own_intrinsics.  The scene comes
// from the file named on the command line (written by the test): n_cam n_pt; per camera: camera_id, fx cx fy cy (start), the true fx,
// the 3 x 4 pose, n_obs and per observation the point index and the pixel; then the points.
#include <cmath>
#include <cstdio>
#include <fstream>

#include "../../easysfm_amd/host/esfm_host.hpp"

using namespace p3dv;

namespace {
int g_failed = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond) && g_failed++ < 40) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);    \
    } while (0)
}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s scene.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    int n_cam = 0, n_pt = 0;
    in >> n_cam >> n_pt;
    std::vector<frame_t> frames;
    std::vector<double> true_fx, start_fx;
    for (int c = 0; c < n_cam; ++c) {
        frame_t fr((unsigned)c, "");
        double fx, cx, fy, cy, tfx;
        in >> fr.camera_id >> fx >> cx >> fy >> cy >> tfx;
        fr.K_cam(0, 0) = float(fx); fr.K_cam(0, 2) = float(cx); fr.K_cam(1, 1) = float(fy); fr.K_cam(1, 2) = float(cy);
        true_fx.push_back(tfx); start_fx.push_back(double(float(fx)));
        for (int r = 0; r < 3; ++r) for (int k = 0; k < 4; ++k) { double v; in >> v; fr.pose_cam(r, k) = float(v); }
        int n_obs = 0;
        in >> n_obs;
        for (int o = 0; o < n_obs; ++o) {
            int pid; double u, v;
            in >> pid >> u >> v;
            KeyPoint kp; kp.pt.x = float(u); kp.pt.y = float(v);
            fr.keypoints.push_back(kp);
            fr.unique_pixel_ids.push_back(pid);
            fr.unique_pixel_has_match.push_back(true);
        }
        frames.push_back(fr);
    }
    pointcloud_sparse_t cloud;
    for (int p = 0; p < n_pt; ++p) {
        double x, y, z;
        in >> x >> y >> z;
        PointXYZRGB q; q.x = float(x); q.y = float(y); q.z = float(z);
        cloud.points.push_back(q);
        cloud.unique_point_ids.push_back(p);
    }
    if (!in) { fprintf(stderr, "cannot read the scene\n"); return 2; }
    std::vector<bool> process(size_t(n_cam), false);
    const Matrix4f pose0 = frames[0].pose_cam;
    const std::vector<frame_t> before = frames;

    BundleAdjustment ba;
    CHECK(ba.doSFMBA(frames, process, cloud, 25.0, 0));
    CHECK(ba.group_camera_ids_ == std::vector<int>({0, 1}) && ba.num_parameters_ == 6 * n_cam + 3 * n_pt + 8);
    CHECK(ba.ref_process_camera_id_ == 0 && ba.summary_.final_cost < ba.summary_.initial_cost);
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 4; ++k) CHECK(std::fabs(frames[0].pose_cam(r, k) - pose0(r, k)) <= 1e-6f);
    int first[2] = {-1, -1};
    for (int c = 0; c < n_cam; ++c) {
        const int g = frames[size_t(c)].camera_id;
        if (first[g] < 0) first[g] = c;
        const Matrix3f &K = frames[size_t(c)].K_cam, &K1 = frames[size_t(first[g])].K_cam;
        // each group's frames receive that group's K, and only it: the float of the group's block
        const double *k4 = ba.mutable_calib() + 4 * g;
        CHECK(K(0, 0) == float(k4[0]) && K(0, 2) == float(k4[1]) && K(1, 1) == float(k4[2]) && K(1, 2) == float(k4[3]));
        CHECK(K(0, 0) == K1(0, 0) && K(0, 2) == K1(0, 2) && K(1, 1) == K1(1, 1) && K(1, 2) == K1(1, 2));
        CHECK(std::fabs(double(K(0, 0)) - true_fx[size_t(c)]) < 0.2 * std::fabs(start_fx[size_t(c)] - true_fx[size_t(c)]));
        const Matrix3f &K0 = before[size_t(c)].K_cam;
        CHECK(std::fabs(K(0, 0) - K0(0, 0)) <= 25.001f && std::fabs(K(0, 2) - K0(0, 2)) <= 25.001f && std::fabs(K(1, 1) - K0(1, 1)) <= 25.001f &&
              std::fabs(K(1, 2) - K0(1, 2)) <= 25.001f);
    }
    CHECK(first[0] >= 0 && first[1] >= 0 && frames[size_t(first[0])].K_cam(0, 0) != frames[size_t(first[1])].K_cam(0, 0));
    printf("fx: camera 0 %.3f (true %.3f), camera 1 %.3f (true %.3f); cost %.4f -> %.4f\n", frames[size_t(first[0])].K_cam(0, 0), true_fx[size_t(first[0])],
           frames[size_t(first[1])].K_cam(0, 0), true_fx[size_t(first[1])], ba.summary_.initial_cost, ba.summary_.final_cost);

    // the same frames with every camera_id 0: the shared block of calibs_[0], one K for all frames afterwards
    std::vector<frame_t> one = before;
    for (frame_t &f : one) f.camera_id = 0;
    pointcloud_sparse_t cloud2;
    cloud2.points = cloud.points; cloud2.unique_point_ids = cloud.unique_point_ids;
    BundleAdjustment bb;
    CHECK(bb.doSFMBA(one, process, cloud2, 25.0, 0));
    CHECK(bb.group_camera_ids_.empty() && bb.num_parameters_ == 6 * n_cam + 3 * n_pt + 4);
    for (const frame_t &f : one) CHECK(f.K_cam(0, 0) == one[0].K_cam(0, 0) && f.K_cam(1, 1) == one[0].K_cam(1, 1));

    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("ba groups host gpu ok\n");
    return 0;
}
