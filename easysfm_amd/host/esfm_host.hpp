// C++ host mirror of the reference's hot-path interface over the C ABI (include/esfm.h).
//
// Same class and member names, argument meaning, defaults and error behaviour as
//   p3dv::FeatureMatching::matchFeaturesORB / matchFeaturesSURF   cpp_code/include/feature_matching.h:17-21
//   p3dv::BundleAdjustment::{initBA,setBAProblem,solveBA,doSFMBA}  cpp_code/include/ba.h:59-84
//   p3dv::MotionEstimator::{estimate2D2D_E5P_RANSAC,getDepthFast,doTriangulation,estimate2D3D_P3P_RANSAC,outlierFilter}
//                                                                  cpp_code/include/estimate_motion.h:17-35
// with the OpenCV / PCL / Eigen value types of cpp_code/include/utility.h:21-102 replaced by the
// plain structs below (the image has none of those libraries).  Header-only; link libesfm_hip.so.
// All compute happens on the GPU behind the C ABI; there is no CPU fallback here.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <memory>
#include <vector>

#include "../../include/esfm.h"
#include "esfm_jpeg.hpp"   // (pulls in esfm_png.hpp and read_image_bgr)

namespace p3dv {

// ---- value types (utility.h) ------------------------------------------------------------------
struct DMatch {  // cv::DMatch
    int queryIdx = -1, trainIdx = -1, imgIdx = 0;
    float distance = 0.f;
    DMatch() = default;
    DMatch(int q, int t, int img, float d) : queryIdx(q), trainIdx(t), imgIdx(img), distance(d) {}
};

struct Point2f { float x = 0.f, y = 0.f; };
struct KeyPoint {  // cv::KeyPoint (only .pt is read downstream, ba.cpp:37)
    Point2f pt;
    float size = 0.f, angle = -1.f, response = 0.f;
    int octave = 0, class_id = -1;
};

// cv::Mat restricted to what descriptors need: CV_32F (SURF, N x 64) or CV_8U (ORB, N x 32), continuous
struct DescMat {
    enum Type { F32 = 0, U8 = 1 };
    int rows = 0, cols = 0;
    Type type = F32;
    std::vector<uint8_t> bytes;
    void create(int r, int c, Type t) { rows = r; cols = c; type = t; bytes.assign(size_t(r) * c * (t == F32 ? 4 : 1), 0); }
    template <class T> T *ptr(int r = 0) { return reinterpret_cast<T *>(bytes.data()) + size_t(r) * cols; }
    template <class T> const T *ptr(int r = 0) const { return reinterpret_cast<const T *>(bytes.data()) + size_t(r) * cols; }
};

template <int R, int C> struct Matf {  // Eigen::Matrix<float,R,C>, (r,c) access
    float v[R * C];
    Matf() { for (auto &x : v) x = 0.f; }
    float &operator()(int r, int c) { return v[r * C + c]; }
    float operator()(int r, int c) const { return v[r * C + c]; }
    static Matf Identity() { Matf m; for (int i = 0; i < (R < C ? R : C); ++i) m(i, i) = 1.f; return m; }
};
using Matrix3f = Matf<3, 3>;
using Matrix4f = Matf<4, 4>;

struct ImageMat {  // cv::Mat, CV_8UC1 / CV_8UC3 (BGR, interleaved), row-major and continuous
    int rows = 0, cols = 0, channels = 3;
    std::vector<uint8_t> data;
    bool empty() const { return data.empty(); }
};
struct DistortMat {  // the 1 x 4 CV_64FC1 matrix sfm.cpp:78 creates: zeros
    double v[4] = {0, 0, 0, 0};
};

struct frame_t {  // utility.h:21-55
    unsigned int frame_id = 0;
    std::string image_file_path;
    ImageMat rgb_image;
    std::vector<KeyPoint> keypoints;
    DescMat descriptors;
    std::vector<int> unique_pixel_ids;
    std::vector<bool> unique_pixel_has_match;
    Matrix4f pose_cam = Matrix4f::Identity();
    Matrix3f K_cam = Matrix3f::Identity();
    int camera_id = 0;  // multiple-camera mode: which physical camera (intrinsics model) took the frame; not in the reference's frame_t
    // free radial distortion (BundleAdjustment's radial_tolerance; not in the reference's frame_t): k1, k2 of the frame's camera, and
    // the pixels as detected (empty: `keypoints` are what bundle adjustment observes)
    double radial_cam[2] = {0.0, 0.0};
    std::vector<Point2f> keypoints_raw;
    frame_t() = default;
    frame_t(unsigned int id, const std::string &path) : frame_id(id), image_file_path(path) {}
    bool init_pixel_ids()
    {
        unique_pixel_ids.assign(keypoints.size(), -1);
        unique_pixel_has_match.assign(keypoints.size(), false);
        return true;
    }
};

struct PointXYZRGB { float x = 0, y = 0, z = 0; uint8_t r = 0, g = 0, b = 0; };  // pcl::PointXYZRGB
// a merged dense point (DenseReconstruction::reconstructMerged): normal (0, 0, 0) = none, members, bit v of views = seen by view v
struct PointXYZRGBNormal { float x = 0, y = 0, z = 0, nx = 0, ny = 0, nz = 0; uint8_t r = 0, g = 0, b = 0; int32_t members = 0; uint64_t views = 0; };
// an indexed triangle mesh (DenseReconstruction::reconstructMesh): oriented, coloured vertices (members and views unused), three
// vertex indices per triangle, and the volume it was extracted from
struct TriangleMesh {
    std::vector<PointXYZRGBNormal> vertices;
    std::vector<int32_t> triangles;
    float voxel_size = 0.f;
    int32_t dims[3] = {0, 0, 0};
    float origin[3] = {0.f, 0.f, 0.f};   // of the volume it was extracted from
};

struct pointcloud_sparse_t {  // utility.h:88-102 (rgb_pointcloud->points flattened)
    std::vector<PointXYZRGB> points;
    std::vector<int> unique_point_ids;
    std::vector<int> is_inlier;
};

// ---- library context ----------------------------------------------------------------------------
class EsfmError : public std::runtime_error {
public:
    int status;
    EsfmError(int s, const std::string &m) : std::runtime_error(m), status(s) {}
};

inline esfm_ctx *default_ctx()
{
    static thread_local esfm_ctx *ctx = nullptr;
    if (!ctx) {
        int rc = esfm_ctx_create(0, nullptr, &ctx);
        if (rc != ESFM_OK) throw EsfmError(rc, esfm_last_error());
    }
    return ctx;
}

// ---- matching (feature_matching.h:17-21) ----------------------------------------------------------
class FeatureMatching {
public:
    // feature_matching.cpp:43-69: SURF::create(minHessian)->detect + SURF::create()->compute on cur_frame.rgb_image (BGR)
    bool detectFeaturesSURF(frame_t &cur_frame, int minHessian = 400, bool show = false)
    {
        (void)show;
        const ImageMat &img = cur_frame.rgb_image;
        if (img.empty()) { std::cerr << "frame has no image" << std::endl; return false; }
        // room for every possible maximum (a quarter of the pixels), NOT zero-filled (the library writes the n rows it returns and
        // nothing else: a value-initialised std::vector of these 28 MB cost 7 - 8 ms per 768 x 512 image in page faults) and KEPT
        // between frames: the device-to-host copies land here, the runtime pins what it copies into, and unmapping pinned pages at the
        // end of every call showed up as 15 - 35 ms stalls in the next frames' calls
        const int cap = img.rows * img.cols / 4 + 1024;
        float *kp = scratch_f32(kp_buf_, kp_cap_, size_t(7) * size_t(cap)), *desc = scratch_f32(desc_buf_, desc_cap_, size_t(64) * size_t(cap));
        int32_t n = 0;
        if (esfm_surf_detect_and_compute(default_ctx(), img.data.data(), img.rows, img.cols, img.channels, double(minHessian), cap, kp, desc, &n) != ESFM_OK) {
            std::cerr << esfm_last_error() << std::endl;
            return false;
        }
        cur_frame.keypoints.resize(size_t(n));
        for (int k = 0; k < n; ++k) {
            KeyPoint &q = cur_frame.keypoints[size_t(k)];
            const float *v = &kp[size_t(7) * size_t(k)];
            q.pt.x = v[0]; q.pt.y = v[1]; q.size = v[2]; q.angle = v[3]; q.response = v[4]; q.octave = int(v[5]); q.class_id = int(v[6]);
        }
        cur_frame.descriptors.create(n, 64, DescMat::F32);
        if (n) std::memcpy(cur_frame.descriptors.ptr<float>(), desc, sizeof(float) * size_t(64) * size_t(n));
        if (!quiet) std::cout << "Found " << n << " features." << std::endl;
        return true;
    }

    // feature_matching.cpp:14-41: ORB::create(max_num)->detect + ->compute on cur_frame.rgb_image (BGR)
    bool detectFeaturesORB(frame_t &cur_frame, int max_num = 5000, bool show = false)
    {
        (void)show;
        const ImageMat &img = cur_frame.rgb_image;
        if (img.empty()) { std::cerr << "frame has no image" << std::endl; return false; }
        const int cap = 2 * max_num + 4096;       // retainBest keeps ties
        float *kp = scratch_f32(kp_buf_, kp_cap_, size_t(7) * size_t(cap));                       // (kept between frames: see detectFeaturesSURF)
        uint8_t *desc = reinterpret_cast<uint8_t *>(scratch_f32(desc_buf_, desc_cap_, size_t(8) * size_t(cap)));
        int32_t n = 0;
        if (esfm_orb_detect_and_compute(default_ctx(), img.data.data(), img.rows, img.cols, img.channels, max_num, cap, kp, desc, &n) != ESFM_OK) {
            std::cerr << esfm_last_error() << std::endl;
            return false;
        }
        cur_frame.keypoints.resize(size_t(n));
        for (int k = 0; k < n; ++k) {
            KeyPoint &q = cur_frame.keypoints[size_t(k)];
            const float *v = &kp[size_t(7) * size_t(k)];
            q.pt.x = v[0]; q.pt.y = v[1]; q.size = v[2]; q.angle = v[3]; q.response = v[4]; q.octave = int(v[5]); q.class_id = int(v[6]);
        }
        cur_frame.descriptors.create(n, 32, DescMat::U8);
        if (n) std::memcpy(cur_frame.descriptors.ptr<uint8_t>(), desc, size_t(32) * size_t(n));
        if (!quiet) std::cout << "Found " << n << " features" << std::endl;
        return true;
    }

    // the Python prototype's SIFT branch (feature_match.py:12-16, SIFT_create(nfeatures) + detectAndCompute); nfeatures 0 = all
    bool detectFeaturesSIFT(frame_t &cur_frame, int nfeatures = 0, bool show = false)
    {
        (void)show;
        const ImageMat &img = cur_frame.rgb_image;
        if (img.empty()) { std::cerr << "frame has no image" << std::endl; return false; }
        const int cap = img.rows * img.cols / 4 + 4096;    // DoG extrema are far sparser (kept between frames: see detectFeaturesSURF)
        float *kp = scratch_f32(kp_buf_, kp_cap_, size_t(7) * size_t(cap)), *desc = scratch_f32(desc_buf_, desc_cap_, size_t(128) * size_t(cap));
        int32_t n = 0;
        if (esfm_sift_detect_and_compute(default_ctx(), img.data.data(), img.rows, img.cols, img.channels, nfeatures, cap, kp, desc, &n) != ESFM_OK) {
            std::cerr << esfm_last_error() << std::endl;
            return false;
        }
        cur_frame.keypoints.resize(size_t(n));
        for (int k = 0; k < n; ++k) {
            KeyPoint &q = cur_frame.keypoints[size_t(k)];
            const float *v = &kp[size_t(7) * size_t(k)];
            q.pt.x = v[0]; q.pt.y = v[1]; q.size = v[2]; q.angle = v[3]; q.response = v[4]; q.octave = int(v[5]); q.class_id = int(v[6]);
        }
        cur_frame.descriptors.create(n, 128, DescMat::F32);
        if (n) std::memcpy(cur_frame.descriptors.ptr<float>(), desc, sizeof(float) * size_t(128) * size_t(n));
        if (!quiet) std::cout << "Found " << n << " features." << std::endl;
        return true;
    }

    // cross_check: keep mutual nearest neighbours (esfm_match_cross_*, the mutual_nn branch of feature_match.py:24-27) that also pass
    // the ratio test in both directions; ratio_thre == 0 in that mode: mutual nearest neighbours alone
    bool matchFeaturesORB(frame_t &cur_frame_1, frame_t &cur_frame_2, std::vector<DMatch> &matches, double ratio_thre = 0.8,
                          bool show = false, bool cross_check = false)
    {
        return run(cur_frame_1, cur_frame_2, matches, ratio_thre, true, "ORB", cross_check);
    }

    bool matchFeaturesSURF(frame_t &cur_frame_1, frame_t &cur_frame_2, std::vector<DMatch> &matches, double ratio_thre = 0.5,
                           bool show = false, bool cross_check = false)
    {
        return run(cur_frame_1, cur_frame_2, matches, ratio_thre, false, "SURF", cross_check);
    }

    // SIFT rows are 128 floats on the same L2 path; 0.7 is the prototype's nn_ratio (feature_match.py:5)
    bool matchFeaturesSIFT(frame_t &cur_frame_1, frame_t &cur_frame_2, std::vector<DMatch> &matches, double ratio_thre = 0.7,
                           bool show = false, bool cross_check = false)
    {
        return run(cur_frame_1, cur_frame_2, matches, ratio_thre, false, "SIFT", cross_check);
    }

    // what the "# Correspondence" line names as the filter
    static const char *filter_name(bool cross_check, double ratio_thre)
    {
        return !cross_check ? "Lowe ratio test" : (ratio_thre == 0.0 ? "cross-check" : "Lowe ratio test + cross-check");
    }

    // Which two frames start the reconstruction (the contract of feature_matching.cpp:160-229, defaults feature_matching.h:26): every
    // track weighs as many frames as see it; a pair (i, j < i) scores the summed weight of the tracks BOTH frames see; pairs whose
    // depth / baseline ratio exceeds the limit are out; the best score of at least min_track_num_init wins, the LATER pair on ties.
    // appro_depth[i][j] = img_match_graph[i][j].appro_depth.  Written over per-frame track lists: a frame's weights are laid out once
    // and every earlier frame sums over its own list -- O(frames x observations) where the reference walks frames^2 x tracks.
    // max_h_inlier_ratio (not in the reference; < 0: off): with h_inlier_ratio[i][j] = the pair's homography inliers / essential-matrix
    // inliers (esfm.h "Homography RANSAC"), a pair that passed the depth guard and exceeds the limit is skipped at the same place -- it
    // is planar or rotation-only; *h_candidate_pairs / *h_skipped_pairs (or NULL) then receive the pairs that reached this test and those
    // it skipped.
    bool findInitializeFramePair(std::vector<std::vector<bool>> &feature_track_matrix, std::vector<frame_t> &frames,
                                 const std::vector<std::vector<double>> &appro_depth, int &initialization_frame_1,
                                 int &initialization_frame_2, double &depth_init, int min_track_num_init = 100,
                                 double max_depth_baseline_ratio_init = 50.0, double max_h_inlier_ratio = -1.0,
                                 const std::vector<std::vector<double>> *h_inlier_ratio = nullptr, int *h_candidate_pairs = nullptr,
                                 int *h_skipped_pairs = nullptr)
    {
        int candidates = 0, skipped = 0;
        const size_t n_frames = frames.size(), n_tracks = feature_track_matrix.empty() ? 0 : feature_track_matrix[0].size();
        std::vector<int> weight(n_tracks, 0);
        std::vector<std::vector<int>> seen(n_frames);            // track ids per frame
        for (size_t f = 0; f < n_frames; ++f) {
            feature_track_matrix[f].resize(n_tracks);
            for (size_t t = 0; t < n_tracks; ++t)
                if (feature_track_matrix[f][t]) { ++weight[t]; seen[f].push_back(int(t)); }
        }
        long long best = min_track_num_init;
        int first = 0, second = 0;
        double best_ratio = 0.0;
        std::vector<int> laid(n_tracks, 0);                        // the weights of the tracks frame i sees, 0 elsewhere
        for (size_t i = 0; i < n_frames; ++i) {
            for (int t : seen[i]) laid[size_t(t)] = weight[size_t(t)];
            for (size_t j = 0; j < i; ++j) {
                const double ratio = appro_depth[i][j];
                if (ratio > max_depth_baseline_ratio_init) continue;
                if (max_h_inlier_ratio >= 0.0 && h_inlier_ratio) {
                    ++candidates;
                    if ((*h_inlier_ratio)[i][j] > max_h_inlier_ratio) { ++skipped; continue; }
                }
                long long score = 0;
                for (int t : seen[j]) score += laid[size_t(t)];
                if (score >= best) { best = score; best_ratio = ratio; first = int(i); second = int(j); }
            }
            for (int t : seen[i]) laid[size_t(t)] = 0;
        }
        if (h_candidate_pairs) *h_candidate_pairs = candidates;
        if (h_skipped_pairs) *h_skipped_pairs = skipped;
        if (first == second) {
            if (!quiet) std::cout << "Failed to find proper frame pair for initialization. Use default frame [1] and frame [0]" << std::endl;
            initialization_frame_1 = 1; initialization_frame_2 = 0;
            return false;                                           // depth_init keeps the caller's value, as in the reference (:217-223)
        }
        initialization_frame_1 = first; initialization_frame_2 = second;
        depth_init = best_ratio;
        return true;
    }

    // The frame to register next (the contract of feature_matching.cpp:231-268): among the frames still to process the one that sees
    // most of the tracks that already have a 3-D point; the FIRST such frame on ties; `next_frame` untouched when none sees any.
    bool findNextFrame(std::vector<std::vector<bool>> &feature_track_matrix, std::vector<bool> &frames_to_process,
                       std::vector<int> &unique_3d_point_ids, int &next_frame)
    {
        int most = 0;
        for (size_t f = 0; f < frames_to_process.size(); ++f) {
            if (!frames_to_process[f]) continue;
            const std::vector<bool> &row = feature_track_matrix[f];
            const int shared = int(std::count_if(unique_3d_point_ids.begin(), unique_3d_point_ids.end(), [&](int id) { return bool(row[size_t(id)]); }));
            if (shared > most) { most = shared; next_frame = int(f); }
        }
        return true;
    }

    bool quiet = false;  // the reference prints timing lines (feature_matching.cpp:96-97,141-142)

    // The pair loop of test/sfm.cpp:140-161 in ONE call: matchFeatures{SURF,ORB}(frames[pairs[p].first], frames[pairs[p].second],
    // matches[p]) for every listed pair -- every frame's descriptors uploaded once, one launch sequence for the whole list
    // (esfm_match_pairs), the per-pair lines of feature_matching.cpp:96-97 / :141-142 printed with the call's time shared out
    // evenly.  matches[p] is appended to, like the single-pair members.  cross_check: as for the single-pair members
    // (esfm_match_cross_pairs).
    bool matchFeaturesAllPairs(std::vector<frame_t> &frames, const std::vector<std::pair<int, int>> &pairs, bool hamming,
                               std::vector<std::vector<DMatch>> &matches, double ratio_thre = -1.0, bool cross_check = false)
    {
        if (ratio_thre < 0) ratio_thre = hamming ? 0.8 : 0.5;               // the members' defaults (feature_matching.h:17-21)
        matches.resize(pairs.size());
        if (pairs.empty()) return true;
        int width = 0;
        for (const frame_t &f : frames) if (f.descriptors.rows > 0) { width = f.descriptors.cols; break; }
        if (width == 0) return true;                                       // no frame has a descriptor: nothing can match
        const size_t row_bytes = hamming ? size_t(width) : size_t(width) * 4;
        std::vector<int32_t> off(frames.size() + 1, 0);
        for (size_t i = 0; i < frames.size(); ++i) {
            const DescMat &d = frames[i].descriptors;
            if (d.rows > 0 && (d.cols != width || d.type != (hamming ? DescMat::U8 : DescMat::F32))) { std::cerr << "descriptor shapes differ\n"; return false; }
            off[i + 1] = off[i] + d.rows;
        }
        std::vector<uint8_t> bank(size_t(off.back()) * row_bytes + 16);
        for (size_t i = 0; i < frames.size(); ++i)
            if (frames[i].descriptors.rows > 0) std::memcpy(bank.data() + size_t(off[i]) * row_bytes, frames[i].descriptors.bytes.data(), size_t(frames[i].descriptors.rows) * row_bytes);
        std::vector<int32_t> pl(2 * pairs.size());
        size_t total = 0;
        for (size_t p = 0; p < pairs.size(); ++p) { pl[2 * p] = pairs[p].first; pl[2 * p + 1] = pairs[p].second; total += size_t(frames[size_t(pairs[p].first)].descriptors.rows); }
        std::vector<int32_t> qi(std::max<size_t>(total, 1)), ti(std::max<size_t>(total, 1)), n_out(pairs.size());
        std::vector<float> d(std::max<size_t>(total, 1));
        std::vector<int64_t> out_off(pairs.size() + 1);
        auto tic = std::chrono::steady_clock::now();
        const int rc = cross_check
                           ? esfm_match_cross_pairs(default_ctx(), hamming ? ESFM_HAMMING : ESFM_L2_F32, bank.data(), off.data(), int(frames.size()), width,
                                                    pl.data(), int(pairs.size()), ratio_thre != 0.0, ratio_thre, qi.data(), ti.data(), d.data(), n_out.data(),
                                                    out_off.data())
                           : esfm_match_pairs(default_ctx(), hamming ? ESFM_HAMMING : ESFM_L2_F32, bank.data(), off.data(), int(frames.size()), width, pl.data(),
                                              int(pairs.size()), ratio_thre, qi.data(), ti.data(), d.data(), n_out.data(), out_off.data());
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        const std::chrono::duration<double> dt = std::chrono::steady_clock::now() - tic;
        for (size_t p = 0; p < pairs.size(); ++p) {
            const size_t o = size_t(out_off[p]);
            for (int k = 0; k < n_out[p]; ++k) matches[p].push_back(DMatch(qi[o + size_t(k)], ti[o + size_t(k)], 0, d[o + size_t(k)]));
            if (!quiet) {
                std::cout << "match " << (hamming ? "ORB" : "SURF") << " cost = " << dt.count() / double(pairs.size()) << " seconds. " << std::endl;
                std::cout << "# Correspondence: Initial [ " << frames[size_t(pairs[p].first)].descriptors.rows << " ]  Filtered by "
                          << filter_name(cross_check, ratio_thre) << " [ " << n_out[p]
                          << " ]" << std::endl;
            }
        }
        return true;
    }

    // Pair selection in front of the pair loop (esfm.h "Image retrieval", esfm_retrieval_pairs; not in the reference, whose to-do
    // "add sequential mode" is the options' window): `pairs` becomes the (i, j < i) pairs that retrieval selects among `frames`, in
    // the loop's order, for matchFeaturesAllPairs or the pair-by-pair loop.  Prints one "Pair selection:" line.
    bool selectPairs(std::vector<frame_t> &frames, bool hamming, const esfm_retrieval_options &options, std::vector<std::pair<int, int>> &pairs)
    {
        pairs.clear();
        const int n = int(frames.size());
        int width = 0;
        for (const frame_t &f : frames) if (f.descriptors.rows > 0) { width = f.descriptors.cols; break; }
        if (width == 0) { std::cerr << "pair selection: no frame has a descriptor\n"; return false; }
        const size_t row_bytes = hamming ? size_t(width) : size_t(width) * 4;
        std::vector<int32_t> off(frames.size() + 1, 0);
        for (size_t i = 0; i < frames.size(); ++i) {
            const DescMat &d = frames[i].descriptors;
            if (d.rows > 0 && (d.cols != width || d.type != (hamming ? DescMat::U8 : DescMat::F32))) { std::cerr << "descriptor shapes differ\n"; return false; }
            off[i + 1] = off[i] + d.rows;
        }
        std::vector<uint8_t> bank(size_t(off.back()) * row_bytes + 16);
        for (size_t i = 0; i < frames.size(); ++i)
            if (frames[i].descriptors.rows > 0) std::memcpy(bank.data() + size_t(off[i]) * row_bytes, frames[i].descriptors.bytes.data(), size_t(frames[i].descriptors.rows) * row_bytes);
        const size_t reach = size_t(std::min(std::max(options.window, 0), std::max(n - 1, 0)));
        std::vector<int32_t> list(2 * std::max<size_t>(size_t(n) * (size_t(std::max(options.top_k, 0)) + reach), 1));
        int32_t count = 0;
        const int rc = esfm_retrieval_pairs(default_ctx(), hamming ? ESFM_HAMMING : ESFM_L2_F32, bank.data(), off.data(), n, width, &options, list.data(), &count);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        for (int32_t p = 0; p < count; ++p) pairs.emplace_back(int(list[2 * size_t(p)]), int(list[2 * size_t(p) + 1]));
        std::cout << "Pair selection: [" << count << "] of [" << n * (n - 1) / 2 << "] pairs, [" << options.top_k << "] nearest of [" << n << "] images, window ["
                  << options.window << "], codebook [" << options.n_centres << "] x [" << (hamming ? 8 * width : width) << "]" << std::endl;
        return true;
    }

    // Epipolar-guided second pass (esfm.h "Epipolar-guided matching", esfm_match_guided_pairs) for pairs that have an essential
    // matrix: E holds 9 doubles per listed pair (what estimate2D2D_E5P_RANSAC[_pairs] returned), K is frame pairs[p].first's for both
    // images as there, max_epipolar_px the RANSAC's threshold, ratio_thre / cross_check the first pass's filter (ratio_thre == 0:
    // cross alone).  matches[p] is REPLACED by the pair's guided list.
    bool matchFeaturesGuidedAllPairs(std::vector<frame_t> &frames, const std::vector<std::pair<int, int>> &pairs, bool hamming,
                                     const std::vector<double> &E, double max_epipolar_px, std::vector<std::vector<DMatch>> &matches,
                                     double ratio_thre = -1.0, bool cross_check = false)
    {
        if (ratio_thre < 0) ratio_thre = hamming ? 0.8 : 0.5;
        matches.assign(pairs.size(), {});
        if (pairs.empty()) return true;
        int width = 0;
        for (const frame_t &f : frames) if (f.descriptors.rows > 0) { width = f.descriptors.cols; break; }
        if (width == 0) return true;
        const size_t row_bytes = hamming ? size_t(width) : size_t(width) * 4;
        std::vector<int32_t> off(frames.size() + 1, 0);
        for (size_t i = 0; i < frames.size(); ++i) {
            const DescMat &d = frames[i].descriptors;
            if (d.rows > 0 && (d.cols != width || d.type != (hamming ? DescMat::U8 : DescMat::F32))) { std::cerr << "descriptor shapes differ\n"; return false; }
            if (size_t(d.rows) != frames[i].keypoints.size()) { std::cerr << "one keypoint per descriptor row\n"; return false; }
            off[i + 1] = off[i] + d.rows;
        }
        std::vector<uint8_t> bank(size_t(off.back()) * row_bytes + 16);
        std::vector<float> kps(size_t(off.back()) * 2 + 2);
        for (size_t i = 0; i < frames.size(); ++i) {
            if (frames[i].descriptors.rows > 0) std::memcpy(bank.data() + size_t(off[i]) * row_bytes, frames[i].descriptors.bytes.data(), size_t(frames[i].descriptors.rows) * row_bytes);
            for (size_t k = 0; k < frames[i].keypoints.size(); ++k) { kps[2 * (size_t(off[i]) + k)] = frames[i].keypoints[k].pt.x; kps[2 * (size_t(off[i]) + k) + 1] = frames[i].keypoints[k].pt.y; }
        }
        std::vector<int32_t> pl(2 * pairs.size());
        std::vector<float> K4(4 * pairs.size());
        size_t total = 0;
        for (size_t p = 0; p < pairs.size(); ++p) {
            pl[2 * p] = pairs[p].first; pl[2 * p + 1] = pairs[p].second; total += size_t(frames[size_t(pairs[p].first)].descriptors.rows);
            const Matrix3f &K = frames[size_t(pairs[p].first)].K_cam;
            K4[4 * p] = K(0, 0); K4[4 * p + 1] = K(0, 2); K4[4 * p + 2] = K(1, 1); K4[4 * p + 3] = K(1, 2);
        }
        std::vector<int32_t> qi(std::max<size_t>(total, 1)), ti(std::max<size_t>(total, 1)), n_out(pairs.size());
        std::vector<float> d(std::max<size_t>(total, 1));
        std::vector<int64_t> out_off(pairs.size() + 1);
        const int rc = esfm_match_guided_pairs(default_ctx(), hamming ? ESFM_HAMMING : ESFM_L2_F32, bank.data(), kps.data(), off.data(), int(frames.size()),
                                               width, pl.data(), int(pairs.size()), E.data(), K4.data(), max_epipolar_px, ratio_thre != 0.0, ratio_thre,
                                               cross_check, qi.data(), ti.data(), d.data(), n_out.data(), out_off.data());
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        for (size_t p = 0; p < pairs.size(); ++p) {
            const size_t o = size_t(out_off[p]);
            for (int k = 0; k < n_out[p]; ++k) matches[p].push_back(DMatch(qi[o + size_t(k)], ti[o + size_t(k)], 0, d[o + size_t(k)]));
            if (!quiet) std::cout << "# Guided correspondence: pair ( " << pairs[p].first << " , " << pairs[p].second << " ) [ " << n_out[p] << " ]" << std::endl;
        }
        return true;
    }

    // The same for one pair (esfm_match_guided_l2_f32 / _hamming); `matches` is replaced.
    bool matchFeaturesGuided(frame_t &f1, frame_t &f2, bool hamming, const double E[9], double max_epipolar_px, std::vector<DMatch> &matches,
                             double ratio_thre = -1.0, bool cross_check = false)
    {
        if (ratio_thre < 0) ratio_thre = hamming ? 0.8 : 0.5;
        matches.clear();
        const DescMat &q = f1.descriptors, &t = f2.descriptors;
        if (q.rows > 0 && t.rows > 0 && (q.cols != t.cols || q.type != t.type)) { std::cerr << "descriptor shapes differ\n"; return false; }
        if ((hamming && q.type != DescMat::U8) || (!hamming && q.type != DescMat::F32)) { std::cerr << "wrong descriptor type\n"; return false; }
        if (size_t(q.rows) != f1.keypoints.size() || size_t(t.rows) != f2.keypoints.size()) { std::cerr << "one keypoint per descriptor row\n"; return false; }
        std::vector<float> kq(2 * f1.keypoints.size() + 2), kt(2 * f2.keypoints.size() + 2);
        for (size_t k = 0; k < f1.keypoints.size(); ++k) { kq[2 * k] = f1.keypoints[k].pt.x; kq[2 * k + 1] = f1.keypoints[k].pt.y; }
        for (size_t k = 0; k < f2.keypoints.size(); ++k) { kt[2 * k] = f2.keypoints[k].pt.x; kt[2 * k + 1] = f2.keypoints[k].pt.y; }
        const float K4[4] = {f1.K_cam(0, 0), f1.K_cam(0, 2), f1.K_cam(1, 1), f1.K_cam(1, 2)};
        std::vector<int32_t> qi(size_t(std::max(q.rows, 1))), ti(size_t(std::max(q.rows, 1)));
        std::vector<float> d(size_t(std::max(q.rows, 1)));
        int32_t n = 0;
        const int rc = hamming ? esfm_match_guided_hamming(default_ctx(), q.ptr<uint8_t>(), kq.data(), q.rows, t.ptr<uint8_t>(), kt.data(), t.rows, q.cols, E, K4,
                                                           max_epipolar_px, ratio_thre != 0.0, ratio_thre, cross_check, qi.data(), ti.data(), d.data(), &n)
                               : esfm_match_guided_l2_f32(default_ctx(), q.ptr<float>(), kq.data(), q.rows, t.ptr<float>(), kt.data(), t.rows, q.cols, E, K4,
                                                          max_epipolar_px, ratio_thre != 0.0, ratio_thre, cross_check, qi.data(), ti.data(), d.data(), &n);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        for (int k = 0; k < n; ++k) matches.push_back(DMatch(qi[size_t(k)], ti[size_t(k)], 0, d[size_t(k)]));
        if (!quiet) std::cout << "# Guided correspondence: [ " << n << " ]" << std::endl;
        return true;
    }

    // The union of a pair's RANSAC inliers and its guided list, in ascending query order: a query both lists hold carries the same
    // train row in both (esfm.h, property (b)), so the guided entries of the queries `inliers` lacks are added.
    static void mergeGuided(std::vector<DMatch> &inliers, const std::vector<DMatch> &guided)
    {
        std::vector<int> held;
        for (const DMatch &m : inliers) held.push_back(m.queryIdx);
        std::sort(held.begin(), held.end());
        for (const DMatch &m : guided)
            if (!std::binary_search(held.begin(), held.end(), m.queryIdx)) inliers.push_back(m);
        std::stable_sort(inliers.begin(), inliers.end(), [](const DMatch &a, const DMatch &b) { return a.queryIdx < b.queryIdx; });
    }

private:
    // detection outputs' landing buffers, uninitialised, grown on demand, kept for the object's life
    std::unique_ptr<float[]> kp_buf_, desc_buf_;
    size_t kp_cap_ = 0, desc_cap_ = 0;
    static float *scratch_f32(std::unique_ptr<float[]> &buf, size_t &cap, size_t n)
    {
        if (n > cap) { buf.reset(new float[n]); cap = n; }
        return buf.get();
    }

    bool run(frame_t &f1, frame_t &f2, std::vector<DMatch> &matches, double ratio, bool hamming, const char *tag, bool cross_check)
    {
        const DescMat &q = f1.descriptors, &t = f2.descriptors;
        if (q.rows > 0 && t.rows > 0 && (q.cols != t.cols || q.type != t.type)) { std::cerr << "descriptor shapes differ\n"; return false; }
        if ((hamming && q.type != DescMat::U8) || (!hamming && q.type != DescMat::F32)) { std::cerr << "wrong descriptor type\n"; return false; }
        auto tic = std::chrono::steady_clock::now();
        std::vector<int32_t> qi(size_t(std::max(q.rows, 1))), ti(size_t(std::max(q.rows, 1)));
        std::vector<float> d(size_t(std::max(q.rows, 1)));
        int32_t n = 0;
        int rc;
        if (cross_check)
            rc = hamming ? esfm_match_cross_hamming(default_ctx(), q.ptr<uint8_t>(), q.rows, t.ptr<uint8_t>(), t.rows, q.cols, ratio != 0.0, ratio,
                                                    qi.data(), ti.data(), d.data(), &n)
                         : esfm_match_cross_l2_f32(default_ctx(), q.ptr<float>(), q.rows, t.ptr<float>(), t.rows, q.cols, ratio != 0.0, ratio, qi.data(),
                                                   ti.data(), d.data(), &n);
        else
            rc = hamming ? esfm_match_hamming(default_ctx(), q.ptr<uint8_t>(), q.rows, t.ptr<uint8_t>(), t.rows, q.cols, ratio, qi.data(),
                                              ti.data(), d.data(), &n)
                         : esfm_match_l2_f32(default_ctx(), q.ptr<float>(), q.rows, t.ptr<float>(), t.rows, q.cols, ratio, qi.data(),
                                             ti.data(), d.data(), &n);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        const size_t before = matches.size();
        for (int k = 0; k < n; ++k) matches.push_back(DMatch(qi[size_t(k)], ti[size_t(k)], 0, d[size_t(k)]));  // appended (:90, :135)
        if (!quiet) {
            std::chrono::duration<double> dt = std::chrono::steady_clock::now() - tic;
            std::cout << "match " << tag << " cost = " << dt.count() << " seconds. " << std::endl;
            std::cout << "# Correspondence: Initial [ " << q.rows << " ]  Filtered by " << filter_name(cross_check, ratio) << " [ " << matches.size() - before
                      << " ]" << std::endl;
        }
        return true;
    }
};

// ---- sparse-cloud post-processing (cloudprocessing.hpp:20-72, data_io.cpp:147-165) ---------------------
// CProceesing<PointT>::SORFilter = pcl::StatisticalOutlierRemoval (MeanK 50, StddevMulThresh 2.0) -> esfm_sor_filter.
template <typename PointT = PointXYZRGB> class CProceesing {
public:
    bool SORFilter(const std::vector<PointT> &incloud, std::vector<PointT> &outcloud, int MeanK = 50, double std = 2.0)
    {
        const int n = int(incloud.size());
        std::vector<float> xyz(size_t(3) * size_t(std::max(n, 1)));
        for (int i = 0; i < n; ++i) { xyz[size_t(3 * i)] = incloud[size_t(i)].x; xyz[size_t(3 * i + 1)] = incloud[size_t(i)].y; xyz[size_t(3 * i + 2)] = incloud[size_t(i)].z; }
        std::vector<uint8_t> keep(size_t(std::max(n, 1)));
        int32_t n_keep = 0;
        const int rc = esfm_sor_filter(default_ctx(), xyz.data(), n, 3, MeanK, std, nullptr, keep.data(), &n_keep, nullptr);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        outcloud.clear();
        for (int i = 0; i < n; ++i) if (keep[size_t(i)]) outcloud.push_back(incloud[size_t(i)]);
        std::cout << "apply SOR filter: [ " << n << " ] points before filtering, [ " << outcloud.size() << " ] points after filtering." << std::endl;
        return true;
    }
};

// DataIO::writePlyFile (data_io.cpp:147-165): width 1, height N, pcl::io::savePLYFile (ASCII, camera element) [upstream
// pcl/io/ply_io.cpp, restated from memory -- the reference ships no example file].
class DataIO {
public:
    // data_io.cpp:17-46: whitespace-separated file names, each joined with the folder; frame ids count up from 0
    bool importImageFilenames(const std::string image_list_path, const std::string image_data_path, std::vector<frame_t> &frames)
    {
        std::ifstream image_list_file(image_list_path.c_str(), std::ios::in);
        if (!image_list_file.is_open()) { std::cout << "open image_list_file failed, file is: " << image_list_path << std::endl; return 0; }
        int count = 0;
        std::string cur_file;
        while (image_list_file >> cur_file) {
            frames.push_back(frame_t(unsigned(count), image_data_path + "/" + cur_file));
            std::cout << count << ": " << frames.back().image_file_path << std::endl;
            ++count;
        }
        std::cout << "Frame number is " << frames.size() << std::endl;
        return 1;
    }

    // data_io.cpp:48-72: cv::imread(path, CV_LOAD_IMAGE_COLOR) -> 8-bit BGR (PNG files; esfm_png.hpp)
    bool importImages(frame_t &cur_frame, bool show = false)
    {
        (void)show;
        ImageMat &img = cur_frame.rgb_image;
        img.channels = 3;
        const std::string err = read_image_bgr(cur_frame.image_file_path, img.rows, img.cols, img.data);
        if (!err.empty()) { img = ImageMat(); std::cout << "No more images" << " (" << err << ")" << std::endl; return false; }
        return true;
    }

    // data_io.cpp:74-95: up to three rows of three numbers into K (later rows of a longer file are ignored)
    bool importCalib(const std::string &fileName, Matrix3f &K_mat)
    {
        std::ifstream in(fileName, std::ios::in);
        if (!in) return false;
        for (int i = 0; i < 3; ++i) {
            float a, b, c;
            if (!(in >> a >> b >> c)) break;
            K_mat(i, 0) = a; K_mat(i, 1) = b; K_mat(i, 2) = c;
        }
        std::cout << "Import camera calibration file done." << std::endl;
        return true;
    }

    bool writePlyFile(const std::string &fileName, const std::vector<PointXYZRGB> &pointCloud)
    {
        std::ofstream fs(fileName);
        if (!fs) { std::cerr << "Couldn't write file " << std::endl; return false; }
        const size_t n = pointCloud.size();
        fs << "ply\nformat ascii 1.0\ncomment PCL generated\nelement vertex " << n
           << "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue"
              "\nelement camera 1\nproperty float view_px\nproperty float view_py\nproperty float view_pz"
              "\nproperty float x_axisx\nproperty float x_axisy\nproperty float x_axisz"
              "\nproperty float y_axisx\nproperty float y_axisy\nproperty float y_axisz"
              "\nproperty float z_axisx\nproperty float z_axisy\nproperty float z_axisz"
              "\nproperty float focal\nproperty float scalex\nproperty float scaley\nproperty float centerx\nproperty float centery"
              "\nproperty int viewportx\nproperty int viewporty\nproperty float k1\nproperty float k2\nend_header\n";
        fs << std::setprecision(8);
        for (const PointXYZRGB &p : pointCloud)
            fs << p.x << " " << p.y << " " << p.z << " " << int(p.r) << " " << int(p.g) << " " << int(p.b) << "\n";
        fs << "0 0 0 1 0 0 0 1 0 0 0 1 0 0 0 0 0 1 " << n << " 0 0\n";
        std::cout << "Output [ " << n << " ] points." << std::endl << "Output ply file done." << std::endl;
        return bool(fs);
    }

    // the merged dense cloud as oriented points: ASCII, properties x y z nx ny nz red green blue (easysfm_amd.cloud.write_ply_normals)
    bool writePlyFileNormals(const std::string &fileName, const std::vector<PointXYZRGBNormal> &pointCloud)
    {
        std::ofstream fs(fileName);
        if (!fs) { std::cerr << "Couldn't write file " << std::endl; return false; }
        const size_t n = pointCloud.size();
        fs << "ply\nformat ascii 1.0\nelement vertex " << n
           << "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz"
              "\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n";
        fs << std::setprecision(8);
        for (const PointXYZRGBNormal &p : pointCloud)
            fs << p.x << " " << p.y << " " << p.z << " " << p.nx << " " << p.ny << " " << p.nz << " " << int(p.r) << " " << int(p.g) << " " << int(p.b) << "\n";
        std::cout << "Output [ " << n << " ] points." << std::endl << "Output ply file done." << std::endl;
        return bool(fs);
    }

    // a triangle mesh: writePlyFileNormals' vertex properties, then the faces as vertex index lists (easysfm_amd.cloud.write_ply_mesh)
    bool writePlyMesh(const std::string &fileName, const TriangleMesh &mesh)
    {
        std::ofstream fs(fileName);
        if (!fs) { std::cerr << "Couldn't write file " << std::endl; return false; }
        const size_t n = mesh.vertices.size(), m = mesh.triangles.size() / 3;
        fs << "ply\nformat ascii 1.0\nelement vertex " << n
           << "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz"
              "\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face " << m
           << "\nproperty list uchar int vertex_indices\nend_header\n";
        fs << std::setprecision(8);
        for (const PointXYZRGBNormal &p : mesh.vertices)
            fs << p.x << " " << p.y << " " << p.z << " " << p.nx << " " << p.ny << " " << p.nz << " " << int(p.r) << " " << int(p.g) << " " << int(p.b) << "\n";
        for (size_t t = 0; t < m; ++t) fs << "3 " << mesh.triangles[3 * t] << " " << mesh.triangles[3 * t + 1] << " " << mesh.triangles[3 * t + 2] << "\n";
        std::cout << "Output [ " << n << " ] vertices, [ " << m << " ] triangles." << std::endl << "Output ply file done." << std::endl;
        return bool(fs);
    }

    // easysfm_amd.cloud.write_ply_textured_mesh: the header names the texture (comment TextureFile <stem>.png), vertices carry x y z nx
    // ny nz, faces their indices and six texture coordinates (u, 1 - v: v runs up in the file, down the atlas rows in uv); the atlas
    // (rows x cols x 3 RGB) goes beside the file as an 8-bit RGB PNG of the same stem.
    bool writePlyTexturedMesh(const std::string &fileName, const TriangleMesh &mesh, const std::vector<float> &uv, int atlas_rows, int atlas_cols,
                              const std::vector<uint8_t> &atlas)
    {
        const std::filesystem::path png = std::filesystem::path(fileName).replace_extension(".png");
        std::ofstream fs(fileName);
        if (!fs) { std::cerr << "Couldn't write file " << std::endl; return false; }
        const size_t n = mesh.vertices.size(), m = mesh.triangles.size() / 3;
        if (uv.size() != 6 * m || atlas.size() != size_t(atlas_rows) * size_t(atlas_cols) * 3) { std::cerr << "texture coordinates or atlas of the wrong size" << std::endl; return false; }
        fs << "ply\nformat ascii 1.0\ncomment TextureFile " << png.filename().string() << "\nelement vertex " << n
           << "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nelement face " << m
           << "\nproperty list uchar int vertex_indices\nproperty list uchar float texcoord\nend_header\n";
        fs << std::setprecision(8);
        for (const PointXYZRGBNormal &p : mesh.vertices) fs << p.x << " " << p.y << " " << p.z << " " << p.nx << " " << p.ny << " " << p.nz << "\n";
        for (size_t t = 0; t < m; ++t) {
            fs << "3 " << mesh.triangles[3 * t] << " " << mesh.triangles[3 * t + 1] << " " << mesh.triangles[3 * t + 2] << " 6";
            for (int k = 0; k < 3; ++k) fs << " " << uv[6 * t + 2 * k] << " " << 1.0f - uv[6 * t + 2 * k + 1];
            fs << "\n";
        }
        if (!fs) return false;
        const std::string e = png::write_rgb(png.string(), atlas_rows, atlas_cols, atlas.data());
        if (!e.empty()) { std::cerr << e << std::endl; return false; }
        std::cout << "Output [ " << n << " ] vertices, [ " << m << " ] triangles, texture [ " << atlas_cols << " x " << atlas_rows << " ]." << std::endl
                  << "Output ply file done." << std::endl;
        return true;
    }

    // DataIO::importDistort (data_io.cpp:97-125): up to three groups of k1 k2 p1 p2 are extracted as floats, then stored with
    // at<float>(0, i) into the CV_64FC1 matrix -- i.e. into its first 16 bytes.  Reproduced: cv::undistort
    // sees v[0] = the double made of the bits of (k1, k2), v[1] = that of (p1, p2), v[2] = v[3] = 0.
    // Multiple-camera mode (the drivers' +cameras token): the calibration file holds 9 G numbers (G row-major matrices) followed by
    // one camera index per image -- exactly 9 G + n_images numbers, every index in [0, G).  false with `error` set otherwise.
    static bool importCameras(const std::string &fileName, int n_images, std::vector<Matrix3f> &K_all, std::vector<int> &camera_of_image, std::string &error)
    {
        std::ifstream in(fileName, std::ios::in);
        if (!in) { error = "cannot read the camera file " + fileName; return false; }
        std::vector<double> vals;
        std::string tok;
        while (in >> tok) {
            char *end = nullptr;
            const double v = std::strtod(tok.c_str(), &end);
            if (end == tok.c_str() || *end != 0) { error = "camera file: not a number: " + tok; return false; }
            vals.push_back(v);
        }
        const long n_k = long(vals.size()) - n_images;
        if (n_k < 9 || n_k % 9 != 0) {
            error = "camera file: " + std::to_string(vals.size()) + " numbers for " + std::to_string(n_images) + " images; expected 9 G + " +
                    std::to_string(n_images) + " (G matrices, then one camera index per image)";
            return false;
        }
        const int G = int(n_k / 9);
        K_all.assign(size_t(G), Matrix3f::Identity());
        for (int g = 0; g < G; ++g) for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K_all[size_t(g)](r, c) = float(vals[size_t(9 * g + 3 * r + c)]);
        camera_of_image.clear();
        for (int i = 0; i < n_images; ++i) {
            const double v = vals[size_t(n_k + i)];
            if (v != double(long(v)) || v < 0 || v >= G) { error = "camera file: a camera index is not an integer in [0, " + std::to_string(G) + ")"; return false; }
            camera_of_image.push_back(int(v));
        }
        return true;
    }

    // ... and its distortion file: unreadable (none: zeros), 4 numbers (all cameras) or 4 G (per camera), each group stored as
    // importDistort stores its four floats.  *imported tells whether a file was read.
    static bool importCameraDistort(const std::string &fileName, int n_cameras, std::vector<DistortMat> &distort_all, bool &imported, std::string &error)
    {
        distort_all.assign(size_t(n_cameras), DistortMat());
        imported = false;
        std::ifstream in(fileName, std::ios::in);
        if (!in) return true;
        std::vector<float> vals;
        std::string tok;
        while (in >> tok) {
            char *end = nullptr;
            const double v = std::strtod(tok.c_str(), &end);
            if (end == tok.c_str() || *end != 0) { error = "distortion file: not a number: " + tok; return false; }
            vals.push_back(float(v));
        }
        if (vals.size() != 4 && vals.size() != size_t(4 * n_cameras)) {
            error = "distortion file: " + std::to_string(vals.size()) + " numbers; expected 4 (all cameras) or " + std::to_string(4 * n_cameras) + " (4 per camera)";
            return false;
        }
        for (int g = 0; g < n_cameras; ++g) std::memcpy(distort_all[size_t(g)].v, vals.data() + (vals.size() == 4 ? 0 : 4 * g), 4 * sizeof(float));
        imported = true;
        return true;
    }

    bool importDistort(const std::string &fileName, DistortMat &distort_coeff)
    {
        std::ifstream in(fileName, std::ios::in);
        if (!in) return false;
        int i = 0;
        float k[4] = {0.f, 0.f, 0.f, 0.f};
        while (!in.eof() && i < 3) {       // the reference's loop spins forever on a fourth group; three are read at most
            in >> k[0] >> k[1] >> k[2] >> k[3];
            if (in.fail()) break;
            ++i;
        }
        in.close();
        std::memcpy(distort_coeff.v, k, sizeof(k));
        std::cout << "Import camera distortion coefficients file done." << std::endl;
        return true;
    }
};

inline void angle_axis_to_rotation(const double aa[3], double R[9]);

// Multiple-camera mode, the pair stage: its kernels take one K per pair and stay as they are.  While an object of this class lives,
// every frame carries its keypoints remapped into the pixels of the canonical camera -- K_ref, the K_cam of the first frame with
// camera_id 0 -- and K_ref itself: u' = (u - cx) fx_ref / fx + cx_ref, likewise v, in double, rounded to float once.  The pair
// stage's thresholds are then in canonical pixels.  Its destructor puts the frames' own pixels and K_cam back.  Frames whose K_cam
// equals K_ref bit for bit are not touched, and nothing is when all frames share one K_cam.
class CanonicalPairView {
public:
    explicit CanonicalPairView(std::vector<frame_t> &frames) : frames_(frames)
    {
        if (frames.empty()) return;
        const frame_t *ref = &frames[0];
        for (const frame_t &f : frames) if (f.camera_id == 0) { ref = &f; break; }
        const Matrix3f K_ref = ref->K_cam;
        for (const frame_t &f : frames) active_ = active_ || !same(f.K_cam, K_ref);
        if (!active_) return;
        for (frame_t &f : frames) {
            saved_K_.push_back(f.K_cam);
            std::vector<Point2f> pts;
            for (const KeyPoint &kp : f.keypoints) pts.push_back(kp.pt);
            saved_pts_.push_back(pts);
            if (!same(f.K_cam, K_ref)) {
                const double fx = f.K_cam(0, 0), cx = f.K_cam(0, 2), fy = f.K_cam(1, 1), cy = f.K_cam(1, 2);
                for (KeyPoint &kp : f.keypoints) {
                    kp.pt.x = float((double(kp.pt.x) - cx) * double(K_ref(0, 0)) / fx + double(K_ref(0, 2)));
                    kp.pt.y = float((double(kp.pt.y) - cy) * double(K_ref(1, 1)) / fy + double(K_ref(1, 2)));
                }
            }
            f.K_cam = K_ref;
        }
    }
    ~CanonicalPairView()
    {
        if (!active_) return;
        for (size_t i = 0; i < frames_.size(); ++i) {
            frames_[i].K_cam = saved_K_[i];
            for (size_t k = 0; k < frames_[i].keypoints.size(); ++k) frames_[i].keypoints[k].pt = saved_pts_[i][k];
        }
    }
    CanonicalPairView(const CanonicalPairView &) = delete;
    CanonicalPairView &operator=(const CanonicalPairView &) = delete;
    bool active() const { return active_; }

private:
    static bool same(const Matrix3f &a, const Matrix3f &b)
    {
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { const float x = a(r, c), y = b(r, c); if (std::memcmp(&x, &y, sizeof(float)) != 0) return false; }
        return true;
    }
    std::vector<frame_t> &frames_;
    std::vector<Matrix3f> saved_K_;
    std::vector<std::vector<Point2f>> saved_pts_;
    bool active_ = false;
};

// ---- two-view / 3-D/2-D geometry (estimate_motion.h) ------------------------------------------------------
class MotionEstimator {
public:
    // estimate_motion.cpp:27-97: cv::findEssentialMat(RANSAC) on the matched pixels with frame 1's K, inliers appended,
    // cv::recoverPose with the RANSAC mask -> T = [R | t; 0 0 0 1]
    bool estimate2D2D_E5P_RANSAC(frame_t &cur_frame_1, frame_t &cur_frame_2, std::vector<DMatch> &matches, std::vector<DMatch> &inlier_matches,
                                 Matrix4f &T, double ransac_thre = 1.0, double ransac_prob = 0.99, bool show = false, double *E_out = nullptr /* 9: the essential matrix */)
    {
        std::vector<float> p1, p2;
        gather(cur_frame_1, cur_frame_2, matches, 1, p1, p2);
        const int n = int(matches.size());
        float K4[4]; k4_of(cur_frame_1.K_cam, K4);
        std::vector<uint8_t> mask(size_t(std::max(n, 1)));
        double E[9], R[9], t[3];
        int rc = esfm_find_essential_mat(default_ctx(), p1.data(), p2.data(), n, K4, ransac_prob, ransac_thre, E, mask.data(), nullptr);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        if (E_out) std::copy(E, E + 9, E_out);
        for (int i = 0; i < n; ++i) if (mask[size_t(i)]) inlier_matches.push_back(matches[size_t(i)]);   // :55-61
        rc = esfm_recover_pose(default_ctx(), E, p1.data(), p2.data(), n, K4, R, t, mask.data(), nullptr);   // :67
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        T = Matrix4f::Identity();
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T(r, c) = float(R[3 * r + c]); T(r, 3) = float(t[r]); }   // :76-85
        if (!quiet) std::cout << "Find [" << inlier_matches.size() << "] inlier matches from [" << matches.size() << "] total matches." << std::endl;
        return true;
    }

    // The homography counterpart (not in the reference; esfm.h "Homography RANSAC"): 4-point RANSAC on the matched pixels, the matches
    // of the RANSAC mask appended to inlier_matches, H (9 doubles, row-major, frame 1's pixels to frame 2's; or NULL).  *n_inliers (or
    // NULL) = esfm_find_homography_pairs' count: the matches within the threshold of the RETURNED, re-fitted H -- the numerator of
    // h_inlier_ratio, which is not the number of matches appended.  false: fewer than 4 matches or no model (*n_inliers = 0).
    bool estimate2D2D_H4P_RANSAC(frame_t &cur_frame_1, frame_t &cur_frame_2, std::vector<DMatch> &matches, std::vector<DMatch> &inlier_matches,
                                 double *H, double ransac_thre = 1.0, double ransac_prob = 0.995, int *n_inliers = nullptr)
    {
        std::vector<float> p1, p2;
        gather(cur_frame_1, cur_frame_2, matches, 1, p1, p2);
        const int n = int(matches.size());
        if (p1.empty()) { p1.assign(2, 0.f); p2.assign(2, 0.f); }
        std::vector<uint8_t> mask(size_t(std::max(n, 1)));
        const int32_t off[2] = {0, n};
        int32_t status = 0, count = 0;
        double Hm[9];
        if (n_inliers) *n_inliers = 0;
        const int rc = esfm_find_homography_pairs(default_ctx(), 1, off, p1.data(), p2.data(), ransac_thre, ransac_prob, Hm, mask.data(), &status, nullptr, &count);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        if (!status) return false;
        if (H) std::copy(Hm, Hm + 9, H);
        if (n_inliers) *n_inliers = int(count);
        for (int i = 0; i < n; ++i) if (mask[size_t(i)]) inlier_matches.push_back(matches[size_t(i)]);
        return true;
    }

    // ... for MANY pairs in shared launches (esfm_find_homography_pairs): n_inliers[p] = job p's matches within the threshold of its
    // returned, re-fitted H (what the per-pair member puts in *n_inliers), 0 without a model
    bool estimate2D2D_H4P_RANSAC_pairs(std::vector<frame_t> &frames, const std::vector<std::pair<int, int>> &jobs, const std::vector<std::vector<DMatch>> &matches,
                                       std::vector<int> &n_inliers, double ransac_thre = 1.0, double ransac_prob = 0.995)
    {
        const size_t nj = jobs.size();
        n_inliers.assign(nj, 0);
        if (nj == 0) return true;
        std::vector<int32_t> off(nj + 1, 0);
        for (size_t p = 0; p < nj; ++p) off[p + 1] = off[p] + int32_t(matches[p].size());
        std::vector<float> p1(size_t(2) * size_t(std::max(off[nj], 1))), p2(p1.size());
        for (size_t p = 0; p < nj; ++p) {
            std::vector<float> a, b;
            gather(frames[size_t(jobs[p].first)], frames[size_t(jobs[p].second)], matches[p], 1, a, b);
            std::copy(a.begin(), a.end(), p1.begin() + 2 * off[p]); std::copy(b.begin(), b.end(), p2.begin() + 2 * off[p]);
        }
        std::vector<double> H(9 * nj);
        std::vector<uint8_t> mask(size_t(std::max(off[nj], 1)));
        std::vector<int32_t> status(nj, 0), count(nj, 0);
        const int rc = esfm_find_homography_pairs(default_ctx(), int(nj), off.data(), p1.data(), p2.data(), ransac_thre, ransac_prob, H.data(), mask.data(),
                                                  status.data(), nullptr, count.data());
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        for (size_t p = 0; p < nj; ++p) n_inliers[p] = status[p] ? int(count[p]) : 0;
        return true;
    }

    // estimate2D2D_E5P_RANSAC + getDepthFast (estimate_motion.cpp:27-97, :234-283; sfm.cpp:163-170) for MANY pairs in shared launches:
    // job p = (frame_1[p], frame_2[p], matches[p]).  ok[p] / inlier_matches[p] / T[p] / appro_depth[p] are what the per-pair members
    // return for that job (appro_depth stays untouched where the per-pair getDepthFast is not reached or fails).
    bool estimate2D2D_E5P_RANSAC_pairs(std::vector<frame_t> &frames, const std::vector<std::pair<int, int>> &jobs, const std::vector<std::vector<DMatch>> &matches,
                                       std::vector<std::vector<DMatch>> &inlier_matches, std::vector<Matrix4f> &T, std::vector<double> &appro_depth,
                                       std::vector<char> &ok, double ransac_thre = 1.0, double ransac_prob = 0.99, int random_rate = 20,
                                       std::vector<double> *E_out = nullptr /* 9 per job: the essential matrices */)
    {
        const size_t nj = jobs.size();
        inlier_matches.assign(nj, {}); T.assign(nj, Matrix4f::Identity()); ok.assign(nj, 0);
        appro_depth.resize(nj, 1.0);
        if (nj == 0) return true;
        std::vector<int32_t> off(nj + 1, 0);
        for (size_t p = 0; p < nj; ++p) off[p + 1] = off[p] + int32_t(matches[p].size());
        std::vector<float> p1(size_t(2) * size_t(std::max(off[nj], 1))), p2(p1.size()), K4(4 * nj);
        for (size_t p = 0; p < nj; ++p) {
            std::vector<float> a, b;
            gather(frames[size_t(jobs[p].first)], frames[size_t(jobs[p].second)], matches[p], 1, a, b);
            std::copy(a.begin(), a.end(), p1.begin() + 2 * off[p]); std::copy(b.begin(), b.end(), p2.begin() + 2 * off[p]);
            k4_of(frames[size_t(jobs[p].first)].K_cam, &K4[4 * p]);                           // frame 1's K for both images (:43-44)
        }
        std::vector<double> E(9 * nj), R(9 * nj), t(3 * nj);
        std::vector<uint8_t> mask(size_t(std::max(off[nj], 1)));
        std::vector<int32_t> status(nj, 0);
        int rc = esfm_find_essential_pairs(default_ctx(), int(nj), off.data(), p1.data(), p2.data(), K4.data(), ransac_prob, ransac_thre, E.data(), mask.data(),
                                           status.data(), nullptr);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        if (E_out) *E_out = E;
        for (size_t p = 0; p < nj; ++p) {
            if (!status[p]) { for (int k = off[p]; k < off[p + 1]; ++k) mask[size_t(k)] = 0; continue; }
            for (int k = off[p]; k < off[p + 1]; ++k) if (mask[size_t(k)]) inlier_matches[p].push_back(matches[p][size_t(k - off[p])]);   // :55-61
        }
        rc = esfm_recover_pose_pairs(default_ctx(), int(nj), off.data(), p1.data(), p2.data(), K4.data(), E.data(), mask.data(), R.data(), t.data(), nullptr);   // :67
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        // getDepthFast: every random_rate-th inlier match between [I | 0] and T_21, one triangulation launch for all jobs
        std::vector<int32_t> doff(1, 0);
        std::vector<float> P1s, P2s, da, db;
        std::vector<size_t> dj;
        for (size_t p = 0; p < nj; ++p) {
            if (!status[p]) { if (!quiet) std::cerr << "no essential matrix for pair ( " << jobs[p].first << " , " << jobs[p].second << " )" << std::endl; continue; }
            ok[p] = 1;
            for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T[p](r, c) = float(R[9 * p + size_t(3 * r + c)]); T[p](r, 3) = float(t[3 * p + size_t(r)]); }   // :76-85
            if (!quiet) std::cout << "Find [" << inlier_matches[p].size() << "] inlier matches from [" << matches[p].size() << "] total matches." << std::endl;
            std::vector<float> a, b;
            frame_t &f1 = frames[size_t(jobs[p].first)];
            gather(f1, frames[size_t(jobs[p].second)], inlier_matches[p], random_rate, a, b);
            if (a.empty()) { appro_depth[p] = std::nan(""); continue; }                  // 0 / 0 in the reference (:280)
            pixel2cam(a, f1.K_cam); pixel2cam(b, f1.K_cam);                               // frame 1's K for both (:245)
            const float I34[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
            P1s.insert(P1s.end(), I34, I34 + 12);
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) P2s.push_back(T[p](r, c));
            da.insert(da.end(), a.begin(), a.end()); db.insert(db.end(), b.begin(), b.end());
            doff.push_back(doff.back() + int32_t(a.size() / 2));
            dj.push_back(p);
        }
        if (!dj.empty()) {
            std::vector<float> hh(size_t(4) * size_t(doff.back()));
            rc = esfm_triangulate_pairs(default_ctx(), int(dj.size()), P1s.data(), P2s.data(), doff.data(), da.data(), db.data(), hh.data());
            if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
            for (size_t s = 0; s < dj.size(); ++s) {
                double depth_sum = 0;
                for (int i = doff[s]; i < doff[s + 1]; ++i) {
                    const float x = hh[size_t(4 * i)] / hh[size_t(4 * i + 3)], y = hh[size_t(4 * i + 1)] / hh[size_t(4 * i + 3)], z = hh[size_t(4 * i + 2)] / hh[size_t(4 * i + 3)];
                    depth_sum += double(std::sqrt(x * x + y * y + z * z));   // Eigen::Vector3f::norm()
                }
                appro_depth[dj[s]] = depth_sum / double(doff[s + 1] - doff[s]);
            }
        }
        return true;
    }

    // estimate_motion.cpp:234-283: every random_rate-th match triangulated between [I|0] and T_21, mean distance from camera 1
    bool getDepthFast(frame_t &cur_frame_1, frame_t &cur_frame_2, Matrix4f &T_21, const std::vector<DMatch> &matches, double &appro_depth,
                      int random_rate = 20)
    {
        std::vector<float> a, b;
        gather(cur_frame_1, cur_frame_2, matches, random_rate, a, b);
        const int n = int(a.size() / 2);
        pixel2cam(a, cur_frame_1.K_cam); pixel2cam(b, cur_frame_2.K_cam);   // the reference: frame 1's K for both (:245); the same when the K's are equal
        float P1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, P2[12];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) P2[4 * r + c] = T_21(r, c);
        std::vector<float> h(size_t(4) * size_t(std::max(n, 1)));
        if (n > 0 && esfm_triangulate_points(default_ctx(), P1, P2, a.data(), b.data(), n, h.data()) != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        double depth_sum = 0;
        for (int i = 0; i < n; ++i) {
            const float x = h[size_t(4 * i)] / h[size_t(4 * i + 3)], y = h[size_t(4 * i + 1)] / h[size_t(4 * i + 3)], z = h[size_t(4 * i + 2)] / h[size_t(4 * i + 3)];
            depth_sum += double(std::sqrt(x * x + y * y + z * z));   // Eigen::Vector3f::norm()
        }
        appro_depth = depth_sum / n;   // 0 / 0 for an empty sample, like the reference
        return true;
    }

    // estimate_motion.cpp:285-367 (without the colour lookup: frame_t carries no image here)
    bool doTriangulation(frame_t &cur_frame_1, frame_t &cur_frame_2, const std::vector<DMatch> &matches, pointcloud_sparse_t &sparse_pointcloud,
                         bool show = false)
    {
        std::unordered_map<int, int> known;
        for (int id : sparse_pointcloud.unique_point_ids) known.emplace(id, 1);
        std::vector<float> a, b;
        int count_new = 0;
        for (const DMatch &m : matches) {
            const int uid = cur_frame_1.unique_pixel_ids[size_t(m.queryIdx)];
            if (known.count(uid)) continue;
            known.emplace(uid, 1);
            sparse_pointcloud.unique_point_ids.push_back(uid);
            sparse_pointcloud.is_inlier.push_back(1);
            a.push_back(cur_frame_1.keypoints[size_t(m.queryIdx)].pt.x); a.push_back(cur_frame_1.keypoints[size_t(m.queryIdx)].pt.y);
            b.push_back(cur_frame_2.keypoints[size_t(m.trainIdx)].pt.x); b.push_back(cur_frame_2.keypoints[size_t(m.trainIdx)].pt.y);
            ++count_new;
        }
        pixel2cam(a, cur_frame_1.K_cam); pixel2cam(b, cur_frame_2.K_cam);
        float P1[12], P2[12];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) { P1[4 * r + c] = cur_frame_1.pose_cam(r, c); P2[4 * r + c] = cur_frame_2.pose_cam(r, c); }
        std::vector<float> h(size_t(4) * size_t(std::max(count_new, 1)));
        if (count_new > 0 && esfm_triangulate_points(default_ctx(), P1, P2, a.data(), b.data(), count_new, h.data()) != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        const ImageMat &img = cur_frame_1.rgb_image;
        for (int i = 0; i < count_new; ++i) {
            PointXYZRGB p;
            p.x = h[size_t(4 * i)] / h[size_t(4 * i + 3)]; p.y = h[size_t(4 * i + 1)] / h[size_t(4 * i + 3)]; p.z = h[size_t(4 * i + 2)] / h[size_t(4 * i + 3)];
            if (!img.empty() && img.channels == 3) {
                // colour from frame 1's image at the keypoint of matches[i] -- the reference indexes the match list with the
                // index of the i-th NEW point (estimate_motion.cpp:345), which is another match once any was skipped
                const Point2f &px = cur_frame_1.keypoints[size_t(matches[size_t(i)].queryIdx)].pt;
                const int y = int(px.y), x = int(px.x);
                if (y >= 0 && y < img.rows && x >= 0 && x < img.cols) {
                    const uint8_t *bgr = &img.data[(size_t(y) * size_t(img.cols) + size_t(x)) * 3];
                    p.b = bgr[0]; p.g = bgr[1]; p.r = bgr[2];
                }
            }
            sparse_pointcloud.points.push_back(p);
        }
        if (!quiet) std::cout << "Triangulate [ " << count_new << " ] new points, [ " << sparse_pointcloud.points.size() << " ] points in total." << std::endl;
        return true;
    }

    // estimate_motion.cpp:99-232: id join (keypoint-major, +-300 gate), solvePnPRansac(EPnP), pose write-back, the reference's
    // inlier bookkeeping (the int index matrix read as float always addresses correspondence 0)
    bool estimate2D3D_P3P_RANSAC(frame_t &cur_frame, pointcloud_sparse_t &cur_map_3d, double ransac_thre = 2.5, int iterationsCount = 50000,
                                 double ransac_prob = 0.99, bool show = false)
    {
        std::unordered_map<int, std::vector<int>> where;
        for (size_t j = 0; j < cur_map_3d.unique_point_ids.size(); ++j) where[cur_map_3d.unique_point_ids[j]].push_back(int(j));
        std::vector<float> p2, p3;
        std::vector<int> index;
        const float dist_thre = 300;
        for (size_t i = 0; i < cur_frame.unique_pixel_ids.size(); ++i) {
            auto it = where.find(cur_frame.unique_pixel_ids[i]);
            if (it == where.end()) continue;
            for (int j : it->second) {
                const PointXYZRGB &q = cur_map_3d.points[size_t(j)];
                if (std::abs(q.x) < dist_thre && std::abs(q.y) < dist_thre && std::abs(q.z) < dist_thre) {
                    p2.push_back(cur_frame.keypoints[i].pt.x); p2.push_back(cur_frame.keypoints[i].pt.y);
                    p3.push_back(q.x); p3.push_back(q.y); p3.push_back(q.z);
                    index.push_back(j);
                }
            }
        }
        const int count = int(index.size());
        float K4[4]; k4_of(cur_frame.K_cam, K4);
        double rv[3], tv[3], R[9];
        int32_t n_inl = 0;
        std::vector<uint8_t> mask(size_t(std::max(count, 1)));
        int rc = esfm_solve_pnp_ransac(default_ctx(), p3.data(), p2.data(), count, K4, iterationsCount, ransac_thre, ransac_prob, rv, tv, R, mask.data(),
                                       &n_inl, nullptr);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        if (n_inl > 0 && !index.empty()) index[0] = -1;   // inliers.at<float>(i, 0) on CV_32S (:169)
        for (int j : index) if (j >= 0) cur_map_3d.is_inlier[size_t(j)] = 0;
        double Rr[9];
        angle_axis_to_rotation(rv, Rr);   // cv::Rodrigues(r_vec, R_mat) (:184)
        cur_frame.pose_cam = Matrix4f::Identity();
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) cur_frame.pose_cam(r, c) = float(Rr[3 * r + c]); cur_frame.pose_cam(r, 3) = float(tv[r]); }
        float reproj_err = 0.f;
        for (int i = 0; i < count; ++i) {
            const double X = p3[size_t(3 * i)], Y = p3[size_t(3 * i + 1)], Z = p3[size_t(3 * i + 2)];
            const double xc = Rr[0] * X + Rr[1] * Y + Rr[2] * Z + tv[0], yc = Rr[3] * X + Rr[4] * Y + Rr[5] * Z + tv[1], zc = Rr[6] * X + Rr[7] * Y + Rr[8] * Z + tv[2];
            const float u = float(xc / zc * double(K4[0]) + double(K4[1])), v = float(yc / zc * double(K4[2]) + double(K4[3]));
            const float dx = u - p2[size_t(2 * i)], dy = v - p2[size_t(2 * i + 1)];
            reproj_err += std::sqrt(dx * dx + dy * dy);
        }
        reproj_err /= float(count);
        const double inlier_ratio = 1.0 * n_inl / count;
        if (!quiet) std::cout << "Inlier count: " << n_inl << std::endl << "Mean reprojection error: " << reproj_err << std::endl;
        return !(reproj_err > 10 && inlier_ratio < 0.5);
    }

    // estimate_motion.cpp:431-441: cv::undistort(cur_frame.rgb_image, undistorted_img, K_cam, distort_coeff)
    bool doUnDistort(frame_t &cur_frame, const DistortMat &distort_coeff)
    {
        ImageMat &img = cur_frame.rgb_image;
        if (img.empty()) { std::cerr << "frame has no image" << std::endl; return false; }
        const double K4[4] = {cur_frame.K_cam(0, 0), cur_frame.K_cam(0, 2), cur_frame.K_cam(1, 1), cur_frame.K_cam(1, 2)};
        std::vector<uint8_t> undistorted_img(img.data.size());
        if (esfm_undistort(default_ctx(), img.data.data(), img.rows, img.cols, img.channels, K4, distort_coeff.v, undistorted_img.data()) != ESFM_OK) {
            std::cerr << esfm_last_error() << std::endl;
            return false;
        }
        img.data.swap(undistorted_img);
        if (!quiet) std::cout << "Undistort the image done." << std::endl;
        return true;
    }

    // estimate_motion.cpp:476-505
    bool outlierFilter(pointcloud_sparse_t &sparse_pointcloud, int MeanK = 40, double std = 2.5)
    {
        const int n = int(sparse_pointcloud.points.size());
        std::vector<float> xyz(size_t(3) * size_t(std::max(n, 1)));
        for (int i = 0; i < n; ++i) { xyz[size_t(3 * i)] = sparse_pointcloud.points[size_t(i)].x; xyz[size_t(3 * i + 1)] = sparse_pointcloud.points[size_t(i)].y; xyz[size_t(3 * i + 2)] = sparse_pointcloud.points[size_t(i)].z; }
        std::vector<uint8_t> keep(size_t(std::max(n, 1)));
        if (esfm_sor_filter(default_ctx(), xyz.data(), n, 3, MeanK, std, nullptr, keep.data(), nullptr, nullptr) != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        pointcloud_sparse_t out;
        for (int i = 0; i < n; ++i) if (keep[size_t(i)]) {
            out.points.push_back(sparse_pointcloud.points[size_t(i)]);
            out.unique_point_ids.push_back(sparse_pointcloud.unique_point_ids[size_t(i)]);
            out.is_inlier.push_back(sparse_pointcloud.is_inlier[size_t(i)]);
        }
        sparse_pointcloud.points.swap(out.points); sparse_pointcloud.unique_point_ids.swap(out.unique_point_ids); sparse_pointcloud.is_inlier.swap(out.is_inlier);
        return true;
    }

    // Not in the reference (esfm.h "Track triangulation"; easysfm_amd/tracks.py refine_tracks is the same routine): every cloud point
    // is re-triangulated from ALL its observations in the registered frames -- every keypoint whose unique_pixel_ids is a cloud id, a
    // track's first observer included, camera-major, keypoint index ascending -- or, with evaluate_only, only judged.  Kept points are
    // written back as floats, the others leave the cloud's three arrays together as in outlierFilter, and unique_pixel_has_match is
    // cleared on the outlier observations of kept points (setBAProblem alone reads that flag).  A point dropped here may be added again
    // by a later doTriangulation and is then judged again.  Prints one "Track refine:" line.
    bool refineTracks(std::vector<frame_t> &frames, const std::vector<bool> &process_frame_id, pointcloud_sparse_t &cloud, const esfm_track_options &opt,
                      bool evaluate_only = false)
    {
        const int n_pt = int(cloud.points.size());
        std::unordered_map<int, int> point_of;
        for (int k = 0; k < n_pt; ++k) point_of.emplace(cloud.unique_point_ids[size_t(k)], k);   // emplace keeps the first
        std::vector<int32_t> cam_idx, pt_idx, kp_idx, frame_of;
        std::vector<float> uv, K4;
        std::vector<double> Rt;
        for (size_t i = 0; i < frames.size(); ++i) {
            if (process_frame_id[i]) continue;
            const frame_t &fr = frames[i];
            const int c = int(frame_of.size());
            frame_of.push_back(int32_t(i));
            float k4[4];
            k4_of(fr.K_cam, k4);
            K4.insert(K4.end(), k4, k4 + 4);
            for (int r = 0; r < 3; ++r) for (int col = 0; col < 4; ++col) Rt.push_back(double(fr.pose_cam(r, col)));
            for (size_t j = 0; j < fr.unique_pixel_ids.size(); ++j) {
                const auto it = point_of.find(fr.unique_pixel_ids[j]);
                if (it == point_of.end()) continue;
                cam_idx.push_back(c); pt_idx.push_back(it->second); kp_idx.push_back(int32_t(j));
                uv.push_back(fr.keypoints[j].pt.x); uv.push_back(fr.keypoints[j].pt.y);
            }
        }
        const int n_obs = int(cam_idx.size()), n_cam = int(frame_of.size());
        std::vector<double> xyz_in(size_t(3) * size_t(std::max(n_pt, 1))), xyz_out(xyz_in.size());
        for (int k = 0; k < n_pt; ++k) { xyz_in[size_t(3 * k)] = cloud.points[size_t(k)].x; xyz_in[size_t(3 * k + 1)] = cloud.points[size_t(k)].y; xyz_in[size_t(3 * k + 2)] = cloud.points[size_t(k)].z; }
        std::vector<uint8_t> inlier(size_t(std::max(n_obs, 1)));
        std::vector<int32_t> status(size_t(std::max(n_pt, 1))), n_inliers(status.size());
        const int rc = evaluate_only
                           ? esfm_track_evaluate(default_ctx(), n_cam, n_pt, n_obs, cam_idx.data(), pt_idx.data(), uv.data(), K4.data(), Rt.data(), xyz_in.data(), &opt,
                                                 inlier.data(), nullptr, status.data(), n_inliers.data(), nullptr, nullptr)
                           : esfm_track_triangulate(default_ctx(), n_cam, n_pt, n_obs, cam_idx.data(), pt_idx.data(), uv.data(), K4.data(), Rt.data(), xyz_in.data(),
                                                    &opt, xyz_out.data(), inlier.data(), nullptr, status.data(), n_inliers.data(), nullptr, nullptr);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        std::vector<int> per_point(size_t(std::max(n_pt, 1)), 0);
        for (int o = 0; o < n_obs; ++o) ++per_point[size_t(pt_idx[size_t(o)])];
        int n_tracks = 0, n_kept = 0, n_obs_dropped = 0;
        for (int k = 0; k < n_pt; ++k) { n_tracks += per_point[size_t(k)] >= 2 ? 1 : 0; n_kept += status[size_t(k)] == 0 ? 1 : 0; }
        for (int o = 0; o < n_obs; ++o) {
            if (inlier[size_t(o)] || status[size_t(pt_idx[size_t(o)])] != 0) continue;
            std::vector<bool> &flags = frames[size_t(frame_of[size_t(cam_idx[size_t(o)])])].unique_pixel_has_match;
            if (flags[size_t(kp_idx[size_t(o)])]) { ++n_obs_dropped; flags[size_t(kp_idx[size_t(o)])] = false; }
        }
        pointcloud_sparse_t out;
        for (int k = 0; k < n_pt; ++k) {
            if (status[size_t(k)] != 0) continue;
            PointXYZRGB p = cloud.points[size_t(k)];
            if (!evaluate_only) { p.x = float(xyz_out[size_t(3 * k)]); p.y = float(xyz_out[size_t(3 * k + 1)]); p.z = float(xyz_out[size_t(3 * k + 2)]); }
            out.points.push_back(p);
            out.unique_point_ids.push_back(cloud.unique_point_ids[size_t(k)]);
            out.is_inlier.push_back(cloud.is_inlier[size_t(k)]);
        }
        cloud.points.swap(out.points); cloud.unique_point_ids.swap(out.unique_point_ids); cloud.is_inlier.swap(out.is_inlier);
        std::cout << "Track refine: [" << n_tracks << "] tracks, [" << (evaluate_only ? 0 : n_kept) << "] re-triangulated, [" << n_pt - n_kept
                  << "] points dropped, [" << n_obs_dropped << "] observations dropped" << std::endl;
        return true;
    }

    bool quiet = false;

private:
    static void k4_of(const Matrix3f &K, float K4[4]) { K4[0] = K(0, 0); K4[1] = K(0, 2); K4[2] = K(1, 1); K4[3] = K(1, 2); }
    static void gather(const frame_t &f1, const frame_t &f2, const std::vector<DMatch> &matches, int rate, std::vector<float> &a, std::vector<float> &b)
    {
        for (size_t i = 0; i < matches.size(); ++i) {
            if (int(i) % rate != 0) continue;
            a.push_back(f1.keypoints[size_t(matches[i].queryIdx)].pt.x); a.push_back(f1.keypoints[size_t(matches[i].queryIdx)].pt.y);
            b.push_back(f2.keypoints[size_t(matches[i].trainIdx)].pt.x); b.push_back(f2.keypoints[size_t(matches[i].trainIdx)].pt.y);
        }
    }
    // estimate_motion.h:41-46, float arithmetic
    static void pixel2cam(std::vector<float> &p, const Matrix3f &K)
    {
        for (size_t i = 0; i + 1 < p.size(); i += 2) { p[i] = (p[i] - K(0, 2)) / K(0, 0); p[i + 1] = (p[i + 1] - K(1, 2)) / K(1, 1); }
    }
};

// ---- cv::Rodrigues as used at ba.cpp:82 (matrix -> vector) and :239 (vector -> matrix) -------------
inline void rotation_to_angle_axis(const double R[9], double aa[3])
{
    const double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = std::sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1.0) * 0.5;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double theta = std::acos(c);
    if (s < 1e-5) {
        if (c > 0) { aa[0] = aa[1] = aa[2] = 0.0; return; }
        double v[3] = {std::sqrt(std::max((R[0] + 1) * 0.5, 0.0)), std::sqrt(std::max((R[4] + 1) * 0.5, 0.0)),
                       std::sqrt(std::max((R[8] + 1) * 0.5, 0.0))};
        if (R[1] < 0) v[1] = -v[1];
        if (R[2] < 0) v[2] = -v[2];
        if ((R[5] > 0) != (v[1] * v[2] > 0)) v[2] = -v[2];
        const double nrm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int i = 0; i < 3; ++i) aa[i] = v[i] * (theta / std::max(nrm, 1e-300));
        return;
    }
    const double k = 0.5 * theta / s;
    aa[0] = rx * k; aa[1] = ry * k; aa[2] = rz * k;
}

inline void angle_axis_to_rotation(const double aa[3], double R[9])
{
    const double theta = std::sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
    if (theta < 2.2204460492503131e-16) { for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
    const double k[3] = {aa[0] / theta, aa[1] / theta, aa[2] / theta};
    const double c = std::cos(theta), s = std::sin(theta), c1 = 1.0 - c;
    R[0] = c + c1 * k[0] * k[0]; R[1] = c1 * k[0] * k[1] - s * k[2]; R[2] = c1 * k[0] * k[2] + s * k[1];
    R[3] = c1 * k[1] * k[0] + s * k[2]; R[4] = c + c1 * k[1] * k[1]; R[5] = c1 * k[1] * k[2] - s * k[0];
    R[6] = c1 * k[2] * k[0] - s * k[1]; R[7] = c1 * k[2] * k[1] + s * k[0]; R[8] = c + c1 * k[2] * k[2];
}

// ---- bundle adjustment (ba.h:28-106) -----------------------------------------------------------------
class BundleAdjustment {
public:
    BundleAdjustment() { initBA(); esfm_ba_options_default(&options_); }

    int num_observations() const { return num_observations_; }
    double *mutable_cameras() { return parameters_.data(); }
    double *mutable_points() { return parameters_.data() + 6 * num_cameras_; }
    double *mutable_calib() { return parameters_.data() + 6 * num_cameras_ + 3 * num_points_; }   // ba.h:45; several blocks: 4 doubles each
    // radial solves: k1, k2 of every group, behind the 4 G pinhole values
    double *mutable_radial() { return mutable_calib() + 4 * group_camera_ids_.size(); }
    // pixels: the box that holds fx, cx, fy, cy in a radial solve with fix_calib_tolerance_BA == 0 (every free block has a box)
    static constexpr double kHeldPinhole = 1e-3;

    bool initBA()  // ba.h:59-75
    {
        point_index_.clear(); camera_index_.clear(); points_2d_.clear(); calibs_.clear(); parameters_.clear();
        camera_group_.clear(); group_camera_ids_.clear();
        radial_tolerance_ = 0.0;
        num_cameras_ = num_points_ = num_parameters_ = num_observations_ = 0;
        ref_process_camera_id_ = -1;
        if (verbose) std::cout << "Bundle Ajustment parameters initialization done." << std::endl;
        return true;
    }

    // ba.cpp:12-130.  Same observation list in the same order (camera-major, point index ascending; for a
    // point the FIRST keypoint with has_match and a matching id, the `break` at :44) as the reference's
    // O(Ncam*Npts*Nkp) triple loop, derived with one hash map per frame.
    // radial_tolerance > 0: every distinct camera_id -- ONE id included -- opens a block fx, cx, fy, cy, k1, k2 that starts from its first
    // processed frame's K_cam and radial_cam; the observations are a frame's keypoints_raw where it has them.  0: as before.
    bool setBAProblem(std::vector<frame_t> &frames, std::vector<bool> &process_frame_id, pointcloud_sparse_t &sfm_sparse_points,
                      double fix_calib_tolerance_BA, int reference_frame_id, double radial_tolerance = 0.0)
    {
        const bool radial = radial_tolerance > 0.0;
        radial_tolerance_ = radial ? radial_tolerance : 0.0;
        num_observations_ = 0; num_cameras_ = 0;
        num_points_ = int(sfm_sparse_points.unique_point_ids.size());
        for (size_t i = 0; i < frames.size(); ++i) {
            if (process_frame_id[i]) continue;  // 0 = registered
            calibs_.push_back(frames[i].K_cam);
            std::unordered_map<int, int> first_kp;  // track id -> lowest keypoint index with has_match
            const frame_t &fr = frames[i];
            for (size_t j = 0; j < fr.unique_pixel_ids.size(); ++j)
                if (fr.unique_pixel_has_match[j]) first_kp.emplace(fr.unique_pixel_ids[j], int(j));  // emplace keeps the first
            for (int k = 0; k < num_points_; ++k) {
                auto it = first_kp.find(sfm_sparse_points.unique_point_ids[size_t(k)]);
                if (it == first_kp.end()) continue;
                points_2d_.push_back(radial && !fr.keypoints_raw.empty() ? fr.keypoints_raw[size_t(it->second)] : fr.keypoints[size_t(it->second)].pt);
                point_index_.push_back(k);
                camera_index_.push_back(num_cameras_);
                ++num_observations_;
            }
            if (int(i) == reference_frame_id) ref_process_camera_id_ = num_cameras_;
            ++num_cameras_;
        }
        // multiple-camera mode: free intrinsics over processed frames of more than one camera_id open one block per distinct id, in
        // order of first appearance; one distinct id leaves the shared block of calibs_[0] in charge
        if (fix_calib_tolerance_BA != 0 || radial) {
            std::vector<int> ids, order;
            for (size_t i = 0; i < frames.size(); ++i) {
                if (process_frame_id[i]) continue;
                ids.push_back(frames[i].camera_id);
                if (std::find(order.begin(), order.end(), frames[i].camera_id) == order.end()) order.push_back(frames[i].camera_id);
            }
            if (order.size() > 1 || (radial && !order.empty())) {
                group_camera_ids_ = order;
                for (int id : ids) camera_group_.push_back(int(std::find(order.begin(), order.end(), id) - order.begin()));
            }
        }
        const int n_blocks = group_camera_ids_.empty() ? 1 : int(group_camera_ids_.size());
        const bool radial_blocks = radial && !group_camera_ids_.empty();
        num_parameters_ = 6 * num_cameras_ + 3 * num_points_ + (fix_calib_tolerance_BA != 0 || radial_blocks ? 4 * n_blocks : 0) + (radial_blocks ? 2 * n_blocks : 0);
        parameters_.assign(size_t(num_parameters_), 0.0);
        int k = 0;
        for (size_t i = 0; i < frames.size(); ++i) {
            if (process_frame_id[i]) continue;
            double R[9], aa[3];
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[3 * r + c] = double(frames[i].pose_cam(r, c));
            rotation_to_angle_axis(R, aa);
            for (int a = 0; a < 3; ++a) {
                parameters_[size_t(6 * k + a)] = double(float(aa[a]));  // rot_vec is CV_32F (:86-88)
                parameters_[size_t(6 * k + 3 + a)] = double(frames[i].pose_cam(a, 3));
            }
            ++k;
        }
        for (int i = 0; i < num_points_; ++i) {
            const PointXYZRGB &p = sfm_sparse_points.points[size_t(i)];
            parameters_[size_t(6 * num_cameras_ + 3 * i)] = p.x;
            parameters_[size_t(6 * num_cameras_ + 3 * i + 1)] = p.y;
            parameters_[size_t(6 * num_cameras_ + 3 * i + 2)] = p.z;
        }
        if ((fix_calib_tolerance_BA != 0 || radial_blocks) && !group_camera_ids_.empty()) {
            // the reference's calibs_[0] rule, per group: a group starts from the K_cam (and radial_cam) of its first processed frame
            std::vector<const frame_t *> processed;
            for (size_t i = 0; i < frames.size(); ++i) if (!process_frame_id[i]) processed.push_back(&frames[i]);
            for (int g = 0; g < n_blocks; ++g) {
                const size_t first = size_t(std::find(camera_group_.begin(), camera_group_.end(), g) - camera_group_.begin());
                double *k4 = mutable_calib() + 4 * g;
                k4[0] = calibs_[first](0, 0); k4[1] = calibs_[first](0, 2); k4[2] = calibs_[first](1, 1); k4[3] = calibs_[first](1, 2);
                if (radial_blocks) { mutable_radial()[2 * g] = processed[first]->radial_cam[0]; mutable_radial()[2 * g + 1] = processed[first]->radial_cam[1]; }
            }
        } else if (fix_calib_tolerance_BA != 0 && !calibs_.empty()) {
            parameters_[size_t(num_parameters_ - 4)] = calibs_[0](0, 0); parameters_[size_t(num_parameters_ - 3)] = calibs_[0](0, 2);
            parameters_[size_t(num_parameters_ - 2)] = calibs_[0](1, 1); parameters_[size_t(num_parameters_ - 1)] = calibs_[0](1, 2);
        }
        if (verbose) {
            std::cout << "Find [ " << num_observations_ << " ] Observations in total." << std::endl;
            std::cout << "There are [ " << num_cameras_ << " ] cameras and [ " << num_points_ << " ] 3D points." << std::endl;
        }
        return 2 * num_observations_ > num_parameters_;  // "Ready to solve" (:120-129)
    }

    // ba.cpp:132-212: ceres::Solve -> esfm_ba_solve_ex.  Fixed intrinsics (:142-164) or the shared free block bounded to
    // +- tolerance (:167-196); a reference frame named in setBAProblem is bounded to +-1e-10 (:134, :155-162).
    // radial_tolerance > 0: the box half width of k1, k2 of every group; positive exactly when setBAProblem's was (the layout of
    // parameters_ is the one set up there)
    bool solveBA(double fix_calib_tolerance_BA, double radial_tolerance = 0.0)
    {
        if ((radial_tolerance > 0.0) != (radial_tolerance_ > 0.0)) {
            std::cerr << "solveBA: radial_tolerance must be positive exactly when setBAProblem's was" << std::endl;
            return false;
        }
        const double fixed_threshold = 1e-10;  // :134
        std::vector<float> K4(size_t(4 * num_cameras_));
        for (int c = 0; c < num_cameras_; ++c) {
            K4[size_t(4 * c)] = calibs_[size_t(c)](0, 0); K4[size_t(4 * c + 1)] = calibs_[size_t(c)](0, 2);
            K4[size_t(4 * c + 2)] = calibs_[size_t(c)](1, 1); K4[size_t(4 * c + 3)] = calibs_[size_t(c)](1, 2);
        }
        options_.verbose = verbose ? 1 : 0;  // minimizer_progress_to_stdout (:204)
        if (radial_tolerance > 0 && !group_camera_ids_.empty()) {   // one block fx, cx, fy, cy, k1, k2 per camera group
            const std::vector<double> tol(group_camera_ids_.size(), fix_calib_tolerance_BA != 0 ? fix_calib_tolerance_BA : kHeldPinhole);
            const std::vector<double> rtol(group_camera_ids_.size(), radial_tolerance);
            int rcr = esfm_ba_solve_radial_groups(default_ctx(), num_cameras_, num_points_, num_observations_, camera_index_.data(), point_index_.data(),
                                                  reinterpret_cast<const float *>(points_2d_.data()), mutable_cameras(), mutable_points(),
                                                  int(group_camera_ids_.size()), camera_group_.data(), mutable_calib(), tol.data(), mutable_radial(),
                                                  rtol.data(), ref_process_camera_id_, fixed_threshold, &options_, nullptr, nullptr, &summary_);
            if (rcr != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
            return true;
        }
        if (fix_calib_tolerance_BA != 0 && !group_camera_ids_.empty()) {   // one free block per camera group, each within +- tolerance
            const std::vector<double> tol(group_camera_ids_.size(), fix_calib_tolerance_BA);
            int rcg = esfm_ba_solve_groups(default_ctx(), num_cameras_, num_points_, num_observations_, camera_index_.data(), point_index_.data(),
                                           reinterpret_cast<const float *>(points_2d_.data()), mutable_cameras(), mutable_points(),
                                           int(group_camera_ids_.size()), camera_group_.data(), mutable_calib(), tol.data(),
                                           ref_process_camera_id_, fixed_threshold, &options_, nullptr, nullptr, &summary_);
            if (rcg != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
            return true;
        }
        int rc = esfm_ba_solve_ex(default_ctx(), num_cameras_, num_points_, num_observations_, camera_index_.data(), point_index_.data(),
                                  reinterpret_cast<const float *>(points_2d_.data()), K4.data(), mutable_cameras(), mutable_points(),
                                  fix_calib_tolerance_BA != 0 ? mutable_calib() : nullptr, fix_calib_tolerance_BA,
                                  ref_process_camera_id_, fixed_threshold, &options_, nullptr, nullptr, &summary_);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        return true;
    }

    // ba.cpp:214-288
    bool doSFMBA(std::vector<frame_t> &frames, std::vector<bool> &process_frame_id, pointcloud_sparse_t &sfm_sparse_points,
                 double fix_calib_tolerance_BA = 0.0, int reference_frame_id = -1, double radial_tolerance = 0.0)
    {
        auto tic = std::chrono::steady_clock::now();
        initBA();
        setBAProblem(frames, process_frame_id, sfm_sparse_points, fix_calib_tolerance_BA, reference_frame_id, radial_tolerance);
        const bool ok = solveBA(fix_calib_tolerance_BA, radial_tolerance);
        const bool radial_blocks = radial_tolerance_ > 0 && !group_camera_ids_.empty();
        int k = 0;
        for (size_t i = 0; i < frames.size(); ++i) {
            if (process_frame_id[i]) continue;
            const double aa[3] = {double(float(parameters_[size_t(6 * k)])), double(float(parameters_[size_t(6 * k + 1)])),
                                  double(float(parameters_[size_t(6 * k + 2)]))};  // rot_vec float (:235-237)
            double R[9];
            angle_axis_to_rotation(aa, R);
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) frames[i].pose_cam(r, c) = float(R[3 * r + c]);
                frames[i].pose_cam(r, 3) = float(parameters_[size_t(6 * k + 3 + r)]);
            }
            ++k;
            if (radial_blocks) {
                frames[i].radial_cam[0] = mutable_radial()[2 * camera_group_[size_t(k - 1)]];
                frames[i].radial_cam[1] = mutable_radial()[2 * camera_group_[size_t(k - 1)] + 1];
            }
            if ((fix_calib_tolerance_BA != 0 || radial_blocks) && !group_camera_ids_.empty()) {   // each group's result goes to that group's frames only
                const double *k4 = mutable_calib() + 4 * camera_group_[size_t(k - 1)];
                frames[i].K_cam(0, 0) = float(k4[0]); frames[i].K_cam(0, 2) = float(k4[1]);
                frames[i].K_cam(1, 1) = float(k4[2]); frames[i].K_cam(1, 2) = float(k4[3]);
            } else if (fix_calib_tolerance_BA != 0) {  // :250-256
                frames[i].K_cam(0, 0) = float(parameters_[size_t(num_parameters_ - 4)]);
                frames[i].K_cam(0, 2) = float(parameters_[size_t(num_parameters_ - 3)]);
                frames[i].K_cam(1, 1) = float(parameters_[size_t(num_parameters_ - 2)]);
                frames[i].K_cam(1, 2) = float(parameters_[size_t(num_parameters_ - 1)]);
            }
        }
        if (verbose && fix_calib_tolerance_BA != 0 && !group_camera_ids_.empty()) {
            std::cout << "Calib intrinsic parameters after BA:" << std::endl;
            for (size_t g = 0; g < group_camera_ids_.size(); ++g) {
                const double *k4 = mutable_calib() + 4 * g;
                std::cout << "camera " << group_camera_ids_[g] << " [fx:" << k4[0] << " ,cx:" << k4[1] << " ,fy:" << k4[2] << " ,cy:" << k4[3] << " ]" << std::endl;
            }
        }
        if (verbose && fix_calib_tolerance_BA != 0 && group_camera_ids_.empty())
            std::cout << "Calib intrinsic parameters after BA:" << std::endl
                      << "[fx:" << parameters_[size_t(num_parameters_ - 4)] << " ,cx:" << parameters_[size_t(num_parameters_ - 3)]
                      << " ,fy:" << parameters_[size_t(num_parameters_ - 2)] << " ,cy:" << parameters_[size_t(num_parameters_ - 1)] << " ]"
                      << std::endl;
        for (int i = 0; i < num_points_; ++i) {  // :277-279, float truncation
            sfm_sparse_points.points[size_t(i)].x = float(parameters_[size_t(6 * num_cameras_ + 3 * i)]);
            sfm_sparse_points.points[size_t(i)].y = float(parameters_[size_t(6 * num_cameras_ + 3 * i + 1)]);
            sfm_sparse_points.points[size_t(i)].z = float(parameters_[size_t(6 * num_cameras_ + 3 * i + 2)]);
        }
        if (verbose) {
            std::chrono::duration<double> dt = std::chrono::steady_clock::now() - tic;
            std::cout << "Bundle Ajustment cost = " << dt.count() << " seconds. " << std::endl << "Bundle Ajustment done." << std::endl;
        }
        return ok;
    }

    bool verbose = false;
    esfm_ba_options options_;
    esfm_ba_summary summary_;
    // the reference's private state (ba.h:86-105), public here for the tests
    int num_cameras_ = 0, num_points_ = 0, num_observations_ = 0, num_parameters_ = 0;
    std::vector<int> point_index_, camera_index_;
    std::vector<double> parameters_;  // [6 per camera (rot, tran) | 3 per point | optional fx,cx,fy,cy]
    std::vector<Point2f> points_2d_;
    std::vector<Matrix3f> calibs_;
    int ref_process_camera_id_ = -1;
    // multiple-camera mode: group of every processed camera and the camera_id of every group (first appearance first); both empty
    // unless the intrinsics are free and the processed frames carry more than one camera_id
    std::vector<int> camera_group_, group_camera_ids_;
    double radial_tolerance_ = 0.0;   // > 0: the problem set up last frees k1, k2 per camera_id (one id included)
};

// ---- dense reconstruction (esfm.h "Dense reconstruction"; the reference README's TODO "add multi-view stereo dense
// reconstruction"): the same CSR of observed cloud points as easysfm_amd/mvs.py, then esfm_mvs_plan, esfm_mvs_depth_maps and
// esfm_mvs_fuse; reconstructMerged adds the merge of the dense cloud (esfm.h "Dense-cloud merge").  process_frame_id as in
// doSFMBA: false = registered.
class DenseReconstruction {
public:
    // returns false (message on stderr) on a library error; n_depth_maps = views with a depth range
    bool reconstruct(const std::vector<frame_t> &frames, const std::vector<bool> &process_frame_id, const pointcloud_sparse_t &cloud,
                     std::vector<PointXYZRGB> &dense, int &n_depth_maps)
    {
        return run(frames, process_frame_id, cloud, dense, n_depth_maps, nullptr, nullptr);
    }

    // reconstruct, then the merge of the dense cloud (easysfm_amd.mvs.dense_merge): esfm_mvs_fuse_ex for each point's pixel,
    // esfm_mvs_normals gathered by it, the view as tag, esfm_cloud_voxel_merge with dense_merge's defaults: a voxel of twice the lower
    // median of the points' pixel footprints depth / fx, kept if two or more views support it.  dense is reconstruct's cloud.  At most
    // 64 frames.
    bool reconstructMerged(const std::vector<frame_t> &frames, const std::vector<bool> &process_frame_id, const pointcloud_sparse_t &cloud,
                           std::vector<PointXYZRGB> &dense, int &n_depth_maps, std::vector<PointXYZRGBNormal> &merged)
    {
        if (frames.size() > 64) { std::cerr << "dense merge tags points by view: at most 64 views" << std::endl; return false; }
        return run(frames, process_frame_id, cloud, dense, n_depth_maps, &merged, nullptr);
    }

    // reconstruct (and the merge, if merged is not NULL), then the surface (easysfm_amd.mesh.dense_mesh with MeshOptions' defaults,
    // esfm.h "Surface reconstruction"): the depth maps masked to the pixels the fusion kept, a voxel of twice the merge's median pixel
    // footprint -- enlarged just enough for 2^24 voxels and 1024 per axis --, the grid around the 1st..99th percentile box of the
    // fused points padded by the truncation distance of 4 voxels, esfm_mvs_mesh.  At most 64 frames.
    bool reconstructMesh(const std::vector<frame_t> &frames, const std::vector<bool> &process_frame_id, const pointcloud_sparse_t &cloud,
                         std::vector<PointXYZRGB> &dense, int &n_depth_maps, std::vector<PointXYZRGBNormal> *merged, TriangleMesh &mesh)
    {
        if (frames.size() > 64) { std::cerr << "dense mesh integrates at most 64 views" << std::endl; return false; }
        return run(frames, process_frame_id, cloud, dense, n_depth_maps, merged, &mesh);
    }

    // esfm.h "Mesh clean-up" with its default options (easysfm_amd.mesh.mesh_clean): small components dropped, Taubin smoothing,
    // normals recomputed from the faces; the mesh is replaced.  n_before / n_after (may be NULL): its components before and after.
    bool cleanMesh(TriangleMesh &mesh, int *n_before = nullptr, int *n_after = nullptr)
    {
        const int nv = int(mesh.vertices.size()), nt = int(mesh.triangles.size() / 3);
        std::vector<float> vtx(size_t(3) * mesh.vertices.size()), out_vtx(vtx.size()), out_nrm(vtx.size());
        std::vector<uint8_t> col(vtx.size()), out_col(vtx.size());
        std::vector<int32_t> out_tri(mesh.triangles.size()), labels(mesh.vertices.size());
        for (size_t k = 0; k < mesh.vertices.size(); ++k) {
            const PointXYZRGBNormal &p = mesh.vertices[k];
            vtx[3 * k] = p.x; vtx[3 * k + 1] = p.y; vtx[3 * k + 2] = p.z;
            col[3 * k] = p.r; col[3 * k + 1] = p.g; col[3 * k + 2] = p.b;
        }
        esfm_mesh_clean_options opt;
        esfm_mesh_clean_options_default(&opt);
        int32_t kv = 0, kt = 0, before = 0, after = 0;
        int rc = n_before ? esfm_mesh_components(default_ctx(), nv, nt, mesh.triangles.data(), labels.data(), nullptr, &before) : ESFM_OK;
        if (rc == ESFM_OK)
            rc = esfm_mesh_clean(default_ctx(), nv, nt, vtx.data(), col.data(), mesh.triangles.data(), &opt, out_vtx.data(), out_nrm.data(), out_col.data(),
                                 out_tri.data(), nullptr, nullptr, &kv, &kt);
        if (rc == ESFM_OK && n_after) rc = esfm_mesh_components(default_ctx(), kv, kt, out_tri.data(), labels.data(), nullptr, &after);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        out_tri.resize(size_t(3) * size_t(kt));
        mesh.triangles.swap(out_tri);
        mesh.vertices.assign(size_t(kv), PointXYZRGBNormal());
        for (size_t k = 0; k < mesh.vertices.size(); ++k) {
            PointXYZRGBNormal &p = mesh.vertices[k];
            p.x = out_vtx[3 * k]; p.y = out_vtx[3 * k + 1]; p.z = out_vtx[3 * k + 2];
            p.nx = out_nrm[3 * k]; p.ny = out_nrm[3 * k + 1]; p.nz = out_nrm[3 * k + 2];
            p.r = out_col[3 * k]; p.g = out_col[3 * k + 1]; p.b = out_col[3 * k + 2];
        }
        if (n_before) *n_before = before;
        if (n_after) *n_after = after;
        return true;
    }

    // esfm.h "Mesh simplification" with its default options (easysfm_amd.mesh.mesh_simplify as run_sfm calls it): all vertices of one
    // cell of cells_per_voxel voxels' side, counted from the volume's origin, become one; the mesh is replaced.
    bool simplifyMesh(TriangleMesh &mesh, float cells_per_voxel, float *cell_used = nullptr)
    {
        const int nv = int(mesh.vertices.size()), nt = int(mesh.triangles.size() / 3);
        std::vector<float> vtx(size_t(3) * mesh.vertices.size()), out_vtx(vtx.size()), out_nrm(vtx.size());
        std::vector<uint8_t> col(vtx.size()), out_col(vtx.size());
        std::vector<int32_t> out_tri(mesh.triangles.size());
        for (size_t k = 0; k < mesh.vertices.size(); ++k) {
            const PointXYZRGBNormal &p = mesh.vertices[k];
            vtx[3 * k] = p.x; vtx[3 * k + 1] = p.y; vtx[3 * k + 2] = p.z;
            col[3 * k] = p.r; col[3 * k + 1] = p.g; col[3 * k + 2] = p.b;
        }
        esfm_mesh_simplify_options opt;
        esfm_mesh_simplify_options_default(&opt);
        const float cell = cells_per_voxel * mesh.voxel_size;
        int32_t kv = 0, kt = 0;
        const int rc = esfm_mesh_simplify(default_ctx(), nv, nt, vtx.data(), col.data(), mesh.triangles.data(), mesh.origin, cell, &opt, out_vtx.data(),
                                          out_nrm.data(), out_col.data(), out_tri.data(), nullptr, nullptr, &kv, &kt);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        out_tri.resize(size_t(3) * size_t(kt));
        mesh.triangles.swap(out_tri);
        mesh.vertices.assign(size_t(kv), PointXYZRGBNormal());
        for (size_t k = 0; k < mesh.vertices.size(); ++k) {
            PointXYZRGBNormal &p = mesh.vertices[k];
            p.x = out_vtx[3 * k]; p.y = out_vtx[3 * k + 1]; p.z = out_vtx[3 * k + 2];
            p.nx = out_nrm[3 * k]; p.ny = out_nrm[3 * k + 1]; p.nz = out_nrm[3 * k + 2];
            p.r = out_col[3 * k]; p.g = out_col[3 * k + 1]; p.b = out_col[3 * k + 2];
        }
        if (cell_used) *cell_used = cell;
        return true;
    }

    // esfm.h "Mesh texturing" with its default options, as run_sfm(dense_mesh_texture=...) runs it: every triangle chooses one of the
    // registered frames (process_frame_id false; at most 64, in frame order), then a square atlas of ceil(sqrt(ceil(T / 2))) squares per
    // row is baked.  texels 0 derives the chart size: the median over the labelled triangles of sqrt(2 score), rounded up, clamped to
    // 4 .. 64.  uv: T x 3 x 2; atlas: atlas_rows x atlas_cols x 3 RGB; texels_used: the chart size.
    // level: not NULL runs levelTexture between the view choice and the bake, as run_sfm(dense_mesh_texture_level=True) does, and
    // receives its counts.
    bool textureMesh(const TriangleMesh &mesh, const std::vector<frame_t> &frames, const std::vector<bool> &process_frame_id, int texels,
                     std::vector<float> &uv, std::vector<uint8_t> &atlas, int &atlas_rows, int &atlas_cols, int &n_labelled, int &n_views, int &texels_used,
                     esfm_mesh_texture_level_stats *level = nullptr)
    {
        uv.clear(); atlas.clear();
        atlas_rows = atlas_cols = n_labelled = n_views = texels_used = 0;
        int rows = -1, cols = -1, ch = -1;
        std::vector<uint8_t> images;
        std::vector<float> K4, poses;
        for (size_t v = 0; v < frames.size(); ++v) {
            if (process_frame_id[v]) continue;
            const frame_t &f = frames[v];
            const ImageMat &im = f.rgb_image;
            if (im.empty()) { std::cerr << "mesh texture: registered frame " << v << " has no image" << std::endl; return false; }
            if (rows < 0) { rows = im.rows; cols = im.cols; ch = im.channels; }
            if (im.rows != rows || im.cols != cols || im.channels != ch) { std::cerr << "mesh texture: frames differ in size" << std::endl; return false; }
            images.insert(images.end(), im.data.begin(), im.data.end());
            const float k4[4] = {f.K_cam(0, 0), f.K_cam(0, 2), f.K_cam(1, 1), f.K_cam(1, 2)};
            K4.insert(K4.end(), k4, k4 + 4);
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) poses.push_back(f.pose_cam(i, j));
            ++n_views;
        }
        const int nv = int(mesh.vertices.size()), nt = int(mesh.triangles.size() / 3);
        std::vector<float> vtx(size_t(3) * mesh.vertices.size());
        std::vector<uint8_t> col(vtx.size());
        for (size_t k = 0; k < mesh.vertices.size(); ++k) {
            const PointXYZRGBNormal &p = mesh.vertices[k];
            vtx[3 * k] = p.x; vtx[3 * k + 1] = p.y; vtx[3 * k + 2] = p.z;
            col[3 * k] = p.r; col[3 * k + 1] = p.g; col[3 * k + 2] = p.b;
        }
        esfm_mesh_texture_options opt;
        esfm_mesh_texture_options_default(&opt);
        std::vector<int32_t> label(size_t(nt), -1);
        std::vector<float> score(size_t(nt), 0.f);
        int rc = esfm_mesh_texture_views(default_ctx(), nv, nt, vtx.data(), mesh.triangles.data(), n_views, rows, cols, K4.data(), poses.data(), &opt,
                                         label.data(), score.data(), nullptr);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        std::vector<double> legs;
        for (int t = 0; t < nt; ++t)
            if (label[size_t(t)] >= 0) { ++n_labelled; legs.push_back(std::sqrt(2.0 * double(score[size_t(t)]))); }
        texels_used = texels;
        if (texels == 0) {
            texels_used = 4;
            if (!legs.empty()) {
                std::sort(legs.begin(), legs.end());
                const size_t h = legs.size() / 2;
                const double median = legs.size() % 2 ? legs[h] : (legs[h - 1] + legs[h]) / 2.0;
                texels_used = int(std::min(64.0, std::max(4.0, std::ceil(median))));
            }
        }
        const int squares = (nt + 1) / 2;
        int width = int(std::ceil(std::sqrt(double(squares))));
        while (width * width < squares) ++width;
        if (width < 1) width = 1;
        int32_t need = 0;
        uv.assign(size_t(6) * size_t(nt), 0.f);
        std::vector<float> offsets;
        if (level && !levelTexture(vtx, mesh.triangles, label, n_views, rows, cols, ch, images, K4, poses, offsets, *level)) return false;
        const float *off = level ? offsets.data() : nullptr;              // NULL: esfm_mesh_texture_bake itself
        rc = esfm_mesh_texture_bake_ex(default_ctx(), nv, nt, vtx.data(), col.data(), mesh.triangles.data(), label.data(), n_views, rows, cols, ch, images.data(),
                                       K4.data(), poses.data(), texels_used, width, 0, nullptr, uv.data(), &need, off);      // the height first
        if (rc != ESFM_OK && need <= 0) { std::cerr << esfm_last_error() << std::endl; return false; }
        atlas_rows = need; atlas_cols = width * texels_used;
        atlas.assign(size_t(atlas_rows) * size_t(atlas_cols) * 3, 0);
        if (need > 0) {
            rc = esfm_mesh_texture_bake_ex(default_ctx(), nv, nt, vtx.data(), col.data(), mesh.triangles.data(), label.data(), n_views, rows, cols, ch,
                                           images.data(), K4.data(), poses.data(), texels_used, width, atlas_rows, atlas.data(), uv.data(), &need, off);
            if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        }
        return true;
    }

    // esfm.h "Mesh texturing", esfm_mesh_texture_level with its default options: one colour offset per triangle corner and channel
    // (T x 3 x 3) that takes the steps out of the seams between triangles of different labels; the bake adds them.
    bool levelTexture(const std::vector<float> &vtx, const std::vector<int32_t> &triangles, const std::vector<int32_t> &label, int n_views, int rows,
                      int cols, int ch, const std::vector<uint8_t> &images, const std::vector<float> &K4, const std::vector<float> &poses,
                      std::vector<float> &offsets, esfm_mesh_texture_level_stats &stats)
    {
        const int nv = int(vtx.size() / 3), nt = int(triangles.size() / 3);
        esfm_mesh_texture_level_options opt;
        esfm_mesh_texture_level_options_default(&opt);
        offsets.assign(size_t(9) * size_t(nt), 0.f);
        const int rc = esfm_mesh_texture_level(default_ctx(), nv, nt, vtx.data(), triangles.data(), label.data(), n_views, rows, cols, ch, images.data(),
                                               K4.data(), poses.data(), &opt, offsets.data(), nullptr, &stats);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        return true;
    }

    // esfm.h "Mesh rendering" with its default options, as run_sfm(dense_mesh_render_dir=...) runs it: the mesh is drawn into every
    // registered frame (process_frame_id false; in frame order, 64 views per call), with the atlas if uv and atlas are given (textureMesh's),
    // else with the vertex colours, and each picture is written to dir/render_%04d.png, numbered by frame index; dir must exist.  covered: the pixels
    // some triangle owns; sum_abs: the sum over them and the three channels of |picture - photograph| (a grey photograph counts as a
    // grey triple).  Integer arithmetic: the mean sum_abs / (3 covered) prints with the digits of easysfm_amd.mesh_render_error's.
    bool renderMesh(const TriangleMesh &mesh, const std::vector<frame_t> &frames, const std::vector<bool> &process_frame_id, const std::vector<float> *uv,
                    int atlas_rows, int atlas_cols, const std::vector<uint8_t> *atlas, const std::string &dir, int &n_views, long long &covered,
                    long long &sum_abs)
    {
        n_views = 0; covered = 0; sum_abs = 0;
        const int nv = int(mesh.vertices.size()), nt = int(mesh.triangles.size() / 3);
        std::vector<float> vtx(size_t(3) * mesh.vertices.size());
        std::vector<uint8_t> col(vtx.size());
        for (size_t k = 0; k < mesh.vertices.size(); ++k) {
            const PointXYZRGBNormal &p = mesh.vertices[k];
            vtx[3 * k] = p.x; vtx[3 * k + 1] = p.y; vtx[3 * k + 2] = p.z;
            col[3 * k] = p.r; col[3 * k + 1] = p.g; col[3 * k + 2] = p.b;
        }
        const bool textured = uv && atlas && !atlas->empty();
        const float no_uv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};             // (no triangle: a pointer that is not NULL goes with the atlas)
        esfm_mesh_render_options opt;
        esfm_mesh_render_options_default(&opt);
        std::vector<size_t> registered;
        for (size_t v = 0; v < frames.size(); ++v) if (!process_frame_id[v]) registered.push_back(v);
        for (size_t first = 0; first < registered.size(); first += 64) {
            const int n = int(std::min<size_t>(64, registered.size() - first));
            const ImageMat &im0 = frames[registered[first]].rgb_image;
            const int rows = im0.rows, cols = im0.cols;
            std::vector<float> K4, poses;
            for (int k = 0; k < n; ++k) {
                const frame_t &f = frames[registered[first + size_t(k)]];
                if (f.rgb_image.empty() || f.rgb_image.rows != rows || f.rgb_image.cols != cols) { std::cerr << "mesh render: frames differ in size or have no image" << std::endl; return false; }
                const float k4[4] = {f.K_cam(0, 0), f.K_cam(0, 2), f.K_cam(1, 1), f.K_cam(1, 2)};
                K4.insert(K4.end(), k4, k4 + 4);
                for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) poses.push_back(f.pose_cam(i, j));
            }
            const size_t pixels = size_t(rows) * size_t(cols);
            std::vector<uint8_t> rgb(size_t(n) * pixels * 3);
            std::vector<int32_t> id(size_t(n) * pixels);
            const int rc = esfm_mesh_render(default_ctx(), nv, nt, vtx.data(), mesh.triangles.data(), textured ? nullptr : col.data(),
                                            textured ? (nt ? uv->data() : no_uv) : nullptr, textured ? atlas_rows : 0, textured ? atlas_cols : 0,
                                            textured ? atlas->data() : nullptr, n, rows, cols, K4.data(), poses.data(), &opt, rgb.data(), nullptr, id.data());
            if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
            for (int k = 0; k < n; ++k) {
                const size_t frame = registered[first + size_t(k)];
                const ImageMat &im = frames[frame].rgb_image;
                const uint8_t *pic = rgb.data() + size_t(k) * pixels * 3;
                for (size_t p = 0; p < pixels; ++p) {
                    if (id[size_t(k) * pixels + p] < 0) continue;
                    ++covered;
                    for (int c = 0; c < 3; ++c) {
                        const int photo = im.channels == 3 ? im.data[3 * p + size_t(2 - c)] : im.data[p];      // BGR photographs, RGB pictures
                        sum_abs += std::abs(int(pic[3 * p + size_t(c)]) - photo);
                    }
                }
                char name[32];
                std::snprintf(name, sizeof(name), "render_%04d.png", int(frame));
                const std::string e = png::write_rgb((std::filesystem::path(dir) / name).string(), rows, cols, pic);
                if (!e.empty()) { std::cerr << e << std::endl; return false; }
                ++n_views;
            }
        }
        return true;
    }

private:
    // easysfm_amd.mesh.mesh_arrays behind the fusion: pixel[k] is the pixel of fused point k
    static bool mesh_of(int n, int rows, int cols, int ch, const std::vector<uint8_t> &images, const std::vector<float> &K4,
                        const std::vector<float> &poses, const std::vector<float> &depth, const std::vector<int32_t> &pixel, size_t N,
                        const std::vector<float> &xyz, TriangleMesh &mesh)
    {
        const size_t view_px = size_t(rows) * size_t(cols);
        std::vector<float> masked(depth.size(), 0.f), foot(N);
        for (size_t k = 0; k < N; ++k) {
            const size_t px = size_t(pixel[k]);
            masked[px] = depth[px];
            foot[k] = depth[px] / K4[size_t(4) * (px / view_px)];
        }
        std::nth_element(foot.begin(), foot.begin() + (N - 1) / 2, foot.end());         // the lower median, sorted[(n - 1) / 2]
        double h = double(2.0f * foot[(N - 1) / 2]);
        double lo[3], hi[3];
        for (int c = 0; c < 3; ++c) {
            std::vector<double> s;
            for (size_t k = 0; k < N; ++k)
                if (std::isfinite(xyz[3 * k]) && std::isfinite(xyz[3 * k + 1]) && std::isfinite(xyz[3 * k + 2])) s.push_back(double(xyz[3 * k + size_t(c)]));
            if (s.empty()) { std::cerr << "dense mesh: no points to place a grid around" << std::endl; return false; }
            std::sort(s.begin(), s.end());
            const double n1 = double(s.size() - 1);
            lo[c] = s[size_t(std::floor(0.01 * n1))]; hi[c] = s[size_t(std::ceil(0.99 * n1))];
        }
        const double trunc_voxels = 4.0, max_voxels = 16777216.0, max_dim = 1024.0;
        double dims[3];
        auto dims_of = [&](double hh) {
            for (int c = 0; c < 3; ++c) dims[c] = std::max(std::ceil((hi[c] - lo[c] + 2.0 * trunc_voxels * hh) / hh) + 1.0, 2.0);
        };
        for (;;) {
            dims_of(h);
            const double top = std::max({dims[0], dims[1], dims[2]}), prod = dims[0] * dims[1] * dims[2];
            if (top <= max_dim && prod <= max_voxels) break;
            h *= std::max({top / max_dim, std::cbrt(prod / max_voxels), 1.0}) * 1.001;
        }
        h = double(float(h));
        dims_of(h);
        esfm_tsdf_grid grid;
        for (int c = 0; c < 3; ++c) {
            dims[c] = std::min(dims[c], max_dim);
            grid.dims[c] = int32_t(dims[c]);
            grid.origin[c] = float((lo[c] + hi[c]) / 2 - dims[c] * h / 2);
        }
        grid.voxel_size = float(h);
        esfm_tsdf_options topt;
        esfm_tsdf_options_default(&topt);
        topt.trunc = float(trunc_voxels) * grid.voxel_size;
        int32_t cap_v = 1 << 18, cap_t = 1 << 19, nv = 0, nt = 0;
        std::vector<float> vtx, nrm;
        std::vector<uint8_t> col;
        for (int attempt = 0; attempt < 2; ++attempt) {         // a guess, then the counts the first call reported
            vtx.assign(size_t(3) * size_t(cap_v), 0.f); nrm.assign(size_t(3) * size_t(cap_v), 0.f); col.assign(size_t(3) * size_t(cap_v), 0);
            mesh.triangles.assign(size_t(3) * size_t(cap_t), 0);
            nv = nt = -1;
            const int rc = esfm_mvs_mesh(default_ctx(), n, rows, cols, ch, images.data(), K4.data(), poses.data(), masked.data(), &grid, &topt, cap_v,
                                         cap_t, vtx.data(), nrm.data(), col.data(), mesh.triangles.data(), &nv, &nt);
            if (rc == ESFM_OK) break;
            if (attempt == 0 && rc == ESFM_ERR_INVALID_ARG && (nv > cap_v || nt > cap_t)) { cap_v = std::max(nv, 1); cap_t = std::max(nt, 1); continue; }
            std::cerr << esfm_last_error() << std::endl;
            return false;
        }
        mesh.triangles.resize(size_t(3) * size_t(nt));
        mesh.vertices.resize(size_t(nv));
        for (size_t k = 0; k < mesh.vertices.size(); ++k) {
            PointXYZRGBNormal &p = mesh.vertices[k];
            p.x = vtx[3 * k]; p.y = vtx[3 * k + 1]; p.z = vtx[3 * k + 2];
            p.nx = nrm[3 * k]; p.ny = nrm[3 * k + 1]; p.nz = nrm[3 * k + 2];
            p.r = col[3 * k]; p.g = col[3 * k + 1]; p.b = col[3 * k + 2];
        }
        mesh.voxel_size = grid.voxel_size;
        for (int c = 0; c < 3; ++c) { mesh.dims[c] = grid.dims[c]; mesh.origin[c] = grid.origin[c]; }
        return true;
    }

    bool run(const std::vector<frame_t> &frames, const std::vector<bool> &process_frame_id, const pointcloud_sparse_t &cloud,
             std::vector<PointXYZRGB> &dense, int &n_depth_maps, std::vector<PointXYZRGBNormal> *merged, TriangleMesh *mesh)
    {
        dense.clear();
        if (merged) merged->clear();
        if (mesh) *mesh = TriangleMesh();
        n_depth_maps = 0;
        const int n = int(frames.size());
        esfm_mvs_options opt;
        esfm_mvs_options_default(&opt);
        int rows = -1, cols = -1, ch = -1;
        for (int v = 0; v < n; ++v) {
            if (process_frame_id[size_t(v)]) continue;
            const ImageMat &im = frames[size_t(v)].rgb_image;
            if (im.empty()) { std::cerr << "dense reconstruction: registered frame " << v << " has no image" << std::endl; return false; }
            if (rows < 0) { rows = im.rows; cols = im.cols; ch = im.channels; }
            if (im.rows != rows || im.cols != cols || im.channels != ch) { std::cerr << "dense reconstruction: frames differ in size" << std::endl; return false; }
        }
        if (rows < 0) return true;
        const size_t plane = size_t(rows) * size_t(cols) * size_t(ch);
        std::vector<uint8_t> images(plane * size_t(n), 0), registered(size_t(n), 0);
        std::vector<float> K4(size_t(4) * n), poses(size_t(12) * n), xyz(size_t(3) * cloud.points.size());
        std::unordered_map<int, int> point_of;
        for (size_t k = 0; k < cloud.points.size(); ++k) {
            xyz[3 * k] = cloud.points[k].x; xyz[3 * k + 1] = cloud.points[k].y; xyz[3 * k + 2] = cloud.points[k].z;
            point_of.emplace(cloud.unique_point_ids[k], int(k));
        }
        std::vector<int32_t> obs_off(size_t(n) + 1, 0), obs_pts;
        for (int v = 0; v < n; ++v) {
            const frame_t &f = frames[size_t(v)];
            registered[size_t(v)] = process_frame_id[size_t(v)] ? 0 : 1;
            if (registered[size_t(v)]) std::copy(f.rgb_image.data.begin(), f.rgb_image.data.end(), images.begin() + plane * size_t(v));
            const float k4[4] = {f.K_cam(0, 0), f.K_cam(0, 2), f.K_cam(1, 1), f.K_cam(1, 2)};
            std::copy(k4, k4 + 4, &K4[size_t(4) * v]);
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) poses[size_t(12) * v + 4 * i + j] = f.pose_cam(i, j);
            // the cloud points whose track id is among the frame's ids, in cloud order
            std::vector<char> seen(cloud.points.size(), 0);
            for (int id : f.unique_pixel_ids) {
                auto it = point_of.find(id);
                if (it != point_of.end()) seen[size_t(it->second)] = 1;
            }
            for (size_t k = 0; k < seen.size(); ++k) if (seen[k]) obs_pts.push_back(int32_t(k));
            obs_off[size_t(v) + 1] = int32_t(obs_pts.size());
        }
        std::vector<int32_t> nb(size_t(n) * opt.max_neighbours);
        std::vector<float> range(size_t(2) * n);
        int rc = esfm_mvs_plan(n, registered.data(), poses.data(), int(cloud.points.size()), xyz.data(), obs_off.data(), obs_pts.data(), &opt,
                               nb.data(), range.data());
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        for (int v = 0; v < n; ++v) n_depth_maps += range[size_t(2) * v] > 0.f;
        const size_t n_px = size_t(n) * rows * cols;
        std::vector<float> depth(n_px), cost(n_px), out_xyz(3 * n_px);
        std::vector<uint8_t> out_rgb(3 * n_px);
        rc = esfm_mvs_depth_maps(default_ctx(), n, rows, cols, ch, images.data(), K4.data(), poses.data(), nb.data(), range.data(), &opt,
                                 depth.data(), cost.data());
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        int32_t n_points = 0;
        std::vector<int32_t> pixel(merged || mesh ? n_px : 0);
        rc = merged || mesh ? esfm_mvs_fuse_ex(default_ctx(), n, rows, cols, ch, images.data(), K4.data(), poses.data(), nb.data(), depth.data(), &opt,
                                               out_xyz.data(), out_rgb.data(), pixel.data(), &n_points)
                            : esfm_mvs_fuse(default_ctx(), n, rows, cols, ch, images.data(), K4.data(), poses.data(), nb.data(), depth.data(), &opt,
                                            out_xyz.data(), out_rgb.data(), &n_points);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        dense.resize(size_t(n_points));
        for (size_t k = 0; k < dense.size(); ++k) {
            PointXYZRGB &p = dense[k];
            p.x = out_xyz[3 * k]; p.y = out_xyz[3 * k + 1]; p.z = out_xyz[3 * k + 2];
            p.r = out_rgb[3 * k]; p.g = out_rgb[3 * k + 1]; p.b = out_rgb[3 * k + 2];
        }
        if (n_points == 0) return true;
        if (mesh && !mesh_of(n, rows, cols, ch, images, K4, poses, depth, pixel, size_t(n_points), out_xyz, *mesh)) return false;
        if (!merged) return true;

        // normals of every depth map, gathered by each point's pixel; the view as tag; footprints for the voxel size
        const size_t N = size_t(n_points);
        std::vector<float> normal_maps(3 * n_px), normals(3 * N), foot(N);
        std::vector<int32_t> tags(N);
        esfm_mvs_normal_options nopt;
        esfm_mvs_normal_options_default(&nopt);
        rc = esfm_mvs_normals(default_ctx(), n, rows, cols, K4.data(), poses.data(), depth.data(), &nopt, normal_maps.data());
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        const size_t view_px = size_t(rows) * size_t(cols);
        for (size_t k = 0; k < N; ++k) {
            const size_t px = size_t(pixel[k]);
            for (int c = 0; c < 3; ++c) normals[3 * k + c] = normal_maps[3 * px + c];
            tags[k] = int32_t(px / view_px);
            foot[k] = depth[px] / K4[size_t(4) * size_t(tags[k])];
        }
        std::nth_element(foot.begin(), foot.begin() + (N - 1) / 2, foot.end());         // the lower median, sorted[(n - 1) / 2]
        const float h = 2.0f * foot[(N - 1) / 2];
        std::vector<float> m_xyz(3 * N), m_nrm(3 * N);
        std::vector<uint8_t> m_rgb(3 * N);
        std::vector<int32_t> m_cnt(N);
        std::vector<uint64_t> m_views(N);
        int32_t n_merged = 0;
        rc = esfm_cloud_voxel_merge(default_ctx(), n_points, out_xyz.data(), out_rgb.data(), normals.data(), tags.data(), h, /*min_points*/ 1, /*min_tags*/ 2,
                                    m_xyz.data(), m_rgb.data(), m_nrm.data(), m_cnt.data(), m_views.data(), &n_merged);
        if (rc != ESFM_OK) { std::cerr << esfm_last_error() << std::endl; return false; }
        merged->resize(size_t(n_merged));
        for (size_t k = 0; k < merged->size(); ++k) {
            PointXYZRGBNormal &p = (*merged)[k];
            p.x = m_xyz[3 * k]; p.y = m_xyz[3 * k + 1]; p.z = m_xyz[3 * k + 2];
            p.nx = m_nrm[3 * k]; p.ny = m_nrm[3 * k + 1]; p.nz = m_nrm[3 * k + 2];
            p.r = m_rgb[3 * k]; p.g = m_rgb[3 * k + 1]; p.b = m_rgb[3 * k + 2];
            p.members = m_cnt[k]; p.views = m_views[k];
        }
        return true;
    }
};

}  // namespace p3dv
