// ./bin/sfm_native -- the reference executable's command line (cpp_code/test/sfm.cpp:32-50, cpp_code/script/run_fountain_small.sh:22-24)
// as a native C++ program over the C ABI of libesfm_hip.so, through the host mirror of the reference's classes
// (esfm_host.hpp).  Same thirteen positional arguments in the same order (an optional fourteenth picks the match filter: ratio,
// the reference's and the default; cross; ratio+cross), same ASCII .ply of PointXYZRGB at argv[5], exit
// status 1 on success like the reference (sfm.cpp:339).  The control flow is the one of
// easysfm_amd/pipeline.py (the Python twin of this file); the (i, j < i) pair loop of sfm.cpp:140-170 is ONE batched call per stage
// (every frame's descriptors uploaded once, one match launch sequence, one RANSAC / pose / depth batch -- INTEGRATION.md section 2;
// ESFM_PAIR_BY_PAIR=1 in the environment runs it pair by pair through host pointers as the reference does, same results):
//   import -> undistort -> SURF or ORB -> all-pairs match + 5-point RANSAC + depth -> track ids -> initial pair -> triangulate -> BA
//   -> (next frame by PnP -> triangulate against every registered frame -> periodic BA)* -> final BA -> SOR -> .ply
// Differences from the reference: ORB's intensity tests use this library's own point pairs (cv::ORB's learned table ships only
// inside OpenCV); the viewer arguments are accepted and ignored (no display); PNG and baseline JPEG images are read.
//   bin/sfm_native --dump-image in.png out.raw   writes rows, cols (int32) and the BGR bytes: the decoder's test hook
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <atomic>
#include <string>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "esfm_host.hpp"

using namespace p3dv;

namespace {

struct frame_pair_t {  // utility.h:57-78
    std::vector<DMatch> matches;
    Matrix4f T_21 = Matrix4f::Identity();
    double appro_depth = 1.0;
    int h_inliers = 0;              // correspondences within the threshold of the returned, re-fitted homography (esfm_find_homography_pairs'
                                    // n_inliers, not the RANSAC mask's count); find_init_frames = 2 only
    double h_inlier_ratio = 0.0;    // ... divided by the essential matrix's RANSAC mask count
};

Matrix4f mul(const Matrix4f &a, const Matrix4f &b)
{
    Matrix4f c;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) s += a(i, k) * b(k, j);
            c(i, j) = s;
        }
    return c;
}

// wall-clock of the stages the reference times with its `... cost = ... seconds` lines (feature_matching.cpp:141, ba.cpp:285), one
// summary line at the end (`stage seconds: ...`) for bench.py's config-1 / config-3 legs
struct StageClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap()
    {
        const auto t1 = std::chrono::steady_clock::now();
        const double s = std::chrono::duration<double>(t1 - t0).count();
        t0 = t1;
        return s;
    }
};

int dump_image(const char *in, const char *out)
{
    int rows = 0, cols = 0;
    std::vector<uint8_t> bgr;
    const std::string err = read_image_bgr(in, rows, cols, bgr);
    if (!err.empty()) { std::cerr << err << std::endl; return 3; }
    std::ofstream f(out, std::ios::binary);
    const int32_t hdr[2] = {rows, cols};
    f.write(reinterpret_cast<const char *>(hdr), sizeof(hdr));
    f.write(reinterpret_cast<const char *>(bgr.data()), std::streamsize(bgr.size()));
    return f ? 0 : 3;
}

// the re-render of the written mesh into the registered frames and its "Mesh render:" line (bin/sfm prints the same form)
bool render_mesh(DenseReconstruction &dr, const TriangleMesh &mesh, const std::vector<frame_t> &frames, const std::vector<bool> &todo,
                 const std::vector<float> *uv, int atlas_rows, int atlas_cols, const std::vector<uint8_t> *atlas, const std::string &dir)
{
    int n_views = 0;
    long long covered = 0, sum_abs = 0;
    if (!dr.renderMesh(mesh, frames, todo, uv, atlas_rows, atlas_cols, atlas, dir, n_views, covered, sum_abs)) return false;
    char mean[64];
    std::snprintf(mean, sizeof(mean), "%.3f", covered ? double(sum_abs) / (3.0 * double(covered)) : 0.0);
    std::cout << "Mesh render: [" << n_views << "] views, [" << covered << "] covered pixels, mean absolute error [" << mean << "]" << std::endl;
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 4 && std::string(argv[1]) == "--dump-image") return dump_image(argv[2], argv[3]);
    // optional 14th argument: the match filter -- ratio (the reference's, default), cross (mutual nearest neighbours) or ratio+cross,
    // or one of these with +guided appended (a second, epipolar-guided pass over the verified pairs; the union is kept); +tracks behind
    // any of them (ratio+tracks, ratio+guided+tracks) re-triangulates the cloud's tracks before every bundle adjustment and filters
    // them after the last (esfm.h "Track triangulation", default options; one "Track refine:" line per call);
    // optional 15th (needs the 14th): a dense .ply path, or none; optional 16th (needs the 15th): a .ply path for the merged dense cloud
    // (one oriented point per voxel), or none; optional 17th (needs the 16th): a .ply path for the surface mesh, or none; clean:mesh.ply
    // cleans the mesh with the defaults of esfm.h "Mesh clean-up" before it is written to mesh.ply, simplify:mesh.ply merges the
    // vertices of every cell of two voxels' side (esfm.h "Mesh simplification"), clean+simplify:mesh.ply does both in that order; with
    // +texture in the prefix (texture:, clean+texture:, simplify+texture:, clean+simplify+texture:) the mesh is then textured from the
    // registered frames (esfm.h "Mesh texturing") and written with texture coordinates, its atlas beside it as mesh.png; +level behind
    // +texture (e.g. clean+simplify+texture+level:mesh.ply) levels the seams between the frames first, +level without +texture is an error;
    // optional 18th (needs a mesh as the 17th): an existing directory, or none: the mesh is drawn into every registered frame (esfm.h "Mesh
    // rendering"; with the atlas if it was textured, else with its vertex colours), the pictures go there as render_%04d.png and one
    // "Mesh render:" line states their mean absolute error against the photographs
    std::string filter_arg = argc >= 15 ? argv[14] : "ratio";
    // +cameras as the final token, behind everything else (ratio+cameras, ratio+guided+tracks+retrieval4+cameras): multiple-camera mode.
    // calib_K_file then holds 9 G numbers (G row-major matrices) and one camera index per image, calib_distort_file none, 4 or 4 G
    // numbers; one "Cameras:" line; the pair stage runs in camera 0's pixels (CanonicalPairView: repro_dis_ransac is then in those
    // canonical pixels), free intrinsics free one block per camera; dense outputs need images of one size.  Stripped first.
    bool multi_camera = false;
    {
        const std::string token = "+cameras";
        if (filter_arg.size() > token.size() && filter_arg.compare(filter_arg.size() - token.size(), token.size(), token) == 0) {
            multi_camera = true;
            filter_arg.erase(filter_arg.size() - token.size());
        }
    }
    // +radial (free radial distortion k1, k2 per camera in every bundle adjustment; at the end of the filter, in front of +cameras):
    // bin/sfm's mode, not provided by this driver -- refused, not ignored
    {
        const std::string token = "+radial";
        if (filter_arg.size() > token.size() && filter_arg.compare(filter_arg.size() - token.size(), token.size(), token) == 0) {
            fprintf(stderr, "sfm_native: +radial (free radial distortion) is not provided by this driver; use bin/sfm\n");
            return 2;
        }
    }
    // calib_K_file auto (the focal length estimated from the pairs' fundamental matrices, esfm.h "Fundamental-matrix RANSAC"): bin/sfm's
    // mode, not provided by this driver -- refused, not read as a file name
    if (argc >= 4 && std::string(argv[3]) == "auto") {
        fprintf(stderr, "sfm_native: calib_K_file auto (focal length from the image pairs) is not provided by this driver; use bin/sfm\n");
        return 2;
    }
    // +retrieval or +retrievalK (K decimal, 1 .. 999) at the very end, behind everything else (ratio+retrieval, ratio+guided+tracks+retrieval4):
    // only the pairs that image retrieval selects are matched (esfm.h "Image retrieval", default options, K = top_k; one "Pair selection:" line)
    bool retrieval = false;
    int retrieval_top_k = 0;                                 // 0: the default
    {
        const std::string token = "+retrieval";
        const size_t at = filter_arg.rfind(token);
        if (at != std::string::npos && at > 0) {
            const std::string k = filter_arg.substr(at + token.size());
            bool well_formed = k.size() <= 3 && (k.empty() || k[0] != '0');
            for (char c : k) well_formed = well_formed && c >= '0' && c <= '9';
            if (well_formed) { retrieval = true; retrieval_top_k = k.empty() ? 0 : std::atoi(k.c_str()); filter_arg.erase(at); }
        }
    }
    const std::string tracks_suffix = "+tracks";
    const bool refine_tracks = filter_arg.size() > tracks_suffix.size() && filter_arg.compare(filter_arg.size() - tracks_suffix.size(), tracks_suffix.size(), tracks_suffix) == 0;
    if (refine_tracks) filter_arg.erase(filter_arg.size() - tracks_suffix.size());
    // +complete (track completion, esfm.h "Track completion"; directly in front of +tracks' position): bin/sfm's mode, not provided by
    // this driver -- refused, not ignored
    {
        const std::string token = "+complete";
        if (filter_arg.size() > token.size() && filter_arg.compare(filter_arg.size() - token.size(), token.size(), token) == 0) {
            fprintf(stderr, "sfm_native: +complete (track completion) is not provided by this driver; use bin/sfm\n");
            return 2;
        }
    }
    const std::string guided_suffix = "+guided";
    const bool guided = filter_arg.size() > guided_suffix.size() && filter_arg.compare(filter_arg.size() - guided_suffix.size(), guided_suffix.size(), guided_suffix) == 0;
    const std::string match_filter = guided ? filter_arg.substr(0, filter_arg.size() - guided_suffix.size()) : filter_arg;      // the first pass's filter
    const std::string dense_file = argc >= 16 && std::string(argv[15]) != "none" ? argv[15] : "";
    const std::string merged_file = argc >= 17 && std::string(argv[16]) != "none" ? argv[16] : "";
    const std::string mesh_arg = argc >= 18 && std::string(argv[17]) != "none" ? argv[17] : "";
    const std::string render_dir = argc == 19 && std::string(argv[18]) != "none" ? argv[18] : "";
    const bool render_alone = !render_dir.empty() && (mesh_arg.empty() || !std::filesystem::is_directory(render_dir));
    bool clean_mesh = false, simplify_mesh = false, texture_mesh = false, level_mesh = false, level_alone = mesh_arg.compare(0, 6, "level:") == 0;
    std::string mesh_file = mesh_arg;
    {
        struct Form { const char *prefix; bool clean, simplify, texture; };
        const Form forms[] = {{"clean+simplify+texture:", true, true, true}, {"clean+texture:", true, false, true}, {"simplify+texture:", false, true, true},
                              {"texture:", false, false, true}, {"clean+simplify:", true, true, false}, {"clean:", true, false, false},
                              {"simplify:", false, true, false}};
        for (const Form &f : forms) {
            const size_t len = std::strlen(f.prefix);
            const std::string levelled = std::string(f.prefix, len - 1) + "+level:";
            if (mesh_arg.compare(0, levelled.size(), levelled) == 0) {
                clean_mesh = f.clean; simplify_mesh = f.simplify; texture_mesh = f.texture;
                level_mesh = f.texture; level_alone = !f.texture;
                mesh_file = mesh_arg.substr(levelled.size());
                break;
            }
            if (mesh_arg.compare(0, len, f.prefix) == 0) {
                clean_mesh = f.clean; simplify_mesh = f.simplify; texture_mesh = f.texture;
                mesh_file = mesh_arg.substr(len);
                break;
            }
        }
    }
    if (argc < 14 || argc > 19 || (match_filter != "ratio" && match_filter != "cross" && match_filter != "ratio+cross") || level_alone || render_alone) {
        std::cerr << "usage: sfm_native image_folder image_list calib_K_file calib_distort_file output.ply feature_type(S | O | I) feature_parameter "
                     "repro_dis_ransac find_init_frames(0 | 1 | 2: as 1, and no planar or rotation-only initial pair) ba_calib_change_tolerance ba_frequency launch_viewer view_sphere [match_filter: ratio | cross | ratio+cross | "
                     "ratio+guided | cross+guided | ratio+cross+guided, each also with +tracks appended, and +retrieval or +retrievalK (K = 1 .. 999 nearest images) at the very end [dense.ply | none [merged.ply | none [simplify:mesh.ply | "
                     "clean+simplify:mesh.ply | mesh.ply | clean:mesh.ply | none [render_dir | none]]]]] (the 17th's prefix also takes +texture: texture:, clean+texture:, "
                     "simplify+texture:, clean+simplify+texture:) (and +level behind +texture: texture+level:, clean+texture+level:, simplify+texture+level:, "
                     "clean+simplify+texture+level:) (render_dir, the 18th: an existing directory for render_%04d.png, one re-render of the mesh per "
                     "registered frame; it needs a mesh)"
                  << std::endl;
        return 2;
    }
    const bool cross_check = match_filter != "ratio";
    const std::string image_data_path = argv[1], image_list_path = argv[2], calib_file_path = argv[3], distort_file_path = argv[4],
                      output_file_path = argv[5];
    char using_feature = argv[6][0];
    const int feature_extract_parameter = std::atoi(argv[7]);
    const double ransac_reproj_distance = std::atof(argv[8]);
    const bool use_track_frames_as_init = std::atoi(argv[9]) != 0;
    const bool init_h_check = std::atoi(argv[9]) == 2;              // 2: the initial pair must not be planar or rotation-only
    const double init_max_h_inlier_ratio = 0.8;
    const double fix_calib_tolerance_BA = std::atof(argv[10]);
    const int frequency_BA = std::max(1, std::atoi(argv[11]));
    if (using_feature != 'S' && using_feature != 'O' && using_feature != 'I') { std::cout << "Wrong feature input. Use SURF as default feature." << std::endl; using_feature = 'S'; }

    try {
        DataIO io;
        FeatureMatching fm;
        MotionEstimator ee;
        std::vector<frame_t> frames;
        double t_import = 0, t_detect = 0, t_match = 0, t_verify = 0, t_tracks = 0, t_ba = 0, t_register = 0, t_sor = 0, t_pnp = 0, t_next = 0;
        int n_ba = 0;
        StageClock total_clock, clk;
        if (!io.importImageFilenames(image_list_path, image_data_path, frames) || frames.size() < 2) { std::cerr << "need at least two images" << std::endl; return 3; }
        const int frame_number = int(frames.size());
        Matrix3f K_mat = Matrix3f::Identity();
        DistortMat distort_coeff;
        std::vector<Matrix3f> K_all;
        std::vector<DistortMat> distort_all;
        std::vector<int> camera_of_image;
        if (multi_camera) {
            std::string error;
            bool imported = false;
            if (!DataIO::importCameras(calib_file_path, frame_number, K_all, camera_of_image, error) ||
                !DataIO::importCameraDistort(distort_file_path, int(K_all.size()), distort_all, imported, error)) { std::cerr << error << std::endl; return 3; }
            std::vector<int> counts(K_all.size(), 0);
            for (int c : camera_of_image) ++counts[size_t(c)];
            std::cout << "Cameras: " << K_all.size() << " models, ";
            for (size_t g = 0; g < counts.size(); ++g) std::cout << (g ? " / " : "") << counts[g];
            std::cout << " images" << std::endl;
            std::cout << (imported ? "Import camera distortion coefficients file done." : "No distortion coefficients imported. Use defualt one (0).") << std::endl;
        } else {
            if (!io.importCalib(calib_file_path, K_mat)) { std::cerr << "cannot read the calibration file " << calib_file_path << std::endl; return 3; }
            if (!io.importDistort(distort_file_path, distort_coeff)) std::cout << "No distortion coefficients imported. Use defualt one (0)." << std::endl;
        }

        // The image files are decoded by a few host threads running ahead of the loop below (a 768 x 512 PNG is ~10 ms of inflate; the
        // first frame's import otherwise also waits for the GPU's first-touch initialisation): frame i is taken when its decode is done,
        // messages and failures appear where the reference's sequential loop has them.
        std::vector<std::string> decode_err((size_t)frame_number);
        std::vector<char> decoded((size_t)frame_number, 0);
        std::mutex decode_mu;
        std::condition_variable decode_cv;
        std::atomic<int> next_decode{0};
        std::vector<std::thread> decoders;
        {
            const int n_thr = std::max(1, std::min<int>({frame_number, 8, (int)std::thread::hardware_concurrency()}));
            for (int w = 0; w < n_thr; ++w)
                decoders.emplace_back([&] {
                    for (int i = next_decode++; i < frame_number; i = next_decode++) {
                        ImageMat &img = frames[size_t(i)].rgb_image;
                        img.channels = 3;
                        std::string err;
                        // a malformed or huge header must end as this frame's "No more images", not as std::terminate in a worker
                        try { err = read_image_bgr(frames[size_t(i)].image_file_path, img.rows, img.cols, img.data); }
                        catch (const std::exception &e) { err = std::string("decoder failed: ") + e.what(); }
                        catch (...) { err = "decoder failed"; }
                        {
                            std::lock_guard<std::mutex> lk(decode_mu);
                            decode_err[size_t(i)] = err;
                            decoded[size_t(i)] = 1;
                        }
                        decode_cv.notify_all();
                    }
                });
        }
        struct Joiner { std::vector<std::thread> &t; ~Joiner() { for (auto &x : t) if (x.joinable()) x.join(); } } joiner{decoders};
        auto import_decoded = [&](int i) {
            {
                std::unique_lock<std::mutex> lk(decode_mu);
                decode_cv.wait(lk, [&] { return decoded[size_t(i)] != 0; });
            }
            if (!decode_err[size_t(i)].empty()) {          // (DataIO::importImages' message)
                frames[size_t(i)].rgb_image = ImageMat();
                std::cout << "No more images" << " (" << decode_err[size_t(i)] << ")" << std::endl;
                return false;
            }
            return true;
        };

        // dense outputs take one image size for all views: checked on the decoded images before any other work
        if (!dense_file.empty() || !merged_file.empty() || !mesh_file.empty())
            for (int i = 0; i < frame_number; ++i) {
                if (!import_decoded(i)) return 3;
                const ImageMat &a = frames[0].rgb_image, &b = frames[size_t(i)].rgb_image;
                if (a.rows != b.rows || a.cols != b.cols) {
                    std::cerr << "dense outputs need images of one size; this run has " << a.rows << " x " << a.cols << " and " << b.rows << " x " << b.cols << std::endl;
                    return 3;
                }
            }

        // ---- per frame: import, undistort, SURF (sfm.cpp:84-126)
        std::cout << "Begin feature extraction" << std::endl;
        const bool frame_trace = std::getenv("ESFM_FRAME_TRACE") != nullptr;       // per-frame milliseconds on stderr (diagnosis of first-touch costs)
        for (int i = 0; i < frame_number; ++i) {
            clk.lap();
            if (!import_decoded(i)) return 3;
            const double t_wait = clk.lap();
            if (multi_camera) {
                frames[size_t(i)].camera_id = camera_of_image[size_t(i)];
                K_mat = K_all[size_t(camera_of_image[size_t(i)])];
                distort_coeff = distort_all[size_t(camera_of_image[size_t(i)])];
            }
            frames[size_t(i)].K_cam = K_mat;
            if (!ee.doUnDistort(frames[size_t(i)], distort_coeff)) return 3;
            const double t_und = clk.lap();
            t_import += t_wait + t_und;
            std::cout << "Feature extraction of Frame [ " << i << " ]" << std::endl;
            if (using_feature == 'O' ? !fm.detectFeaturesORB(frames[size_t(i)], feature_extract_parameter)          // sfm.cpp:112-117
                : using_feature == 'I' ? !fm.detectFeaturesSIFT(frames[size_t(i)], feature_extract_parameter)    // SIFT: the parameter is nfeatures
                                     : !fm.detectFeaturesSURF(frames[size_t(i)], feature_extract_parameter)) return 3;
            frames[size_t(i)].init_pixel_ids();
            const double t_det = clk.lap();
            t_detect += t_det;
            if (frame_trace)
                std::cerr << "[frame " << i << "] decode wait " << t_wait * 1e3 << " ms, undistort " << t_und * 1e3 << " ms, detect " << t_det * 1e3 << " ms" << std::endl;
        }
        std::cout << "Feature extraction done" << std::endl;

        // ---- all pairs (i, j < i): match, verify, relative depth (sfm.cpp:140-167)
        // (frames that do not all share one K_cam: in the canonical camera's pixels and with its K until the pair stage is done)
        auto pair_view = std::make_unique<CanonicalPairView>(frames);
        const int num_min_pair = 20;
        const size_t nf = size_t(frame_number);
        std::vector<std::vector<frame_pair_t>> graph(nf, std::vector<frame_pair_t>(nf));
        const double guided_ratio = match_filter == "cross" ? 0.0 : using_feature == 'O' ? 0.8 : using_feature == 'I' ? 0.7 : 0.5;
        const bool pair_by_pair = std::getenv("ESFM_PAIR_BY_PAIR") != nullptr && std::atoi(std::getenv("ESFM_PAIR_BY_PAIR")) != 0;
        // the pairs to match: every (i, j < i), or those image retrieval selects, in the same order
        std::vector<std::pair<int, int>> pairs;
        if (retrieval) {
            esfm_retrieval_options ro;
            esfm_retrieval_options_default(&ro);
            if (retrieval_top_k > 0) ro.top_k = retrieval_top_k;
            StageClock sc;
            if (!fm.selectPairs(frames, using_feature == 'O', ro, pairs)) return 3;
            t_match += sc.lap();
        } else
            for (int i = 0; i < frame_number; ++i) for (int j = 0; j < i; ++j) pairs.emplace_back(i, j);
        if (pair_by_pair) {
            for (const std::pair<int, int> &chosen : pairs) {
                {
                    const int i = chosen.first, j = chosen.second;
                    frame_pair_t &g = graph[size_t(i)][size_t(j)];
                    std::vector<DMatch> temp_matches, inlier_matches;
                    StageClock pc;
                    if (using_feature == 'O') fm.matchFeaturesORB(frames[size_t(i)], frames[size_t(j)], temp_matches, match_filter == "cross" ? 0.0 : 0.8, false, cross_check);   // sfm.cpp:153-160
                    else if (using_feature == 'I') fm.matchFeaturesSIFT(frames[size_t(i)], frames[size_t(j)], temp_matches, match_filter == "cross" ? 0.0 : 0.7, false, cross_check);
                    else fm.matchFeaturesSURF(frames[size_t(i)], frames[size_t(j)], temp_matches, match_filter == "cross" ? 0.0 : 0.5, false, cross_check);
                    t_match += pc.lap();
                    if (int(temp_matches.size()) > num_min_pair) {
                        Matrix4f T = Matrix4f::Identity();
                        double E[9];
                        if (ee.estimate2D2D_E5P_RANSAC(frames[size_t(i)], frames[size_t(j)], temp_matches, inlier_matches, T, ransac_reproj_distance, 0.99, false, E)) {
                            g.T_21 = T;
                            if (init_h_check) {  // the same correspondences under the homography model
                                std::vector<DMatch> h_matches;
                                int h_count = 0;
                                if (ee.estimate2D2D_H4P_RANSAC(frames[size_t(i)], frames[size_t(j)], temp_matches, h_matches, nullptr, ransac_reproj_distance, 0.995, &h_count)) g.h_inliers = h_count;
                                g.h_inlier_ratio = inlier_matches.empty() ? 0.0 : double(g.h_inliers) / double(inlier_matches.size());
                            }
                            double depth = 1.0;
                            if (ee.getDepthFast(frames[size_t(i)], frames[size_t(j)], T, inlier_matches, depth)) g.appro_depth = depth;
                            if (guided) {        // second pass along the epipolar lines, same filter; T_21 and the depth stay the first pass's
                                std::vector<DMatch> guided_matches;
                                if (!fm.matchFeaturesGuided(frames[size_t(i)], frames[size_t(j)], using_feature == 'O', E, ransac_reproj_distance, guided_matches,
                                                            guided_ratio, cross_check)) return 3;
                                FeatureMatching::mergeGuided(inlier_matches, guided_matches);
                            }
                            g.matches.swap(inlier_matches);
                            if (!g.matches.empty()) std::cout << "Pair ( " << i << " , " << j << " ): [" << g.matches.size() << "] verified matches." << std::endl;
                        }
                    }
                    t_verify += pc.lap();
                }
            }
        } else {
            // the same loop, batched: one match call for the whole (i, j < i) list, one RANSAC + pose + depth batch for the pairs with
            // more than num_min_pair matches (none of them depends on another pair's result)
            StageClock pc;
            std::vector<std::vector<DMatch>> temp_matches;
            const double ratio_thre = match_filter == "cross" ? 0.0 : using_feature == 'I' ? 0.7 : -1.0;        // -1: the S / O members' defaults
            if (!fm.matchFeaturesAllPairs(frames, pairs, using_feature == 'O', temp_matches, ratio_thre, cross_check)) return 3;
            t_match += pc.lap();
            std::vector<std::pair<int, int>> jobs;
            std::vector<std::vector<DMatch>> job_matches;
            for (size_t p = 0; p < pairs.size(); ++p)
                if (int(temp_matches[p].size()) > num_min_pair) { jobs.push_back(pairs[p]); job_matches.push_back(std::move(temp_matches[p])); }
            std::vector<std::vector<DMatch>> inliers;
            std::vector<Matrix4f> Ts;
            std::vector<double> depths;
            std::vector<char> ok;
            std::vector<double> Es;
            if (!ee.estimate2D2D_E5P_RANSAC_pairs(frames, jobs, job_matches, inliers, Ts, depths, ok, ransac_reproj_distance, 0.99, 20, &Es)) {
                // A batch entry point fails as a whole when ONE pair is unusable (a non-finite essential matrix, say); the reference's
                // loop -- and ESFM_PAIR_BY_PAIR=1 above -- only loses that pair (estimate_motion.cpp:27-97 returns false, sfm.cpp:165
                // carries on).  Same here: the batch's pairs are verified one by one, a failing pair is skipped.
                std::cout << "batched verification failed (" << esfm_last_error() << "): verifying pair by pair" << std::endl;
                inliers.assign(jobs.size(), {}); Ts.assign(jobs.size(), Matrix4f::Identity()); depths.assign(jobs.size(), 1.0); ok.assign(jobs.size(), 0);
                Es.assign(9 * jobs.size(), 0.0);
                for (size_t p = 0; p < jobs.size(); ++p) {
                    frame_t &fi = frames[size_t(jobs[p].first)], &fj = frames[size_t(jobs[p].second)];
                    Matrix4f T = Matrix4f::Identity();
                    if (!ee.estimate2D2D_E5P_RANSAC(fi, fj, job_matches[p], inliers[p], T, ransac_reproj_distance, 0.99, false, &Es[9 * p])) continue;
                    double depth = 1.0;
                    Ts[p] = T;
                    if (ee.getDepthFast(fi, fj, T, inliers[p], depth)) depths[p] = depth;
                    ok[p] = 1;
                }
            }
            if (init_h_check) {  // ONE homography batch over the same correspondences; the ratio is taken against the essential matrix's RANSAC inliers
                std::vector<int> h_inliers;
                if (!ee.estimate2D2D_H4P_RANSAC_pairs(frames, jobs, job_matches, h_inliers, ransac_reproj_distance)) return 3;
                for (size_t p = 0; p < jobs.size(); ++p) {
                    if (!ok[p]) continue;
                    frame_pair_t &g = graph[size_t(jobs[p].first)][size_t(jobs[p].second)];
                    g.h_inliers = h_inliers[p];
                    g.h_inlier_ratio = inliers[p].empty() ? 0.0 : double(h_inliers[p]) / double(inliers[p].size());
                }
            }
            if (guided) {       // ONE guided call for every pair with a model, the first pass's filter; each keeps the union
                std::vector<std::pair<int, int>> gjobs;
                std::vector<double> gE;
                std::vector<size_t> gidx;
                for (size_t p = 0; p < jobs.size(); ++p)
                    if (ok[p]) { gjobs.push_back(jobs[p]); gE.insert(gE.end(), Es.begin() + 9 * long(p), Es.begin() + 9 * long(p) + 9); gidx.push_back(p); }
                std::vector<std::vector<DMatch>> guided_matches;
                if (!fm.matchFeaturesGuidedAllPairs(frames, gjobs, using_feature == 'O', gE, ransac_reproj_distance, guided_matches, guided_ratio, cross_check)) return 3;
                for (size_t s = 0; s < gidx.size(); ++s) FeatureMatching::mergeGuided(inliers[gidx[s]], guided_matches[s]);
            }
            for (size_t p = 0; p < jobs.size(); ++p) {
                if (!ok[p]) continue;
                frame_pair_t &g = graph[size_t(jobs[p].first)][size_t(jobs[p].second)];
                g.T_21 = Ts[p];
                g.appro_depth = depths[p];
                g.matches.swap(inliers[p]);
                if (!g.matches.empty()) std::cout << "Pair ( " << jobs[p].first << " , " << jobs[p].second << " ): [" << g.matches.size() << "] verified matches." << std::endl;
            }
            t_verify += pc.lap();
        }
        pair_view.reset();          // back to every frame's own pixels and K_cam

        // ---- track ids (sfm.cpp:173-216): a keypoint takes the id of its verified match in an earlier frame unless the frame
        // already uses that id; the rest get fresh ids
        clk.lap();
        size_t total_kp = 0;
        for (const frame_t &f : frames) total_kp += f.keypoints.size();
        std::vector<std::vector<bool>> track(nf, std::vector<bool>(std::max<size_t>(total_kp, 1), false));
        int cur_id = 0;
        std::vector<char> id_in_frame(std::max<size_t>(total_kp, 1), 0);     // which ids the current frame's keypoints hold (ids < total_kp)
        for (int i = 0; i < frame_number; ++i) {
            frame_t &fi = frames[size_t(i)];
            // the reference walks the frame's whole id list for every match ("is this id used already?", sfm.cpp:190-199):
            // O(matches x keypoints) per frame.  The same question from a flag per id that follows every assignment.
            std::vector<int> held;
            for (int j = 0; j < i; ++j) {
                const frame_t &fj = frames[size_t(j)];
                for (const DMatch &m : graph[size_t(i)][size_t(j)].matches) {
                    const int tid = fj.unique_pixel_ids[size_t(m.trainIdx)];
                    int &mine = fi.unique_pixel_ids[size_t(m.queryIdx)];
                    if (mine >= 0 && mine == tid) continue;
                    if (!id_in_frame[size_t(tid)]) {
                        if (mine >= 0) id_in_frame[size_t(mine)] = 0;      // (this keypoint was the only holder of its old id)
                        mine = tid; id_in_frame[size_t(tid)] = 1; held.push_back(tid);
                        fi.unique_pixel_has_match[size_t(m.queryIdx)] = true;
                    }
                }
            }
            for (int v : held) id_in_frame[size_t(v)] = 0;
            int fresh = 0;
            for (size_t k = 0; k < fi.unique_pixel_ids.size(); ++k) {
                if (fi.unique_pixel_ids[k] < 0) fi.unique_pixel_ids[k] = cur_id + fresh++;
                track[size_t(i)][size_t(fi.unique_pixel_ids[k])] = true;
            }
            cur_id += fresh;
        }
        std::cout << "The total unique feature point number is " << cur_id << std::endl;
        t_tracks += clk.lap();

        // ---- initial pair (sfm.cpp:218-247)
        int init_1 = 1, init_2 = 0;
        double depth_init = 10.0;
        if (use_track_frames_as_init) {
            std::vector<std::vector<double>> depth(nf, std::vector<double>(nf, 0.0));
            for (int i = 0; i < frame_number; ++i) for (int j = 0; j < i; ++j) depth[size_t(i)][size_t(j)] = graph[size_t(i)][size_t(j)].appro_depth;
            if (init_h_check) {
                std::vector<std::vector<double>> h_ratio(nf, std::vector<double>(nf, 0.0));
                for (int i = 0; i < frame_number; ++i) for (int j = 0; j < i; ++j) h_ratio[size_t(i)][size_t(j)] = graph[size_t(i)][size_t(j)].h_inlier_ratio;
                int h_candidates = 0, h_skipped = 0;
                fm.findInitializeFramePair(track, frames, depth, init_1, init_2, depth_init, 100, 50.0, init_max_h_inlier_ratio, &h_ratio, &h_candidates, &h_skipped);
                std::cout << "Init pair: skipped " << h_skipped << " of " << h_candidates << " candidate pairs as planar or panoramic" << std::endl;
            } else
                fm.findInitializeFramePair(track, frames, depth, init_1, init_2, depth_init);
        }
        std::cout << "Initialization frames: [ " << init_1 << " ] and [ " << init_2 << " ]" << std::endl;
        pointcloud_sparse_t cloud;
        frames[size_t(init_1)].pose_cam = Matrix4f::Identity();
        frames[size_t(init_2)].pose_cam = mul(graph[size_t(init_1)][size_t(init_2)].T_21, frames[size_t(init_1)].pose_cam);
        ee.doTriangulation(frames[size_t(init_1)], frames[size_t(init_2)], graph[size_t(init_1)][size_t(init_2)].matches, cloud);
        std::vector<bool> todo(nf, true);
        todo[size_t(init_1)] = todo[size_t(init_2)] = false;
        BundleAdjustment ba;
        esfm_track_options track_options;
        esfm_track_options_default(&track_options);
        if (refine_tracks && !ee.refineTracks(frames, todo, cloud, track_options)) return 3;
        t_register += clk.lap();
        ba.doSFMBA(frames, todo, cloud, fix_calib_tolerance_BA);
        t_ba += clk.lap(); ++n_ba;

        // ---- register the remaining frames (sfm.cpp:262-321)
        int remaining = frame_number - 2;
        double t_next_prev = 0;
        double reproj = ransac_reproj_distance;
        while (remaining > 0) {
            int nxt = -1;
            fm.findNextFrame(track, todo, cloud.unique_point_ids, nxt);
            if (nxt < 0) break;                      // no unregistered frame sees the map (the reference would index with an uninitialised value)
            t_next += clk.lap(); t_register += t_next - t_next_prev; t_next_prev = t_next;
            const bool ok = ee.estimate2D3D_P3P_RANSAC(frames[size_t(nxt)], cloud, reproj);
            { const double dt = clk.lap(); t_pnp += dt; t_register += dt; }
            reproj += 1.0;
            for (int i = 0; i < frame_number; ++i) {
                if (todo[size_t(i)]) continue;
                if (nxt > i) ee.doTriangulation(frames[size_t(nxt)], frames[size_t(i)], graph[size_t(nxt)][size_t(i)].matches, cloud);
                else ee.doTriangulation(frames[size_t(i)], frames[size_t(nxt)], graph[size_t(i)][size_t(nxt)].matches, cloud);
            }
            if (!ok) ee.outlierFilter(cloud);
            todo[size_t(nxt)] = false;
            --remaining;
            t_register += clk.lap();
            if (remaining % frequency_BA == 0) {
                ba.initBA();
                if (refine_tracks) { if (!ee.refineTracks(frames, todo, cloud, track_options)) return 3; t_register += clk.lap(); }
                ba.doSFMBA(frames, todo, cloud, fix_calib_tolerance_BA);
                reproj = ransac_reproj_distance;
                t_ba += clk.lap(); ++n_ba;
            }
            std::cout << "Progress: [ " << frame_number - remaining << " / " << frame_number << " ]" << std::endl;
        }
        if (refine_tracks && !ee.refineTracks(frames, todo, cloud, track_options)) return 3;
        clk.lap();
        ba.doSFMBA(frames, todo, cloud);
        t_ba += clk.lap(); ++n_ba;
        if (refine_tracks && !ee.refineTracks(frames, todo, cloud, track_options, true)) return 3;

        // ---- final cloud: SOR filter, .ply (sfm.cpp:329-337)
        std::vector<PointXYZRGB> filtered;
        CProceesing<PointXYZRGB> cp;
        if (!cp.SORFilter(cloud.points, filtered)) return 3;
        const std::filesystem::path out_dir = std::filesystem::path(output_file_path).parent_path();
        if (!out_dir.empty()) std::filesystem::create_directories(out_dir);
        t_sor += clk.lap();
        if (!io.writePlyFile(output_file_path, filtered)) return 3;
        std::cout << "stage seconds: import+undistort " << t_import << " detect " << t_detect << " match " << t_match << " verify " << t_verify << " tracks " << t_tracks
                  << " register " << t_register << " register_next_frame " << t_next << " register_pnp " << t_pnp << " ba " << t_ba << " ba_calls " << n_ba << " sor " << t_sor << " total " << total_clock.lap()
                  << " frames " << frame_number << " pairs " << frame_number * (frame_number - 1) / 2 << " batched " << (pair_by_pair ? 0 : 1) << std::endl;
        if (!dense_file.empty() || !merged_file.empty() || !mesh_file.empty()) {
            // dense reconstruction after the final BA, on the cloud before the filter (it carries the track ids)
            clk.lap();
            std::vector<PointXYZRGB> dense;
            std::vector<PointXYZRGBNormal> merged;
            int n_maps = 0;
            TriangleMesh mesh;
            DenseReconstruction dr;
            if (!(!mesh_file.empty()    ? dr.reconstructMesh(frames, todo, cloud, dense, n_maps, merged_file.empty() ? nullptr : &merged, mesh)
                  : merged_file.empty() ? dr.reconstruct(frames, todo, cloud, dense, n_maps)
                                        : dr.reconstructMerged(frames, todo, cloud, dense, n_maps, merged)))
                return 3;
            const double t_dense = clk.lap();
            if (!dense_file.empty()) {
                std::cout << "Dense reconstruction: [" << n_maps << "] depth maps, [" << dense.size() << "] points." << std::endl;
                const std::filesystem::path dense_dir = std::filesystem::path(dense_file).parent_path();
                if (!dense_dir.empty()) std::filesystem::create_directories(dense_dir);
                if (!io.writePlyFile(dense_file, dense)) return 3;
                std::cout << "dense seconds: reconstruct " << t_dense << " write " << clk.lap() << std::endl;
            }
            if (!merged_file.empty()) {
                size_t with_normal = 0;
                for (const PointXYZRGBNormal &p : merged) with_normal += p.nx != 0.f || p.ny != 0.f || p.nz != 0.f;
                std::cout << "Dense merge: [" << dense.size() << "] points into [" << merged.size() << "] voxels, [" << with_normal << "] with a normal." << std::endl;
                const std::filesystem::path merged_dir = std::filesystem::path(merged_file).parent_path();
                if (!merged_dir.empty()) std::filesystem::create_directories(merged_dir);
                if (!io.writePlyFileNormals(merged_file, merged)) return 3;
            }
            if (!mesh_file.empty()) {
                std::cout << "Dense mesh: [" << mesh.vertices.size() << "] vertices, [" << mesh.triangles.size() / 3 << "] triangles from [" << mesh.dims[0]
                          << "] x [" << mesh.dims[1] << "] x [" << mesh.dims[2] << "] voxels of [" << mesh.voxel_size << "]." << std::endl;
                if (clean_mesh) {
                    int n_before = 0, n_after = 0;
                    if (!dr.cleanMesh(mesh, &n_before, &n_after)) return 3;
                    std::cout << "Mesh clean: [" << n_after << "] of [" << n_before << "] components kept, [" << mesh.vertices.size() << "] vertices, ["
                              << mesh.triangles.size() / 3 << "] triangles." << std::endl;
                }
                if (simplify_mesh) {
                    const size_t n_v = mesh.vertices.size(), n_t = mesh.triangles.size() / 3;
                    float cell = 0.f;
                    if (!dr.simplifyMesh(mesh, 2.0f, &cell)) return 3;
                    std::cout << "Mesh simplify: [" << n_v << "] vertices, [" << n_t << "] triangles into [" << mesh.vertices.size() << "] vertices, ["
                              << mesh.triangles.size() / 3 << "] triangles, cells of [" << cell << "]." << std::endl;
                }
                const std::filesystem::path mesh_dir = std::filesystem::path(mesh_file).parent_path();
                if (!mesh_dir.empty()) std::filesystem::create_directories(mesh_dir);
                if (texture_mesh) {
                    std::vector<float> uv;
                    std::vector<uint8_t> atlas;
                    int atlas_rows = 0, atlas_cols = 0, n_labelled = 0, n_views = 0, texels = 0;
                    esfm_mesh_texture_level_stats level = {0, 0, 0, 0};
                    if (!dr.textureMesh(mesh, frames, todo, 0, uv, atlas, atlas_rows, atlas_cols, n_labelled, n_views, texels, level_mesh ? &level : nullptr)) return 3;
                    if (level_mesh)
                        std::cout << "Mesh texture level: [" << level.nodes << "] nodes, [" << level.seam_vertices << "] seam vertices, [" << level.iterations
                                  << "] iterations" << std::endl;
                    std::cout << "Mesh texture: [" << mesh.triangles.size() / 3 << "] triangles, [" << n_labelled << "] labelled from [" << n_views
                              << "] views, charts of [" << texels << "] texels, atlas [" << atlas_cols << "] x [" << atlas_rows << "]." << std::endl;
                    if (!io.writePlyTexturedMesh(mesh_file, mesh, uv, atlas_rows, atlas_cols, atlas)) return 3;
                    if (!render_dir.empty() && !render_mesh(dr, mesh, frames, todo, &uv, atlas_rows, atlas_cols, &atlas, render_dir)) return 3;
                } else {
                    if (!io.writePlyMesh(mesh_file, mesh)) return 3;
                    if (!render_dir.empty() && !render_mesh(dr, mesh, frames, todo, nullptr, 0, 0, nullptr, render_dir)) return 3;
                }
            }
        }
    } catch (const std::exception &e) {       // 1 is the reference's SUCCESS status: a failure must not look like one
        std::cerr << "sfm_native: " << e.what() << std::endl;
        return 3;
    }
    return 1;
}
