// Stand-alone host check of track triangulation's host code (no GPU call is made): easysfm_amd/csrc/track_api.cpp -- the argument
// checks, the grouping and esfm_track_triangulate_host / esfm_track_evaluate_host over track_core.hpp -- is compiled INTO this
// program, so that -fsanitize=address,undefined sees every index it forms, and run on the track-length edges (0, 1, 2, 3, 11, 12,
// 63, 64, 65, 129, 300 observations, interleaved), on degenerate tracks, at the options' edges and with the optional outputs
// absent.  Every output is compared, bit for bit, with the library's own build of the same entry points (found with dlsym).
// Built by tests/test_tracks_cpu.py, once plainly and once with the sanitizers.
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../easysfm_amd/csrc/track_api.cpp"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

namespace {

using TriFn = decltype(&esfm_track_triangulate_host);
using EvalFn = decltype(&esfm_track_evaluate_host);

struct Rng {   // a 64-bit LCG: the scene only has to be the same on every run
    uint64_t s;
    double uniform() { s = s * 6364136223846793005ull + 1442695040888963407ull; return double(s >> 11) / 9007199254740992.0; }
    double range(double a, double b) { return a + (b - a) * uniform(); }
};

struct Scene {
    int n_cam = 0, n_pt = 0;
    std::vector<int32_t> cam_idx, pt_idx;
    std::vector<float> uv, K4;
    std::vector<double> Rt, truth;
    int n_obs() const { return int(cam_idx.size()); }
};

// cameras on a ring of radius 10 looking at the origin; track p has lengths[p] observations, every fifth displaced by tens of pixels;
// the observation list is interleaved round-robin over the tracks
Scene ring_scene(const std::vector<int> &lengths, int n_cam, uint64_t seed)
{
    Scene s;
    Rng rng{seed};
    s.n_cam = n_cam; s.n_pt = int(lengths.size());
    const double fx = 2759.48, cx = 1520.69, fy = 2764.16, cy = 1006.81;
    for (int c = 0; c < n_cam; ++c) {
        const double ang = 2.0 * 3.14159265358979323846 * c / n_cam;
        const double C[3] = {10.0 * std::cos(ang), 0.6 * std::sin(2.0 * ang), 10.0 * std::sin(ang)};
        const double nc = std::sqrt(C[0] * C[0] + C[1] * C[1] + C[2] * C[2]);
        const double z[3] = {-C[0] / nc, -C[1] / nc, -C[2] / nc};
        double x[3] = {z[2], 0.0, -z[0]};                           // (0, 1, 0) x z
        const double nx = std::sqrt(x[0] * x[0] + x[2] * x[2]);
        for (double &v : x) v /= nx;
        const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
        const double *rows[3] = {x, y, z};
        for (int r = 0; r < 3; ++r) {
            for (int j = 0; j < 3; ++j) s.Rt.push_back(rows[r][j]);
            s.Rt.push_back(-(rows[r][0] * C[0] + rows[r][1] * C[1] + rows[r][2] * C[2]));
        }
        const float k[4] = {float(fx), float(cx), float(fy), float(cy)};
        s.K4.insert(s.K4.end(), k, k + 4);
    }
    std::vector<int> start(lengths.size());
    int longest = 0;
    for (size_t p = 0; p < lengths.size(); ++p) {
        for (int j = 0; j < 3; ++j) s.truth.push_back(rng.range(-2.0, 2.0));
        start[p] = int(rng.uniform() * n_cam) % n_cam;
        longest = lengths[p] > longest ? lengths[p] : longest;
    }
    for (int k = 0; k < longest; ++k)
        for (size_t p = 0; p < lengths.size(); ++p) {
            if (k >= lengths[p]) continue;
            const int c = (start[p] + 3 * k) % n_cam;
            const double *Rt = &s.Rt[size_t(12 * c)], *X = &s.truth[3 * p];
            double q[3];
            for (int r = 0; r < 3; ++r) q[r] = Rt[4 * r] * X[0] + Rt[4 * r + 1] * X[1] + Rt[4 * r + 2] * X[2] + Rt[4 * r + 3];
            double u = fx * q[0] / q[2] + cx + rng.range(-0.6, 0.6), v = fy * q[1] / q[2] + cy + rng.range(-0.6, 0.6);
            if (lengths[p] >= 5 && k % 5 == 4) { u += rng.range(20.0, 50.0); v -= rng.range(20.0, 50.0); }
            s.cam_idx.push_back(c); s.pt_idx.push_back(int32_t(p)); s.uv.push_back(float(u)); s.uv.push_back(float(v));
        }
    return s;
}

struct Out {
    std::vector<double> xyz, min_cos, mse;
    std::vector<uint8_t> inlier;
    std::vector<float> err2;
    std::vector<int32_t> status, n_inliers;
    // exact sizes: a write past an array's end lands in a red zone
    Out(int n_pt, int n_obs) : xyz(size_t(3 * n_pt)), min_cos(size_t(n_pt)), mse(size_t(n_pt)), inlier(size_t(n_obs)), err2(size_t(n_obs)), status(size_t(n_pt)), n_inliers(size_t(n_pt)) {}
    bool same(const Out &o) const
    {
        auto eq = [](const auto &a, const auto &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0); };
        return eq(xyz, o.xyz) && eq(min_cos, o.min_cos) && eq(mse, o.mse) && eq(inlier, o.inlier) && eq(err2, o.err2) && eq(status, o.status) && eq(n_inliers, o.n_inliers);
    }
};

int triangulate(TriFn fn, const Scene &s, const esfm_track_options &opt, const double *xyz_in, Out &o)
{
    return fn(s.n_cam, s.n_pt, s.n_obs(), s.cam_idx.data(), s.pt_idx.data(), s.uv.data(), s.K4.data(), s.Rt.data(), xyz_in, &opt, o.xyz.data(), o.inlier.data(),
              o.err2.data(), o.status.data(), o.n_inliers.data(), o.min_cos.data(), o.mse.data());
}

int evaluate(EvalFn fn, const Scene &s, const esfm_track_options &opt, const double *xyz, Out &o)
{
    return fn(s.n_cam, s.n_pt, s.n_obs(), s.cam_idx.data(), s.pt_idx.data(), s.uv.data(), s.K4.data(), s.Rt.data(), xyz, &opt, o.inlier.data(), o.err2.data(),
              o.status.data(), o.n_inliers.data(), o.min_cos.data(), o.mse.data());
}

}  // namespace

int main(int argc, char **argv)
{
    CHECK(argc == 2);
    void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    CHECK(lib);
    const TriFn lib_tri = reinterpret_cast<TriFn>(dlsym(lib, "esfm_track_triangulate_host"));
    const EvalFn lib_eval = reinterpret_cast<EvalFn>(dlsym(lib, "esfm_track_evaluate_host"));
    CHECK(lib_tri && lib_eval && lib_tri != &esfm_track_triangulate_host);
    esfm_track_options def;
    esfm_track_options_default(&def);
    CHECK(def.max_reproj_error_px == 4.0 && def.min_angle_deg == 1.5 && def.min_views == 2 && def.max_hypotheses == 64 && def.refine_iterations == 5);

    // 1  the track-length edges, default options and the options' edges; then the same points judged as given
    const std::vector<int> lengths = {0, 1, 2, 3, 11, 12, 0, 63, 64, 65, 129, ESFM_TRACK_STAGE_CAP + 44, 0};
    const Scene edge = ring_scene(lengths, 160, 7);
    std::vector<esfm_track_options> opts(4, def);
    opts[1].min_views = 3; opts[2].refine_iterations = 0; opts[3].max_hypotheses = 1;
    for (const esfm_track_options &opt : opts) {
        Out mine(edge.n_pt, edge.n_obs()), theirs(edge.n_pt, edge.n_obs());
        CHECK(triangulate(&esfm_track_triangulate_host, edge, opt, nullptr, mine) == ESFM_OK);
        CHECK(triangulate(lib_tri, edge, opt, nullptr, theirs) == ESFM_OK);
        CHECK(mine.same(theirs));
        for (size_t p = 0; p < lengths.size(); ++p) {
            CHECK(mine.status[p] == (lengths[p] < 2 ? 1 : (lengths[p] == 2 && opt.min_views == 3) ? 3 : 0));
            if (mine.status[p] == 0) for (int j = 0; j < 3; ++j) CHECK(std::fabs(mine.xyz[3 * p + size_t(j)] - edge.truth[3 * p + size_t(j)]) < 0.05);
            if (lengths[p] >= 5 && opt.max_hypotheses > 1) CHECK(mine.n_inliers[p] == lengths[p] - lengths[p] / 5);
        }
        Out ev(edge.n_pt, edge.n_obs()), ev_lib(edge.n_pt, edge.n_obs());
        CHECK(evaluate(&esfm_track_evaluate_host, edge, opt, mine.xyz.data(), ev) == ESFM_OK);
        CHECK(evaluate(lib_eval, edge, opt, mine.xyz.data(), ev_lib) == ESFM_OK);
        ev.xyz = ev_lib.xyz;
        CHECK(ev.same(ev_lib));
        for (size_t p = 0; p < lengths.size(); ++p) if (mine.status[p] == 0) CHECK(ev.status[p] == 0 && ev.n_inliers[p] == mine.n_inliers[p] && ev.mse[p] == mine.mse[p]);
    }

    // 2  degenerate tracks: two observations from one camera (status 2), a NaN pixel and an infinite focal length (status 5)
    {
        Scene s = ring_scene({2, 6, 6, 6}, 12, 21);
        s.K4.insert(s.K4.end(), s.K4.begin(), s.K4.begin() + 4); s.K4[size_t(4 * 12)] = std::numeric_limits<float>::infinity();
        s.Rt.insert(s.Rt.end(), s.Rt.begin(), s.Rt.begin() + 12); s.n_cam = 13;
        int seen[4] = {0, 0, 0, 0};
        for (int o = 0; o < s.n_obs(); ++o) {
            const int p = s.pt_idx[size_t(o)], k = seen[p]++;
            if (p == 0 && k == 1) s.cam_idx[size_t(o)] = s.cam_idx[0];
            if (p == 1 && k == 3) s.uv[size_t(2 * o + 1)] = std::numeric_limits<float>::quiet_NaN();
            if (p == 2 && k == 2) s.cam_idx[size_t(o)] = 12;
        }
        CHECK(s.pt_idx[0] == 0);
        const std::vector<double> xin = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
        Out mine(s.n_pt, s.n_obs()), theirs(s.n_pt, s.n_obs());
        CHECK(triangulate(&esfm_track_triangulate_host, s, def, xin.data(), mine) == ESFM_OK && triangulate(lib_tri, s, def, xin.data(), theirs) == ESFM_OK);
        CHECK(mine.same(theirs));
        CHECK(mine.status[0] == 2 && mine.status[1] == 5 && mine.status[2] == 5 && mine.status[3] == 0);
        CHECK(std::memcmp(mine.xyz.data(), xin.data(), sizeof(double) * 9) == 0 && mine.xyz[9] != xin[9]);   // xyz_in comes back for the three
    }

    // 3  the optional outputs absent; no observation at all; no point at all
    {
        const Scene s = ring_scene({4, 0, 7}, 24, 5);
        Out full(s.n_pt, s.n_obs()), part(s.n_pt, s.n_obs());
        CHECK(triangulate(&esfm_track_triangulate_host, s, def, nullptr, full) == ESFM_OK);
        CHECK(esfm_track_triangulate_host(s.n_cam, s.n_pt, s.n_obs(), s.cam_idx.data(), s.pt_idx.data(), s.uv.data(), s.K4.data(), s.Rt.data(), nullptr, &def, part.xyz.data(),
                                          part.inlier.data(), nullptr, part.status.data(), part.n_inliers.data(), nullptr, nullptr) == ESFM_OK);
        CHECK(part.xyz == full.xyz && part.inlier == full.inlier && part.status == full.status && part.n_inliers == full.n_inliers);
        Out none(s.n_pt, 0);
        CHECK(esfm_track_triangulate_host(s.n_cam, s.n_pt, 0, nullptr, nullptr, nullptr, s.K4.data(), s.Rt.data(), nullptr, &def, none.xyz.data(), nullptr, nullptr,
                                          none.status.data(), none.n_inliers.data(), none.min_cos.data(), none.mse.data()) == ESFM_OK);
        for (int p = 0; p < s.n_pt; ++p) CHECK(none.status[size_t(p)] == 1 && none.min_cos[size_t(p)] == 1.0);
        CHECK(esfm_track_triangulate_host(0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &def, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ESFM_OK);
    }

    // 4  what is refused, with nothing written
    {
        Scene s = ring_scene({3}, 24, 3);
        Out o(s.n_pt, s.n_obs());
        o.status[0] = 77;
        esfm_track_options bad = def; bad.min_views = 1;
        CHECK(triangulate(&esfm_track_triangulate_host, s, bad, nullptr, o) == ESFM_ERR_INVALID_ARG);
        bad = def; bad.max_hypotheses = 0;
        CHECK(triangulate(&esfm_track_triangulate_host, s, bad, nullptr, o) == ESFM_ERR_INVALID_ARG);
        bad = def; bad.max_reproj_error_px = std::numeric_limits<double>::quiet_NaN();
        CHECK(triangulate(&esfm_track_triangulate_host, s, bad, nullptr, o) == ESFM_ERR_INVALID_ARG);
        s.pt_idx[1] = 1;
        CHECK(triangulate(&esfm_track_triangulate_host, s, def, nullptr, o) == ESFM_ERR_INVALID_ARG);
        s.pt_idx[1] = 0; s.cam_idx[2] = -1;
        CHECK(triangulate(&esfm_track_triangulate_host, s, def, nullptr, o) == ESFM_ERR_INVALID_ARG);
        s.cam_idx[2] = 0;
        CHECK(evaluate(&esfm_track_evaluate_host, s, def, nullptr, o) == ESFM_ERR_INVALID_ARG);        // evaluate needs the points
        CHECK(o.status[0] == 77);
        CHECK(esfm_track_triangulate(nullptr, s.n_cam, s.n_pt, s.n_obs(), s.cam_idx.data(), s.pt_idx.data(), s.uv.data(), s.K4.data(), s.Rt.data(), nullptr, &def,
                                     o.xyz.data(), o.inlier.data(), nullptr, o.status.data(), o.n_inliers.data(), nullptr, nullptr) == ESFM_ERR_INVALID_ARG);   // no context
    }
    std::printf("track check ok\n");
    return 0;
}
