// C-ABI entry points of dense reconstruction (include/esfm.h, "Dense reconstruction"): the reference README's TODO "add
// multi-view stereo dense reconstruction".  Host side: argument checks, the view-selection / depth-range plan (host only),
// the plane inverse depths and homographies (double, explicit scalar loops, rounded to f32 once), uploads and launches.
// The pixel work runs in mvs_kernels.hip; tests/mvs_ref.py restates all of it.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mvs_kernels.hpp"
#include "scratch_layout.hpp"
#include "surf_kernels.hpp"

using esfm::MvsCam;
using esfm::MvsView;

namespace {

int check_options(const esfm_mvs_options *o)
{
    ESFM_REQUIRE(o, "options are NULL");
    ESFM_REQUIRE(o->num_planes >= 3 && o->num_planes <= 1024, "num_planes must be 3..1024");
    ESFM_REQUIRE(o->window_radius >= 1 && o->window_radius <= esfm::kMvsMaxRadius, "window_radius must be 1..7");
    ESFM_REQUIRE(o->max_neighbours >= 1 && o->max_neighbours <= esfm::kMvsMaxNb, "max_neighbours must be 1..8");
    ESFM_REQUIRE(o->min_shared_points >= 1, "min_shared_points must be >= 1");
    ESFM_REQUIRE(o->best_k >= 1 && o->best_k <= o->max_neighbours, "best_k must be 1..max_neighbours");
    ESFM_REQUIRE(o->depth_margin >= 0.f && std::isfinite(o->depth_margin), "depth_margin must be finite and >= 0");
    ESFM_REQUIRE(!std::isnan(o->max_cost), "max_cost is NaN");
    ESFM_REQUIRE(o->min_var > 0.f && std::isfinite(o->min_var), "min_var must be finite and > 0");
    ESFM_REQUIRE(o->fuse_min_views >= 1 && o->fuse_min_views <= o->max_neighbours, "fuse_min_views must be 1..max_neighbours");
    ESFM_REQUIRE(o->fuse_reproj_px > 0.f && std::isfinite(o->fuse_reproj_px), "fuse_reproj_px must be finite and > 0");
    ESFM_REQUIRE(o->fuse_rel_depth > 0.f && std::isfinite(o->fuse_rel_depth), "fuse_rel_depth must be finite and > 0");
    return ESFM_OK;
}

// the arguments both compute entry points share
int check_views(int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4, const float *poses,
                const int32_t *neighbours, const esfm_mvs_options *opt)
{
    if (int rc = check_options(opt)) return rc;
    ESFM_REQUIRE(n_views >= 1 && images && K4 && poses && neighbours, "NULL argument or no views");
    ESFM_REQUIRE(channels == 1 || channels == 3, "images must be rows x cols x {1, 3}");
    ESFM_REQUIRE(rows <= 16384 && cols <= 16384, "image sides are limited to 16384");
    const int win = 2 * opt->window_radius + 1;
    ESFM_REQUIRE(rows >= win && cols >= win, "image smaller than the window");
    ESFM_REQUIRE((int64_t)n_views * rows * cols <= ((int64_t)1 << 31) - 256, "more than 2^31 pixels in one call");
    for (int v = 0; v < n_views; ++v) {
        for (int j = 0; j < opt->max_neighbours; ++j) {
            const int s = neighbours[(size_t)v * opt->max_neighbours + j];
            ESFM_REQUIRE(s >= -1 && s < n_views && s != v, "a neighbour index is out of range or equals its view");
        }
        const float *k = K4 + 4 * (size_t)v;
        ESFM_REQUIRE(k[0] != 0.f && k[2] != 0.f && std::isfinite(k[0]) && std::isfinite(k[1]) && std::isfinite(k[2]) && std::isfinite(k[3]),
                     "K4 must be finite with non-zero focal lengths");
    }
    return ESFM_OK;
}

int check_ctx(esfm_ctx *ctx)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    return esfm::set_device(ctx);
}

// H_k = K_s (R_sr + t_sr [0 0 invd]) K_r^-1 in double, each sum from 0 over l = 0, 1, 2; rounded to f32 once
void homography(const float *Kr, const float *Pr, const float *Ks, const float *Ps, double invd, float H[9])
{
    double Rr[3][3], tr[3], Rs[3][3], ts[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { Rr[i][j] = Pr[4 * i + j]; Rs[i][j] = Ps[4 * i + j]; }
        tr[i] = Pr[4 * i + 3]; ts[i] = Ps[4 * i + 3];
    }
    double Rsr[3][3], tsr[3], M[3][3], A[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int l = 0; l < 3; ++l) s += Rs[i][l] * Rr[j][l];
            Rsr[i][j] = s;
        }
    for (int i = 0; i < 3; ++i) {
        double s = 0;
        for (int l = 0; l < 3; ++l) s += Rsr[i][l] * tr[l];
        tsr[i] = ts[i] - s;
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) M[i][j] = Rsr[i][j];
        M[i][2] += tsr[i] * invd;
    }
    const double fx = Kr[0], cx = Kr[1], fy = Kr[2], cy = Kr[3];
    const double Ki[3][3] = {{1 / fx, 0, -cx / fx}, {0, 1 / fy, -cy / fy}, {0, 0, 1}};
    const double Kt[3][3] = {{(double)Ks[0], 0, (double)Ks[1]}, {0, (double)Ks[2], (double)Ks[3]}, {0, 0, 1}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int l = 0; l < 3; ++l) s += M[i][l] * Ki[l][j];
            A[i][j] = s;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int l = 0; l < 3; ++l) s += Kt[i][l] * A[l][j];
            H[3 * i + j] = (float)s;
        }
}

// esfm_mvs_fuse and esfm_mvs_fuse_ex: one body; pixel_index NULL = the index is neither computed nor copied
int fuse(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4, const float *poses,
         const int32_t *neighbours, const float *depth, const esfm_mvs_options *opt, float *xyz, uint8_t *rgb, int32_t *pixel_index,
         int32_t *n_points)
{
    if (int rc = check_views(n_views, rows, cols, channels, images, K4, poses, neighbours, opt)) return rc;
    ESFM_REQUIRE(depth && xyz && rgb && n_points, "NULL argument");
    if (int rc = check_ctx(ctx)) return rc;
    *n_points = 0;
    hipStream_t st = ctx->stream;
    const int nb = opt->max_neighbours;
    std::vector<MvsCam> cams((size_t)n_views);
    for (int v = 0; v < n_views; ++v) {
        MvsCam &c = cams[(size_t)v];
        memcpy(c.K, K4 + 4 * (size_t)v, sizeof(c.K));
        memcpy(c.P, poses + 12 * (size_t)v, sizeof(c.P));
        for (int j = 0; j < esfm::kMvsMaxNb; ++j) c.nb[j] = j < nb ? neighbours[(size_t)v * nb + j] : -1;
    }
    const size_t n_px = (size_t)n_views * rows * cols;
    const size_t n_blocks = (n_px + 255) / 256;
    // stage_a: images | depth | cams | block counts + n_points; stage_b: per-pixel points | colours | keep; stage_c: output
    const size_t img_b = esfm::align256(n_px * channels), dep_b = esfm::align256(sizeof(float) * n_px), cam_b = esfm::align256(sizeof(MvsCam) * cams.size());
    const size_t cnt_b = esfm::align256(sizeof(int32_t) * (n_blocks + 1));
    esfm::DevBuf &b_in = ctx->stage_a, &b_stage = ctx->stage_b, &b_out = ctx->stage_c;
    if (int rc = b_in.reserve(img_b + dep_b + cam_b + cnt_b)) return rc;
    if (int rc = b_stage.reserve(esfm::align256(sizeof(float) * 3 * n_px) + esfm::align256(3 * n_px) + esfm::align256(n_px))) return rc;
    if (int rc = b_out.reserve(esfm::align256(sizeof(float) * 3 * n_px) + esfm::align256(3 * n_px) + (pixel_index ? sizeof(int32_t) * n_px : 0))) return rc;
    uint8_t *p_in = b_in.as<uint8_t>(), *p_stage = b_stage.as<uint8_t>(), *p_out = b_out.as<uint8_t>();
    esfm::MvsFuseArgs a;
    a.images = p_in;
    a.depth = reinterpret_cast<const float *>(p_in + img_b);
    a.cams = reinterpret_cast<const MvsCam *>(p_in + img_b + dep_b);
    a.block_count = reinterpret_cast<int32_t *>(p_in + img_b + dep_b + cam_b);
    a.n_points = a.block_count + n_blocks;
    a.stage_xyz = reinterpret_cast<float *>(p_stage);
    a.stage_rgb = p_stage + esfm::align256(sizeof(float) * 3 * n_px);
    a.keep = a.stage_rgb + esfm::align256(3 * n_px);
    a.xyz = reinterpret_cast<float *>(p_out);
    a.rgb = p_out + esfm::align256(sizeof(float) * 3 * n_px);
    a.pixel_index = pixel_index ? reinterpret_cast<int32_t *>(a.rgb + esfm::align256(3 * n_px)) : nullptr;
    a.n_px = (int64_t)n_px;
    a.rows = rows; a.cols = cols; a.channels = channels; a.n_nb = nb; a.min_views = opt->fuse_min_views;
    a.reproj2 = opt->fuse_reproj_px * opt->fuse_reproj_px;
    a.rel_depth = opt->fuse_rel_depth;
    ESFM_HIP_TRY(esfm::copy_h2d(p_in, images, n_px * channels, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_in + img_b, depth, sizeof(float) * n_px, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_in + img_b + dep_b, cams.data(), sizeof(MvsCam) * cams.size(), st));
    {
        esfm::KernelTimer tm(ctx, ESFM_K_MVS_FUSE);
        if (int rc = esfm::launch_mvs_fuse(st, a)) return rc;
    }
    int32_t n = 0;
    ESFM_HIP_TRY(esfm::copy_d2h(&n, a.n_points, sizeof(int32_t), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    ESFM_HIP_TRY(esfm::copy_d2h(xyz, a.xyz, sizeof(float) * 3 * (size_t)n, st));
    ESFM_HIP_TRY(esfm::copy_d2h(rgb, a.rgb, 3 * (size_t)n, st));
    if (pixel_index) ESFM_HIP_TRY(esfm::copy_d2h(pixel_index, a.pixel_index, sizeof(int32_t) * (size_t)n, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    *n_points = n;
    return ESFM_OK;
}

}  // namespace

extern "C" {

void esfm_mvs_options_default(esfm_mvs_options *opt)
{
    if (!opt) return;
    opt->num_planes = 128;
    opt->window_radius = 3;
    opt->max_neighbours = 4;
    opt->min_shared_points = 20;
    opt->best_k = 2;
    opt->depth_margin = 0.25f;
    opt->max_cost = 0.5f;
    opt->min_var = 4.0f;
    opt->fuse_min_views = 2;
    opt->fuse_reproj_px = 1.0f;
    opt->fuse_rel_depth = 0.01f;
}

int esfm_mvs_plan(int n_views, const uint8_t *registered, const float *poses, int n_points, const float *xyz, const int32_t *obs_offsets,
                  const int32_t *obs_points, const esfm_mvs_options *opt, int32_t *neighbours, float *depth_range)
{
    if (int rc = check_options(opt)) return rc;
    ESFM_REQUIRE(n_views >= 1 && n_points >= 0 && registered && poses && obs_offsets && neighbours && depth_range, "NULL argument or no views");
    ESFM_REQUIRE(n_points == 0 || xyz, "xyz is NULL");
    ESFM_REQUIRE(obs_offsets[0] == 0, "obs_offsets[0] must be 0");
    for (int v = 0; v < n_views; ++v) ESFM_REQUIRE(obs_offsets[v + 1] >= obs_offsets[v], "obs_offsets must not decrease");
    ESFM_REQUIRE(obs_offsets[n_views] == 0 || obs_points, "obs_points is NULL");
    for (int32_t i = 0; i < obs_offsets[n_views]; ++i) ESFM_REQUIRE(obs_points[i] >= 0 && obs_points[i] < n_points, "obs_points out of range");
    const int nb = opt->max_neighbours;

    // obs(v) as sorted sets of point indices (duplicates count once)
    std::vector<std::vector<int32_t>> obs((size_t)n_views);
    for (int v = 0; v < n_views; ++v) {
        if (!registered[v]) continue;
        obs[v].assign(obs_points + obs_offsets[v], obs_points + obs_offsets[v + 1]);
        std::sort(obs[v].begin(), obs[v].end());
        obs[v].erase(std::unique(obs[v].begin(), obs[v].end()), obs[v].end());
    }
    std::vector<int32_t> nbr((size_t)n_views * nb, -1);
    std::vector<float> range((size_t)n_views * 2, 0.f);
    for (int r = 0; r < n_views; ++r) {
        if (!registered[r]) continue;
        std::vector<std::pair<int64_t, int>> cand;   // (-score, view): best first, ties to the lower index
        for (int v = 0; v < n_views; ++v) {
            if (v == r || !registered[v]) continue;
            std::vector<int32_t> both;
            std::set_intersection(obs[r].begin(), obs[r].end(), obs[v].begin(), obs[v].end(), std::back_inserter(both));
            if ((int64_t)both.size() >= opt->min_shared_points) cand.push_back({-(int64_t)both.size(), v});
        }
        std::sort(cand.begin(), cand.end());
        for (int j = 0; j < nb && j < (int)cand.size(); ++j) nbr[(size_t)r * nb + j] = cand[(size_t)j].second;
        if (cand.empty()) continue;
        const float *P = poses + 12 * (size_t)r;
        std::vector<float> z;
        for (int32_t p : obs[r]) {
            const float *X = xyz + 3 * (size_t)p;
            const float zz = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
            if (zz > 0.f) z.push_back(zz);
        }
        if (z.size() < 10) continue;
        std::sort(z.begin(), z.end());
        const double n1 = (double)(z.size() - 1);
        const float lo = z[(size_t)std::floor(0.02 * n1)], hi = z[(size_t)std::ceil(0.98 * n1)];
        const float g = 1.f + opt->depth_margin;
        range[2 * (size_t)r] = lo / g;
        range[2 * (size_t)r + 1] = hi * g;
    }
    memcpy(neighbours, nbr.data(), sizeof(int32_t) * nbr.size());
    memcpy(depth_range, range.data(), sizeof(float) * range.size());
    return ESFM_OK;
}

int esfm_mvs_depth_maps(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4,
                        const float *poses, const int32_t *neighbours, const float *depth_range, const esfm_mvs_options *opt, float *depth,
                        float *cost)
{
    if (int rc = check_views(n_views, rows, cols, channels, images, K4, poses, neighbours, opt)) return rc;
    ESFM_REQUIRE(depth_range && depth && cost, "NULL argument");
    for (int v = 0; v < n_views; ++v) {
        const float lo = depth_range[2 * (size_t)v], hi = depth_range[2 * (size_t)v + 1];
        ESFM_REQUIRE((lo == 0.f && hi == 0.f) || (lo > 0.f && lo < hi && std::isfinite(hi)),
                     "a depth range must be (0, 0) or finite with 0 < d_min < d_max");
    }
    if (int rc = check_ctx(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const int D = opt->num_planes, nb = opt->max_neighbours;

    // per-view table, (float) invd_k, homographies
    std::vector<MvsView> views((size_t)n_views);
    std::vector<float> invd, H;
    for (int v = 0; v < n_views; ++v) {
        MvsView &V = views[(size_t)v];
        memset(&V, 0, sizeof(V));
        const float lo = depth_range[2 * (size_t)v], hi = depth_range[2 * (size_t)v + 1];
        if (!(lo > 0.f)) continue;
        V.active = 1;
        for (int j = 0; j < nb; ++j) {
            const int s = neighbours[(size_t)v * nb + j];
            if (s >= 0) V.src[V.n_src++] = s;
        }
        const double step = (1.0 / (double)lo - 1.0 / (double)hi) / (D - 1);
        V.step = (float)step;
        V.invd_off = (int64_t)invd.size();
        V.h_off = (int64_t)H.size();
        for (int k = 0; k < D; ++k) invd.push_back((float)(1.0 / (double)hi + k * step));
        for (int si = 0; si < V.n_src; ++si)
            for (int k = 0; k < D; ++k) {
                float h[9];
                homography(K4 + 4 * (size_t)v, poses + 12 * (size_t)v, K4 + 4 * (size_t)V.src[si], poses + 12 * (size_t)V.src[si],
                           1.0 / (double)hi + k * step, h);
                H.insert(H.end(), h, h + 9);
            }
    }
    invd.push_back(0.f); H.push_back(0.f);     // (never empty)

    const size_t n_px = (size_t)n_views * rows * cols;
    esfm::DevBuf &b_img = ctx->stage_a, &b_out = ctx->stage_b, &b_tab = ctx->stage_c;
    const size_t gray_bytes = (n_px + 255) / 256 * 256;
    if (int rc = b_img.reserve(gray_bytes + (channels == 3 ? n_px * 3 : 0))) return rc;
    if (int rc = b_out.reserve(sizeof(float) * 2 * n_px)) return rc;
    const size_t views_bytes = sizeof(MvsView) * views.size(), invd_off = (views_bytes + 255) / 256 * 256,
                 h_off = invd_off + (sizeof(float) * invd.size() + 255) / 256 * 256, tab_bytes = h_off + sizeof(float) * H.size();
    if (int rc = b_tab.reserve(tab_bytes)) return rc;
    uint8_t *d_gray = b_img.as<uint8_t>(), *d_tab = b_tab.as<uint8_t>();
    float *d_depth = b_out.as<float>(), *d_cost = d_depth + n_px;
    if (channels == 3) {
        uint8_t *d_bgr = d_gray + gray_bytes;
        ESFM_HIP_TRY(esfm::copy_h2d(d_bgr, images, n_px * 3, st));
        if (int rc = esfm::launch_surf_gray(st, d_bgr, (int)n_px, d_gray)) return rc;   // cvtColor's fixed-point weights, as SURF
    } else {
        ESFM_HIP_TRY(esfm::copy_h2d(d_gray, images, n_px, st));
    }
    ESFM_HIP_TRY(esfm::copy_h2d(d_tab, views.data(), views_bytes, st));
    ESFM_HIP_TRY(esfm::copy_h2d(d_tab + invd_off, invd.data(), sizeof(float) * invd.size(), st));
    ESFM_HIP_TRY(esfm::copy_h2d(d_tab + h_off, H.data(), sizeof(float) * H.size(), st));

    esfm::MvsSweepArgs a;
    a.gray = d_gray;
    a.views = reinterpret_cast<const MvsView *>(d_tab);
    a.invd = reinterpret_cast<const float *>(d_tab + invd_off);
    a.H = reinterpret_cast<const float *>(d_tab + h_off);
    a.depth = d_depth; a.cost = d_cost;
    a.rows = rows; a.cols = cols; a.D = D; a.best_k = opt->best_k;
    a.tiles_x = (cols + esfm::kMvsTile - 1) / esfm::kMvsTile;
    a.max_src = 0;
    for (const MvsView &V : views) a.max_src = std::max(a.max_src, (int32_t)V.n_src);
    const int n_taps = (2 * opt->window_radius + 1) * (2 * opt->window_radius + 1);
    a.min_var_n = (float)n_taps * opt->min_var;
    a.max_cost = opt->max_cost;
    {
        esfm::KernelTimer tm(ctx, ESFM_K_MVS_SWEEP);
        if (int rc = esfm::launch_mvs_sweep(st, a, opt->window_radius, n_views)) return rc;
    }
    ESFM_HIP_TRY(esfm::copy_d2h(depth, d_depth, sizeof(float) * n_px, st));
    ESFM_HIP_TRY(esfm::copy_d2h(cost, d_cost, sizeof(float) * n_px, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

int esfm_mvs_fuse(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4, const float *poses,
                  const int32_t *neighbours, const float *depth, const esfm_mvs_options *opt, float *xyz, uint8_t *rgb, int32_t *n_points)
{
    return fuse(ctx, n_views, rows, cols, channels, images, K4, poses, neighbours, depth, opt, xyz, rgb, nullptr, n_points);
}

int esfm_mvs_fuse_ex(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4, const float *poses,
                     const int32_t *neighbours, const float *depth, const esfm_mvs_options *opt, float *xyz, uint8_t *rgb,
                     int32_t *pixel_index, int32_t *n_points)
{
    return fuse(ctx, n_views, rows, cols, channels, images, K4, poses, neighbours, depth, opt, xyz, rgb, pixel_index, n_points);
}

void esfm_mvs_normal_options_default(esfm_mvs_normal_options *opt)
{
    if (!opt) return;
    opt->normal_radius = 3;
    opt->normal_min_taps = 25;
    opt->normal_rel_step = 0.05f;
}

int esfm_mvs_normals(esfm_ctx *ctx, int n_views, int rows, int cols, const float *K4, const float *poses, const float *depth,
                     const esfm_mvs_normal_options *opt, float *normals)
{
    ESFM_REQUIRE(opt, "options are NULL");
    ESFM_REQUIRE(opt->normal_radius >= 1 && opt->normal_radius <= esfm::kMvsMaxRadius, "normal_radius must be 1..7");
    const int win = 2 * opt->normal_radius + 1;
    ESFM_REQUIRE(opt->normal_min_taps >= 3 && opt->normal_min_taps <= win * win, "normal_min_taps must be 3..(2 normal_radius + 1)^2");
    ESFM_REQUIRE(opt->normal_rel_step > 0.f && std::isfinite(opt->normal_rel_step), "normal_rel_step must be finite and > 0");
    ESFM_REQUIRE(n_views >= 1 && K4 && poses && depth && normals, "NULL argument or no views");
    ESFM_REQUIRE(rows >= 1 && cols >= 1 && rows <= 16384 && cols <= 16384, "image sides must be 1..16384");
    ESFM_REQUIRE((int64_t)n_views * rows * cols <= ((int64_t)1 << 31) - 256, "more than 2^31 pixels in one call");
    for (int v = 0; v < n_views; ++v) {
        const float *k = K4 + 4 * (size_t)v;
        ESFM_REQUIRE(k[0] != 0.f && k[2] != 0.f && std::isfinite(k[0]) && std::isfinite(k[1]) && std::isfinite(k[2]) && std::isfinite(k[3]),
                     "K4 must be finite with non-zero focal lengths");
    }
    if (int rc = check_ctx(ctx)) return rc;
    hipStream_t st = ctx->stream;
    std::vector<MvsCam> cams((size_t)n_views);
    for (int v = 0; v < n_views; ++v) {
        MvsCam &c = cams[(size_t)v];
        memcpy(c.K, K4 + 4 * (size_t)v, sizeof(c.K));
        memcpy(c.P, poses + 12 * (size_t)v, sizeof(c.P));
        for (int j = 0; j < esfm::kMvsMaxNb; ++j) c.nb[j] = -1;
    }
    const size_t n_px = (size_t)n_views * rows * cols;
    const size_t dep_b = (sizeof(float) * n_px + 255) / 256 * 256;
    if (int rc = ctx->stage_a.reserve(dep_b + sizeof(MvsCam) * cams.size())) return rc;
    if (int rc = ctx->stage_b.reserve(sizeof(float) * 3 * n_px)) return rc;
    uint8_t *p_in = ctx->stage_a.as<uint8_t>();
    ESFM_HIP_TRY(esfm::copy_h2d(p_in, depth, sizeof(float) * n_px, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_in + dep_b, cams.data(), sizeof(MvsCam) * cams.size(), st));
    esfm::MvsNormalArgs a;
    a.depth = reinterpret_cast<const float *>(p_in);
    a.cams = reinterpret_cast<const MvsCam *>(p_in + dep_b);
    a.normals = ctx->stage_b.as<float>();
    a.rows = rows; a.cols = cols; a.tiles_x = (cols + esfm::kMvsTile - 1) / esfm::kMvsTile;
    a.radius = opt->normal_radius; a.min_taps = opt->normal_min_taps; a.rel_step = opt->normal_rel_step;
    if (int rc = esfm::launch_mvs_normals(st, a, n_views)) return rc;
    ESFM_HIP_TRY(esfm::copy_d2h(normals, a.normals, sizeof(float) * 3 * n_px, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

}  // extern "C"
