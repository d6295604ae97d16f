// C-ABI entry points of track triangulation (include/esfm.h "Track triangulation").  The host validates the arguments (it holds the
// index arrays anyway: host pointers) and sizes the scratch; grouping, hypotheses, refit and verdicts run in track_kernels.hip.
// The *_host forms run track_core.hpp's solve_host over the same records, grouped by a stable counting sort.
#include <cmath>
#include <vector>

#include "mesh_kernels.hpp"
#include "scratch_layout.hpp"
#include "track_core.hpp"
#include "track_kernels.hpp"

namespace {

using esfm::track::Obs;

struct Call {
    int n_cam, n_pt, n_obs;
    const int32_t *cam_idx, *pt_idx;
    const float *uv, *K4;
    const double *Rt, *xyz_in;
    const esfm_track_options *opt;
    double *xyz_out;
    uint8_t *obs_inlier;
    float *obs_err2;
    int32_t *pt_status, *pt_n_inliers;
    double *pt_min_cos, *pt_mse;
    bool evaluate;
};

// the argument rules of both forms; count[p] = observations of point p; *longest = the longest track
int validate(const Call &c, esfm::track::Options *o, std::vector<int32_t> *count, int *longest)
{
    ESFM_REQUIRE(c.n_cam >= 0 && c.n_pt >= 0 && c.n_obs >= 0, "negative count");
    ESFM_REQUIRE(c.opt, "options are NULL");
    const esfm_track_options &p = *c.opt;
    ESFM_REQUIRE(std::isfinite(p.max_reproj_error_px) && p.max_reproj_error_px > 0.0, "max_reproj_error_px must be finite and > 0");
    ESFM_REQUIRE(p.cos_min_angle == p.cos_min_angle, "cos_min_angle is NaN");
    ESFM_REQUIRE(p.min_views >= 2, "min_views must be >= 2");
    ESFM_REQUIRE(p.max_hypotheses >= 1 && p.max_hypotheses <= 4096, "max_hypotheses must be in 1 .. 4096");
    ESFM_REQUIRE(p.refine_iterations >= 0 && p.refine_iterations <= 100, "refine_iterations must be in 0 .. 100");
    ESFM_REQUIRE(c.n_pt == 0 || (c.pt_status && c.pt_n_inliers && (c.evaluate || c.xyz_out)), "NULL point output");
    ESFM_REQUIRE(c.n_pt == 0 || !c.evaluate || c.xyz_in, "evaluate needs xyz_in");
    ESFM_REQUIRE(c.n_obs == 0 || (c.cam_idx && c.pt_idx && c.uv && c.K4 && c.Rt && c.obs_inlier), "NULL observation or camera array");
    o->thr2 = p.max_reproj_error_px * p.max_reproj_error_px; o->cos_min_angle = p.cos_min_angle;
    o->min_views = p.min_views; o->max_hypotheses = p.max_hypotheses; o->refine_iterations = p.refine_iterations;
    count->assign((size_t)c.n_pt, 0);
    for (int i = 0; i < c.n_obs; ++i) {
        ESFM_REQUIRE(c.cam_idx[i] >= 0 && c.cam_idx[i] < c.n_cam, "cam_idx out of range");
        ESFM_REQUIRE(c.pt_idx[i] >= 0 && c.pt_idx[i] < c.n_pt, "pt_idx out of range");
        ++(*count)[(size_t)c.pt_idx[i]];
    }
    *longest = 0;
    for (int32_t n : *count) *longest = n > *longest ? n : *longest;
    if (*longest > esfm::track::kMaxObs) { esfm::set_error("a track has %d observations (at most %d)", *longest, esfm::track::kMaxObs); return ESFM_ERR_UNSUPPORTED; }
    return ESFM_OK;
}

int run_device(esfm_ctx *ctx, const Call &c)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    esfm::track::Options o;
    std::vector<int32_t> count;
    int longest = 0;
    if (int rc = validate(c, &o, &count, &longest)) return rc;
    if (c.n_pt == 0) return ESFM_OK;
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const size_t P = (size_t)c.n_pt, N = (size_t)c.n_obs, M = (size_t)c.n_cam, N1 = N ? N : 1, M1 = M ? M : 1;
    size_t sort_b = 0;
    if (N) if (int rc = esfm::mesh_sort_scratch_bytes((int64_t)N, esfm::track_key_bits(c.n_pt), &sort_b, st)) return rc;

    // stage_a: inputs | grouping | outputs;  stage_b: the records of the tracks above the staging cap
    esfm::ScratchCarver at;
    const size_t i_cam = at.take(sizeof(int32_t) * N1), i_pt = at.take(sizeof(int32_t) * N1), i_uv = at.take(sizeof(float) * 2 * N1),
                 i_K = at.take(sizeof(float) * 4 * M1), i_Rt = at.take(sizeof(double) * 12 * M1), i_xyz = at.take(c.xyz_in ? sizeof(double) * 3 * P : 0);
    const size_t g_keys = at.take(sizeof(uint64_t) * N1), g_sorted = at.take(sizeof(uint64_t) * N1),
                 g_blocks = at.take(sizeof(int32_t) * ((N1 + 255) / 256 + 1)), g_first = at.take(sizeof(int32_t) * (N1 + 1)), g_sort = at.take(sort_b);
    const size_t o_xyz = at.take(c.evaluate ? 0 : sizeof(double) * 3 * P), o_inl = at.take(N1), o_err = at.take(c.obs_err2 ? sizeof(float) * N1 : 0),
                 o_status = at.take(sizeof(int32_t) * P), o_ninl = at.take(sizeof(int32_t) * P), o_cos = at.take(c.pt_min_cos ? sizeof(double) * P : 0),
                 o_mse = at.take(c.pt_mse ? sizeof(double) * P : 0);
    if (int rc = ctx->stage_a.reserve(at.at)) return rc;
    const bool any_long = longest > esfm::track::kStageCap;
    if (any_long) if (int rc = ctx->stage_b.reserve(sizeof(Obs) * N)) return rc;
    uint8_t *d = ctx->stage_a.as<uint8_t>();

    esfm::TrackArgs a;
    a.n_cam = c.n_cam; a.n_pt = c.n_pt; a.n_obs = c.n_obs; a.evaluate = c.evaluate ? 1 : 0; a.opt = o;
    a.cam_idx = reinterpret_cast<int32_t *>(d + i_cam); a.pt_idx = reinterpret_cast<int32_t *>(d + i_pt);
    a.uv = reinterpret_cast<float *>(d + i_uv); a.K4 = reinterpret_cast<float *>(d + i_K); a.Rt = reinterpret_cast<double *>(d + i_Rt);
    a.xyz_in = c.xyz_in ? reinterpret_cast<double *>(d + i_xyz) : nullptr;
    a.keys = reinterpret_cast<uint64_t *>(d + g_keys); a.sorted = reinterpret_cast<uint64_t *>(d + g_sorted);
    a.head_blocks = reinterpret_cast<int32_t *>(d + g_blocks); a.track_first = reinterpret_cast<int32_t *>(d + g_first);
    a.long_rec = any_long ? ctx->stage_b.as<Obs>() : nullptr;
    a.xyz_out = c.evaluate ? nullptr : reinterpret_cast<double *>(d + o_xyz);
    a.obs_inlier = d + o_inl; a.obs_err2 = c.obs_err2 ? reinterpret_cast<float *>(d + o_err) : nullptr;
    a.pt_status = reinterpret_cast<int32_t *>(d + o_status); a.pt_n_inliers = reinterpret_cast<int32_t *>(d + o_ninl);
    a.pt_min_cos = c.pt_min_cos ? reinterpret_cast<double *>(d + o_cos) : nullptr;
    a.pt_mse = c.pt_mse ? reinterpret_cast<double *>(d + o_mse) : nullptr;

    if (N) {
        ESFM_HIP_TRY(esfm::copy_h2d(d + i_cam, c.cam_idx, sizeof(int32_t) * N, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d + i_pt, c.pt_idx, sizeof(int32_t) * N, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d + i_uv, c.uv, sizeof(float) * 2 * N, st));
    }
    if (M) {
        ESFM_HIP_TRY(esfm::copy_h2d(d + i_K, c.K4, sizeof(float) * 4 * M, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d + i_Rt, c.Rt, sizeof(double) * 12 * M, st));
    }
    if (c.xyz_in) ESFM_HIP_TRY(esfm::copy_h2d(d + i_xyz, c.xyz_in, sizeof(double) * 3 * P, st));
    if (N) {
        if (int rc = esfm::launch_track_solve(st, a, d + g_sort, sort_b)) return rc;
    } else if (int rc = esfm::launch_track_defaults(st, a)) return rc;
    if (!c.evaluate) ESFM_HIP_TRY(esfm::copy_d2h(c.xyz_out, d + o_xyz, sizeof(double) * 3 * P, st));
    if (N) ESFM_HIP_TRY(esfm::copy_d2h(c.obs_inlier, d + o_inl, N, st));
    if (N && c.obs_err2) ESFM_HIP_TRY(esfm::copy_d2h(c.obs_err2, d + o_err, sizeof(float) * N, st));
    ESFM_HIP_TRY(esfm::copy_d2h(c.pt_status, d + o_status, sizeof(int32_t) * P, st));
    ESFM_HIP_TRY(esfm::copy_d2h(c.pt_n_inliers, d + o_ninl, sizeof(int32_t) * P, st));
    if (c.pt_min_cos) ESFM_HIP_TRY(esfm::copy_d2h(c.pt_min_cos, d + o_cos, sizeof(double) * P, st));
    if (c.pt_mse) ESFM_HIP_TRY(esfm::copy_d2h(c.pt_mse, d + o_mse, sizeof(double) * P, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

int run_host(const Call &c)
{
    esfm::track::Options o;
    std::vector<int32_t> count;
    int longest = 0;
    if (int rc = validate(c, &o, &count, &longest)) return rc;
    const size_t P = (size_t)c.n_pt, N = (size_t)c.n_obs;
    // stable counting sort: order[start[p] ..] = the input indices of point p, ascending
    std::vector<int32_t> start(P + 1, 0), fill(P, 0), order(N);
    for (size_t p = 0; p < P; ++p) start[p + 1] = start[p] + count[p];
    for (size_t i = 0; i < N; ++i) { const size_t p = (size_t)c.pt_idx[i]; order[(size_t)(start[p] + fill[p]++)] = (int32_t)i; }
    std::vector<Obs> rec((size_t)(longest > 0 ? longest : 1));
    for (size_t p = 0; p < P; ++p) {
        const int n = count[p];
        const int32_t *idx = order.data() + start[p];
        esfm::track::Result r;
        r.status = esfm::track::kTooFew; r.n_inliers = 0; r.min_cos = 1.0; r.mse = 0.0; r.X[0] = r.X[1] = r.X[2] = 0.0;
        bool solved = false;
        if (n >= 2) {
            bool ok = true;
            if (c.evaluate) for (int j = 0; j < 3; ++j) ok = ok && esfm::track::finite_d(c.xyz_in[3 * p + j]);
            for (int k = 0; k < n; ++k) {
                const size_t i = (size_t)idx[k];
                const int32_t cam = c.cam_idx[i];
                ok = esfm::track::make_obs(c.Rt + 12 * (size_t)cam, c.K4 + 4 * (size_t)cam, c.uv[2 * i], c.uv[2 * i + 1], cam, rec[(size_t)k]) && ok;
            }
            if (!ok) r.status = esfm::track::kNonFinite;
            else {
                esfm::track::solve_host(rec.data(), n, c.Rt, c.K4, o, c.evaluate ? c.xyz_in + 3 * p : nullptr, r);
                solved = r.status != esfm::track::kNoHypothesis;
            }
        }
        for (int k = 0; k < n; ++k) {
            const size_t i = (size_t)idx[k];
            c.obs_inlier[i] = solved ? (uint8_t)(rec[(size_t)k].flags & 1) : 0;
            if (c.obs_err2) c.obs_err2[i] = solved ? esfm::track::err2_out(rec[(size_t)k].C[0]) : (float)INFINITY;
        }
        c.pt_status[p] = r.status; c.pt_n_inliers[p] = r.n_inliers;
        if (c.pt_min_cos) c.pt_min_cos[p] = r.min_cos;
        if (c.pt_mse) c.pt_mse[p] = r.mse;
        if (!c.evaluate) for (int j = 0; j < 3; ++j) c.xyz_out[3 * p + j] = r.status == esfm::track::kKept ? r.X[j] : (c.xyz_in ? c.xyz_in[3 * p + j] : 0.0);
    }
    return ESFM_OK;
}

}  // namespace

extern "C" {

void esfm_track_options_default(esfm_track_options *opt)
{
    if (!opt) return;
    opt->max_reproj_error_px = 4.0;
    opt->min_angle_deg = 1.5;
    opt->cos_min_angle = std::cos(opt->min_angle_deg * (3.14159265358979323846 / 180.0));
    opt->min_views = 2; opt->max_hypotheses = 64; opt->refine_iterations = 5; opt->reserved = 0;
}

int esfm_track_triangulate(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                           const float *K4_per_cam, const double *Rt12_per_cam, const double *xyz_in, const esfm_track_options *opt, double *xyz_out,
                           uint8_t *obs_inlier, float *obs_err2, int32_t *pt_status, int32_t *pt_n_inliers, double *pt_min_cos, double *pt_mse)
{
    return run_device(ctx, Call{n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, K4_per_cam, Rt12_per_cam, xyz_in, opt, xyz_out, obs_inlier, obs_err2,
                                pt_status, pt_n_inliers, pt_min_cos, pt_mse, false});
}

int esfm_track_evaluate(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                        const float *K4_per_cam, const double *Rt12_per_cam, const double *xyz_in, const esfm_track_options *opt, uint8_t *obs_inlier,
                        float *obs_err2, int32_t *pt_status, int32_t *pt_n_inliers, double *pt_min_cos, double *pt_mse)
{
    return run_device(ctx, Call{n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, K4_per_cam, Rt12_per_cam, xyz_in, opt, nullptr, obs_inlier, obs_err2,
                                pt_status, pt_n_inliers, pt_min_cos, pt_mse, true});
}

int esfm_track_triangulate_host(int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                                const float *K4_per_cam, const double *Rt12_per_cam, const double *xyz_in, const esfm_track_options *opt,
                                double *xyz_out, uint8_t *obs_inlier, float *obs_err2, int32_t *pt_status, int32_t *pt_n_inliers, double *pt_min_cos,
                                double *pt_mse)
{
    return run_host(Call{n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, K4_per_cam, Rt12_per_cam, xyz_in, opt, xyz_out, obs_inlier, obs_err2, pt_status,
                         pt_n_inliers, pt_min_cos, pt_mse, false});
}

int esfm_track_evaluate_host(int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                             const float *K4_per_cam, const double *Rt12_per_cam, const double *xyz_in, const esfm_track_options *opt,
                             uint8_t *obs_inlier, float *obs_err2, int32_t *pt_status, int32_t *pt_n_inliers, double *pt_min_cos, double *pt_mse)
{
    return run_host(Call{n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, K4_per_cam, Rt12_per_cam, xyz_in, opt, nullptr, obs_inlier, obs_err2, pt_status,
                         pt_n_inliers, pt_min_cos, pt_mse, true});
}

}  // extern "C"
