// C-ABI entry points for bundle adjustment (include/esfm.h, rows a-4..a-8 of SURVEY.md section 8) except the solve itself
// (ba_solve.cpp): argument checks, problem set-up and tear-down, parameter access, the one-shot wrappers, and the host-only helpers.
// A problem's index tables come from ba_layout.cpp, the forms of its size-dependent kernels from ba_forms (ba_forms.cpp); this file
// allocates and uploads.
#include <climits>
#include <cmath>
#include <cfloat>
#include <vector>

#include "ba_problem.hpp"
#include "ba_linesearch.hpp"
#include "ba_sparse_plan.hpp"

using esfm::BADev;

namespace esfm {

constexpr size_t kArenaChunk = size_t(4) << 20;
int ba_dev_alloc_bytes(esfm_ba_problem *p, void **out, size_t array_bytes)
{
    const size_t bytes = (std::max<size_t>(array_bytes, 1) + 255) / 256 * 256 + 256;
    if (bytes > p->arena_left) {
        void *ptr = nullptr;
        size_t chunk = std::max(bytes, kArenaChunk);
        // a chunk the context kept from a destroyed problem, the smallest that fits (esfm_ba_problem_destroy synchronised the stream
        // before it handed the chunk over)
        auto &pool = p->ctx->ba_chunks;
        int best = -1;
        for (int i = 0; i < (int)pool.size(); ++i)
            if (pool[(size_t)i].bytes >= bytes && (best < 0 || pool[(size_t)i].bytes < pool[(size_t)best].bytes)) best = i;
        if (best >= 0) {
            ptr = pool[(size_t)best].ptr; chunk = pool[(size_t)best].bytes;
            pool.erase(pool.begin() + best);
        } else {
            hipError_t e = hipMalloc(&ptr, chunk);
            if (e != hipSuccess) {
                esfm::set_error("hipMalloc(%zu) failed: %s", chunk, hipGetErrorString(e));
                return e == hipErrorOutOfMemory ? ESFM_ERR_OOM : ESFM_ERR_HIP;
            }
        }
        p->allocs.push_back({ptr, chunk});
        p->arena_cur = static_cast<char *>(ptr);
        p->arena_left = chunk;
    }
    *out = p->arena_cur;
    p->arena_cur += bytes;
    p->arena_left -= bytes;
    return ESFM_OK;
}

void ba_options_default(esfm_ba_options *o)
{
    o->max_num_iterations = 50;  // ba.cpp:202
    o->jacobi_scaling = 1;
    o->max_num_consecutive_invalid_steps = 5;
    o->verbose = 0;
    o->cauchy_a = 0.5;  // ba.cpp:150
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
}

}  // namespace esfm

namespace {

// The free intrinsics blocks of a problem: n == 0 fixed intrinsics; else n blocks fx, cx, fy, cy (calib4: 4 n doubles), block g boxed
// to calib4 +- tol[g] and used by the cameras with group_of_cam[c] == g (NULL: every camera uses block 0).
struct CalibGroups {
    int n = 0;
    const int32_t *group_of_cam = nullptr;
    const double *calib4 = nullptr;
    const double *tol = nullptr;
    const double *radial2 = nullptr;      // radial problems: k1, k2 per block (2 n doubles) boxed to radial2 +- radial_tol[g]; else NULL
    const double *radial_tol = nullptr;
    bool checked = false;      // the grouped entry points validate these arrays before anything else (checked_groups)
};

int check_create_args(esfm_ctx *ctx, int n_real, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                      const float *K4_per_cam, const CalibGroups &cg, const double *cams, const double *pts, esfm_ba_problem **out)
{
    if (!ctx || !out) { esfm::set_error("ctx/out is NULL"); return ESFM_ERR_INVALID_ARG; }
    *out = nullptr;
    ESFM_REQUIRE(n_real >= 0 && n_pt >= 0 && n_obs >= 0, "negative size");
    ESFM_REQUIRE(n_obs == 0 || (cam_idx && pt_idx && obs_uv), "observation arrays are NULL");
    ESFM_REQUIRE(n_real == 0 || ((K4_per_cam || cg.n) && cams), "camera arrays are NULL");
    ESFM_REQUIRE(n_pt == 0 || pts, "pts is NULL");
    // Ceres rejects a variable block whose lower bound is not below its upper bound (Program::IsFeasible)
    // (the one shared block of the older entry points: its place among their checks, and their codes -- a NaN tolerance is "not
    // positive" there; the grouped entry points have validated theirs already)
    if (!cg.checked) {
        ESFM_REQUIRE(cg.n == 0 || cg.tol[0] > 0.0, "intrinsics tolerance must be positive");
        for (int i = 0; i < 4 * cg.n; ++i) if (!std::isfinite(cg.calib4[i])) { esfm::set_error("non-finite intrinsics"); return ESFM_ERR_NUMERIC; }
    }
    const int64_t n_cam = (int64_t)n_real + cg.n;   // 6-wide blocks of the reduced system
    ESFM_REQUIRE(6 * n_cam < 46000, "reduced system too large for this build (6 n_cam < 46000)");
    for (int k = 0; k < n_obs; ++k)
        ESFM_REQUIRE(cam_idx[k] >= 0 && cam_idx[k] < n_real && pt_idx[k] >= 0 && pt_idx[k] < n_pt, "observation index out of range");
    for (size_t i = 0; i < (size_t)6 * n_real; ++i) if (!std::isfinite(cams[i])) { esfm::set_error("non-finite camera parameter"); return ESFM_ERR_NUMERIC; }
    for (size_t i = 0; i < (size_t)3 * n_pt; ++i) if (!std::isfinite(pts[i])) { esfm::set_error("non-finite point parameter"); return ESFM_ERR_NUMERIC; }
    return ESFM_OK;
}

// cg.n == 0: fixed per-camera intrinsics K4_per_cam; else the free blocks fx, cx, fy, cy -- the one shared block or one per camera
// group -- carried as cg.n more 6-wide camera-side blocks behind the n_real cameras (ba_kernels.hpp).
int create_impl(esfm_ctx *ctx, int n_real, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx,
                const float *obs_uv, const float *K4_per_cam, const CalibGroups &cg, const double *cams,
                const double *pts, esfm_ba_problem **out)
{
    if (int rc = check_create_args(ctx, n_real, n_pt, n_obs, cam_idx, pt_idx, obs_uv, K4_per_cam, cg, cams, pts, out)) return rc;
    if (int rc = esfm::set_device(ctx)) return rc;
    const bool calib = cg.n > 0;
    const int n_cam = n_real + cg.n;   // 6-wide blocks of the reduced system
    const bool radial = calib && cg.radial2;
    const esfm::BaForms forms = esfm::ba_forms(n_real, calib, n_obs, calib ? cg.n : 1, radial);
    const esfm::BaLayout L = esfm::make_ba_layout(n_real, n_pt, n_obs, cam_idx, pt_idx, ctx->num_cu, forms.schur == esfm::BaForms::SCHUR_TABLES);
    std::vector<float> s_uv((size_t)2 * n_obs);
    for (size_t t = 0; t < (size_t)n_obs; ++t) {
        const size_t k = (size_t)L.order[t];
        s_uv[2 * t] = obs_uv[2 * k]; s_uv[2 * t + 1] = obs_uv[2 * k + 1];
    }

    auto P = new esfm_ba_problem();
    P->ctx = ctx;
    P->parts.forms = forms;
    P->cam_nobs_local.assign((size_t)n_cam, 0.0);
    for (int c = 0; c < n_real; ++c) P->cam_nobs_local[(size_t)c] = (double)L.cam_nobs[(size_t)c];
    if (calib) {
        // every observation involves the intrinsics block of its camera's group
        if (cg.n == 1 && !radial) P->cam_nobs_local[(size_t)n_real] = (double)n_obs;
        else for (int c = 0; c < n_real; ++c) P->cam_nobs_local[(size_t)n_real + cg.group_of_cam[c]] += (double)L.cam_nobs[(size_t)c];
        P->calib_center.assign(cg.calib4, cg.calib4 + 4 * (size_t)cg.n);
        P->calib_tol.assign(cg.tol, cg.tol + cg.n);
        if (radial) { P->radial_center.assign(cg.radial2, cg.radial2 + 2 * (size_t)cg.n); P->radial_tol.assign(cg.radial_tol, cg.radial_tol + cg.n); }
    }
    if (!calib && forms.solve == esfm::BaForms::SOLVE_TILED) { P->h_pt_start = L.pt_start; P->h_obs_cam = L.cam; }   // (for the reduced system's structure)
    BADev &d = P->d;
    d.n_cam = n_cam; d.n_pt = n_pt; d.n_obs = n_obs;
    d.n_real_cam = n_real; d.has_calib = cg.n; d.radial = radial ? 1 : 0;
    d.parts = &P->parts;
    d.n_cchunks = (int)L.cchunk_cam.size();
    for (int tb = 0; tb < 2; ++tb) d.n_mchunks[tb] = (int)L.mchunk_cam0[tb].size();
    d.n_chunks = (int)L.chunk_cam0.size(); d.n_chunks_b = (int)L.chunk_cam0_b.size();
    d.n_wide_obs = (int)L.wide_obs.size();
    d.n_pchunks = (int)L.pchunk_pt0.size() - 1;

    // every array with a host image, once: where it goes, what goes there (NULL: filled later), how many bytes
    struct Table { void **dev; const void *src; size_t bytes; };
    std::vector<Table> tables;
    auto table = [&](auto **dev, const auto *src, size_t count) { tables.push_back({reinterpret_cast<void **>(dev), src, sizeof(*src) * count}); };
    auto index_table = [&](int32_t **dev, const std::vector<int32_t> &v) { table(dev, v.data(), v.size()); };
    index_table(&d.obs_cam, L.cam); index_table(&d.obs_pt, L.pt);
    table(&d.obs_uv, s_uv.data(), s_uv.size());
    index_table(&d.pt_start, L.pt_start);
    table(&d.K4, calib ? (const float *)nullptr : K4_per_cam, 4 * (size_t)n_real);
    index_table(&d.cam_obs, L.cam_obs); index_table(&d.cchunk_cam, L.cchunk_cam); index_table(&d.cchunk_beg, L.cchunk_beg);
    index_table(&d.cchunk_end, L.cchunk_end); index_table(&d.cam_chunk0, L.cam_chunk0);
    for (int tb = 0; tb < 2; ++tb) {
        index_table(&d.mslot_pc[tb], L.mslot_pc[tb]); index_table(&d.mslot_obs[tb], L.mslot_obs[tb]); index_table(&d.mbatch_slot[tb], L.mbatch_slot[tb]);
        index_table(&d.mchunk_batch0[tb], L.mchunk_batch0[tb]); index_table(&d.mchunk_cam0[tb], L.mchunk_cam0[tb]);
    }
    index_table(&d.slot_obs, L.slot_obs); index_table(&d.chunk_slot, L.chunk_slot); index_table(&d.chunk_cam0, L.chunk_cam0);
    index_table(&d.slot_obs_b, L.slot_obs_b); index_table(&d.chunk_slot_b, L.chunk_slot_b); index_table(&d.chunk_cam0_b, L.chunk_cam0_b);
    index_table(&d.wide_obs, L.wide_obs);
    index_table(&d.pchunk_pt0, L.pchunk_pt0);
    table(&d.pchunk_info, L.pchunk_info.data(), L.pchunk_info.size());
    if (cg.n > 1 || radial) table(&d.cam_group, cg.group_of_cam, (size_t)n_real);

    // the tables first, then the work arrays (an empty table takes one padded slot of the arena like any other array)
    const size_t no = (size_t)n_obs, nc6 = (size_t)6 * n_cam, np3 = (size_t)3 * n_pt;
    int rc = ESFM_OK;
    for (const Table &t : tables) if (rc == ESFM_OK) rc = esfm::ba_dev_alloc_bytes(P, t.dev, t.bytes);
    auto A = [&](auto **ptr, size_t count) { if (rc == ESFM_OK) rc = esfm::ba_dev_alloc(P, ptr, count); };
    if (calib) A(&d.Jk, (radial ? 8 : 4) * no);
    A(&d.lo_c, nc6); A(&d.up_c, nc6); A(&d.delta_c, nc6); A(&d.delta_p, np3);
    A(&d.cam_nobs, (size_t)n_cam);
    A(&d.x_c, nc6); A(&d.x_p, np3); A(&d.cand_c, nc6); A(&d.cand_p, np3); A(&d.x0_p, np3);
    A(&d.Jc, 12 * no); A(&d.Jp, 6 * no); A(&d.res, 2 * no);
    A(&d.scale_c, nc6); A(&d.scale_p, np3);
    A(&d.EtE, (size_t)6 * n_pt); A(&d.Etr, np3); A(&d.Minv, (size_t)6 * n_pt); A(&d.Aig, np3);
    A(&d.camacc, esfm::ba_camacc_doubles(n_cam)); A(&d.red, esfm::ba_red_doubles(n_cam));
    A(&d.y_c, nc6); A(&d.scal, (size_t)esfm::SC_COUNT);
    // (the tiled solve's work space; the in-LDS solves take none, the packed matrix is not read on those paths)
    A(&d.chol, forms.solve == esfm::BaForms::SOLVE_TILED ? esfm::ba_chol_large_doubles(n_cam) : (nc6 + 1) * (nc6 + 2) / 2 + 2);
    if (forms.schur == esfm::BaForms::SCHUR_LDS_SLABS) d.slab_cap = esfm::ba_schur_slab_doubles(n_cam) * (size_t)ctx->num_cu;
    if (d.slab_cap) A(&d.slabs, d.slab_cap);
    if (forms.sweep_sums_in_lds) {
        d.lin_slab_cap = esfm::ba_lin_slab_doubles(n_cam) * 2 * (size_t)ctx->num_cu;
        A(&d.lin_slabs, d.lin_slab_cap);
    }
    A(&d.cam_part, L.cchunk_cam.size() * (size_t)esfm::kCamPart);
    if (radial) A(&d.cam_part_k, L.cchunk_cam.size() * (size_t)esfm::kRadialPart);
    // room for a few launches' partials per slot between two read-backs (a full slot is flushed by an extra reduce launch)
    d.scal_cap = std::max(1 << 12, 4 * (std::max((n_pt + 63) / 64, (n_obs + 255) / 256) + n_pt / 256 + 2));
    A(&d.scal_part, (size_t)esfm::SC_SUM_COUNT * (size_t)d.scal_cap);
    A(&d.qexp, nc6);
    if (rc != ESFM_OK) { esfm_ba_problem_destroy(P); return rc; }

    hipStream_t st = ctx->stream;
    auto up = [&](void *dst, const void *src, size_t bytes) {
        if (rc == ESFM_OK && src && bytes) {
            hipError_t e = esfm::copy_h2d(dst, src, bytes, st);
            if (e != hipSuccess) { esfm::set_error("hipMemcpyAsync H2D failed: %s", hipGetErrorString(e)); rc = ESFM_ERR_HIP; }
        }
    };
    for (const Table &t : tables) up(*t.dev, t.src, t.bytes);
    std::vector<double> calib_blocks(6 * (size_t)cg.n, 0.0);      // four unknowns and two padding unknowns per block
    for (int g = 0; g < cg.n; ++g) for (int i = 0; i < 4; ++i) calib_blocks[6 * (size_t)g + i] = cg.calib4[4 * (size_t)g + i];
    for (int g = 0; g < cg.n && radial; ++g) for (int i = 0; i < 2; ++i) calib_blocks[6 * (size_t)g + 4 + i] = cg.radial2[2 * (size_t)g + i];
    if (calib) up(d.x_c + 6 * (size_t)n_real, calib_blocks.data(), sizeof(double) * calib_blocks.size());
    up(d.x_c, cams, sizeof(double) * 6 * (size_t)n_real); up(d.x_p, pts, sizeof(double) * np3);
    // red: the entries no kernel ever writes (blocks above the diagonal) must read as zero
    if (rc == ESFM_OK && hipMemsetAsync(d.red, 0, sizeof(double) * esfm::ba_red_doubles(n_cam), st) != hipSuccess) { esfm::set_error("memset failed"); rc = ESFM_ERR_HIP; }
    if (rc == ESFM_OK && hipStreamSynchronize(st) != hipSuccess) { esfm::set_error("stream sync failed"); rc = ESFM_ERR_HIP; }
    if (rc != ESFM_OK) { esfm_ba_problem_destroy(P); return rc; }
    *out = P;
    return ESFM_OK;
}

CalibGroups one_block(const double *calib4, const double *tol)
{
    CalibGroups cg;
    cg.n = 1; cg.calib4 = calib4; cg.tol = tol;
    return cg;
}

// the group arguments of the grouped entry points, checked before anything else is looked at (nothing is written on failure)
int checked_groups(int n_real, int n_groups, const int32_t *group_of_cam, const double *calib4, const double *tol, esfm_ba_problem **out, CalibGroups &cg)
{
    if (out) *out = nullptr;
    ESFM_REQUIRE(n_groups >= 1, "n_groups must be at least 1");
    ESFM_REQUIRE(calib4 && tol, "calib4 / calib_tolerance is NULL");
    ESFM_REQUIRE(n_real <= 0 || group_of_cam, "group_of_cam is NULL");
    ESFM_REQUIRE((int64_t)6 * ((int64_t)std::max(n_real, 0) + n_groups) < 46000, "reduced system too large for this build (6 (n_cam + n_groups) < 46000)");
    for (int g = 0; g < n_groups; ++g) {
        if (tol[g] != tol[g] || std::isinf(tol[g])) { esfm::set_error("non-finite intrinsics tolerance"); return ESFM_ERR_NUMERIC; }
        ESFM_REQUIRE(tol[g] > 0.0, "intrinsics tolerance must be positive");
    }
    for (int i = 0; i < 4 * n_groups; ++i) if (!std::isfinite(calib4[i])) { esfm::set_error("non-finite intrinsics"); return ESFM_ERR_NUMERIC; }
    for (int c = 0; c < n_real; ++c) ESFM_REQUIRE(group_of_cam[c] >= 0 && group_of_cam[c] < n_groups, "camera group index out of range");
    cg.n = n_groups; cg.group_of_cam = group_of_cam; cg.calib4 = calib4; cg.tol = tol; cg.checked = true;
    return ESFM_OK;
}

// the radial arguments of the radial entry points, checked like the group arguments and right behind them
int checked_radial(int n_groups, const double *radial2, const double *radial_tol, CalibGroups &cg)
{
    ESFM_REQUIRE(radial2 && radial_tol, "radial2 / radial_tolerance is NULL");
    for (int g = 0; g < n_groups; ++g) {
        if (radial_tol[g] != radial_tol[g] || std::isinf(radial_tol[g])) { esfm::set_error("non-finite radial tolerance"); return ESFM_ERR_NUMERIC; }
        ESFM_REQUIRE(radial_tol[g] > 0.0, "radial tolerance must be positive");
    }
    for (int i = 0; i < 2 * n_groups; ++i) if (!std::isfinite(radial2[i])) { esfm::set_error("non-finite radial coefficient"); return ESFM_ERR_NUMERIC; }
    cg.radial2 = radial2; cg.radial_tol = radial_tol;
    return ESFM_OK;
}

}  // namespace

extern "C" {

void esfm_ba_options_default(esfm_ba_options *opt) { if (opt) esfm::ba_options_default(opt); }

int esfm_ba_problem_create(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx,
                           const float *obs_uv, const float *K4_per_cam, const double *cams, const double *pts,
                           esfm_ba_problem **out)
{
    if (n_cam > 0 && !K4_per_cam) { esfm::set_error("K4_per_cam is NULL"); return ESFM_ERR_INVALID_ARG; }
    return create_impl(ctx, n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, K4_per_cam, CalibGroups(), cams, pts, out);
}

int esfm_ba_problem_create_free_calib(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx,
                                      const float *obs_uv, const double *calib4, double calib_tolerance, const double *cams,
                                      const double *pts, esfm_ba_problem **out)
{
    if (!calib4) { esfm::set_error("calib4 is NULL"); return ESFM_ERR_INVALID_ARG; }
    return create_impl(ctx, n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, nullptr, one_block(calib4, &calib_tolerance), cams, pts, out);
}

int esfm_ba_problem_create_calib_groups(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx,
                                        const float *obs_uv, int n_groups, const int32_t *group_of_cam, const double *calib4,
                                        const double *calib_tolerance, const double *cams, const double *pts, esfm_ba_problem **out)
{
    CalibGroups cg;
    if (int rc = checked_groups(n_cam, n_groups, group_of_cam, calib4, calib_tolerance, out, cg)) return rc;
    return create_impl(ctx, n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, nullptr, cg, cams, pts, out);
}

int esfm_ba_problem_calib_groups(const esfm_ba_problem *P) { return P ? P->d.has_calib : 0; }

int esfm_ba_problem_create_radial_groups(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx,
                                         const float *obs_uv, int n_groups, const int32_t *group_of_cam, const double *calib4,
                                         const double *calib_tolerance, const double *radial2, const double *radial_tolerance,
                                         const double *cams, const double *pts, esfm_ba_problem **out)
{
    CalibGroups cg;
    if (int rc = checked_groups(n_cam, n_groups, group_of_cam, calib4, calib_tolerance, out, cg)) return rc;
    if (int rc = checked_radial(n_groups, radial2, radial_tolerance, cg)) return rc;
    return create_impl(ctx, n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, nullptr, cg, cams, pts, out);
}

int esfm_ba_problem_radial_groups(const esfm_ba_problem *P) { return P && P->d.radial ? P->d.has_calib : 0; }

int esfm_ba_problem_set_radial_groups(esfm_ba_problem *P, const double *radial2, const double *radial_tolerance)
{
    if (!P || !radial2 || !radial_tolerance) { esfm::set_error("NULL argument"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(P->d.radial, "problem was created without free radial distortion");
    const int G = P->d.has_calib;
    CalibGroups cg;
    if (int rc = checked_radial(G, radial2, radial_tolerance, cg)) return rc;
    if (int rc = esfm::set_device(P->ctx)) return rc;
    P->radial_center.assign(radial2, radial2 + 2 * (size_t)G);
    P->radial_tol.assign(radial_tolerance, radial_tolerance + G);
    // slots 4 and 5 of every block; the four pinhole values in front of them stay as they are
    std::vector<double> blocks(6 * (size_t)G);
    ESFM_HIP_TRY(esfm::copy_d2h(blocks.data(), P->d.x_c + 6 * (size_t)P->d.n_real_cam, sizeof(double) * blocks.size(), P->ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(P->ctx->stream));
    for (int g = 0; g < G; ++g) for (int i = 0; i < 2; ++i) blocks[6 * (size_t)g + 4 + i] = radial2[2 * (size_t)g + i];
    ESFM_HIP_TRY(esfm::copy_h2d(P->d.x_c + 6 * (size_t)P->d.n_real_cam, blocks.data(), sizeof(double) * blocks.size(), P->ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(P->ctx->stream));
    return ESFM_OK;
}

int esfm_ba_problem_get_radial_groups(esfm_ba_problem *P, double *radial2)
{
    if (!P || !radial2) { esfm::set_error("NULL argument"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(P->d.radial, "problem was created without free radial distortion");
    if (int rc = esfm::set_device(P->ctx)) return rc;
    const int G = P->d.has_calib;
    std::vector<double> blocks(6 * (size_t)G);
    ESFM_HIP_TRY(esfm::copy_d2h(blocks.data(), P->d.x_c + 6 * (size_t)P->d.n_real_cam, sizeof(double) * blocks.size(), P->ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(P->ctx->stream));
    for (int g = 0; g < G; ++g) for (int i = 0; i < 2; ++i) radial2[2 * (size_t)g + i] = blocks[6 * (size_t)g + 4 + i];
    return ESFM_OK;
}

int esfm_ba_problem_set_calib_groups(esfm_ba_problem *P, const double *calib4, const double *calib_tolerance)
{
    if (!P || !calib4 || !calib_tolerance) { esfm::set_error("NULL argument"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(P->d.has_calib, "problem was created with fixed intrinsics");
    const int G = P->d.has_calib;
    for (int g = 0; g < G; ++g) ESFM_REQUIRE(calib_tolerance[g] > 0.0 && std::isfinite(calib_tolerance[g]), "intrinsics tolerance must be positive and finite");
    for (int i = 0; i < 4 * G; ++i) if (!std::isfinite(calib4[i])) { esfm::set_error("non-finite intrinsics"); return ESFM_ERR_NUMERIC; }
    if (int rc = esfm::set_device(P->ctx)) return rc;
    P->calib_center.assign(calib4, calib4 + 4 * (size_t)G);
    P->calib_tol.assign(calib_tolerance, calib_tolerance + G);
    std::vector<double> blocks(6 * (size_t)G, 0.0);
    // (a radial problem: k1, k2 in slots 4 and 5 stay as they are)
    if (P->d.radial) {
        ESFM_HIP_TRY(esfm::copy_d2h(blocks.data(), P->d.x_c + 6 * (size_t)P->d.n_real_cam, sizeof(double) * blocks.size(), P->ctx->stream));
        ESFM_HIP_TRY(hipStreamSynchronize(P->ctx->stream));
    }
    for (int g = 0; g < G; ++g) for (int i = 0; i < 4; ++i) blocks[6 * (size_t)g + i] = calib4[4 * (size_t)g + i];
    ESFM_HIP_TRY(esfm::copy_h2d(P->d.x_c + 6 * (size_t)P->d.n_real_cam, blocks.data(), sizeof(double) * blocks.size(), P->ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(P->ctx->stream));
    return ESFM_OK;
}

int esfm_ba_problem_get_calib_groups(esfm_ba_problem *P, double *calib4)
{
    if (!P || !calib4) { esfm::set_error("NULL argument"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(P->d.has_calib, "problem was created with fixed intrinsics");
    if (int rc = esfm::set_device(P->ctx)) return rc;
    const int G = P->d.has_calib;
    std::vector<double> blocks(6 * (size_t)G);
    ESFM_HIP_TRY(esfm::copy_d2h(blocks.data(), P->d.x_c + 6 * (size_t)P->d.n_real_cam, sizeof(double) * blocks.size(), P->ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(P->ctx->stream));
    for (int g = 0; g < G; ++g) for (int i = 0; i < 4; ++i) calib4[4 * (size_t)g + i] = blocks[6 * (size_t)g + i];
    return ESFM_OK;
}

int esfm_ba_problem_set_calib(esfm_ba_problem *P, const double *calib4, double calib_tolerance)
{
    if (!P || !calib4) { esfm::set_error("NULL argument"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(P->d.has_calib, "problem was created with fixed intrinsics");
    ESFM_REQUIRE(P->d.has_calib == 1 && !P->d.radial, "problem has several intrinsics blocks or a radial one: use esfm_ba_problem_set_calib_groups");
    ESFM_REQUIRE(calib_tolerance > 0.0, "intrinsics tolerance must be positive");
    for (int i = 0; i < 4; ++i) if (!std::isfinite(calib4[i])) { esfm::set_error("non-finite intrinsics"); return ESFM_ERR_NUMERIC; }
    if (int rc = esfm::set_device(P->ctx)) return rc;
    P->calib_center.assign(calib4, calib4 + 4);
    P->calib_tol.assign(1, calib_tolerance);
    ESFM_HIP_TRY(esfm::copy_h2d(P->d.x_c + 6 * (size_t)P->d.n_real_cam, calib4, sizeof(double) * 4, P->ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(P->ctx->stream));
    return ESFM_OK;
}

int esfm_ba_problem_get_calib(esfm_ba_problem *P, double *calib4)
{
    if (!P || !calib4) { esfm::set_error("NULL argument"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(P->d.has_calib, "problem was created with fixed intrinsics");
    ESFM_REQUIRE(P->d.has_calib == 1 && !P->d.radial, "problem has several intrinsics blocks or a radial one: use esfm_ba_problem_get_calib_groups");
    if (int rc = esfm::set_device(P->ctx)) return rc;
    ESFM_HIP_TRY(esfm::copy_d2h(calib4, P->d.x_c + 6 * (size_t)P->d.n_real_cam, sizeof(double) * 4, P->ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(P->ctx->stream));
    return ESFM_OK;
}

int esfm_ba_problem_fix_camera(esfm_ba_problem *P, int cam, double threshold)
{
    if (!P) { esfm::set_error("problem is NULL"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(cam < P->d.n_real_cam, "camera index out of range");
    ESFM_REQUIRE(cam < 0 || threshold > 0.0, "threshold must be positive");
    P->ref_cam = cam < 0 ? -1 : cam;
    P->ref_threshold = cam < 0 ? 0.0 : threshold;
    return ESFM_OK;
}

double esfm_ba_line_search_next_step(double f0, double g0, double x_prev, double f_prev, double g_prev, int prev_valid,
                                     double x_cur, double f_cur, double g_cur, int cur_valid)
{
    namespace ls = esfm::linesearch;
    ls::Sample ini, prev, cur;
    ini.x = 0.0; ini.f = f0; ini.g = g0; ini.valid = true;
    prev.x = x_prev; prev.f = f_prev; prev.g = g_prev; prev.valid = prev_valid != 0;
    cur.x = x_cur; cur.f = f_cur; cur.g = g_cur; cur.valid = cur_valid != 0;
    return ls::next_step(ini, prev, cur);
}

int esfm_ba_problem_set_params(esfm_ba_problem *P, const double *cams, const double *pts)
{
    if (!P || (!cams && P->d.n_real_cam) || (!pts && P->d.n_pt)) { esfm::set_error("NULL argument"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(P->ctx)) return rc;
    hipStream_t st = P->ctx->stream;
    if (P->d.n_real_cam) ESFM_HIP_TRY(esfm::copy_h2d(P->d.x_c, cams, sizeof(double) * 6 * (size_t)P->d.n_real_cam, st));
    if (P->d.n_pt) ESFM_HIP_TRY(esfm::copy_h2d(P->d.x_p, pts, sizeof(double) * 3 * (size_t)P->d.n_pt, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

int esfm_ba_problem_get_params(esfm_ba_problem *P, double *cams, double *pts)
{
    if (!P || (!cams && P->d.n_real_cam) || (!pts && P->d.n_pt)) { esfm::set_error("NULL argument"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(P->ctx)) return rc;
    hipStream_t st = P->ctx->stream;
    if (P->d.n_real_cam) ESFM_HIP_TRY(esfm::copy_d2h(cams, P->d.x_c, sizeof(double) * 6 * (size_t)P->d.n_real_cam, st));
    if (P->d.n_pt) ESFM_HIP_TRY(esfm::copy_d2h(pts, P->d.x_p, sizeof(double) * 3 * (size_t)P->d.n_pt, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

int esfm_ba_problem_destroy(esfm_ba_problem *P)
{
    if (!P) return ESFM_OK;
    if (P->ctx) { (void)hipSetDevice(P->ctx->device); (void)hipStreamSynchronize(P->ctx->stream); }
    // small chunks and the mailbox stay with the context for its next problem (at most kKeepChunks chunks of at most kKeepBytes)
    constexpr size_t kKeepChunks = 6, kKeepBytes = size_t(64) << 20;
    for (const auto &c : P->allocs) {
        if (P->ctx && c.bytes <= kKeepBytes && P->ctx->ba_chunks.size() < kKeepChunks) P->ctx->ba_chunks.push_back(c);
        else (void)hipFree(c.ptr);
    }
    esfm::ba_sparse_destroy(P->sparse);
    if (P->h_scal) {
        if (P->ctx && P->ctx->ba_mailboxes.size() < 2) P->ctx->ba_mailboxes.push_back(P->h_scal);
        else (void)hipHostFree(P->h_scal);
    }
    delete P;
    return ESFM_OK;
}

int esfm_ba_problem_cost(esfm_ba_problem *P, double cauchy_a, double *cost)
{
    if (!P || !cost) { esfm::set_error("NULL argument"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(P->ctx)) return rc;
    hipStream_t st = P->ctx->stream;
    ESFM_HIP_TRY(hipMemsetAsync(P->d.scal, 0, sizeof(double) * esfm::SC_COUNT, st));
    esfm::ba_scal_discard(P->d, 0, esfm::SC_SUM_COUNT);
    if (int rc = esfm::ba_cost(st, P->d, P->ctx->num_cu, P->d.x_c, P->d.x_p, cauchy_a, esfm::SC_CAND_COST, esfm::SC_CAND_BAD)) return rc;
    if (int rc = esfm::ba_scal_reduce(st, P->d)) return rc;
    double h[esfm::SC_COUNT];
    ESFM_HIP_TRY(esfm::copy_d2h(h, P->d.scal, sizeof(h), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    *cost = h[esfm::SC_CAND_BAD] > 0.0 ? DBL_MAX : h[esfm::SC_CAND_COST];
    return ESFM_OK;
}

int esfm_ba_solve(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                  const float *K4_per_cam, double *cams, double *pts, const esfm_ba_options *options, esfm_allreduce_fn allreduce,
                  void *allreduce_user, esfm_ba_summary *summary)
{
    esfm_ba_problem *P = nullptr;
    if (int rc = esfm_ba_problem_create(ctx, n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, K4_per_cam, cams, pts, &P)) return rc;
    int rc = esfm_ba_problem_solve(P, options, allreduce, allreduce_user, summary);
    if (rc == ESFM_OK || rc == ESFM_ERR_NUMERIC) {
        const int rc2 = esfm_ba_problem_get_params(P, cams, pts);
        if (rc == ESFM_OK) rc = rc2;
    }
    esfm_ba_problem_destroy(P);
    return rc;
}

int esfm_ba_solve_ex(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                     const float *K4_per_cam, double *cams, double *pts, double *calib4, double calib_tolerance, int ref_cam,
                     double ref_threshold, const esfm_ba_options *options, esfm_allreduce_fn allreduce, void *allreduce_user,
                     esfm_ba_summary *summary)
{
    esfm_ba_problem *P = nullptr;
    if (int rc = create_impl(ctx, n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, K4_per_cam, calib4 ? one_block(calib4, &calib_tolerance) : CalibGroups(), cams, pts,
                             &P)) return rc;
    int rc = esfm_ba_problem_fix_camera(P, ref_cam, ref_threshold);
    if (rc == ESFM_OK) rc = esfm_ba_problem_solve(P, options, allreduce, allreduce_user, summary);
    if (rc == ESFM_OK || rc == ESFM_ERR_NUMERIC) {
        int rc2 = esfm_ba_problem_get_params(P, cams, pts);
        if (rc2 == ESFM_OK && calib4) rc2 = esfm_ba_problem_get_calib(P, calib4);
        if (rc == ESFM_OK) rc = rc2;
    }
    esfm_ba_problem_destroy(P);
    return rc;
}

int esfm_ba_solve_groups(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                         double *cams, double *pts, int n_groups, const int32_t *group_of_cam, double *calib4, const double *calib_tolerance,
                         int ref_cam, double ref_threshold, const esfm_ba_options *options, esfm_allreduce_fn allreduce, void *allreduce_user,
                         esfm_ba_summary *summary)
{
    esfm_ba_problem *P = nullptr;
    if (int rc = esfm_ba_problem_create_calib_groups(ctx, n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, n_groups, group_of_cam, calib4, calib_tolerance,
                                                     cams, pts, &P)) return rc;
    int rc = esfm_ba_problem_fix_camera(P, ref_cam, ref_threshold);
    if (rc == ESFM_OK) rc = esfm_ba_problem_solve(P, options, allreduce, allreduce_user, summary);
    if (rc == ESFM_OK || rc == ESFM_ERR_NUMERIC) {
        int rc2 = esfm_ba_problem_get_params(P, cams, pts);
        if (rc2 == ESFM_OK) rc2 = esfm_ba_problem_get_calib_groups(P, calib4);
        if (rc == ESFM_OK) rc = rc2;
    }
    esfm_ba_problem_destroy(P);
    return rc;
}

int esfm_ba_solve_radial_groups(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                                double *cams, double *pts, int n_groups, const int32_t *group_of_cam, double *calib4, const double *calib_tolerance,
                                double *radial2, const double *radial_tolerance, int ref_cam, double ref_threshold, const esfm_ba_options *options,
                                esfm_allreduce_fn allreduce, void *allreduce_user, esfm_ba_summary *summary)
{
    esfm_ba_problem *P = nullptr;
    if (int rc = esfm_ba_problem_create_radial_groups(ctx, n_cam, n_pt, n_obs, cam_idx, pt_idx, obs_uv, n_groups, group_of_cam, calib4, calib_tolerance,
                                                      radial2, radial_tolerance, cams, pts, &P)) return rc;
    int rc = esfm_ba_problem_fix_camera(P, ref_cam, ref_threshold);
    if (rc == ESFM_OK) rc = esfm_ba_problem_solve(P, options, allreduce, allreduce_user, summary);
    if (rc == ESFM_OK || rc == ESFM_ERR_NUMERIC) {
        int rc2 = esfm_ba_problem_get_params(P, cams, pts);
        if (rc2 == ESFM_OK) rc2 = esfm_ba_problem_get_calib_groups(P, calib4);
        if (rc2 == ESFM_OK) rc2 = esfm_ba_problem_get_radial_groups(P, radial2);
        if (rc == ESFM_OK) rc = rc2;
    }
    esfm_ba_problem_destroy(P);
    return rc;
}

// Greedy balance of observation counts over shards, points in index order.
int esfm_ba_shard_points(int n_pt, int n_obs, const int32_t *pt_idx, int world, int32_t *shard_of_point)
{
    if (n_pt < 0 || n_obs < 0 || world < 1 || (n_obs && !pt_idx) || (n_pt && !shard_of_point)) {
        esfm::set_error("esfm_ba_shard_points: bad arguments");
        return ESFM_ERR_INVALID_ARG;
    }
    std::vector<int64_t> cnt((size_t)n_pt, 0);
    for (int k = 0; k < n_obs; ++k) {
        if (pt_idx[k] < 0 || pt_idx[k] >= n_pt) { esfm::set_error("point index out of range"); return ESFM_ERR_INVALID_ARG; }
        cnt[(size_t)pt_idx[k]]++;
    }
    // contiguous ranges with ~n_obs/world observations each: keeps a shard's points (and their
    // observations, which are sorted by point on the device) contiguous
    const double target = world > 0 ? (double)n_obs / world : 0.0;
    int shard = 0;
    int64_t acc = 0;
    for (int p = 0; p < n_pt; ++p) {
        if (shard < world - 1 && (double)acc >= target * (shard + 1)) ++shard;
        shard_of_point[p] = shard;
        acc += cnt[(size_t)p];
    }
    return ESFM_OK;
}

// Host-only: the structure-aware plan of the reduced camera system for this observation list (ba_sparse_plan.hpp) -- what
// esfm_ba_problem_solve builds for itself; exported for tests and tools.
int esfm_ba_reduced_plan(int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, int leaf_max,
                         int32_t *col_src, int col_cap, int32_t *tiles, int tile_cap, int32_t *info)
{
    if (n_cam < 0 || n_pt < 0 || n_obs < 0 || (n_obs && (!cam_idx || !pt_idx)) || !info || col_cap < 0 || tile_cap < 0) {
        esfm::set_error("esfm_ba_reduced_plan: bad arguments");
        return ESFM_ERR_INVALID_ARG;
    }
    for (int k = 0; k < n_obs; ++k)
        if (cam_idx[k] < 0 || cam_idx[k] >= n_cam || pt_idx[k] < 0 || pt_idx[k] >= n_pt) { esfm::set_error("observation index out of range"); return ESFM_ERR_INVALID_ARG; }
    const esfm::BaPointSort s = esfm::ba_sort_by_point(n_pt, n_obs, cam_idx, pt_idx);
    const esfm::CamGraph g = esfm::cam_graph_from_tracks(n_cam, n_pt, s.pt_start.data(), s.cam.data());
    const esfm::SparsePlan pl = esfm::make_sparse_plan(g, leaf_max > 0 ? leaf_max : 32);
    info[0] = pl.nb; info[1] = (int32_t)pl.tiles.size(); info[2] = pl.chain; info[3] = pl.dense_nb; info[4] = pl.worthwhile() ? 1 : 0;
    info[5] = (int32_t)std::min<long long>(pl.update_steps, INT32_MAX); info[6] = (int32_t)pl.node_kind.size(); info[7] = (int32_t)pl.wgs.size();
    info[8] = (int32_t)(g.adj.size() / 2 + (size_t)n_cam);       // camera blocks (a, b <= a) that can be non-zero: what several ranks exchange
    info[9] = 0;
    if ((size_t)col_cap < pl.col_src.size() || (size_t)tile_cap < pl.tiles.size()) {
        if (col_src || tiles) { esfm::set_error("esfm_ba_reduced_plan: output arrays too small (need %zu columns, %zu tiles)", pl.col_src.size(), pl.tiles.size()); return ESFM_ERR_INVALID_ARG; }
        return ESFM_OK;          // sizing call
    }
    if (col_src) for (size_t k = 0; k < pl.col_src.size(); ++k) col_src[k] = pl.col_src[k];
    if (tiles) for (size_t k = 0; k < pl.tiles.size(); ++k) { tiles[2 * k] = pl.tiles[k].I; tiles[2 * k + 1] = pl.tiles[k].J; }
    return ESFM_OK;
}

}  // extern "C"
