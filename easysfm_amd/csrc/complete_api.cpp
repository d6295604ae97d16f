// C-ABI entry points of track completion (include/esfm.h "Track completion").  The host validates the arguments and groups the
// observations by point (it holds the index arrays anyway: host pointers; a stable counting sort, so a point's observations keep
// their input order and its first max_refs are its reference rows); grid, jobs, search and claims run in complete_kernels.hip.
// esfm_track_complete_host runs complete_core.hpp over every (point, camera, keypoint) by brute force: no grid, no GPU.
#include <cmath>
#include <vector>

#include "block_scan.hpp"
#include "complete_core.hpp"
#include "complete_kernels.hpp"
#include "mesh_kernels.hpp"

namespace {

namespace cp = esfm::complete;

struct Call {
    esfm_metric metric;
    const void *desc;
    const float *kp;
    const uint8_t *kp_free;
    const int32_t *row_off;
    int n_cam, width;
    const float *K4;
    const double *Rt;
    int n_pt;
    const double *xyz;
    int n_obs;
    const int32_t *cam_idx, *pt_idx, *obs_kp;
    const esfm_track_complete_options *opt;
    int32_t *kp_point;
    float *kp_dist;
    int64_t *stats;
};

// the observations grouped by point: first[p] .. first[p + 1] index cam / row, each point's observations in input order
struct Tracks { std::vector<int32_t> first, cam, row; };

// the argument rules of all three forms; nothing is written before they have passed
int validate(const Call &c, cp::Options *o, Tracks *t, int64_t *n_rows)
{
    ESFM_REQUIRE(c.metric == ESFM_L2_F32 || c.metric == ESFM_HAMMING, "unknown metric");
    ESFM_REQUIRE(c.n_cam >= 0 && c.n_pt >= 0 && c.n_obs >= 0, "negative count");
    ESFM_REQUIRE(c.opt, "options are NULL");
    const esfm_track_complete_options &p = *c.opt;
    ESFM_REQUIRE(std::isfinite(p.search_radius_px) && p.search_radius_px > 0.0, "search_radius_px must be finite and > 0");
    ESFM_REQUIRE(p.max_distance == p.max_distance, "max_distance is NaN");
    ESFM_REQUIRE(p.ratio == p.ratio, "ratio is NaN");
    ESFM_REQUIRE(p.max_refs >= 1 && p.max_refs <= cp::kMaxRefs, "max_refs must be in 1 .. 8");
    ESFM_REQUIRE(c.width >= 1, "descriptor width must be positive");
    ESFM_REQUIRE(c.metric != ESFM_HAMMING || c.width == 16 || c.width == 32 || c.width == 64, "hamming descriptors must be 16, 32 or 64 bytes");
    ESFM_REQUIRE(c.row_off, "set_row_offset is NULL");
    ESFM_REQUIRE(c.row_off[0] == 0, "set_row_offset[0] must be 0");
    for (int i = 0; i < c.n_cam; ++i) {
        const int64_t n = (int64_t)c.row_off[i + 1] - c.row_off[i];
        ESFM_REQUIRE(n >= 0, "set_row_offset decreases");
        ESFM_REQUIRE(n < (1 << cp::kRowBits), "sets are limited to 2^21-1 rows");
    }
    *n_rows = c.row_off[c.n_cam];
    ESFM_REQUIRE(*n_rows == 0 || (c.desc && c.kp && c.kp_free && c.kp_point && c.kp_dist), "NULL keypoint, descriptor or output array");
    ESFM_REQUIRE(c.n_cam == 0 || (c.K4 && c.Rt), "NULL camera array");
    ESFM_REQUIRE(c.n_pt == 0 || c.xyz, "xyz is NULL");
    ESFM_REQUIRE(c.n_obs == 0 || (c.cam_idx && c.pt_idx && c.obs_kp), "NULL observation array");
    t->first.assign((size_t)c.n_pt + 1, 0);
    for (int i = 0; i < c.n_obs; ++i) {
        ESFM_REQUIRE(c.cam_idx[i] >= 0 && c.cam_idx[i] < c.n_cam, "cam_idx out of range");
        ESFM_REQUIRE(c.pt_idx[i] >= 0 && c.pt_idx[i] < c.n_pt, "pt_idx out of range");
        ESFM_REQUIRE(c.obs_kp[i] >= 0 && c.obs_kp[i] < c.row_off[c.cam_idx[i] + 1] - c.row_off[c.cam_idx[i]], "obs_kp out of range");
        ++t->first[(size_t)c.pt_idx[i] + 1];
    }
    if (c.n_cam >= (1 << 22) || (int64_t)c.n_pt * c.n_cam > INT32_MAX) {
        esfm::set_error("track completion takes fewer than 2^22 cameras and at most 2^31 - 1 (point, camera) combinations");
        return ESFM_ERR_UNSUPPORTED;
    }
    for (int p = 0; p < c.n_pt; ++p) t->first[(size_t)p + 1] += t->first[(size_t)p];
    t->cam.resize((size_t)c.n_obs); t->row.resize((size_t)c.n_obs);
    std::vector<int32_t> fill(t->first.begin(), t->first.end() - 1);
    for (int i = 0; i < c.n_obs; ++i) {
        const size_t at = (size_t)fill[(size_t)c.pt_idx[i]]++;
        t->cam[at] = c.cam_idx[i]; t->row[at] = c.row_off[c.cam_idx[i]] + c.obs_kp[i];
    }
    const double r = p.search_radius_px;
    o->thr2 = r * r; o->pad = 2.0 * r; o->max_distance = p.max_distance; o->ratio = p.ratio; o->max_refs = p.max_refs;
    o->whole = o->thr2 <= DBL_MAX ? 0 : 1;
    return ESFM_OK;
}

// desc / kp and the three outputs are device pointers; the rest of `c` is the caller's host memory
int run_device(esfm_ctx *ctx, const Call &c)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    cp::Options o;
    Tracks t;
    int64_t n_rows = 0;
    if (int rc = validate(c, &o, &t, &n_rows)) return rc;
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    if (n_rows == 0) {
        if (c.stats) ESFM_HIP_TRY(hipMemsetAsync(c.stats, 0, sizeof(int64_t) * 4, st));
        return ESFM_OK;
    }
    const size_t R = (size_t)n_rows, M = (size_t)c.n_cam, P1 = c.n_pt ? (size_t)c.n_pt : 1, N1 = c.n_obs ? (size_t)c.n_obs : 1;
    const int64_t combos = (int64_t)c.n_pt * c.n_cam;
    const size_t job_blocks = (size_t)esfm::blocks_of(combos) + 1;
    size_t sort_b = 0;
    if (int rc = esfm::mesh_sort_scratch_bytes(n_rows, esfm::complete_key_bits(c.n_cam), &sort_b, st)) return rc;

    esfm::ScratchCarver at;
    const size_t i_free = at.take(R), i_off = at.take(sizeof(int32_t) * (M + 1)), i_K = at.take(sizeof(float) * 4 * M),
                 i_Rt = at.take(sizeof(double) * 12 * M), i_xyz = at.take(sizeof(double) * 3 * P1), i_first = at.take(sizeof(int32_t) * (P1 + 1)),
                 i_cam = at.take(sizeof(int32_t) * N1), i_row = at.take(sizeof(int32_t) * N1);
    const size_t g_grid = at.take(sizeof(cp::CamGrid) * M), g_keys = at.take(sizeof(uint64_t) * R), g_sorted = at.take(sizeof(uint64_t) * R),
                 g_sort = at.take(sort_b), g_blocks = at.take(sizeof(int32_t) * job_blocks), g_claim = at.take(sizeof(uint64_t) * R),
                 g_count = at.take(sizeof(uint64_t) * 4);
    if (int rc = ctx->complete.reserve(at.at)) return rc;
    uint8_t *d = ctx->complete.as<uint8_t>();

    ESFM_HIP_TRY(esfm::copy_h2d(d + i_free, c.kp_free, R, st));
    ESFM_HIP_TRY(esfm::copy_h2d(d + i_off, c.row_off, sizeof(int32_t) * (M + 1), st));
    ESFM_HIP_TRY(esfm::copy_h2d(d + i_K, c.K4, sizeof(float) * 4 * M, st));
    ESFM_HIP_TRY(esfm::copy_h2d(d + i_Rt, c.Rt, sizeof(double) * 12 * M, st));
    if (c.n_pt) {
        ESFM_HIP_TRY(esfm::copy_h2d(d + i_xyz, c.xyz, sizeof(double) * 3 * (size_t)c.n_pt, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d + i_first, t.first.data(), sizeof(int32_t) * ((size_t)c.n_pt + 1), st));
    }
    if (c.n_obs) {
        ESFM_HIP_TRY(esfm::copy_h2d(d + i_cam, t.cam.data(), sizeof(int32_t) * (size_t)c.n_obs, st));
        ESFM_HIP_TRY(esfm::copy_h2d(d + i_row, t.row.data(), sizeof(int32_t) * (size_t)c.n_obs, st));
    }
    ESFM_HIP_TRY(hipMemsetAsync(d + g_claim, 0xFF, sizeof(uint64_t) * R, st));
    ESFM_HIP_TRY(hipMemsetAsync(d + g_count, 0, sizeof(uint64_t) * 4, st));

    esfm::CompleteArgs a;
    a.n_cam = c.n_cam; a.n_pt = c.n_pt; a.n_obs = c.n_obs; a.n_rows = (int32_t)n_rows; a.metric = (int32_t)c.metric; a.width = c.width; a.opt = o;
    a.desc = c.desc; a.kp = c.kp; a.kp_free = d + i_free; a.row_off = reinterpret_cast<int32_t *>(d + i_off);
    a.K4 = reinterpret_cast<float *>(d + i_K); a.Rt = reinterpret_cast<double *>(d + i_Rt); a.xyz = reinterpret_cast<double *>(d + i_xyz);
    a.pt_first = reinterpret_cast<int32_t *>(d + i_first); a.obs_cam = reinterpret_cast<int32_t *>(d + i_cam);
    a.obs_row = reinterpret_cast<int32_t *>(d + i_row);
    a.grid = reinterpret_cast<cp::CamGrid *>(d + g_grid); a.keys = reinterpret_cast<uint64_t *>(d + g_keys);
    a.sorted = reinterpret_cast<uint64_t *>(d + g_sorted); a.job_blocks = reinterpret_cast<int32_t *>(d + g_blocks); a.jobs = nullptr;
    a.claim = reinterpret_cast<unsigned long long *>(d + g_claim); a.counters = reinterpret_cast<unsigned long long *>(d + g_count);
    a.kp_point = c.kp_point; a.kp_dist = c.kp_dist; a.stats = c.stats;

    int32_t n_jobs = 0;
    if (combos > 0 && c.n_obs > 0) {
        {
            esfm::KernelTimer tm(ctx, ESFM_K_COMPLETE_GRID);
            if (int rc = esfm::launch_complete_grid(st, a, d + g_sort, sort_b)) return rc;
        }
        {
            esfm::KernelTimer tm(ctx, ESFM_K_COMPLETE_JOBS);
            if (int rc = esfm::launch_complete_job_count(st, a)) return rc;
        }
        // the one wait of the call: the job list is sized by the count (n_pt x n_cam entries would be 1.2 GB at 300 k points x 512 cameras)
        ESFM_HIP_TRY(hipMemcpyAsync(&n_jobs, a.job_blocks + (job_blocks - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
    }
    if (n_jobs > 0) {
        // (the job list gets a buffer of its own: growing the carved one would move what is already in it)
        if (int rc = ctx->stage_a.reserve(sizeof(uint64_t) * (size_t)n_jobs)) return rc;
        a.jobs = ctx->stage_a.as<uint64_t>();
        {
            esfm::KernelTimer tm(ctx, ESFM_K_COMPLETE_JOBS);
            if (int rc = esfm::launch_complete_jobs(st, a)) return rc;
        }
        esfm::KernelTimer tm(ctx, ESFM_K_COMPLETE_SEARCH);
        if (int rc = esfm::launch_complete_search(st, a, n_jobs)) return rc;
        return esfm::launch_complete_decode(st, a);
    }
    esfm::KernelTimer tm(ctx, ESFM_K_COMPLETE_SEARCH);
    return esfm::launch_complete_decode(st, a);
}

int run_host_pointers(esfm_ctx *ctx, const Call &c)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    {
        cp::Options o;          // (argument checks before anything is uploaded or written)
        Tracks t;
        int64_t n_rows = 0;
        if (int rc = validate(c, &o, &t, &n_rows)) return rc;
        if (n_rows == 0) { if (c.stats) for (int k = 0; k < 4; ++k) c.stats[k] = 0; return ESFM_OK; }
    }
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const size_t R = (size_t)c.row_off[c.n_cam];
    const size_t row_bytes = c.metric == ESFM_L2_F32 ? sizeof(float) * (size_t)c.width : (size_t)c.width;
    esfm::ScratchCarver at;
    const size_t o_kp = at.take(sizeof(float) * 2 * R), o_point = at.take(sizeof(int32_t) * R), o_dist = at.take(sizeof(float) * R),
                 o_stats = at.take(sizeof(int64_t) * 4);
    if (int rc = ctx->complete_bank.reserve(row_bytes * R)) return rc;
    if (int rc = ctx->complete_kp.reserve(at.at)) return rc;
    uint8_t *k = ctx->complete_kp.as<uint8_t>();
    ESFM_HIP_TRY(esfm::copy_h2d(ctx->complete_bank.ptr, c.desc, row_bytes * R, st));
    ESFM_HIP_TRY(esfm::copy_h2d(k + o_kp, c.kp, sizeof(float) * 2 * R, st));
    Call dev = c;
    dev.desc = ctx->complete_bank.ptr; dev.kp = reinterpret_cast<float *>(k + o_kp);
    dev.kp_point = reinterpret_cast<int32_t *>(k + o_point); dev.kp_dist = reinterpret_cast<float *>(k + o_dist);
    dev.stats = c.stats ? reinterpret_cast<int64_t *>(k + o_stats) : nullptr;
    if (int rc = run_device(ctx, dev)) return rc;
    // into the caller's arrays only after the whole chain has run
    std::vector<int32_t> point(R);
    std::vector<float> dist(R);
    int64_t stats[4] = {0, 0, 0, 0};
    ESFM_HIP_TRY(esfm::copy_d2h(point.data(), k + o_point, sizeof(int32_t) * R, st));
    ESFM_HIP_TRY(esfm::copy_d2h(dist.data(), k + o_dist, sizeof(float) * R, st));
    if (c.stats) ESFM_HIP_TRY(esfm::copy_d2h(stats, k + o_stats, sizeof(stats), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    memcpy(c.kp_point, point.data(), sizeof(int32_t) * R);
    memcpy(c.kp_dist, dist.data(), sizeof(float) * R);
    if (c.stats) memcpy(c.stats, stats, sizeof(stats));
    return ESFM_OK;
}

float host_distance(const Call &c, int32_t ra, int32_t rb)
{
    if (c.metric == ESFM_L2_F32) {
        const float *d = static_cast<const float *>(c.desc);
        return sqrtf(cp::l2sqr_host(d + (size_t)ra * c.width, d + (size_t)rb * c.width, c.width));
    }
    const uint8_t *d = static_cast<const uint8_t *>(c.desc);
    return cp::hamming_host(d + (size_t)ra * c.width, d + (size_t)rb * c.width, c.width);
}

int run_host(const Call &c)
{
    cp::Options o;
    Tracks t;
    int64_t n_rows = 0;
    if (int rc = validate(c, &o, &t, &n_rows)) return rc;
    const size_t R = (size_t)n_rows;
    std::vector<uint64_t> claim(R, cp::kNoClaim);
    int64_t n_adm = 0, n_prop = 0, n_won = 0;
    std::vector<int32_t> seen((size_t)c.n_cam, -1);          // seen[cam] == p: the camera is in point p's track
    for (int p = 0; p < c.n_pt && R; ++p) {
        const int32_t first = t.first[(size_t)p], n_all = t.first[(size_t)p + 1] - first;
        if (n_all == 0) continue;
        const int32_t n_ref = n_all < o.max_refs ? n_all : o.max_refs;
        for (int32_t k = 0; k < n_all; ++k) seen[(size_t)t.cam[(size_t)(first + k)]] = p;
        for (int cam = 0; cam < c.n_cam; ++cam) {
            if (seen[(size_t)cam] == p) continue;
            const cp::Pixel q = cp::project_pixel(c.Rt + 12 * (size_t)cam, c.K4 + 4 * (size_t)cam, c.xyz + 3 * (size_t)p);
            if (!q.front) continue;
            cp::Best2 best = cp::empty_best();
            bool any = false;
            const int32_t r0 = c.row_off[cam], r1 = c.row_off[cam + 1];
            for (int32_t r = r0; r < r1; ++r) {
                if (!c.kp_free[r] || !cp::admissible(q, c.kp[2 * (size_t)r], c.kp[2 * (size_t)r + 1], o.thr2)) continue;
                any = true;
                float d = NAN;
                for (int32_t k = 0; k < n_ref; ++k) d = cp::min_score(d, host_distance(c, t.row[(size_t)(first + k)], r));
                if (cp::is_candidate(d)) cp::insert(best, d, r - r0);
            }
            n_adm += any ? 1 : 0;
            if (!cp::proposes(best, o)) continue;
            ++n_prop;
            uint64_t &slot = claim[(size_t)(r0 + best.k0)];
            const uint64_t key = cp::claim_key(best.d0, p);
            slot = key < slot ? key : slot;
        }
    }
    for (size_t r = 0; r < R; ++r) {
        const bool won = claim[r] != cp::kNoClaim;
        n_won += won ? 1 : 0;
        c.kp_point[r] = won ? (int32_t)(uint32_t)claim[r] : -1;
        c.kp_dist[r] = won ? cp::bits_float((uint32_t)(claim[r] >> 32)) : FLT_MAX;
    }
    if (c.stats) { c.stats[0] = n_adm; c.stats[1] = n_prop; c.stats[2] = n_prop - n_won; c.stats[3] = n_won; }
    return ESFM_OK;
}

}  // namespace

extern "C" {

void esfm_track_complete_options_default(esfm_track_complete_options *opt)
{
    if (!opt) return;
    opt->search_radius_px = 4.0;
    opt->max_distance = (double)INFINITY;
    opt->ratio = 0.8;
    opt->max_refs = 8; opt->reserved = 0;
}

int esfm_track_complete_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const float *kp_dev, const uint8_t *kp_free,
                            const int32_t *set_row_offset, int n_cam, int width, const float *K4_per_cam, const double *Rt12_per_cam, int n_pt,
                            const double *xyz, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const int32_t *obs_kp,
                            const esfm_track_complete_options *opt, int32_t *kp_point_dev, float *kp_dist_dev, int64_t *stats_dev)
{
    return run_device(ctx, Call{metric, desc_dev, kp_dev, kp_free, set_row_offset, n_cam, width, K4_per_cam, Rt12_per_cam, n_pt, xyz, n_obs, cam_idx,
                                pt_idx, obs_kp, opt, kp_point_dev, kp_dist_dev, stats_dev});
}

int esfm_track_complete(esfm_ctx *ctx, esfm_metric metric, const void *desc, const float *kp, const uint8_t *kp_free, const int32_t *set_row_offset,
                        int n_cam, int width, const float *K4_per_cam, const double *Rt12_per_cam, int n_pt, const double *xyz, int n_obs,
                        const int32_t *cam_idx, const int32_t *pt_idx, const int32_t *obs_kp, const esfm_track_complete_options *opt,
                        int32_t *kp_point, float *kp_dist, int64_t *stats)
{
    return run_host_pointers(ctx, Call{metric, desc, kp, kp_free, set_row_offset, n_cam, width, K4_per_cam, Rt12_per_cam, n_pt, xyz, n_obs, cam_idx,
                                       pt_idx, obs_kp, opt, kp_point, kp_dist, stats});
}

int esfm_track_complete_host(esfm_metric metric, const void *desc, const float *kp, const uint8_t *kp_free, const int32_t *set_row_offset, int n_cam,
                             int width, const float *K4_per_cam, const double *Rt12_per_cam, int n_pt, const double *xyz, int n_obs,
                             const int32_t *cam_idx, const int32_t *pt_idx, const int32_t *obs_kp, const esfm_track_complete_options *opt,
                             int32_t *kp_point, float *kp_dist, int64_t *stats)
{
    return run_host(Call{metric, desc, kp, kp_free, set_row_offset, n_cam, width, K4_per_cam, Rt12_per_cam, n_pt, xyz, n_obs, cam_idx, pt_idx, obs_kp,
                         opt, kp_point, kp_dist, stats});
}

}  // extern "C"
