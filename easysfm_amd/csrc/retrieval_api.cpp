// C-ABI entry points of image retrieval (include/esfm.h "Image retrieval").  The host validates the arguments and carves one scratch
// buffer; the stages run in retrieval_kernels.hip on the context's stream with no read-back between them (the k-means loop
// included); the pair list is retrieval_host.hpp's.
#include <cmath>
#include <vector>

#include "retrieval_host.hpp"
#include "retrieval_kernels.hpp"
#include "scratch_layout.hpp"

namespace {

namespace R = esfm::retrieval;

struct Shape {
    esfm::RetrievalShape k;
    int n_sets;
    int64_t total, longest;
    size_t row_bytes;
    int D() const { return k.n_centres * k.d; }
};

#define RETRIEVAL_REQUIRE_TEXT(text)                               \
    do {                                                           \
        if (const char *why__ = (text)) {                          \
            ::esfm::set_error("%s: %s", __func__, why__);          \
            return ESFM_ERR_INVALID_ARG;                           \
        }                                                          \
    } while (0)

// the shape rules shared by every entry point that takes descriptor rows
int make_shape(int metric, const int32_t *off, int n_sets, int width, int n_centres, Shape *s)
{
    ESFM_REQUIRE(metric == ESFM_L2_F32 || metric == ESFM_HAMMING, "unknown metric");
    RETRIEVAL_REQUIRE_TEXT(R::offsets_error(off, n_sets));
    const int d = R::working_dim(metric, width);
    ESFM_REQUIRE(d > 0, "width must be in 1 .. 256 (L2) or 1 .. 64 bytes (Hamming)");
    ESFM_REQUIRE(n_centres >= 1 && n_centres <= R::kMaxCentres, "n_centres must be in 1 .. 256");
    if (n_sets > ESFM_RETRIEVAL_MAX_SETS) { esfm::set_error("%d sets (at most %d)", n_sets, ESFM_RETRIEVAL_MAX_SETS); return ESFM_ERR_UNSUPPORTED; }
    if (n_centres * d > ESFM_RETRIEVAL_MAX_DIM) { esfm::set_error("D = %d x %d exceeds %d", n_centres, d, ESFM_RETRIEVAL_MAX_DIM); return ESFM_ERR_UNSUPPORTED; }
    s->k.metric = metric; s->k.width = width; s->k.d = d; s->k.n_centres = n_centres;
    s->n_sets = n_sets;
    s->total = (int64_t)off[n_sets] - off[0];
    ESFM_REQUIRE(off[0] == 0, "set_row_offset must start at 0");
    s->longest = 0;
    for (int i = 0; i < n_sets; ++i) s->longest = std::max<int64_t>(s->longest, off[i + 1] - off[i]);
    s->row_bytes = metric == ESFM_L2_F32 ? sizeof(float) * (size_t)width : (size_t)width;
    return ESFM_OK;
}

bool values_ok(const float *v, size_t n)
{
    for (size_t e = 0; e < n; ++e) if (!(std::fabs(v[e]) <= 16384.0f)) return false;
    return true;
}

// the chain's device arrays, carved out of ctx->retrieval
struct Scratch {
    int32_t *off, *off_train, *flag, *assign, *counts, *norm2, *dots, *nearest;
    float *centres;
    int64_t *sums;
    int8_t *vp, *flat;
    double *root, *scores;
    int n16, pitch;
};

int carve(esfm_ctx *ctx, const Shape &s, int n_rank, int D_rank, int top_k, bool want_scores, Scratch *x)
{
    const size_t n = (size_t)std::max(s.n_sets, n_rank), D = (size_t)std::max(s.n_sets ? s.D() : 0, D_rank), rows = (size_t)std::max<int64_t>(s.total, 1);
    x->n16 = (int)((n + 15) / 16 * 16); x->pitch = (int)((D + 63) / 64 * 64);
    esfm::ScratchCarver at;
    const size_t o_off = at.take(sizeof(int32_t) * (n + 1)), o_tr = at.take(sizeof(int32_t) * 2), o_flag = at.take(sizeof(int32_t)),
                 o_assign = at.take(sizeof(int32_t) * rows), o_counts = at.take(sizeof(int32_t) * std::max<size_t>(n, 1) * R::kMaxCentres),
                 o_norm2 = at.take(sizeof(int32_t) * std::max<size_t>(n, 1)), o_dots = at.take(sizeof(int32_t) * std::max<size_t>(n * n, 1)),
                 o_near = at.take(sizeof(int32_t) * std::max<size_t>(n * (size_t)top_k, 1)), o_cent = at.take(sizeof(float) * std::max<size_t>(D, 1)),
                 o_sums = at.take(sizeof(int64_t) * std::max<size_t>(n * D, 1)), o_vp = at.take((size_t)x->n16 * x->pitch + 64),
                 o_flat = at.take(std::max<size_t>(n * D, 1)), o_root = at.take(sizeof(double) * std::max<size_t>(n, 1)),
                 o_scores = at.take(want_scores ? sizeof(double) * std::max<size_t>(n * n, 1) : 0);
    if (int rc = ctx->retrieval.reserve(at.at)) return rc;
    uint8_t *d = ctx->retrieval.as<uint8_t>();
    x->off = reinterpret_cast<int32_t *>(d + o_off); x->off_train = reinterpret_cast<int32_t *>(d + o_tr); x->flag = reinterpret_cast<int32_t *>(d + o_flag);
    x->assign = reinterpret_cast<int32_t *>(d + o_assign); x->counts = reinterpret_cast<int32_t *>(d + o_counts);
    x->norm2 = reinterpret_cast<int32_t *>(d + o_norm2); x->dots = reinterpret_cast<int32_t *>(d + o_dots);
    x->nearest = reinterpret_cast<int32_t *>(d + o_near); x->centres = reinterpret_cast<float *>(d + o_cent);
    x->sums = reinterpret_cast<int64_t *>(d + o_sums); x->vp = reinterpret_cast<int8_t *>(d + o_vp); x->flat = reinterpret_cast<int8_t *>(d + o_flat);
    x->root = reinterpret_cast<double *>(d + o_root); x->scores = want_scores ? reinterpret_cast<double *>(d + o_scores) : nullptr;
    return ESFM_OK;
}

int upload_rows(esfm_ctx *ctx, const Shape &s, const void *desc_host, const void **desc_dev)
{
    const size_t bytes = (size_t)s.total * s.row_bytes;
    if (int rc = ctx->retrieval_bank.reserve(bytes ? bytes : 1)) return rc;
    if (bytes) ESFM_HIP_TRY(esfm::copy_h2d(ctx->retrieval_bank.ptr, desc_host, bytes, ctx->stream));
    *desc_dev = ctx->retrieval_bank.ptr;
    return ESFM_OK;
}

// the codebook into x.centres: initialisation and kmeans_iterations steps, all enqueued
int train_dev(esfm_ctx *ctx, const Shape &s, const void *desc, const esfm_retrieval_options &o, const Scratch &x)
{
    hipStream_t st = ctx->stream;
    int64_t stride = 1, nt = 0;
    R::train_sample(s.total, o.max_train, &stride, &nt);
    int32_t *tab = static_cast<int32_t *>(ctx->pinned);
    tab[0] = 0; tab[1] = (int32_t)nt;
    ESFM_HIP_TRY(hipMemcpyAsync(x.off_train, tab, sizeof(int32_t) * 2, hipMemcpyHostToDevice, st));
    if (int rc = esfm::launch_retrieval_init(st, s.k, desc, stride, nt, x.centres)) return rc;
    const size_t D = (size_t)s.D();
    for (int it = 0; it < o.kmeans_iterations; ++it) {
        if (int rc = esfm::launch_retrieval_assign(st, s.k, desc, stride, nt, x.centres, x.assign)) return rc;
        ESFM_HIP_TRY(hipMemsetAsync(x.sums, 0, sizeof(int64_t) * D, st));
        ESFM_HIP_TRY(hipMemsetAsync(x.counts, 0, sizeof(int32_t) * (size_t)s.k.n_centres, st));
        if (int rc = esfm::launch_retrieval_accumulate(st, s.k, desc, x.off_train, 1, nt, stride, x.assign, x.sums, x.counts)) return rc;
        if (int rc = esfm::launch_retrieval_update(st, s.k, x.sums, x.counts, x.centres)) return rc;
    }
    return ESFM_OK;
}

// x.centres -> x.assign and the per-image sums and counts (finalize_dev turns them into S, x.vp and x.norm2), all enqueued; x.off
// holds the offsets already
int sums_dev(esfm_ctx *ctx, const Shape &s, const void *desc, const Scratch &x)
{
    hipStream_t st = ctx->stream;
    const size_t D = (size_t)s.D(), n = (size_t)s.n_sets;
    if (int rc = esfm::launch_retrieval_assign(st, s.k, desc, 1, s.total, x.centres, x.assign)) return rc;
    ESFM_HIP_TRY(hipMemsetAsync(x.sums, 0, sizeof(int64_t) * n * D, st));
    ESFM_HIP_TRY(hipMemsetAsync(x.counts, 0, sizeof(int32_t) * n * (size_t)s.k.n_centres, st));
    return esfm::launch_retrieval_accumulate(st, s.k, desc, x.off, s.n_sets, s.longest, 1, x.assign, x.sums, x.counts);
}

int finalize_dev(esfm_ctx *ctx, const Shape &s, const Scratch &x)
{
    ESFM_HIP_TRY(hipMemsetAsync(x.vp, 0, (size_t)x.n16 * x.pitch, ctx->stream));
    return esfm::launch_retrieval_finalize(ctx->stream, s.k, s.n_sets, x.sums, x.counts, x.centres, x.vp, x.pitch, x.norm2);
}

int rank_dev(esfm_ctx *ctx, int n, int top_k, const Scratch &x)
{
    if (int rc = esfm::launch_retrieval_dots(ctx->stream, x.vp, x.n16, x.pitch, n, x.dots)) return rc;
    return esfm::launch_retrieval_rank(ctx->stream, n, x.dots, top_k, x.root, x.nearest, x.scores);
}

int upload_offsets(esfm_ctx *ctx, const int32_t *off, int n_sets, const Scratch &x)
{
    ESFM_HIP_TRY(esfm::copy_h2d(x.off, off, sizeof(int32_t) * ((size_t)n_sets + 1), ctx->stream));
    return ESFM_OK;
}

// the whole chain over resident rows; rows_checked: the host has validated the values already
int pairs_common(esfm_ctx *ctx, const Shape &s, const void *desc, const int32_t *off, const esfm_retrieval_options &o, bool rows_checked,
                 int32_t *pairs, int32_t *n_pairs)
{
    const char *why = nullptr;
    std::vector<int32_t> nearest((size_t)s.n_sets * (size_t)o.top_k);
    if (o.top_k > 0 && s.n_sets > 0) {
        hipStream_t st = ctx->stream;
        Scratch x;
        if (int rc = carve(ctx, s, 0, 0, o.top_k, false, &x)) return rc;
        if (int rc = ctx->pin(sizeof(int32_t) * 4)) return rc;
        ESFM_HIP_TRY(hipMemsetAsync(x.flag, 0, sizeof(int32_t), st));
        if (!rows_checked && s.k.metric == ESFM_L2_F32)
            if (int rc = esfm::launch_retrieval_check_values(st, static_cast<const float *>(desc), s.total * s.k.width, x.flag)) return rc;
        if (int rc = upload_offsets(ctx, off, s.n_sets, x)) return rc;
        // esfm_ctx_set_kernel_timing: events around the four stages (esfm_retrieval_last_stage_ms)
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        auto mark = [&](int k) { if (ctx->timing) { ev[k] = ctx->take_event(); (void)hipEventRecord(ev[k], st); } };
        mark(0);
        if (int rc = train_dev(ctx, s, desc, o, x)) return rc;
        mark(1);
        if (int rc = sums_dev(ctx, s, desc, x)) return rc;
        mark(2);
        if (int rc = finalize_dev(ctx, s, x)) return rc;
        mark(3);
        if (int rc = rank_dev(ctx, s.n_sets, o.top_k, x)) return rc;
        mark(4);
        int32_t *flag = static_cast<int32_t *>(ctx->pinned) + 2;
        ESFM_HIP_TRY(hipMemcpyAsync(flag, x.flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        ESFM_HIP_TRY(esfm::copy_d2h(nearest.data(), x.nearest, sizeof(int32_t) * nearest.size(), st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
        for (int k = 0; k < 4 && ctx->timing; ++k) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
            ctx->retrieval_stage_ms[k] = (double)ms;
        }
        for (hipEvent_t e : ev) if (e) ctx->event_pool.push_back(e);
        ESFM_REQUIRE(*flag == 0, "a descriptor value is not finite or exceeds 16384 in magnitude");
    }
    const int rc = R::pair_list(s.n_sets, o.top_k, nearest.data(), o.window, pairs, n_pairs, &why);
    if (rc) esfm::set_error("esfm_retrieval_pairs: %s", why);
    return rc;
}

int pairs_entry(esfm_ctx *ctx, int metric, const void *desc, bool resident, const int32_t *off, int n_sets, int width, const esfm_retrieval_options *opt,
                int32_t *pairs, int32_t *n_pairs)
{
    RETRIEVAL_REQUIRE_TEXT(R::options_error(opt));
    Shape s;
    if (int rc = make_shape(metric, off, n_sets, width, opt->n_centres, &s)) return rc;
    ESFM_REQUIRE(n_pairs, "n_pairs is NULL");
    ESFM_REQUIRE(pairs || n_sets < 2, "pairs is NULL");
    const bool chain = opt->top_k > 0 && n_sets > 0;
    ESFM_REQUIRE(!chain || s.total > 0, "no descriptor rows");
    ESFM_REQUIRE(!chain || desc, "descriptors are NULL");
    if (chain && !resident && metric == ESFM_L2_F32)
        ESFM_REQUIRE(values_ok(static_cast<const float *>(desc), (size_t)s.total * (size_t)width), "a descriptor value is not finite or exceeds 16384 in magnitude");
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (chain) {
        if (int rc = esfm::set_device(ctx)) return rc;
        if (!resident) if (int rc = upload_rows(ctx, s, desc, &desc)) return rc;
    }
    return pairs_common(ctx, s, desc, off, *opt, !resident, pairs, n_pairs);
}

}  // namespace

extern "C" {

void esfm_retrieval_options_default(esfm_retrieval_options *opt)
{
    if (!opt) return;
    opt->n_centres = 64; opt->kmeans_iterations = 10; opt->max_train = 65536; opt->top_k = 10; opt->window = 0; opt->reserved = 0;
}

int esfm_retrieval_train(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets, int width,
                         const esfm_retrieval_options *opt, float *centres)
{
    RETRIEVAL_REQUIRE_TEXT(R::options_error(opt));
    Shape s;
    if (int rc = make_shape(metric, set_row_offset, n_sets, width, opt->n_centres, &s)) return rc;
    ESFM_REQUIRE(s.total > 0, "no descriptor rows");
    ESFM_REQUIRE(desc_host && centres, "a required pointer is NULL");
    if (metric == ESFM_L2_F32)
        ESFM_REQUIRE(values_ok(static_cast<const float *>(desc_host), (size_t)s.total * (size_t)width), "a descriptor value is not finite or exceeds 16384 in magnitude");
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(ctx)) return rc;
    const void *desc = nullptr;
    if (int rc = upload_rows(ctx, s, desc_host, &desc)) return rc;
    Scratch x;
    Shape one = s;
    one.n_sets = 1;                    // the training scratch: one set's sums
    if (int rc = carve(ctx, one, 0, 0, 0, false, &x)) return rc;
    if (int rc = ctx->pin(sizeof(int32_t) * 4)) return rc;
    if (int rc = train_dev(ctx, s, desc, *opt, x)) return rc;
    ESFM_HIP_TRY(esfm::copy_d2h(centres, x.centres, sizeof(float) * (size_t)s.D(), ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ESFM_OK;
}

int esfm_retrieval_vlad(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets, int width, int n_centres,
                        const float *centres, int8_t *vlad, int32_t *norm2, int32_t *assign, int64_t *sums)
{
    Shape s;
    if (int rc = make_shape(metric, set_row_offset, n_sets, width, n_centres, &s)) return rc;
    ESFM_REQUIRE(centres, "centres are NULL");
    ESFM_REQUIRE(n_sets == 0 || (vlad && norm2), "a required output is NULL");
    ESFM_REQUIRE(s.total == 0 || desc_host, "descriptors are NULL");
    ESFM_REQUIRE(values_ok(centres, (size_t)s.D()), "a centre value is not finite or exceeds 16384 in magnitude");
    if (metric == ESFM_L2_F32 && s.total)
        ESFM_REQUIRE(values_ok(static_cast<const float *>(desc_host), (size_t)s.total * (size_t)width), "a descriptor value is not finite or exceeds 16384 in magnitude");
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (n_sets == 0) return ESFM_OK;
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const void *desc = nullptr;
    if (int rc = upload_rows(ctx, s, desc_host, &desc)) return rc;
    Scratch x;
    if (int rc = carve(ctx, s, 0, 0, 0, false, &x)) return rc;
    const size_t D = (size_t)s.D(), n = (size_t)n_sets;
    if (int rc = upload_offsets(ctx, set_row_offset, n_sets, x)) return rc;
    ESFM_HIP_TRY(esfm::copy_h2d(x.centres, centres, sizeof(float) * D, st));
    if (int rc = sums_dev(ctx, s, desc, x)) return rc;
    if (int rc = finalize_dev(ctx, s, x)) return rc;
    if (int rc = esfm::launch_retrieval_repitch(st, x.vp, x.pitch, x.flat, (int)D, n_sets, (int)D)) return rc;
    ESFM_HIP_TRY(esfm::copy_d2h(vlad, x.flat, n * D, st));
    ESFM_HIP_TRY(esfm::copy_d2h(norm2, x.norm2, sizeof(int32_t) * n, st));
    if (assign && s.total) ESFM_HIP_TRY(esfm::copy_d2h(assign, x.assign, sizeof(int32_t) * (size_t)s.total, st));
    if (sums) ESFM_HIP_TRY(esfm::copy_d2h(sums, x.sums, sizeof(int64_t) * n * D, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

int esfm_retrieval_rank(esfm_ctx *ctx, int n_sets, int D, const int8_t *vlad, int top_k, int32_t *nearest, int32_t *dots, double *scores)
{
    ESFM_REQUIRE(n_sets >= 0, "n_sets is negative");
    ESFM_REQUIRE(D >= 1, "D must be >= 1");
    ESFM_REQUIRE(top_k >= 0 && top_k <= R::kMaxTopK, "top_k must be in 0 .. 1024");
    if (n_sets > ESFM_RETRIEVAL_MAX_SETS || D > ESFM_RETRIEVAL_MAX_DIM) { esfm::set_error("%d sets of dimension %d (at most %d of %d)", n_sets, D, ESFM_RETRIEVAL_MAX_SETS, ESFM_RETRIEVAL_MAX_DIM); return ESFM_ERR_UNSUPPORTED; }
    ESFM_REQUIRE(n_sets == 0 || vlad, "vlad is NULL");
    ESFM_REQUIRE(n_sets == 0 || top_k == 0 || nearest, "nearest is NULL");
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (n_sets == 0) return ESFM_OK;
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    Shape none{};
    Scratch x;
    if (int rc = carve(ctx, none, n_sets, D, top_k, scores != nullptr, &x)) return rc;
    const size_t n = (size_t)n_sets;
    ESFM_HIP_TRY(esfm::copy_h2d(x.flat, vlad, n * (size_t)D, st));
    ESFM_HIP_TRY(hipMemsetAsync(x.vp, 0, (size_t)x.n16 * x.pitch, st));
    if (int rc = esfm::launch_retrieval_repitch(st, x.flat, D, x.vp, x.pitch, n_sets, D)) return rc;
    if (int rc = rank_dev(ctx, n_sets, top_k, x)) return rc;
    if (top_k) ESFM_HIP_TRY(esfm::copy_d2h(nearest, x.nearest, sizeof(int32_t) * n * (size_t)top_k, st));
    if (dots) ESFM_HIP_TRY(esfm::copy_d2h(dots, x.dots, sizeof(int32_t) * n * n, st));
    if (scores) ESFM_HIP_TRY(esfm::copy_d2h(scores, x.scores, sizeof(double) * n * n, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

int esfm_retrieval_pair_list(int n_sets, int top_k, const int32_t *nearest, int window, int32_t *pairs, int32_t *n_pairs)
{
    const char *why = nullptr;
    const int rc = R::pair_list(n_sets, top_k, nearest, window, pairs, n_pairs, &why);
    if (rc) esfm::set_error("esfm_retrieval_pair_list: %s", why);
    return rc;
}

int esfm_retrieval_last_stage_ms(esfm_ctx *ctx, double *ms)
{
    if (!ctx || !ms) { esfm::set_error("esfm_retrieval_last_stage_ms: NULL argument"); return ESFM_ERR_INVALID_ARG; }
    for (int k = 0; k < 4; ++k) ms[k] = ctx->retrieval_stage_ms[k];
    return ESFM_OK;
}

int esfm_retrieval_pairs(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets, int width,
                         const esfm_retrieval_options *opt, int32_t *pairs, int32_t *n_pairs)
{
    return pairs_entry(ctx, metric, desc_host, false, set_row_offset, n_sets, width, opt, pairs, n_pairs);
}

int esfm_retrieval_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const int32_t *set_row_offset, int n_sets, int width,
                             const esfm_retrieval_options *opt, int32_t *pairs, int32_t *n_pairs)
{
    return pairs_entry(ctx, metric, desc_dev, true, set_row_offset, n_sets, width, opt, pairs, n_pairs);
}

}  // extern "C"
