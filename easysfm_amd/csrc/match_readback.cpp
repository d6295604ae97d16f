// The packed read-back of esfm_match_pairs, esfm_match_cross_pairs and esfm_match_guided_pairs (match_lists.hpp).
#include "match_lists.hpp"

namespace esfm {

int reserve_match_list_stage(esfm_ctx *ctx, size_t n_slots, int n_pairs)
{
    if (int rc = ctx->stage_b.reserve(sizeof(int32_t) * n_slots)) return rc;
    if (int rc = ctx->stage_c.reserve(sizeof(int32_t) * n_slots)) return rc;
    if (int rc = ctx->stage_d.reserve(sizeof(float) * n_slots)) return rc;
    return ctx->stage_e.reserve(sizeof(int32_t) * (size_t)n_pairs);
}

int read_back_match_lists(esfm_ctx *ctx, int n_pairs, const int64_t *list_off, size_t n_slots, bool whole_when_dense, int32_t *query_idx,
                          int32_t *train_idx, float *distance, int32_t *n_out)
{
    hipStream_t st = ctx->stream;
    ESFM_HIP_TRY(copy_d2h(n_out, ctx->stage_e.ptr, sizeof(int32_t) * (size_t)n_pairs, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    // a ratio test keeps a few per cent of sum(nq) slots: packed on the device, read back as three dense arrays and placed from a
    // host copy, config 4's shape (267 M slots, 4.4 M matches) moves 52 MB over PCIe instead of 3.2 GB
    size_t total = 0;
    for (int p = 0; p < n_pairs; ++p) total += (size_t)n_out[p];
    if (total == 0) return ESFM_OK;
    if (whole_when_dense && total * 4 >= n_slots) {
        ESFM_HIP_TRY(copy_d2h(query_idx, ctx->stage_b.ptr, sizeof(int32_t) * n_slots, st));
        ESFM_HIP_TRY(copy_d2h(train_idx, ctx->stage_c.ptr, sizeof(int32_t) * n_slots, st));
        ESFM_HIP_TRY(copy_d2h(distance, ctx->stage_d.ptr, sizeof(float) * n_slots, st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
        return ESFM_OK;
    }
    std::vector<long long> tab(2 * (size_t)n_pairs);      // per pair {source offset, packed offset}
    long long run = 0;
    for (int p = 0; p < n_pairs; ++p) { tab[2 * (size_t)p] = list_off[p]; tab[2 * (size_t)p + 1] = run; run += n_out[p]; }
    const size_t tab_bytes = (sizeof(long long) * tab.size() + 255) & ~(size_t)255;
    if (int rc = ctx->stage_a.reserve(tab_bytes + 12 * total + 64)) return rc;
    char *base = ctx->stage_a.as<char>();
    int32_t *dq = reinterpret_cast<int32_t *>(base + tab_bytes), *dtn = dq + total;
    float *dd = reinterpret_cast<float *>(dtn + total);
    ESFM_HIP_TRY(copy_h2d(base, tab.data(), sizeof(long long) * tab.size(), st));
    if (int rc = launch_pack_match_lists(st, reinterpret_cast<const long long *>(base), ctx->stage_e.as<int32_t>(), n_pairs, ctx->stage_b.as<int32_t>(),
                                         ctx->stage_c.as<int32_t>(), ctx->stage_d.as<float>(), dq, dtn, dd))
        return rc;
    std::vector<int32_t> hq(2 * total);
    std::vector<float> hd(total);
    ESFM_HIP_TRY(copy_d2h(hq.data(), dq, sizeof(int32_t) * 2 * total, st));
    ESFM_HIP_TRY(copy_d2h(hd.data(), dd, sizeof(float) * total, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    for (int p = 0; p < n_pairs; ++p) {
        const size_t n = (size_t)n_out[p], so = (size_t)tab[2 * (size_t)p], dof = (size_t)tab[2 * (size_t)p + 1];
        if (!n) continue;
        memcpy(query_idx + so, hq.data() + dof, sizeof(int32_t) * n);
        memcpy(train_idx + so, hq.data() + total + dof, sizeof(int32_t) * n);
        memcpy(distance + so, hd.data() + dof, sizeof(float) * n);
    }
    return ESFM_OK;
}

}  // namespace esfm
