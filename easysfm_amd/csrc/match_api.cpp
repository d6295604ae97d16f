// C-ABI entry points for pairwise matching (include/esfm.h, rows a-1..a-3 of SURVEY.md section 8).
// Host logic only: argument checks, the pair table, scratch management, kernel sequencing.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "match_kernels.hpp"
#include "match_plan.hpp"

using esfm::PairDesc;
using esfm::PairPlan;

namespace {

// Upload the pair table through a pinned staging buffer.  The context remembers the last table:
// an identical pair list (the common case in a loop over the same frames) is not re-sent.
int upload_pairs(esfm_ctx *ctx, const PairPlan &plan, const PairDesc **dev_tab)
{
    esfm::MatchState &m = ctx->match;
    // one blob: the pair table, then the pairs' indices sorted by train set (pair_order_of below), then the front pass's block table
    const size_t tab_bytes = plan.tab.size() * sizeof(PairDesc), ord_bytes = plan.by_train.size() * sizeof(int32_t);
    const size_t bytes = tab_bytes + ord_bytes + plan.blk_pair.size() * sizeof(int32_t);
    if (bytes == 0) { *dev_tab = nullptr; return ESFM_OK; }
    std::vector<char> blob(bytes);
    memcpy(blob.data(), plan.tab.data(), tab_bytes);
    memcpy(blob.data() + tab_bytes, plan.by_train.data(), ord_bytes);
    if (!plan.blk_pair.empty()) memcpy(blob.data() + tab_bytes + ord_bytes, plan.blk_pair.data(), bytes - tab_bytes - ord_bytes);
    if (m.pair_tab.cap >= bytes && ctx->pinned_cap >= bytes && m.last_pair_bytes == bytes && memcmp(ctx->pinned, blob.data(), bytes) == 0) {
        *dev_tab = m.pair_tab.as<PairDesc>();
        return ESFM_OK;
    }
    // the pinned buffer may still be the source of an in-flight copy: drain before rewriting it
    m.last_pair_bytes = 0;   // the cache is valid only once the new table's copy has been enqueued
    ESFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (int rc = ctx->pin(bytes)) return rc;
    if (int rc = m.pair_tab.reserve(bytes)) return rc;
    memcpy(ctx->pinned, blob.data(), bytes);
    ESFM_HIP_TRY(esfm::copy_h2d(m.pair_tab.ptr, ctx->pinned, bytes, ctx->stream));
    m.last_pair_bytes = bytes;
    *dev_tab = m.pair_tab.as<PairDesc>();
    return ESFM_OK;
}
inline const int32_t *pair_order_of(const PairDesc *dev_tab, int n_pairs) { return reinterpret_cast<const int32_t *>(dev_tab + n_pairs); }
inline const int32_t *blk_pair_of(const PairDesc *dev_tab, int n_pairs) { return pair_order_of(dev_tab, n_pairs) + n_pairs; }

// (re)allocates a buffer of counters that must read zero: a fresh allocation is cleared once, after that the kernels leave it clean
int reserve_zeroed(esfm::DevBuf &b, size_t bytes, hipStream_t st, bool *grew = nullptr)
{
    if (bytes <= b.cap) return ESFM_OK;
    if (int rc = b.reserve(bytes)) return rc;
    ESFM_HIP_TRY(hipMemsetAsync(b.ptr, 0, b.cap, st));
    if (grew) *grew = true;
    return ESFM_OK;
}

bool is_prepared(const esfm::MatchState &m, esfm_metric metric, const void *desc_dev, int64_t total_rows, int width)
{
    return m.prep_desc != nullptr && m.prep_desc == desc_dev && m.prep_metric == (int)metric && m.prep_rows == total_rows && m.prep_width == width;
}

// esfm_ctx_set_prepared_check(ctx, 1): a call that is about to rely on prepared operands first re-derives the buffer's fingerprint
// and compares it with the one taken at prepare time (one read of the buffer + one host round trip per call: a debugging aid, off
// by default).  A buffer that was rewritten in place -- or freed and replaced by another allocation at the same address -- fails
// the call with ESFM_ERR_STALE_PREPARED and ends the prepared state, instead of matching against the old rows' images.
int verify_prepared(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, int64_t total_rows, int width)
{
    esfm::MatchState &m = ctx->match;
    if (!m.prep_check) return ESFM_OK;
    if (!m.prep_has_sum) { m.prep_desc = nullptr; return ESFM_OK; }      // prepared before the check was switched on: re-derive
    unsigned long long *sums = m.prep_sum.as<unsigned long long>();
    if (int rc = esfm::launch_buffer_checksum(ctx->stream, desc_dev, (size_t)total_rows * esfm::match_row_bytes(metric, width), sums + 1)) return rc;
    unsigned long long h[2] = {0ull, 0ull};
    ESFM_HIP_TRY(esfm::copy_d2h(h, sums, sizeof(h), ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (h[0] == h[1]) return ESFM_OK;
    m.prep_desc = nullptr;
    esfm::set_error("the descriptor buffer %p was modified (or replaced by another allocation at the same address) after esfm_match_prepare_dev: "
                    "call esfm_match_prepare_dev again, or esfm_match_release_prepared before rewriting / freeing a prepared buffer", desc_dev);
    return ESFM_ERR_STALE_PREPARED;
}

// The kernel paths of the matcher, one per row of DESIGN.md section 4.4.
enum class MatchPath { L2_ONE_PRODUCT, L2_THREE_PRODUCT, L2_F32_MFMA, L2_EXACT, HM_FP4, HM_I8, HM_VALU };

// The one rule that picks a path.  max_nt: the call's largest train set; audit: esfm_ctx_set_l2_audit's mode (2 sends every L2
// query to the exact scan).  ESFM_L2_PASS and ESFM_HM_PASS act through l2_bf16_pass, l2_one_product_pass and hamming_fp4_supported.
MatchPath select_path(esfm_metric metric, int width, int max_nt, int audit)
{
    if (metric == ESFM_HAMMING) {
        if (esfm::hamming_fp4_supported(width, max_nt)) return MatchPath::HM_FP4;
        return esfm::hamming_expanded_bytes(width, 1) > 0 ? MatchPath::HM_I8 : MatchPath::HM_VALU;   // (256-bit rows have a byte image)
    }
    if (!esfm::l2_mfma_supported(width) || audit == 2) return MatchPath::L2_EXACT;
    if (!esfm::l2_bf16_pass(width)) return MatchPath::L2_F32_MFMA;
    return esfm::l2_one_product_pass() && esfm::l2_x1_supported(max_nt) ? MatchPath::L2_ONE_PRODUCT : MatchPath::L2_THREE_PRODUCT;
}

// What the caller of knn2_core wants: RAW every query's exact 2-NN (ratio +inf); SCREENED the table of a pass that screens with
// `ratio`, the queries it drops marked (knn2_screened, cross-check); LISTS the ratio test's match lists -- a path may run the test
// + compaction itself, into the four outputs.
struct MatchRequest {
    enum Kind { RAW, SCREENED, LISTS } kind;
    double ratio;
    int32_t *query_idx = nullptr, *train_idx = nullptr;
    float *distance = nullptr;
    int32_t *n_out = nullptr;
};

// One knn2_core call as its path function sees it.
struct Pass {
    esfm_ctx *ctx; esfm::MatchState &m; hipStream_t st;
    const void *desc; int width;
    const PairPlan &plan; const PairDesc *dev_tab;
    int32_t *knn_idx; float *knn_dist;
    const MatchRequest &req;
    bool prepared;   // the derived operands of `desc` are in the context (esfm_match_prepare_dev)
    int n_pairs() const { return (int)plan.tab.size(); }
    int flag_cap() const { return (int)std::min<int64_t>(plan.total_queries, (int64_t)1 << 30); }
};

// counters: [0,16) and [16,32) the two phases of the one-product path, [32,48) the other L2 passes, [48,64) scratch, [64] the fused
// launch's hand-over failure word (sticky: raised by the device, cleared by match_handover_check)
constexpr int kOtherCounters = 32, kScratchCounters = 48, kHandoverFailWord = 64, kCounterInts = 80;


// The one-product pass's per-row operands of `desc`: bf16 images, norms, residual norms (esfm_match_prepare_dev, or a call on an
// unprepared buffer).  Needs the context's counters.
int derive_l2_images(esfm_ctx *ctx, const float *desc, int64_t total_rows)
{
    esfm::MatchState &m = ctx->match;
    if (int rc = m.norms.reserve(sizeof(float) * (size_t)std::max<int64_t>(total_rows, 1))) return rc;
    if (int rc = m.l2_hi.reserve(esfm::l2_hi_bytes(total_rows))) return rc;
    return esfm::launch_l2_split_bf16(ctx->stream, desc, total_rows, nullptr, m.norms.as<float>(), m.counters.as<int32_t>() + kScratchCounters,
                                      nullptr, 0, m.l2_hi.ptr, nullptr);
}

// 64-float rows, train sets within the position code.  Launch 1 (only when the descriptor buffer has not been prepared): bf16
// images, norms, residual norms.  Launch 2: one bf16 product per f32 product, fused top-K fold, ratio screen (l2_knn_bf16x1_kernel).
// Launch 3: exact re-rank of the screen's survivors + certificate, the uncertified ones through the threshold filter, overflowed
// chunks by brute force, ratio test + compaction (l2_finish_kernel).  Audit modes: 1 no brute force, 3 / 4 launch 3 stops after the
// re-rank.  A prepared buffer stays prepared.
// Match lists (outside the audit modes 3 / 4): launches 2 and 3 are ONE, l2_fused_kernel -- the finish workgroups trail the pass's
// in the same grid (esfm_ctx_set_l2_two_launch / ESFM_X1_GRID keep the two).  The phase scheme is the same either way.
int run_l2_one_product(const Pass &p, bool &compacted)
{
    esfm::MatchState &m = p.m;
    hipStream_t st = p.st;
    const PairPlan &plan = p.plan;
    const int n_pairs = p.n_pairs();
    const float *desc = static_cast<const float *>(p.desc);
    const bool audit_front = m.l2_audit == 3 || m.l2_audit == 4;
    const bool fuse = p.req.kind == MatchRequest::LISTS && !audit_front;   // ratio test + compaction in l2_finish_kernel
    if (int rc = m.pair_list2.reserve(sizeof(int32_t) * (size_t)plan.total_queries)) return rc;
    if (int rc = m.knn_d2.reserve(sizeof(float) * (size_t)plan.total_queries)) return rc;
    if (int rc = m.surv_list.reserve(esfm::l2_survivor_entry_bytes() * (size_t)plan.total_queries)) return rc;
    for (int k = 0; k < 2; ++k) {
        bool grew = false;
        if (int rc = reserve_zeroed(m.unc_cnt[k], sizeof(int32_t) * (size_t)n_pairs, st, &grew)) return rc;
        if (int rc = reserve_zeroed(m.surv_cnt[k], sizeof(int32_t) * (size_t)n_pairs, st, &grew)) return rc;
        if (grew) {                      // a fresh allocation is clean as a whole; its sibling is cleared with it
            ESFM_HIP_TRY(hipMemsetAsync(m.unc_cnt[k].ptr, 0, m.unc_cnt[k].cap, st));
            ESFM_HIP_TRY(hipMemsetAsync(m.surv_cnt[k].ptr, 0, m.surv_cnt[k].cap, st));
            m.l2_phase_pairs[k] = 0;
        }
    }
    if (int rc = reserve_zeroed(m.fin_done, sizeof(int32_t) * (size_t)n_pairs, st)) return rc;
    // One launch instead of two saves the fixed costs between them (about 30 us per call) and costs the finish role a third of its
    // occupancy (two workgroups per CU instead of three): about 4 us per million queries.  Measured on all pairs of n images x 4096 rows:
    // 3.2 M queries 1.242 against 1.286 ms, 6.3 M 2.448 against 2.472, 12.9 M 4.946 against 4.923, 25 M 9.70 against 9.63: long lists
    // keep the two launches.
    static const int64_t kFusedMaxQueries = [] { const char *e = getenv("ESFM_L2_FUSED_MAX_QUERIES"); return e ? (int64_t)atoll(e) : (int64_t)1 << 23; }();     // (the variable: measurement)
    const bool one_launch = fuse && !m.l2_two_launch && esfm::l2_x1_forced_grid() <= 0 && plan.total_queries <= kFusedMaxQueries;
    if (one_launch) { if (int rc = reserve_zeroed(m.pass_done, sizeof(int32_t) * (size_t)n_pairs, st)) return rc; }
    const int ph = m.l2_phase, oth = 1 - ph;
    int32_t *counters = m.counters.as<int32_t>();
    m.counters_cur = counters + 16 * ph;
    if (!p.prepared) {
        m.prep_desc = nullptr;          // the images below replace whatever was prepared
        if (int rc = derive_l2_images(p.ctx, desc, plan.total_rows)) return rc;
    }
    if (one_launch) {
        // (timed as the pass: ESFM_K_L2_SECOND records no launch on this path)
        esfm::KernelTimer tm(p.ctx, ESFM_K_L2_KNN);
        if (int rc = esfm::launch_l2_fused(st, desc, m.l2_hi.ptr, plan.total_rows, m.norms.as<float>(), p.dev_tab, blk_pair_of(p.dev_tab, n_pairs),
                                           plan.n_blocks2, pair_order_of(p.dev_tab, n_pairs), n_pairs, p.knn_idx, p.knn_dist, m.counters_cur,
                                           m.flagged.as<int32_t>(), p.flag_cap(), m.surv_cnt[ph].as<int32_t>(), m.surv_list.ptr,
                                           m.unc_cnt[ph].as<int32_t>(), m.pair_list2.as<int32_t>(), m.knn_d2.as<float>(), m.unc_cnt[oth].as<int32_t>(),
                                           m.surv_cnt[oth].as<int32_t>(), m.l2_phase_pairs[oth], counters + 16 * oth, m.fin_done.as<int32_t>(),
                                           m.pass_done.as<int32_t>(), counters + kHandoverFailWord, m.l2_audit, p.req.ratio, p.req.query_idx,
                                           p.req.train_idx, p.req.distance, p.req.n_out))
            return rc;
        m.handover_pending = true;
        m.l2_phase_pairs[oth] = 0;
        m.l2_phase_pairs[ph] = n_pairs;
        m.l2_phase = oth;
        compacted = true;
        return ESFM_OK;
    }
    {
        esfm::KernelTimer tm(p.ctx, ESFM_K_L2_KNN);
        if (int rc = esfm::launch_l2_knn_bf16x1(st, p.ctx->num_cu, desc, m.l2_hi.ptr, plan.total_rows, m.norms.as<float>(), p.dev_tab,
                                                blk_pair_of(p.dev_tab, n_pairs), plan.n_blocks2, p.knn_idx, p.knn_dist, m.counters_cur, p.flag_cap(),
                                                m.surv_cnt[ph].as<int32_t>(), m.surv_list.ptr, p.req.ratio,
                                                /* markers: only where something reads the table itself */ !fuse,
                                                m.l2_audit == 4 ? m.flagged.as<int32_t>() : nullptr, m.unc_cnt[oth].as<int32_t>(),
                                                m.surv_cnt[oth].as<int32_t>(), m.l2_phase_pairs[oth], counters + 16 * oth))
            return rc;
    }
    m.l2_phase_pairs[oth] = 0;
    m.l2_phase_pairs[ph] = n_pairs;
    m.l2_phase = oth;
    esfm::KernelTimer tm(p.ctx, ESFM_K_L2_SECOND);
    if (int rc = esfm::launch_l2_finish(st, desc, m.l2_hi.ptr, plan.total_rows, m.norms.as<float>(), p.dev_tab, pair_order_of(p.dev_tab, n_pairs),
                                        n_pairs, m.surv_cnt[ph].as<int32_t>(), m.surv_list.ptr, m.unc_cnt[ph].as<int32_t>(), m.pair_list2.as<int32_t>(),
                                        m.knn_d2.as<float>(), p.knn_idx, p.knn_dist, m.counters_cur, m.flagged.as<int32_t>(), p.flag_cap(),
                                        m.fin_done.as<int32_t>(), m.l2_audit, fuse, p.req.ratio, p.req.query_idx, p.req.train_idx, p.req.distance,
                                        p.req.n_out))
        return rc;
    compacted = fuse;   // (audit 3 / 4: the first pass's own answers and failures / rejections)
    return ESFM_OK;
}

// 64-float rows without the one-product pass (ESFM_L2_PASS=bf16x3, train sets of more than 65536 rows): the three-product kernel of
// round 2 + the exact re-scan of its uncertified queries, pair by pair.  Audit mode 1 stops before the re-scan.
int run_l2_three_product(const Pass &p)
{
    esfm::MatchState &m = p.m;
    const int n_pairs = p.n_pairs();
    const float *desc = static_cast<const float *>(p.desc);
    int32_t *cnt = m.counters.as<int32_t>() + kOtherCounters;
    m.prep_desc = nullptr;   // the pass writes its own norms and images
    if (int rc = m.norms.reserve(sizeof(float) * (size_t)std::max<int64_t>(p.plan.total_rows, 1))) return rc;
    if (int rc = m.hm_exp.reserve(esfm::l2_split_bytes(p.width, p.plan.total_rows))) return rc;
    if (int rc = m.pair_cnt.reserve(sizeof(int32_t) * (size_t)n_pairs)) return rc;
    if (int rc = m.pair_list.reserve(sizeof(int32_t) * (size_t)p.plan.total_queries)) return rc;
    if (int rc = esfm::launch_l2_split_bf16(p.st, desc, p.plan.total_rows, m.hm_exp.ptr, m.norms.as<float>(), cnt, m.pair_cnt.as<int32_t>(), n_pairs,
                                            nullptr, nullptr))
        return rc;
    {
        esfm::KernelTimer tm(p.ctx, ESFM_K_L2_KNN);
        if (int rc = esfm::launch_l2_knn_bf16(p.st, desc, m.hm_exp.ptr, p.plan.total_rows, m.norms.as<float>(), p.dev_tab, n_pairs, p.plan.n_blocks,
                                              p.knn_idx, p.knn_dist, m.flagged.as<int32_t>(), cnt, p.flag_cap(), m.pair_cnt.as<int32_t>(),
                                              m.pair_list.as<int32_t>()))
            return rc;
    }
    if (m.l2_audit == 1) return ESFM_OK;   // audit: leave the pass's own answer in place
    // certificate failures, binned per pair by the pass: exact re-scan, the pair's queries sharing every train row
    esfm::KernelTimer tm(p.ctx, ESFM_K_L2_RESCAN);
    return esfm::launch_l2_rescan64_pairs(p.st, desc, p.dev_tab, n_pairs, m.pair_cnt.as<int32_t>(), m.pair_list.as<int32_t>(), p.knn_idx, p.knn_dist);
}

// 128-float rows (and 64 with ESFM_L2_PASS=f32): the f32-input MFMA kernel + an exact scan of its certificate failures, grid-stride
// over the device-side count (no host sync).  Audit mode 1 stops before the scan.
int run_l2_f32_mfma(const Pass &p)
{
    esfm::MatchState &m = p.m;
    const float *desc = static_cast<const float *>(p.desc);
    int32_t *cnt = m.counters.as<int32_t>() + kOtherCounters;
    m.prep_desc = nullptr;   // the pass writes its own norms
    if (int rc = m.norms.reserve(sizeof(float) * (size_t)std::max<int64_t>(p.plan.total_rows, 1))) return rc;
    ESFM_HIP_TRY(hipMemsetAsync(cnt, 0, 64, p.st));
    if (int rc = esfm::launch_l2_norms(p.st, desc, p.width, p.plan.total_rows, m.norms.as<float>())) return rc;
    {
        esfm::KernelTimer tm(p.ctx, ESFM_K_L2_KNN);
        if (int rc = esfm::launch_l2_knn_mfma(p.st, p.width, desc, m.norms.as<float>(), p.dev_tab, p.n_pairs(), p.plan.n_blocks, p.knn_idx,
                                              p.knn_dist, m.flagged.as<int32_t>(), cnt, p.flag_cap()))
            return rc;
    }
    if (m.l2_audit == 1) return ESFM_OK;   // audit: leave the pass's own answer in place
    const int grid = (int)std::min<int64_t>(p.plan.total_queries, 8 * (int64_t)p.ctx->num_cu);
    esfm::KernelTimer tm(p.ctx, ESFM_K_L2_RESCAN);
    return esfm::launch_l2_exact_scan(p.st, p.width, desc, p.dev_tab, p.n_pairs(), m.flagged.as<int32_t>(), cnt, p.plan.total_queries, grid,
                                      p.knn_idx, p.knn_dist);
}

// No MFMA build for this width (or audit mode 2): exact scan of every query (correct, not fast).  The prepared state stays.
int run_l2_exact(const Pass &p)
{
    int32_t *cnt = p.m.counters.as<int32_t>() + kOtherCounters;
    ESFM_HIP_TRY(hipMemsetAsync(cnt, 0, 64, p.st));
    const int grid = (int)std::min<int64_t>(p.plan.total_queries, 64 * (int64_t)p.ctx->num_cu);
    return esfm::launch_l2_exact_scan(p.st, p.width, static_cast<const float *>(p.desc), p.dev_tab, p.n_pairs(), nullptr, cnt,
                                      p.plan.total_queries, grid, p.knn_idx, p.knn_dist);
}

// 256-bit rows, train sets within the position code: the FP4-MFMA form (hamming_fp4_kernel) with its exact ratio screen; for match
// lists, the ratio test + compaction inside the same launch (the last block of a pair does it).  What esfm_match_prepare_dev left
// in hm_exp counts only if it is this form (both Hamming paths: otherwise the launch derives its own and the prepared state ends).
int run_hamming_fp4(const Pass &p, bool &compacted)
{
    esfm::MatchState &m = p.m;
    const bool expanded = p.prepared && m.prep_hm_fp4;
    if (!expanded) { m.prep_desc = nullptr; if (int rc = m.hm_exp.reserve(esfm::hamming_expanded_bytes(p.width, p.plan.total_rows))) return rc; }
    const bool fuse = p.req.kind == MatchRequest::LISTS;
    esfm::KernelTimer tm(p.ctx, ESFM_K_HAMMING_KNN);
    if (fuse) { if (int rc = reserve_zeroed(m.fin_done, sizeof(int32_t) * (size_t)p.n_pairs(), p.st)) return rc; }
    if (int rc = esfm::launch_hamming_fp4(p.st, p.desc, p.plan.total_rows, m.hm_exp.ptr, p.dev_tab, blk_pair_of(p.dev_tab, p.n_pairs()),
                                          p.plan.n_blocks2, p.knn_idx, p.knn_dist, p.req.ratio, expanded, fuse ? m.fin_done.as<int32_t>() : nullptr,
                                          p.n_pairs(), p.req.query_idx, p.req.train_idx, p.req.distance, p.req.n_out))
        return rc;
    compacted = fuse;
    return ESFM_OK;
}

// HM_I8 (256-bit rows beyond the FP4 form's position code, ESFM_HM_PASS=i8: byte-per-bit i8 MFMA) and HM_VALU (128 / 512 bits:
// XOR-popcount): one launcher, which picks the kernel by width.
int run_hamming_knn(const Pass &p)
{
    const bool expanded = p.prepared && !p.m.prep_hm_fp4;
    if (!expanded) { p.m.prep_desc = nullptr; if (int rc = p.m.hm_exp.reserve(esfm::hamming_expanded_bytes(p.width, p.plan.total_rows))) return rc; }
    esfm::KernelTimer tm(p.ctx, ESFM_K_HAMMING_KNN);
    return esfm::launch_hamming_knn(p.st, p.width, p.desc, p.plan.total_rows, p.m.hm_exp.ptr, p.dev_tab, p.n_pairs(),
                                    p.plan.n_blocks, p.knn_idx, p.knn_dist, expanded);
}

// 2-NN table for every query of every pair, written to knn_idx/knn_dist (device, 2 per query), by the path select_path picks.
// `compacted`: the path also ran the ratio test + compaction of a LISTS request (else the caller does).
int knn2_core(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, int width, const PairPlan &plan, const PairDesc *dev_tab,
              int32_t *knn_idx, float *knn_dist, const MatchRequest &req, bool &compacted)
{
    compacted = false;
    if (plan.tab.empty() || plan.total_queries == 0) return ESFM_OK;
    esfm::MatchState &m = ctx->match;
    if (is_prepared(m, metric, desc_dev, plan.total_rows, width))
        if (int rc = verify_prepared(ctx, metric, desc_dev, plan.total_rows, width)) return rc;
    const Pass p{ctx, m, ctx->stream, desc_dev, width, plan, dev_tab, knn_idx, knn_dist, req, is_prepared(m, metric, desc_dev, plan.total_rows, width)};
    const MatchPath path = select_path(metric, width, plan.max_nt, m.l2_audit);
    if (int rc = esfm::check_hamming_width(metric, width)) return rc;
    if (metric == ESFM_L2_F32) {
        if (int rc = reserve_zeroed(m.counters, kCounterInts * sizeof(int32_t), ctx->stream)) return rc;
        if ((m.l2_audit == 3 || m.l2_audit == 4) && path != MatchPath::L2_ONE_PRODUCT) {
            esfm::set_error("audit modes 3 and 4 need the one-product pass (64-float descriptors, train sets <= 65536 rows, ESFM_L2_PASS unset)");
            return ESFM_ERR_UNSUPPORTED;
        }
        m.last_n_queries = plan.total_queries;
        m.counters_cur = m.counters.as<int32_t>() + kOtherCounters;   // the passes that zero their counters themselves
        if (path != MatchPath::L2_EXACT)
            if (int rc = m.flagged.reserve(sizeof(int32_t) * 2 * (size_t)p.flag_cap())) return rc;
    }
    switch (path) {
    case MatchPath::L2_ONE_PRODUCT: return run_l2_one_product(p, compacted);
    case MatchPath::L2_THREE_PRODUCT: return run_l2_three_product(p);
    case MatchPath::L2_F32_MFMA: return run_l2_f32_mfma(p);
    case MatchPath::L2_EXACT: return run_l2_exact(p);
    case MatchPath::HM_FP4: return run_hamming_fp4(p, compacted);
    case MatchPath::HM_I8:
    case MatchPath::HM_VALU: return run_hamming_knn(p);
    }
    return ESFM_ERR_INVALID_ARG;
}

int check_common(esfm_ctx *ctx, esfm_metric metric, int width)
{
    if (int rc = esfm::check_metric_width(ctx, metric, width, "descriptor width must be positive")) return rc;
    return esfm::set_device(ctx);
}

int check_cross(int use_ratio, double ratio)
{
    ESFM_REQUIRE(use_ratio == 0 || use_ratio == 1, "use_ratio must be 0 (cross) or 1 (ratio+cross)");
    ESFM_REQUIRE(use_ratio == 0 || ratio == ratio, "ratio is NaN");
    return ESFM_OK;
}

// The front of the pair-list entry points: context checks and the plan over `pairs`, out_offset its prefix sum.  mirror (the
// cross-check): the plan runs over the caller's P pairs followed by (t, q) for each of them, so one pass writes both directions'
// tables; the caller's out_offset is the forward pairs' prefix sum (they come first).
int plan_pairs(esfm_ctx *ctx, esfm_metric metric, int width, const int32_t *set_row_offset, int n_sets, const int32_t *pairs, int n_pairs,
               bool mirror, int64_t *out_offset, PairPlan *plan)
{
    if (int rc = check_common(ctx, metric, width)) return rc;
    ESFM_REQUIRE(out_offset != nullptr, "out_offset is NULL");
    if (mirror) ESFM_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || pairs != nullptr), "pairs/n_pairs");      // (the mirrored form looks at the pair list first)
    const int query_block = metric == ESFM_L2_F32 ? esfm::l2_query_block(width) : esfm::hamming_query_block(width);
    return esfm::make_plan(set_row_offset, n_sets, pairs, n_pairs, query_block, esfm::l2_x1_query_block(), mirror, esfm::kPlainPlanRules, out_offset, plan);
}

// esfm_knn2_pairs_dev / _screened_dev: the 2-NN tables into the caller's device arrays.
int knn2_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const int32_t *set_row_offset, int n_sets, int width,
                   const int32_t *pairs, int n_pairs, const MatchRequest &req, int32_t *knn_idx_dev, float *knn_dist_dev, int64_t *out_offset)
{
    PairPlan plan;
    if (int rc = plan_pairs(ctx, metric, width, set_row_offset, n_sets, pairs, n_pairs, false, out_offset, &plan)) return rc;
    if (plan.total_queries == 0) return ESFM_OK;
    ESFM_REQUIRE(desc_dev && knn_idx_dev && knn_dist_dev, "device pointer is NULL");
    const PairDesc *dev_tab = nullptr;
    if (int rc = upload_pairs(ctx, plan, &dev_tab)) return rc;
    bool compacted = false;
    return knn2_core(ctx, metric, desc_dev, width, plan, dev_tab, knn_idx_dev, knn_dist_dev, req, compacted);
}

// The match lists of a pair list into the caller's device arrays: Lowe's ratio test (esfm_match_pairs_dev, the call bench.py
// times) or, `cross`, the cross-check with (use_ratio) or without it (esfm_match_cross_pairs_dev).  Cross-check: one knn2_core
// pass over the mirrored plan writes both directions' tables with their markers; ratio+cross passes `ratio` so the screen drops
// rows in both directions (a dropped row cannot match), cross alone +inf (every row's exact 2-NN); cross_check_compact_kernel
// joins pair p with pair P + p.
int match_lists_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const int32_t *set_row_offset, int n_sets, int width,
                    const int32_t *pairs, int n_pairs, bool cross, int use_ratio, double ratio, int32_t *query_idx_dev, int32_t *train_idx_dev,
                    float *distance_dev, int32_t *n_out_dev, int64_t *out_offset)
{
    if (cross) { if (int rc = check_cross(use_ratio, ratio)) return rc; }
    PairPlan plan;
    if (int rc = plan_pairs(ctx, metric, width, set_row_offset, n_sets, pairs, n_pairs, cross, out_offset, &plan)) return rc;
    if (n_pairs == 0) return ESFM_OK;
    ESFM_REQUIRE(n_out_dev != nullptr, "n_out_dev is NULL");
    ESFM_REQUIRE(out_offset[n_pairs] == 0 || (query_idx_dev && train_idx_dev && distance_dev), "device pointer is NULL");
    ESFM_REQUIRE(plan.total_queries == 0 || desc_dev, "desc_dev is NULL");
    if (plan.total_queries == 0) {
        ESFM_HIP_TRY(hipMemsetAsync(n_out_dev, 0, sizeof(int32_t) * (size_t)n_pairs, ctx->stream));
        return ESFM_OK;
    }
    esfm::MatchState &m = ctx->match;
    const PairDesc *dev_tab = nullptr;
    if (int rc = upload_pairs(ctx, plan, &dev_tab)) return rc;
    if (int rc = m.knn_idx.reserve(sizeof(int32_t) * 2 * (size_t)plan.total_queries)) return rc;
    if (int rc = ctx->knn_dist.reserve(sizeof(float) * 2 * (size_t)plan.total_queries)) return rc;
    int32_t *knn_idx = m.knn_idx.as<int32_t>();
    float *knn_dist = ctx->knn_dist.as<float>();
    const MatchRequest req = !cross ? MatchRequest{MatchRequest::LISTS, ratio, query_idx_dev, train_idx_dev, distance_dev, n_out_dev}
                                    : use_ratio ? MatchRequest{MatchRequest::SCREENED, ratio} : MatchRequest{MatchRequest::RAW, (double)INFINITY};
    bool compacted = false;
    if (int rc = knn2_core(ctx, metric, desc_dev, width, plan, dev_tab, knn_idx, knn_dist, req, compacted)) return rc;
    if (cross) {
        esfm::KernelTimer tm(ctx, ESFM_K_CROSS_CHECK);
        return esfm::launch_cross_check_compact(ctx->stream, dev_tab, n_pairs, knn_idx, knn_dist, use_ratio, ratio, query_idx_dev, train_idx_dev,
                                                distance_dev, n_out_dev);
    }
    if (compacted) return ESFM_OK;
    return esfm::launch_ratio_compact(ctx->stream, dev_tab, n_pairs, knn_idx, knn_dist, ratio, query_idx_dev, train_idx_dev, distance_dev, n_out_dev);
}

// What a host-pointer single pair returns: the 2-NN table, or the match lists of the ratio test or the cross-check.
enum class Result { KNN2, RATIO, CROSS };

// Host-pointer single pair: stage [train rows | query rows] into one device buffer, run the pair (1, 0) through the pair-list
// driver of `what`, copy back.  KNN2: o_a / o_c the [nq, 2] tables; else the lists (o_a, o_b, o_c) and their length.
int single_pair(esfm_ctx *ctx, esfm_metric metric, const void *q, int nq, const void *t, int nt, int width, Result what, int use_ratio,
                double ratio, int32_t *o_a, int32_t *o_b, float *o_c, int32_t *n_out)
{
    if (what == Result::KNN2 && nq > 0 && (!o_a || !o_c)) { esfm::set_error("idx/dist is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (what != Result::KNN2 && (!n_out || (nq > 0 && (!o_a || !o_b || !o_c)))) { esfm::set_error("output pointer is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = check_common(ctx, metric, width)) return rc;
    ESFM_REQUIRE(nq >= 0 && nt >= 0, "negative row count");
    ESFM_REQUIRE(nq == 0 || q != nullptr, "q is NULL");
    ESFM_REQUIRE(nt == 0 || t != nullptr, "t is NULL");
    if (what == Result::CROSS) { if (int rc = check_cross(use_ratio, ratio)) return rc; }
    if (what != Result::KNN2) *n_out = 0;
    if (nq == 0) return ESFM_OK;
    const size_t row_bytes = esfm::match_row_bytes(metric, width);
    const size_t tb = row_bytes * (size_t)nt, qb = row_bytes * (size_t)nq;
    if (int rc = ctx->stage_a.reserve(tb + qb + 16)) return rc;
    hipStream_t st = ctx->stream;
    char *d = ctx->stage_a.as<char>();
    if (tb) ESFM_HIP_TRY(esfm::copy_h2d(d, t, tb, st));
    ESFM_HIP_TRY(esfm::copy_h2d(d + tb, q, qb, st));
    const int32_t offs[3] = {0, nt, nt + nq};
    const int32_t pr[2] = {1, 0};
    int64_t out_off[2];
    if (what == Result::KNN2) {
        esfm::DevBuf &idx = ctx->match.knn_idx, &dist = ctx->knn_dist;
        if (int rc = idx.reserve(sizeof(int32_t) * 2 * (size_t)nq)) return rc;
        if (int rc = dist.reserve(sizeof(float) * 2 * (size_t)nq)) return rc;
        if (int rc = knn2_pairs_dev(ctx, metric, d, offs, 2, width, pr, 1, MatchRequest{MatchRequest::RAW, (double)INFINITY}, idx.as<int32_t>(),
                                    dist.as<float>(), out_off))
            return rc;
        ESFM_HIP_TRY(esfm::copy_d2h(o_a, idx.ptr, sizeof(int32_t) * 2 * (size_t)nq, st));
        ESFM_HIP_TRY(esfm::copy_d2h(o_c, dist.ptr, sizeof(float) * 2 * (size_t)nq, st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
        return ESFM_OK;
    }
    if (int rc = esfm::reserve_match_list_stage(ctx, (size_t)nq, 1)) return rc;
    if (int rc = match_lists_dev(ctx, metric, d, offs, 2, width, pr, 1, what == Result::CROSS, use_ratio, ratio, ctx->stage_b.as<int32_t>(),
                                 ctx->stage_c.as<int32_t>(), ctx->stage_d.as<float>(), ctx->stage_e.as<int32_t>(), out_off))
        return rc;
    int32_t n = 0;
    ESFM_HIP_TRY(esfm::copy_d2h(&n, ctx->stage_e.ptr, sizeof(int32_t), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    if (int rc = esfm::match_handover_check(ctx)) return rc;
    if (n > 0) {
        ESFM_HIP_TRY(esfm::copy_d2h(o_a, ctx->stage_b.ptr, sizeof(int32_t) * (size_t)n, st));
        ESFM_HIP_TRY(esfm::copy_d2h(o_b, ctx->stage_c.ptr, sizeof(int32_t) * (size_t)n, st));
        ESFM_HIP_TRY(esfm::copy_d2h(o_c, ctx->stage_d.ptr, sizeof(float) * (size_t)n, st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
    }
    *n_out = n;
    return ESFM_OK;
}

// Host-pointer form of the batched pair loop (SURVEY 8b's esfm_match_pairs): upload once, prepare once, one launch sequence for
// the whole pair list, one read-back.  The uploaded rows stay in the context (ctx->match.bank) and stay prepared, so a second call
// on the same host buffer contents would still re-upload (the library cannot know the rows are unchanged) -- callers that match
// the same sets repeatedly keep them on the device and use esfm_match_pairs_dev.  (cross: as match_lists_dev)
int match_pairs_host(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets, int width,
                     const int32_t *pairs, int n_pairs, bool cross, int use_ratio, double ratio, int32_t *query_idx, int32_t *train_idx,
                     float *distance, int32_t *n_out, int64_t *out_offset)
{
    if (cross) { if (int rc = check_cross(use_ratio, ratio)) return rc; }
    PairPlan plan;
    if (int rc = plan_pairs(ctx, metric, width, set_row_offset, n_sets, pairs, n_pairs, false, out_offset, &plan)) return rc;
    if (n_pairs == 0) return ESFM_OK;
    ESFM_REQUIRE(n_out != nullptr, "n_out is NULL");
    for (int p = 0; p < n_pairs; ++p) n_out[p] = 0;
    if (plan.total_queries == 0) return ESFM_OK;
    ESFM_REQUIRE(desc_host && query_idx && train_idx && distance, "host pointer is NULL");
    hipStream_t st = ctx->stream;
    esfm::DevBuf &bank = ctx->match.bank;
    const size_t bytes = esfm::match_row_bytes(metric, width) * (size_t)plan.total_rows;
    ctx->match.prep_desc = nullptr;                // the bank below is rewritten: whatever was prepared from it is stale
    if (int rc = bank.reserve(bytes + 16)) return rc;
    ESFM_HIP_TRY(esfm::copy_h2d(bank.ptr, desc_host, bytes, st));
    if (int rc = esfm_match_prepare_dev(ctx, metric, bank.ptr, plan.total_rows, width)) return rc;
    const size_t nq = (size_t)plan.total_queries;
    if (int rc = esfm::reserve_match_list_stage(ctx, nq, n_pairs)) return rc;
    std::vector<int64_t> off2((size_t)n_pairs + 1);
    if (int rc = match_lists_dev(ctx, metric, bank.ptr, set_row_offset, n_sets, width, pairs, n_pairs, cross, use_ratio, ratio, ctx->stage_b.as<int32_t>(),
                                 ctx->stage_c.as<int32_t>(), ctx->stage_d.as<float>(), ctx->stage_e.as<int32_t>(), off2.data()))
        return rc;
    // packed on the device when the matches are less than a quarter of the slots, otherwise the arrays go back whole
    if (int rc = esfm::read_back_match_lists(ctx, n_pairs, off2.data(), nq, true, query_idx, train_idx, distance, n_out)) return rc;
    return esfm::match_handover_check(ctx);
}

// The first n of the last L2 call's 16 counters (zeros before any L2 call); synchronises.
int read_last_counters(esfm_ctx *ctx, int32_t *dst, int n)
{
    if (int rc = esfm::set_device(ctx)) return rc;
    std::fill(dst, dst + n, 0);
    if (!ctx->match.counters_cur) return ESFM_OK;
    ESFM_HIP_TRY(esfm::copy_d2h(dst, ctx->match.counters_cur, sizeof(int32_t) * (size_t)n, ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return esfm::match_handover_check(ctx);
}

}  // namespace

// After a synchronisation of the stream: did a finish workgroup of a fused launch give up waiting for its pair's pass blocks?  (Never
// seen; the wait is bounded so that a broken launch cannot hang the device.)  The call's lists are incomplete then, and its
// hand-over and arrival counters are left dirty: they are cleared here, and the caller gets an error.
int esfm::match_handover_check(esfm_ctx *ctx)
{
    esfm::MatchState &m = ctx->match;
    if (!m.handover_pending || !m.counters.ptr) return ESFM_OK;
    int32_t w = 0;
    ESFM_HIP_TRY(esfm::copy_d2h(&w, m.counters.as<int32_t>() + kHandoverFailWord, sizeof(w), ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    m.handover_pending = false;
    if (w == 0) return ESFM_OK;
    ESFM_HIP_TRY(hipMemsetAsync(m.counters.as<int32_t>() + kHandoverFailWord, 0, sizeof(int32_t), ctx->stream));
    if (m.pass_done.ptr) ESFM_HIP_TRY(hipMemsetAsync(m.pass_done.ptr, 0, m.pass_done.cap, ctx->stream));
    if (m.fin_done.ptr) ESFM_HIP_TRY(hipMemsetAsync(m.fin_done.ptr, 0, m.fin_done.cap, ctx->stream));
    ESFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    esfm::set_error("matcher: a finish workgroup of the fused L2 launch timed out waiting for its pair's distance-pass blocks; the last match lists are incomplete");
    return ESFM_ERR_HIP;
}

extern "C" {

int esfm_knn2_l2_f32(esfm_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim, int32_t *idx, float *dist)
{
    return single_pair(ctx, ESFM_L2_F32, q, nq, t, nt, dim, Result::KNN2, 0, 0.0, idx, nullptr, dist, nullptr);
}

int esfm_knn2_hamming(esfm_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int nbytes, int32_t *idx, float *dist)
{
    return single_pair(ctx, ESFM_HAMMING, q, nq, t, nt, nbytes, Result::KNN2, 0, 0.0, idx, nullptr, dist, nullptr);
}

int esfm_match_l2_f32(esfm_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim, double ratio,
                      int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    return single_pair(ctx, ESFM_L2_F32, q, nq, t, nt, dim, Result::RATIO, 0, ratio, query_idx, train_idx, distance, n_out);
}

int esfm_match_hamming(esfm_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int nbytes, double ratio,
                       int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    return single_pair(ctx, ESFM_HAMMING, q, nq, t, nt, nbytes, Result::RATIO, 0, ratio, query_idx, train_idx, distance, n_out);
}

int esfm_knn2_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const int32_t *set_row_offset, int n_sets,
                        int width, const int32_t *pairs, int n_pairs, int32_t *knn_idx_dev, float *knn_dist_dev,
                        int64_t *out_offset)
{
    return knn2_pairs_dev(ctx, metric, desc_dev, set_row_offset, n_sets, width, pairs, n_pairs, MatchRequest{MatchRequest::RAW, (double)INFINITY},
                          knn_idx_dev, knn_dist_dev, out_offset);
}

// Audit of the Hamming matcher's ratio screen (tests): the raw table of a call that screens with `ratio` -- the queries the pass
// dropped as "cannot pass d0 < ratio d1" carry train index -2 in both slots, every other query its exact 2-NN.
int esfm_knn2_pairs_screened_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const int32_t *set_row_offset, int n_sets,
                                 int width, const int32_t *pairs, int n_pairs, double ratio, int32_t *knn_idx_dev, float *knn_dist_dev,
                                 int64_t *out_offset)
{
    if (metric != ESFM_HAMMING) { esfm::set_error("esfm_knn2_pairs_screened_dev: Hamming only (the L2 screen is audited through esfm_ctx_set_l2_audit mode 4)"); return ESFM_ERR_UNSUPPORTED; }
    if (!(ratio == ratio)) { esfm::set_error("ratio is NaN"); return ESFM_ERR_INVALID_ARG; }
    return knn2_pairs_dev(ctx, metric, desc_dev, set_row_offset, n_sets, width, pairs, n_pairs, MatchRequest{MatchRequest::SCREENED, ratio},
                          knn_idx_dev, knn_dist_dev, out_offset);
}

int esfm_match_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const int32_t *set_row_offset, int n_sets,
                         int width, const int32_t *pairs, int n_pairs, double ratio, int32_t *query_idx_dev,
                         int32_t *train_idx_dev, float *distance_dev, int32_t *n_out_dev, int64_t *out_offset)
{
    return match_lists_dev(ctx, metric, desc_dev, set_row_offset, n_sets, width, pairs, n_pairs, false, 0, ratio, query_idx_dev, train_idx_dev,
                           distance_dev, n_out_dev, out_offset);
}

int esfm_match_pairs(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets, int width,
                     const int32_t *pairs, int n_pairs, double ratio, int32_t *query_idx, int32_t *train_idx, float *distance,
                     int32_t *n_out, int64_t *out_offset)
{
    return match_pairs_host(ctx, metric, desc_host, set_row_offset, n_sets, width, pairs, n_pairs, false, 0, ratio, query_idx, train_idx, distance,
                            n_out, out_offset);
}

// ---- cross-check (include/esfm.h "Cross-check matching")
int esfm_match_cross_l2_f32(esfm_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim, int use_ratio, double ratio,
                            int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    return single_pair(ctx, ESFM_L2_F32, q, nq, t, nt, dim, Result::CROSS, use_ratio, ratio, query_idx, train_idx, distance, n_out);
}

int esfm_match_cross_hamming(esfm_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int nbytes, int use_ratio,
                             double ratio, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    return single_pair(ctx, ESFM_HAMMING, q, nq, t, nt, nbytes, Result::CROSS, use_ratio, ratio, query_idx, train_idx, distance, n_out);
}

int esfm_match_cross_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const int32_t *set_row_offset, int n_sets,
                               int width, const int32_t *pairs, int n_pairs, int use_ratio, double ratio, int32_t *query_idx_dev,
                               int32_t *train_idx_dev, float *distance_dev, int32_t *n_out_dev, int64_t *out_offset)
{
    return match_lists_dev(ctx, metric, desc_dev, set_row_offset, n_sets, width, pairs, n_pairs, true, use_ratio, ratio, query_idx_dev, train_idx_dev,
                           distance_dev, n_out_dev, out_offset);
}

int esfm_match_cross_pairs(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets, int width,
                           const int32_t *pairs, int n_pairs, int use_ratio, double ratio, int32_t *query_idx, int32_t *train_idx,
                           float *distance, int32_t *n_out, int64_t *out_offset)
{
    return match_pairs_host(ctx, metric, desc_host, set_row_offset, n_sets, width, pairs, n_pairs, true, use_ratio, ratio, query_idx, train_idx,
                            distance, n_out, out_offset);
}

int esfm_match_prepare_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, int64_t total_rows, int width)
{
    if (int rc = check_common(ctx, metric, width)) return rc;
    ESFM_REQUIRE(total_rows >= 0 && total_rows < ((int64_t)1 << 31), "total_rows");
    ESFM_REQUIRE(total_rows == 0 || desc_dev != nullptr, "desc_dev is NULL");
    esfm::MatchState &m = ctx->match;
    m.prep_desc = nullptr;
    if (total_rows == 0) return ESFM_OK;
    hipStream_t st = ctx->stream;
    // what the product path of this metric and width derives, whatever the audit mode; max_nt 0: a later call whose train sets do
    // not fit the position code re-derives (L2: its fallback writes its own operands; Hamming: the i8 form's byte image)
    const MatchPath path = select_path(metric, width, 0, 0);
    if (path == MatchPath::L2_ONE_PRODUCT) {
        if (int rc = reserve_zeroed(m.counters, kCounterInts * sizeof(int32_t), st)) return rc;
        if (int rc = derive_l2_images(ctx, static_cast<const float *>(desc_dev), total_rows)) return rc;
    } else if (path == MatchPath::HM_FP4 || path == MatchPath::HM_I8) {
        if (int rc = m.hm_exp.reserve(esfm::hamming_expanded_bytes(width, total_rows))) return rc;
        m.prep_hm_fp4 = path == MatchPath::HM_FP4;
        if (m.prep_hm_fp4) { if (int rc = esfm::launch_hamming_expand_fp4(st, desc_dev, total_rows, m.hm_exp.ptr)) return rc; }
        else if (int rc = esfm::launch_hamming_expand(st, width, desc_dev, total_rows, m.hm_exp.ptr)) return rc;
    } else {
        return ESFM_OK;       // nothing to derive for this metric / width: the match calls work on the rows themselves
    }
    m.prep_has_sum = false;
    if (m.prep_check) {
        if (int rc = m.prep_sum.reserve(2 * sizeof(unsigned long long))) return rc;
        if (int rc = esfm::launch_buffer_checksum(st, desc_dev, (size_t)total_rows * esfm::match_row_bytes(metric, width), m.prep_sum.as<unsigned long long>())) return rc;
        m.prep_has_sum = true;
    }
    m.prep_desc = desc_dev; m.prep_metric = (int)metric; m.prep_rows = total_rows; m.prep_width = width;
    return ESFM_OK;
}

int esfm_ctx_set_prepared_check(esfm_ctx *ctx, int enable)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    ctx->match.prep_check = enable ? 1 : 0;
    return ESFM_OK;
}

int esfm_match_release_prepared(esfm_ctx *ctx)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    ctx->match.prep_desc = nullptr;
    return ESFM_OK;
}

int esfm_match_release_prepared_buffer(esfm_ctx *ctx, const void *desc_dev)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (ctx->match.prep_desc == desc_dev) ctx->match.prep_desc = nullptr;
    return ESFM_OK;
}

int esfm_match_prepared_buffer(esfm_ctx *ctx, const void **desc_dev_out)
{
    if (!ctx || !desc_dev_out) { esfm::set_error("esfm_match_prepared_buffer: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    *desc_dev_out = ctx->match.prep_desc;
    return ESFM_OK;
}

int esfm_match_last_stats(esfm_ctx *ctx, int64_t *n_queries, int64_t *n_rescanned)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    int32_t c = 0;
    if (int rc = read_last_counters(ctx, &c, 1)) return rc;
    if (n_queries) *n_queries = ctx->match.last_n_queries;
    if (n_rescanned) *n_rescanned = c;
    return ESFM_OK;
}

int esfm_match_last_second_pass(esfm_ctx *ctx, int64_t *n_second_pass)
{
    if (!ctx || !n_second_pass) { esfm::set_error("esfm_match_last_second_pass: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    int32_t c[2];
    if (int rc = read_last_counters(ctx, c, 2)) return rc;
    *n_second_pass = c[1];
    return ESFM_OK;
}

int esfm_match_debug_counters(esfm_ctx *ctx, int32_t *out16)
{
    if (!ctx || !out16) { esfm::set_error("esfm_match_debug_counters: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    return read_last_counters(ctx, out16, 16);
}

int esfm_ctx_set_l2_audit(esfm_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 4) { esfm::set_error("esfm_ctx_set_l2_audit: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    ctx->match.l2_audit = mode;
    return ESFM_OK;
}

int esfm_ctx_set_l2_two_launch(esfm_ctx *ctx, int enable)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    ctx->match.l2_two_launch = enable ? 1 : 0;
    return ESFM_OK;
}

int esfm_match_last_flagged(esfm_ctx *ctx, int32_t *out, int64_t cap, int64_t *n)
{
    if (!ctx || !n || cap < 0 || (cap > 0 && !out)) { esfm::set_error("esfm_match_last_flagged: bad arguments"); return ESFM_ERR_INVALID_ARG; }
    int32_t c = 0;
    if (int rc = read_last_counters(ctx, &c, 1)) return rc;
    *n = c;
    const esfm::DevBuf &flagged = ctx->match.flagged;
    const int64_t k = std::min<int64_t>(std::min<int64_t>(c, cap), (int64_t)(flagged.cap / (2 * sizeof(int32_t))));
    if (k > 0) {
        ESFM_HIP_TRY(esfm::copy_d2h(out, flagged.ptr, sizeof(int32_t) * 2 * (size_t)k, ctx->stream));
        ESFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return ESFM_OK;
}

// Pair list of the reference's loop (sfm.cpp:140-143), sharded.  Greedy longest-processing-time
// over pairs sorted by descending cost keeps shards within one pair's cost of each other; inside a
// shard the reference order (i ascending, j ascending) is kept so results concatenate trivially.
int esfm_shard_pair_list(int n_frames, const int32_t *rows_per_frame, int rank, int world, int32_t *pairs_out)
{
    if (n_frames < 0 || world < 1 || rank < 0 || rank >= world || !pairs_out) {
        esfm::set_error("esfm_shard_pair_list: bad arguments");
        return ESFM_ERR_INVALID_ARG;
    }
    struct Item { int i, j; double cost; };
    std::vector<Item> items;
    items.reserve((size_t)n_frames * (size_t)std::max(n_frames - 1, 0) / 2);
    for (int i = 0; i < n_frames; ++i)
        for (int j = 0; j < i; ++j)
            items.push_back({i, j, rows_per_frame ? (double)rows_per_frame[i] * (double)rows_per_frame[j] : 1.0});
    std::vector<int> order(items.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = (int)k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return items[(size_t)a].cost > items[(size_t)b].cost; });
    std::vector<double> load((size_t)world, 0.0);
    std::vector<char> mine(items.size(), 0);
    for (int k : order) {
        int best = 0;
        for (int w = 1; w < world; ++w) if (load[(size_t)w] < load[(size_t)best]) best = w;
        load[(size_t)best] += items[(size_t)k].cost;
        if (best == rank) mine[(size_t)k] = 1;
    }
    int n = 0;
    for (size_t k = 0; k < items.size(); ++k)
        if (mine[k]) { pairs_out[2 * n] = items[k].i; pairs_out[2 * n + 1] = items[k].j; ++n; }
    return n;
}

}  // extern "C"
