// Shared host-side plumbing of libesfm_hip.so: context, error reporting, device scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/esfm.h"
#include "error.hpp"   // set_error, get_error, ESFM_REQUIRE

namespace esfm {

#define ESFM_HIP_TRY(expr)                                                                      \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            ::esfm::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, \
                              __LINE__);                                                        \
            (void)hipGetLastError();   /* reported here: not left for the next call's launch check */ \
            return e__ == hipErrorOutOfMemory ? ESFM_ERR_OOM : ESFM_ERR_HIP;                    \
        }                                                                                       \
    } while (0)

// Host <-> device copies of caller-owned memory (ordered on `st` like hipMemcpyAsync; pageable memory makes them synchronous).
// The HIP runtime PINS a pageable buffer of 1 MiB or more for the transfer -- a userptr registration with the kernel driver -- and
// the driver stops every queue of the process while it re-validates such a registration after ordinary heap activity in the same
// mapping (malloc / free trimming the heap): bin/sfm_native's 768 x 512 x 3 images (1.18 MB) stalled a third of the frames for
// 20 - 38 ms each, ten times what their detection takes (profiles/r05_driver_surf_undistort_pnp.txt: the time sits inside hipMemcpyAsync; with
// GPU_PINNED_MIN_XFER_SIZE raised the stalls are gone).  Pieces below that size go through the runtime's own staging buffer
// instead, whatever the process' environment says.
// A buffer the caller has registered or allocated through HIP (hipHostRegister / hipHostMalloc) is pinned already and goes in one
// asynchronous transfer.  Price of the pieces: a pageable transfer runs at the speed of the host's copy into the staging buffer,
// 16 GB/s, instead of the DMA engines' 49 GB/s (esfm_undistort of a 3072 x 2048 x 3 image, both directions: 0.8 -> 2.3 ms;
// from registered memory 0.77 ms; the same record) -- bounded and proportional, unlike the stalls.
constexpr size_t kCopyPiece = 512u << 10;
inline bool host_memory_is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }      // (an ordinary malloc'ed pointer: "invalid value"; the sticky error is cleared)
    return a.type == hipMemoryTypeHost;
}
inline hipError_t copy_pieces(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, const void *host_side, hipStream_t st)
{
    if (bytes <= kCopyPiece || host_memory_is_pinned(host_side)) return bytes ? hipMemcpyAsync(dst, src, bytes, kind, st) : hipSuccess;
    for (size_t off = 0; off < bytes; off += kCopyPiece) {
        const size_t n = bytes - off < kCopyPiece ? bytes - off : kCopyPiece;
        const hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + off, static_cast<const char *>(src) + off, n, kind, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
inline hipError_t copy_h2d(void *dst_dev, const void *src_host, size_t bytes, hipStream_t st) { return copy_pieces(dst_dev, src_host, bytes, hipMemcpyHostToDevice, src_host, st); }
inline hipError_t copy_d2h(void *dst_host, const void *src_dev, size_t bytes, hipStream_t st) { return copy_pieces(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, dst_host, st); }

// A grow-only device buffer (scratch reused across calls; 288 GB of HBM makes
// holding on to the high-water mark the right trade).
struct DevBuf {
    void *ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes);
    void release();
    template <class T> T *as() const { return reinterpret_cast<T *>(ptr); }
};

// The matcher's context state (match_api.cpp alone touches it).
struct MatchState {
    DevBuf bank;   // esfm_match_pairs (host-pointer batched form): the uploaded descriptor rows of all sets
    DevBuf norms, pair_tab, knn_idx, flagged, counters;
    DevBuf pair_cnt, pair_list;   // three-product pass: its uncertified queries binned per pair (one counter per pair; the pair's slice of the query numbering)
    // one-product pass, per-pair counters in two phases (a call fills phase l2_phase, its first kernel zeroes the other for the next
    // call): the queries the re-rank left uncertified, listed in pair_list2, and the ratio screen's survivors, 48-byte entries in surv_list
    DevBuf unc_cnt[2], surv_cnt[2], pair_list2, surv_list;
    int l2_phase = 0;                  // phase the NEXT one-product call fills
    int l2_phase_pairs[2] = {0, 0};    // entries of each phase that may be non-zero
    int32_t *counters_cur = nullptr;   // the 16 counters of the last L2 call (esfm_match_last_stats / _second_pass / _flagged)
    DevBuf fin_done;   // l2_finish_kernel / hamming_fp4_kernel: per-pair arrival counters
    DevBuf pass_done;  // l2_fused_kernel: per-pair count of finished pass blocks, the hand-over to the pair's finish workgroups (zero between calls)
    int l2_two_launch = 0;          // esfm_ctx_set_l2_two_launch (ESFM_L2_TWO_LAUNCH at context creation): keep pass and finish as two launches
    bool handover_pending = false;  // a fused launch has been enqueued since the failure word (counters[kHandoverFailWord]) was last read
    DevBuf knn_d2;     // exact second-best d^2 of the queries the one-product pass left uncertified (the refine pass's thresholds)
    DevBuf l2_hi;      // one-product pass: bf16(t) and bf16(-2 q) images (128 B per row each) and the two residual norms per row
    DevBuf hm_exp;     // Hamming: the FP4 form's nibble images or the i8 form's 0/1 bytes + start values (260 B per row); three-product pass: its split images
    // esfm_match_prepare_dev: the derived per-row operands (bf16 images, norms, residual norms; the Hamming images) in l2_hi / norms /
    // hm_exp belong to this descriptor buffer and are not recomputed by the match calls
    const void *prep_desc = nullptr;
    int prep_metric = 0, prep_width = 0;
    bool prep_hm_fp4 = false;   // Hamming: hm_exp holds the FP4 form's nibble images (hamming_fp4_kernel), not the byte image of the i8 form
    int64_t prep_rows = 0;
    // esfm_ctx_set_prepared_check: the prepared buffer's fingerprint ([0] at prepare, [1] re-derived by every match call that relies on it)
    int prep_check = 0;
    bool prep_has_sum = false;
    DevBuf prep_sum;
    int64_t last_n_queries = 0;
    size_t last_pair_bytes = 0;   // the pair table last uploaded (its copy is in esfm_ctx::pinned)
    int l2_audit = 0;   // esfm_ctx_set_l2_audit: 0 product path, 1 no re-scan, 2 exact scan of every query, 3 one-product pass alone, 4 one-product pass alone with the ratio screen's rejections listed
    void release()   // (every DevBuf above)
    {
        for (DevBuf *b : {&bank, &norms, &pair_tab, &knn_idx, &flagged, &counters, &pair_cnt, &pair_list, &unc_cnt[0], &unc_cnt[1], &surv_cnt[0],
                          &surv_cnt[1], &pair_list2, &surv_list, &fin_done, &pass_done, &knn_d2, &l2_hi, &hm_exp, &prep_sum}) b->release();
    }
};

}  // namespace esfm

struct esfm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    int num_cu = 256;
    // shared scratch of the API modules (stage_b .. stage_e: the host-pointer matchers' device-side lists, stage_a their packed
    // read-back, match_readback.cpp); knn_dist is also ORB detection's keypoint scratch (orb_api.cpp), the rest of the matcher's
    // state is in `match`
    esfm::DevBuf knn_dist, stage_a, stage_b, stage_c, stage_d, stage_e;
    esfm::MatchState match;
    // the guided matcher's own scratch (guided_api.cpp alone touches it; nothing of `match` is shared with it): pair + geometry tables,
    // both directions' 2-NN tables, and the host-pointer forms' uploaded descriptor rows and keypoints
    esfm::DevBuf guided_tab, guided_idx, guided_dist, guided_bank, guided_kp;
    // image retrieval's own scratch (retrieval_api.cpp alone touches it): every intermediate of the chain in one carved buffer, and
    // the host-pointer forms' uploaded descriptor rows
    esfm::DevBuf retrieval, retrieval_bank;
    double retrieval_stage_ms[4] = {0, 0, 0, 0};   // under esfm_ctx_set_kernel_timing: the last esfm_retrieval_pairs[_dev] call's train, assign + accumulate, finalise, rank
    // track completion's own scratch (complete_api.cpp alone touches it): every intermediate in one carved buffer, and the
    // host-pointer form's uploaded descriptor rows and keypoints
    esfm::DevBuf complete, complete_bank, complete_kp;
    // pinned host staging for small tables / counters
    void *pinned = nullptr;
    size_t pinned_cap = 0;
    int pin(size_t bytes);
    // a second pinned area for the per-round tables of the RANSAC loops (samples up, model counts and inlier counts down)
    void *pinned_rounds = nullptr;
    size_t pinned_rounds_cap = 0;
    int pin_rounds(size_t bytes);
    // device chunks and pinned scalar mailboxes of destroyed BA problems, kept for the next problem of this context (an incremental
    // reconstruction sets one up and tears it down every ba_frequency frames: ba_api.cpp ba_dev_alloc_bytes / esfm_ba_problem_destroy)
    struct BaChunk { void *ptr; size_t bytes; };
    std::vector<BaChunk> ba_chunks;
    std::vector<void *> ba_mailboxes;
    // optional per-kernel hipEvent timing (esfm_ctx_set_kernel_timing)
    bool timing = false;
    struct TimedLaunch { int id; hipEvent_t a, b; };
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t take_event();
    void time_begin(int id);
    void time_end();
};

namespace esfm {
// RAII bracket: records events around a launch when timing is enabled, otherwise does nothing.
struct KernelTimer {
    esfm_ctx *c;
    KernelTimer(esfm_ctx *ctx, int id) : c(ctx && ctx->timing ? ctx : nullptr) { if (c) c->time_begin(id); }
    ~KernelTimer() { if (c) c->time_end(); }
};
// match_api.cpp: after a stream synchronisation, the fused L2 launch's hand-over failure word as an error (ESFM_OK when no fused
// launch has been enqueued since the last look: no device traffic then)
int match_handover_check(esfm_ctx *ctx);
inline int set_device(const esfm_ctx *ctx)
{
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) { set_error("hipSetDevice(%d): %s", ctx->device, hipGetErrorString(e)); return ESFM_ERR_HIP; }
    return ESFM_OK;
}
}  // namespace esfm
