/*
 * esfm.h -- C ABI of the MI355X-native EasySFM hot path (libesfm_hip.so).
 *
 * The reference (YuePanEdward/EasySFM) has no plugin/FFI layer: its de-facto
 * boundary for this path is three C++ member functions called from
 * cpp_code/test/sfm.cpp (the pair loop :140-161 and the BA sites :262,:314,:325):
 *
 *   FeatureMatching::matchFeaturesORB   cpp_code/include/feature_matching.h:17-18
 *   FeatureMatching::matchFeaturesSURF  cpp_code/include/feature_matching.h:20-21
 *   BundleAdjustment::doSFMBA           cpp_code/include/ba.h:84
 *
 * Every entry point below is what a binding for one of those call sites would
 * bind (plain pointers and sizes, no C++/torch/OpenCV types).  INTEGRATION.md
 * shows the few lines a maintainer adds to feature_matching.cpp / ba.cpp.
 *
 * Conventions
 *   - return value: ESFM_OK (0) or a negative esfm_status; nothing throws.
 *   - esfm_last_error() returns a thread-local, human-readable message for
 *     the last failing call on this thread.
 *   - "host" pointers are ordinary CPU memory; "_dev" entry points take HIP
 *     device pointers that are already resident in HBM and enqueue all work on
 *     the context's stream without synchronising (the caller synchronises).
 *     Host buffers travel in 512-KiB pieces through the runtime's staging
 *     buffer (the runtime would otherwise pin buffers of 1 MiB and more in
 *     place, which stalls the process' queues when the heap around them
 *     changes); a buffer the caller has registered (hipHostRegister) or
 *     allocated with hipHostMalloc goes in one DMA transfer -- worth doing for
 *     images and descriptor banks that are handed over repeatedly.
 *   - one esfm_ctx per host thread and per GPU; a context is not thread-safe.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute
 *     entry point fails with ESFM_ERR_NO_DEVICE.
 */
#ifndef ESFM_H_
#define ESFM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESFM_VERSION_MAJOR 0
#define ESFM_VERSION_MINOR 1

typedef enum esfm_status {
    ESFM_OK = 0,
    ESFM_ERR_INVALID_ARG = -1,
    ESFM_ERR_NO_DEVICE = -2,   /* no HIP device / not gfx950 / HIP runtime error at init */
    ESFM_ERR_HIP = -3,         /* a HIP runtime call failed; see esfm_last_error()        */
    ESFM_ERR_OOM = -4,
    ESFM_ERR_UNSUPPORTED = -5, /* e.g. descriptor width the kernels are not built for     */
    ESFM_ERR_NUMERIC = -6,     /* BA: non-finite input or an unusable linear system       */
    ESFM_ERR_COMM = -7,        /* BA: the all-reduce callback reported failure             */
    ESFM_ERR_STALE_PREPARED = -8 /* matching: a prepared descriptor buffer no longer holds the rows it was prepared from
                                    (only detected under esfm_ctx_set_prepared_check)       */
} esfm_status;

typedef struct esfm_ctx esfm_ctx;

/* ---- library / context -------------------------------------------------- */

/* "major.minor" of the ABI above. */
const char *esfm_version(void);
/* Message for the last error raised on the calling thread ("" if none). */
const char *esfm_last_error(void);
/* Number of visible HIP devices (0 when there is none; never fails). */
int esfm_device_count(void);

/* Creates a context on HIP device `device`.  `hip_stream` is a hipStream_t the
 * caller owns (e.g. torch.cuda.current_stream().cuda_stream) or NULL, in which
 * case the context creates and owns a non-blocking stream. */
int esfm_ctx_create(int device, void *hip_stream, esfm_ctx **out);
int esfm_ctx_destroy(esfm_ctx *ctx);
/* Blocks until everything enqueued on the context's stream has finished. */
int esfm_ctx_synchronize(esfm_ctx *ctx);
/* The hipStream_t the context enqueues on (for HIP-event timing by the caller). */
void *esfm_ctx_stream(esfm_ctx *ctx);

/* Per-kernel device timing (measurement only; off by default).  When enabled,
 * the library brackets each launch of the kernels below with hipEvents on the
 * context's stream.  esfm_ctx_kernel_time() synchronises the stream, adds the
 * elapsed times of all launches since the last call for that kernel to
 * *total_ms / *launches (caller zero-initialises) and recycles the events. */
typedef enum esfm_kernel_id {
    ESFM_K_L2_KNN = 0,        /* l2_knn_bf16x1_kernel (dim 64) / l2_knn_mfma_kernel: MFMA distance pass + fused top-k + re-rank */
    ESFM_K_HAMMING_KNN = 1,   /* hamming_fp4_kernel (256 bit; + its expansion when the buffer is not prepared) / hamming_knn_mfma_kernel / hamming_knn_kernel */
    ESFM_K_BA_LINEARIZE = 2,  /* ba_linearize_kernel: the Jacobian sweep                        */
    ESFM_K_BA_SCHUR = 3,      /* ba_schur_kernel                                                */
    ESFM_K_BA_SOLVE = 4,      /* ba_chol_solve_kernel                                           */
    ESFM_K_L2_RESCAN = 5,     /* l2_exact_scan_kernel                                           */
    ESFM_K_SOR_KNN = 6,       /* sor_knn_mean_kernel: k-NN mean distances of the outlier filter   */
    ESFM_K_TRIANGULATE = 7,   /* triangulate_dlt_kernel                                         */
    ESFM_K_RANSAC = 8,        /* essential_setup + _roots + _score kernels (one chunk); homography_solve + _score (one chunk) */
    ESFM_K_SURF_DET = 9,      /* surf_det_trace_kernel                                          */
    ESFM_K_SURF_DESC = 10,    /* the four descriptor launches: surf_orient / window / rowsum / vector */
    ESFM_K_UNDISTORT = 11,    /* undistort_remap_kernel                                         */
    ESFM_K_ORB_FAST = 12,     /* orb_fast_kernel: FAST-9/16 score of every pyramid pixel          */
    ESFM_K_L2_SECOND = 13,    /* l2_finish_kernel: everything behind the one-product pass (re-rank of the ratio screen's survivors, threshold filter, ratio test, compaction) */
    ESFM_K_CROSS_CHECK = 14,  /* cross_check_compact_kernel: the mutual-nearest-neighbour join of esfm_match_cross_*       */
    ESFM_K_SIFT_PYR = 15,     /* esfm_sift_detect_and_compute: Gaussian pyramid, DoG and extrema (all octaves, one bracket) */
    ESFM_K_SIFT_DESC = 16,    /* esfm_sift_detect_and_compute: sift_orient_kernel and sift_describe_kernel                   */
    ESFM_K_MVS_SWEEP = 17,    /* esfm_mvs_depth_maps: mvs_sweep_kernel (plane sweep, all views x tiles in one launch)       */
    ESFM_K_MVS_FUSE = 18,     /* esfm_mvs_fuse: mvs_fuse_kernel, the block-offset scan and the ordered write                */
    ESFM_K_COUNT = 19,        /* the ids above; its value is pinned (tests/test_mvs_cpu.py), so later ids follow it and ESFM_K_END bounds them */
    ESFM_K_COMPLETE_GRID = 19,   /* esfm_track_complete: complete_box_kernel, complete_keys_kernel and the radix sort of the grid keys  */
    ESFM_K_COMPLETE_JOBS = 20,   /* esfm_track_complete: the job count over n_pt x n_cam, its block scan and complete_jobs_kernel      */
    ESFM_K_COMPLETE_SEARCH = 21, /* esfm_track_complete: complete_search_kernel (with the claims), complete_decode_kernel, the stats   */
    ESFM_K_END = 22           /* one past the last id esfm_ctx_kernel_time accepts */
} esfm_kernel_id;
int esfm_ctx_set_kernel_timing(esfm_ctx *ctx, int enable);
int esfm_ctx_kernel_time(esfm_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);

/* ---- pairwise matching ---------- */

/*
 * 2-NN search, the replacement for
 *   matcher.knnMatch(q.descriptors, t.descriptors, nn2, 2)
 * at cpp_code/src/feature_matching.cpp:125 (SURF, float L2; exact brute force
 * as in python_code/feature_match.py:33-34) and :80 (ORB, "BruteForce-Hamming").
 *
 * Output for query row i: idx[2*i+k], dist[2*i+k], k = 0 (nearest), 1 (second).
 * Ordering rule: ascending (distance, train index); ties go to the lower
 * train index.  L2 distance = sqrtf of the float squared distance summed in the
 * order documented in oracle/match_ref.c; Hamming distance is the exact bit
 * count as float.  Missing neighbours (nt < 2) are reported as idx -1,
 * dist FLT_MAX.  Host pointers.
 */
int esfm_knn2_l2_f32(esfm_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim,
                     int32_t *idx /*2*nq*/, float *dist /*2*nq*/);
int esfm_knn2_hamming(esfm_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int nbytes,
                      int32_t *idx /*2*nq*/, float *dist /*2*nq*/);

/*
 * Whole body of FeatureMatching::matchFeaturesSURF / matchFeaturesORB
 * (cpp_code/src/feature_matching.cpp:115-142 / :71-97) minus printing and GUI:
 * 2-NN, then keep query i iff (double)d0 < ratio * (double)d1 (:133 / :88),
 * survivors in ascending query order.  Writes at most nq entries to each output
 * array (cv::DMatch::queryIdx, ::trainIdx, ::distance) and the count to *n_out.
 * With nt < 2 (undefined behaviour in the reference) nothing is emitted.
 * Host pointers.
 */
int esfm_match_l2_f32(esfm_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim, double ratio,
                      int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out);
int esfm_match_hamming(esfm_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int nbytes,
                       double ratio, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out);

/*
 * Batched form of the pair loop cpp_code/test/sfm.cpp:140-161: all descriptor
 * sets live in ONE device buffer (`desc_dev`, rows concatenated, row stride =
 * dim floats or nbytes bytes); set s owns rows [set_row_offset[s],
 * set_row_offset[s+1]).  pairs[2*p] = query set, pairs[2*p+1] = train set
 * (the reference uses query = later frame i, train = earlier frame j < i).
 *
 * Outputs are device buffers: pair p owns the slice
 * [out_offset[p], out_offset[p] + nq_p) of query_idx/train_idx/distance, of
 * which the first n_out[p] entries are valid, query-ascending.  out_offset is
 * a HOST array of n_pairs+1 entries filled by the call (exclusive prefix sum
 * of nq_p), so the device arrays need sum(nq_p) entries.
 * set_row_offset and pairs are HOST arrays.  Work is enqueued on the context's
 * stream; the call does not synchronise.
 */
typedef enum esfm_metric { ESFM_L2_F32 = 0, ESFM_HAMMING = 1 } esfm_metric;

int esfm_match_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev,
                         const int32_t *set_row_offset, int n_sets, int width /*dim or nbytes*/,
                         const int32_t *pairs, int n_pairs, double ratio,
                         int32_t *query_idx_dev, int32_t *train_idx_dev, float *distance_dev,
                         int32_t *n_out_dev /*n_pairs*/, int64_t *out_offset /*host, n_pairs+1*/);

/* The same with HOST pointers in and out (what a C++ host without a device allocator of its own calls once for the whole pair loop,
 * sfm.cpp:140-161): `desc_host` holds the rows of all sets back to back; they are uploaded once, prepared (below) once, every pair is
 * matched in one launch sequence and the per-pair slices come back in one read-back.  query_idx / train_idx / distance need
 * sum(nq_p) entries, n_out n_pairs, out_offset n_pairs + 1 (all host).  Synchronises.
 * Only the first n_out[p] entries of a pair's range are written (sparse results are packed on the device before the read-back: the
 * transfer is proportional to the matches, not to the queries); the rest of the range is left as the caller passed it. */
int esfm_match_pairs(esfm_ctx *ctx, esfm_metric metric, const void *desc_host,
                     const int32_t *set_row_offset, int n_sets, int width /*dim or nbytes*/,
                     const int32_t *pairs, int n_pairs, double ratio,
                     int32_t *query_idx, int32_t *train_idx, float *distance,
                     int32_t *n_out /*n_pairs*/, int64_t *out_offset /*n_pairs+1*/);

/*
 * Optional, once per resident descriptor buffer: derive and keep what the matcher computes from the rows before it can start --
 * for 64-float L2 descriptors the bf16 operand images, |row|^2 and the rounding residual norms of every row (l2_split_bf16_kernel),
 * for 32-byte Hamming descriptors the nibble-per-bit images of the FP4 matrix-core form -- so that the esfm_match_pairs_dev / esfm_knn2_pairs_dev calls that follow
 * on the SAME (desc_dev, total rows, width) skip that launch.  The reference has no counterpart: it re-reads cv::Mat rows in every
 * knnMatch call (feature_matching.cpp:80,125); here the frames' descriptors are uploaded once for the whole pair loop
 * (sfm.cpp:140-161) and this is part of the upload.  The caller promises not to modify the rows while they are prepared;
 * esfm_match_release_prepared, another prepare, or a match call on a different buffer ends it.  Other widths: a no-op.
 */
int esfm_match_prepare_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, int64_t total_rows, int width);
int esfm_match_release_prepared(esfm_ctx *ctx);
/* The same, but only if `desc_dev` IS the buffer currently prepared on this context (a no-op otherwise): what an owner of one of
 * several descriptor buffers calls when ITS buffer goes away, without taking the prepared state from whoever holds it now. */
int esfm_match_release_prepared_buffer(esfm_ctx *ctx, const void *desc_dev);
/* Which buffer is prepared on this context right now (NULL: none). */
int esfm_match_prepared_buffer(esfm_ctx *ctx, const void **desc_dev_out);
/* The prepared state is keyed on (desc_dev, metric, total_rows, width) and there is ONE per context: a second prepare replaces the
 * first.  The library cannot see a hipFree or an in-place rewrite, and a same-size hipMalloc routinely returns the address just
 * freed: a prepared buffer MUST be released (esfm_match_release_prepared) or prepared again BEFORE it is freed, rewritten or
 * replaced -- otherwise the next match call on that address runs on the old rows' operand images and returns wrong matches
 * without an error.  esfm_ctx_set_prepared_check(ctx, 1) is the debugging aid for exactly that: prepare then also keeps a 64-bit
 * fingerprint of the buffer, and every match call that is about to rely on the prepared operands re-derives it first (one read of
 * the buffer and one host round trip per call) and fails with ESFM_ERR_STALE_PREPARED -- ending the prepared state -- when the rows
 * have changed.  Off by default; the environment variable ESFM_CHECK_PREPARED=1 switches it on for every new context. */
int esfm_ctx_set_prepared_check(esfm_ctx *ctx, int enable);

/* Same pass, but returns the raw 2-NN table instead of the filtered list:
 * knn_idx_dev / knn_dist_dev hold 2 entries per query row, pair p at
 * [2*out_offset[p], 2*(out_offset[p]+nq_p)). */
int esfm_knn2_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev,
                        const int32_t *set_row_offset, int n_sets, int width,
                        const int32_t *pairs, int n_pairs,
                        int32_t *knn_idx_dev, float *knn_dist_dev, int64_t *out_offset);

/* Audit of the Hamming matcher's ratio screen (tests only; metric must be ESFM_HAMMING -- the L2 screen is audited through
 * esfm_ctx_set_l2_audit mode 4): the raw table of a pass that screens with `ratio` as esfm_match_pairs_dev's does.  A query
 * the pass dropped as "cannot pass d0 < ratio d1" (feature_matching.cpp:88) carries train index -2 in both slots; every other
 * query its exact 2-NN.  Every dropped query must fail the reference's test on the unscreened table. */
int esfm_knn2_pairs_screened_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev,
                                 const int32_t *set_row_offset, int n_sets, int width,
                                 const int32_t *pairs, int n_pairs, double ratio,
                                 int32_t *knn_idx_dev, float *knn_dist_dev, int64_t *out_offset);

/*
 * Cross-check matching: the mutual-nearest-neighbour filter of the reference's Python prototype (python_code/feature_match.py:24-27,
 * its `mutual_nn` branch: cv2.BFMatcher(cv2.NORM_L2, crossCheck=True).match), which the C++ matcher lacks (SURVEY.md:196: one direction
 * only, no cross-check).  Distances, the (distance, index) ordering with ties to the lower index, and NaN handling are esfm_knn2_*'s.
 * For one pair (query set Q, train set T): F(q) = the nearest train row of query row q, R(t) = the nearest query row of train row t
 * (the same rule with the roles swapped: ties go to the lower QUERY index).
 *   use_ratio = 0 (cross; `ratio` ignored): q emits (q, F(q), d(q, F(q))) iff F(q) >= 0 and R(F(q)) == q -- strict mutual nearest
 *                 neighbour, also with nq == 1 or nt == 1.
 *   use_ratio = 1 (ratio+cross): the same, and the ratio test of esfm_match_pairs_dev ((double)d0 < ratio * (double)d1) holds for
 *                 row q of the forward table AND for row F(q) of the reverse one (both directions, as COLMAP does).  The result of
 *                 pair (i, j) is then exactly the transpose of that of pair (j, i), and a subset of esfm_match_pairs_dev's list.
 * This is the strict rule; OpenCV's crossCheck is not claimed: it may keep, for a query, the closest of the train rows whose nearest
 * query it is, which is not always a mutual pair.  Output layout as esfm_match_pairs_dev (pair p owns [out_offset[p], out_offset[p] + nq_p),
 * the first n_out[p] entries valid, query-ascending; the distance is the forward d0, bit-identical to the reverse one).
 * use_ratio outside {0, 1}, or a NaN ratio with use_ratio = 1: ESFM_ERR_INVALID_ARG.
 * Both directions run in one knn pass over a mirrored pair list (the pairs, then each with query and train swapped), so every query
 * set is also a train set: sets are limited to 2^21 - 1 rows, and a 64-float L2 query set of more than 65 536 rows takes the
 * three-product fallback instead of the one-product pass (correct, slower).  The prepared state (esfm_match_prepare_dev) serves both.
 */
int esfm_match_cross_l2_f32(esfm_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim, int use_ratio, double ratio,
                            int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out);
int esfm_match_cross_hamming(esfm_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int nbytes, int use_ratio,
                             double ratio, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out);
int esfm_match_cross_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const int32_t *set_row_offset, int n_sets,
                               int width, const int32_t *pairs, int n_pairs, int use_ratio, double ratio, int32_t *query_idx_dev,
                               int32_t *train_idx_dev, float *distance_dev, int32_t *n_out_dev, int64_t *out_offset /*host, n_pairs+1*/);
/* Host-pointer form, as esfm_match_pairs: upload once, prepare once, packed read-back.  Synchronises. */
int esfm_match_cross_pairs(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets,
                           int width, const int32_t *pairs, int n_pairs, int use_ratio, double ratio, int32_t *query_idx,
                           int32_t *train_idx, float *distance, int32_t *n_out /*n_pairs*/, int64_t *out_offset /*n_pairs+1*/);

/*
 * Epipolar-guided matching: a second matching pass for image pairs that already have an essential matrix (COLMAP's guided_matching;
 * the reference has none -- its README lists "try more robust outlier filter" as a to-do).  The descriptor search of a query row is
 * restricted to the train rows that lie on the query's epipolar line, so that a repeated structure's twin elsewhere in the image no
 * longer makes the ratio test reject the match.
 * For one pair: query set Q (nq descriptor rows and keypoints), train set T (nt), E[9] row-major double, K4 = fx, cx, fy, cy (float; the
 * query frame's, used for both images as estimate2D2D_E5P_RANSAC does), max_epipolar_px (double).
 * 1. Admissibility.  adm(q, t) is exactly the inlier test of esfm_find_essential_mat's RANSAC (sampson_inlier in ransac_kernels.hip,
 *    find_inliers in oracle/ransac_ref.c):
 *      x1 = ((double)uq - cx) / fx, y1 = ((double)vq - cy) / fy for the query keypoint, x2, y2 the same for the train keypoint;
 *      thr = max_epipolar_px / ((fx + fy) / 2.0), tsq = (float)(thr * thr);
 *      Ex0 = E0*x1 + E1*y1 + E2, Ex1 = E3*x1 + E4*y1 + E5, Ex2 = E6*x1 + E7*y1 + E8;
 *      Et0 = E0*x2 + E3*y2 + E6, Et1 = E1*x2 + E4*y2 + E7;
 *      v = x2*Ex0 + y2*Ex1 + Ex2;  err = (float)(v*v / (Ex0*Ex0 + Ex1*Ex1 + Et0*Et0 + Et1*Et1));  adm = err <= tsq.
 *    All arithmetic in double, left to right, no fused multiply-add; a NaN anywhere makes the row inadmissible.  There is ONE predicate
 *    per (query row, train row): the reverse direction of the cross-check evaluates this same expression with the same operand roles.
 * 2. Guided 2-NN.  For each query the two best ADMISSIBLE train rows under esfm_knn2_*'s ordering (ascending (distance, train index),
 *    ties to the lower index, a NaN distance never inserted), distances as esfm_knn2_* (L2: sqrtf of the canonical sum; Hamming: the
 *    bit count as float).  A missing neighbour is index -1, distance FLT_MAX.  n_adm[q]: the number of admissible train rows.
 * 3. Filters, on that table and on the reverse one (for each train row its two best admissible query rows, ties to the lower query index).
 *      use_ratio:   row q passes iff it has TWO admissible neighbours and (double)d0 < ratio * (double)d1; a query with fewer than two
 *                   admissible rows emits nothing (the convention of nt < 2 in esfm_match_*).
 *      cross_check: q emits iff R(F(q)) == q on the guided tables; with use_ratio the ratio test must hold on the forward row q and on
 *                   the reverse row F(q) (the strict rule of esfm_match_cross_*).
 *    At least one of the two must be on.  use_ratio or cross_check outside {0, 1}, neither on, a NaN ratio with use_ratio = 1,
 *    max_epipolar_px NaN or <= 0: ESFM_ERR_INVALID_ARG.  max_epipolar_px = +inf is allowed: every row with a finite error is admissible.
 * 4. Output as esfm_match_pairs_dev: pair p owns [out_offset[p], out_offset[p] + nq_p), the first n_out[p] entries valid, query-ascending,
 *    the distance the forward d0.
 * Two properties follow.  (a) With max_epipolar_px = +inf and finite keypoints the lists equal esfm_match_pairs' (ratio) and
 * esfm_match_cross_pairs' (cross, ratio+cross) on the same data, entry for entry.  (b) A plain match (q, t) that passes filter f and is
 * admissible: if q emits anything under guided-f, it emits the same t (and with a cross filter no other query can claim t), so the union
 * of the plain RANSAC inliers and the guided list has one train row per query -- and one query per train row with a cross filter.
 * kp_dev: float2 (u, v) per row, concatenated like the descriptors.  E (9 doubles per pair) and K4_per_pair (4 floats per pair) are HOST
 * arrays.  L2 of any dim >= 1, Hamming of 16, 32 or 64 bytes, empty sets, sets of at most 2^21 - 1 rows.  The call reads the raw
 * descriptor rows only: it neither needs nor disturbs esfm_match_prepare_dev's state.  Enqueues on the context's stream; does not
 * synchronise.  The results are bit-reproducible from run to run.
 */
int esfm_match_guided_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const float *kp_dev, const int32_t *set_row_offset,
                                int n_sets, int width /*dim or nbytes*/, const int32_t *pairs, int n_pairs, const double *E /*host, 9 per pair*/,
                                const float *K4_per_pair /*host, 4 per pair*/, double max_epipolar_px, int use_ratio, double ratio,
                                int cross_check, int32_t *query_idx_dev, int32_t *train_idx_dev, float *distance_dev,
                                int32_t *n_out_dev /*n_pairs*/, int64_t *out_offset /*host, n_pairs+1*/);
/* Host-pointer form, as esfm_match_pairs: descriptors and keypoints are uploaded once, the lists come back packed.  Synchronises. */
int esfm_match_guided_pairs(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const float *kp_host, const int32_t *set_row_offset,
                            int n_sets, int width, const int32_t *pairs, int n_pairs, const double *E, const float *K4_per_pair,
                            double max_epipolar_px, int use_ratio, double ratio, int cross_check, int32_t *query_idx, int32_t *train_idx,
                            float *distance, int32_t *n_out /*n_pairs*/, int64_t *out_offset /*n_pairs+1*/);
/* The raw forward table of step 2 (layout as esfm_knn2_pairs_dev) and n_adm per query (n_adm_dev: sum(nq_p) entries, may be NULL). */
int esfm_knn2_guided_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const float *kp_dev, const int32_t *set_row_offset,
                               int n_sets, int width, const int32_t *pairs, int n_pairs, const double *E, const float *K4_per_pair,
                               double max_epipolar_px, int32_t *knn_idx_dev, float *knn_dist_dev, int32_t *n_adm_dev, int64_t *out_offset);
/* One pair, host pointers (kp_q / kp_t: 2 floats per row).  Synchronise. */
int esfm_match_guided_l2_f32(esfm_ctx *ctx, const float *q, const float *kp_q, int nq, const float *t, const float *kp_t, int nt, int dim,
                             const double *E, const float *K4, double max_epipolar_px, int use_ratio, double ratio, int cross_check,
                             int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out);
int esfm_match_guided_hamming(esfm_ctx *ctx, const uint8_t *q, const float *kp_q, int nq, const uint8_t *t, const float *kp_t, int nt, int nbytes,
                              const double *E, const float *K4, double max_epipolar_px, int use_ratio, double ratio, int cross_check,
                              int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out);

/* Counters of the last L2 batched call on this context (after a synchronise):
 * queries whose MFMA candidate list could not be certified and were re-scanned
 * exactly (see DESIGN.md "certified re-rank").  For tests and profiling. */
int esfm_match_last_stats(esfm_ctx *ctx, int64_t *n_queries, int64_t *n_rescanned);
/* 64-float descriptors: queries the one-product bf16 pass could not certify and handed to the threshold-filter
 * pass (inside l2_finish_kernel), of which n_rescanned went on to the exact re-scan.  0 for other widths.  Queries the
 * ratio screen dropped (esfm_match_*: provably d0 >= ratio d1) are in neither count. */
int esfm_match_last_second_pass(esfm_ctx *ctx, int64_t *n_second_pass);

/* Audit of the L2 certificate (tests only; the default mode 0 is the product path).
 *   mode 1: the MFMA pass runs but the exact re-scan of uncertified queries is SKIPPED, so the
 *           2-NN table holds the pass's own answer for every query;
 *   mode 2: every query is brute-forced by l2_exact_scan_kernel (no MFMA pass);
 *   mode 3: (64-float descriptors) the one-product bf16 pass ALONE: the table holds its answer for every query and
 *           esfm_match_last_flagged() lists what it could not certify (mode 1 audits the two MFMA passes together);
 *   mode 4: (64-float descriptors, esfm_match_pairs_dev) the one-product pass alone WITH its ratio screen:
 *           esfm_match_last_flagged() lists the queries it dropped as "cannot pass d0 < ratio d1" (the reference's
 *           test, feature_matching.cpp:133).  Every listed query must fail that test on the brute-force table
 *           (rejected_but_would_pass == 0).  The match lists of a mode-4 call are not final (no second pass).
 * Diffing the two tables row by row and removing the rows esfm_match_last_flagged() lists gives
 * the number of queries the certificate accepted with a wrong answer; it must be 0. */
int esfm_ctx_set_l2_audit(esfm_ctx *ctx, int mode);
/* The 64-float match-list path runs its distance pass and its finish stages as ONE launch (the finish workgroups trail the pass's
 * in the same grid and wait, pair by pair, for the pair's pass blocks).  enable = 1 keeps them as two launches on one stream -- the
 * same results, for A/B measurements and tests; 0 restores the default.  ESFM_L2_TWO_LAUNCH=1 in the environment sets the default
 * of contexts created afterwards.  Pair lists of more than 8 Mi (2^23) queries keep the two launches whatever the switch says: there
 * the finish workgroups' lower occupancy inside the fused launch costs more than the launch boundary (a limit measured on lists of
 * 4096-row sets; ESFM_L2_FUSED_MAX_QUERIES in the environment moves it, for measurements).  Should a finish workgroup's wait ever run out (2 s; never seen), the call's lists are incomplete
 * and the next synchronising matcher call on the context returns ESFM_ERR_HIP. */
int esfm_ctx_set_l2_two_launch(esfm_ctx *ctx, int enable);
/* The 16 device-side counters of the last L2 batched call ([0] re-scanned, [1] second pass, the rest: instrumented builds only). */
int esfm_match_debug_counters(esfm_ctx *ctx, int32_t *out16);
/* The (pair, query row) entries the last L2 batched call flagged as uncertified: writes
 * min(*n, cap) entries of 2 x int32 to `out` (host) and the count to *n.  Synchronises. */
int esfm_match_last_flagged(esfm_ctx *ctx, int32_t *out, int64_t cap, int64_t *n);

/* Host-only helper (no GPU needed): the (i, j<i) pair list of sfm.cpp:140-143
 * for n_frames frames, restricted to shard `rank` of `world` by a cost-balanced
 * partition (cost = nq*nt when rows_per_frame is given, else 1).  Writes pairs
 * (query=i, train=j) to pairs_out (capacity n_frames*(n_frames-1)/2 pairs) and
 * returns the number written, or a negative esfm_status. */
int esfm_shard_pair_list(int n_frames, const int32_t *rows_per_frame /*or NULL*/, int rank, int world,
                         int32_t *pairs_out);

/* ---- bundle adjustment (SURVEY.md section 8 rows a-4 .. a-8) ------------- */

/* Solver options.  Defaults (esfm_ba_options_default) are what
 * cpp_code/src/ba.cpp:146-151,201-204 sets plus Ceres' own defaults for
 * TRUST_REGION / LEVENBERG_MARQUARDT / DENSE_SCHUR ([upstream]). */
typedef struct esfm_ba_options {
    int32_t max_num_iterations;            /* 50      ba.cpp:202                     */
    int32_t jacobi_scaling;                /* 1                                      */
    int32_t max_num_consecutive_invalid_steps; /* 5                                  */
    int32_t verbose;                       /* 1 = print Ceres-like progress lines     */
    double cauchy_a;                       /* 0.5     ba.cpp:150; <= 0: squared loss  */
    double initial_trust_region_radius;    /* 1e4                                    */
    double max_trust_region_radius;        /* 1e16                                   */
    double min_trust_region_radius;        /* 1e-32                                  */
    double min_relative_decrease;          /* 1e-3                                   */
    double min_lm_diagonal;                /* 1e-6                                   */
    double max_lm_diagonal;                /* 1e32                                   */
    double function_tolerance;             /* 1e-6                                   */
    double gradient_tolerance;             /* 1e-10                                  */
    double parameter_tolerance;            /* 1e-8                                   */
} esfm_ba_options;

typedef enum esfm_ba_termination {
    ESFM_BA_CONVERGENCE = 0,     /* a tolerance was reached                   */
    ESFM_BA_NO_CONVERGENCE = 1,  /* max_num_iterations reached                */
    ESFM_BA_FAILURE = 2          /* too many invalid steps / numeric failure  */
} esfm_ba_termination;

typedef struct esfm_ba_iteration {
    int32_t iteration;
    int32_t step_is_valid;
    int32_t step_is_successful;
    int32_t line_search_steps;   /* Armijo contractions this iteration (bounds-constrained problems only) */
    double cost;                 /* as Ceres logs it: candidate cost on a rejected step */
    double cost_change;
    double gradient_max_norm;
    double step_norm;
    double relative_decrease;    /* "tr_ratio" */
    double trust_region_radius;  /* radius AFTER this iteration's update */
    double model_cost_change;
} esfm_ba_iteration;

#define ESFM_BA_MAX_LOG 256

typedef struct esfm_ba_summary {
    int32_t termination;         /* esfm_ba_termination */
    int32_t num_iterations;      /* entries in `iterations` minus 1 = LM iterations run */
    int32_t num_successful_steps;
    int32_t num_unsuccessful_steps;
    int32_t num_active_cameras;  /* cameras / points with at least one observation */
    int32_t num_active_points;
    double initial_cost;
    double final_cost;
    double solve_seconds;        /* wall time of the LM loop (inputs already resident) */
    esfm_ba_iteration iterations[ESFM_BA_MAX_LOG]; /* [0] is iteration 0 */
} esfm_ba_summary;

void esfm_ba_options_default(esfm_ba_options *opt);

/* In-place all-reduce over `count` doubles at device pointer `buf_dev`, ordered
 * on `hip_stream`; op = ESFM_REDUCE_SUM or ESFM_REDUCE_MAX.  Return 0 on success.
 * Used only when the caller shards observations over several GPUs (one rank per
 * GPU); NULL = single GPU.  A torch.distributed (RCCL) implementation is in
 * easysfm_amd/ba.py; the library's own RCCL one is esfm_comm_allreduce below.
 * Per LM iteration the solver issues one SUM over the reduced camera system,
 * packed block-lower-triangular (36 n_cam (n_cam + 1) / 2 + 6 n_cam doubles:
 * 11.8 k at 25 cameras, 4.73 M = 37.8 MB at 512), one SUM over the
 * per-camera F'F / F'r blocks (42 n_cam doubles, accepted steps only), and SUM /
 * MAX over a handful of scalars. */
#define ESFM_REDUCE_SUM 0
#define ESFM_REDUCE_MAX 1
typedef int (*esfm_allreduce_fn)(void *user, double *buf_dev, int64_t count, int op, void *hip_stream);

/* The library's own exchange: RCCL over xGMI, one communicator per rank (= per GPU, per esfm_ctx).
 * Rank 0 calls esfm_comm_get_unique_id and hands the ESFM_COMM_ID_BYTES bytes to the other ranks by whatever the
 * host program has (a file, MPI, a torch.distributed store); every rank then calls esfm_comm_create with the same
 * id (collective: returns once all `world` ranks have joined).  esfm_comm_allreduce IS an esfm_allreduce_fn whose
 * `user` is the esfm_comm*, so a sharded solve is
 *     esfm_ba_problem_solve(p, opt, esfm_comm_allreduce, comm, &summary);
 * with no callback into the host language.  librccl is bound at run time; without it these return ESFM_ERR_COMM. */
#define ESFM_COMM_ID_BYTES 128
typedef struct esfm_comm esfm_comm;
int esfm_comm_get_unique_id(void *id_out /*ESFM_COMM_ID_BYTES*/);
int esfm_comm_create(esfm_ctx *ctx, const void *id /*ESFM_COMM_ID_BYTES*/, int rank, int world, esfm_comm **out);
int esfm_comm_destroy(esfm_comm *comm);
int esfm_comm_rank(const esfm_comm *comm);
int esfm_comm_world(const esfm_comm *comm);
/* ranks of the communicator as RCCL reports them (ncclCommCount; -1 on failure): "did RCCL see N ranks" for logs and bench lines */
int esfm_comm_rccl_ranks(const esfm_comm *comm);
int esfm_comm_allreduce(void *comm, double *buf_dev, int64_t count, int op, void *hip_stream);

/*
 * The replacement for setBAProblem's parameter packing + solveBA's
 * ceres::Solve (cpp_code/src/ba.cpp:58-114, :132-212) with calibration fixed
 * (ReprojectErrorTerm_fixcalib, cpp_code/include/ba.h:108-164):
 *
 *   residual_k = uv_k - project(K[cam_k], AngleAxis(cams[cam_k][0..2]) * pts[pt_k] + cams[cam_k][3..5])
 *   cost = 1/2 * sum_k rho(|residual_k|^2),  rho = Cauchy(a)  (ba.cpp:150)
 *
 * minimised by Levenberg-Marquardt with point-block Schur elimination
 * (DENSE_SCHUR, ba.cpp:201).  cams (6 doubles per camera: angle-axis, then
 * translation) and pts (3 doubles per point) are updated in place; parameter
 * blocks with no observation are left bit-identical.  K4_per_cam holds
 * fx, cx, fy, cy per camera (the four entries ba.h:142-143 reads).
 * Observations may come in any order.  Host pointers.
 *
 * Multi-GPU: each rank passes its own shard of the observations (all cameras,
 * all points, n_obs = local count) and the same allreduce callback; every rank
 * ends with identical cams and the full pts.
 */
int esfm_ba_solve(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs,
                  const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv /*2*n_obs*/,
                  const float *K4_per_cam /*4*n_cam*/,
                  double *cams /*6*n_cam*/, double *pts /*3*n_pt*/,
                  const esfm_ba_options *options /*NULL = defaults*/,
                  esfm_allreduce_fn allreduce /*or NULL*/, void *allreduce_user,
                  esfm_ba_summary *summary /*or NULL*/);

/* Resident form: upload once, iterate many times (what bench.py times). */
typedef struct esfm_ba_problem esfm_ba_problem;

int esfm_ba_problem_create(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs,
                           const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                           const float *K4_per_cam, const double *cams, const double *pts,
                           esfm_ba_problem **out);
/* Re-upload the parameter vector (restart from a new initial guess). */
int esfm_ba_problem_set_params(esfm_ba_problem *p, const double *cams, const double *pts);
int esfm_ba_problem_solve(esfm_ba_problem *p, const esfm_ba_options *options,
                          esfm_allreduce_fn allreduce, void *allreduce_user, esfm_ba_summary *summary);
int esfm_ba_problem_get_params(esfm_ba_problem *p, double *cams, double *pts);
int esfm_ba_problem_destroy(esfm_ba_problem *p);

/* One evaluation of the robustified cost 1/2 sum rho(|r|^2) at the problem's
 * current parameters (tests, and the candidate-cost kernel in isolation). */
int esfm_ba_problem_cost(esfm_ba_problem *p, double cauchy_a, double *cost);

/* ---- free shared intrinsics and box bounds ----------------------------------------------------
 * BundleAdjustment::solveBA(fix_calib_tolerance_BA != 0) (ba.cpp:167-196): the cost functor becomes
 * ReprojectErrorTerm_updatecalib (ba.h:170-222) over ONE shared parameter block fx, cx, fy, cy
 * (ba.cpp:107-113 takes it from calibs_[0]; ba.h:199-202 fixes the order), bounded to its initial value
 * +- tolerance (ba.cpp:190-194).  Independently, the reference frame's six pose parameters are bounded to
 * [-1e-10, +1e-10] (ba.cpp:134, :155-162 / :181-188), i.e. held at the origin.  With any bound Ceres runs its
 * constrained trust-region loop (projection onto the box, projected gradient norm, Armijo line search along
 * the LM step); esfm_ba_iteration.line_search_steps reports the contractions per iteration.
 *
 * esfm_ba_problem_create_free_calib: as esfm_ba_problem_create, without per-camera K4 and with calib4[4] =
 * fx, cx, fy, cy (doubles, as parameters_ holds them) and calib_tolerance > 0 (Ceres rejects an empty box).
 * The multi-GPU rules are unchanged: every rank passes the same calib4; the intrinsics ride in the all-reduced
 * reduced system like one more camera. */
int esfm_ba_problem_create_free_calib(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs,
                                      const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                                      const double *calib4, double calib_tolerance,
                                      const double *cams, const double *pts, esfm_ba_problem **out);
/* new start value and box centre of the intrinsics (problems created with free intrinsics only) */
int esfm_ba_problem_set_calib(esfm_ba_problem *p, const double *calib4, double calib_tolerance);
int esfm_ba_problem_get_calib(esfm_ba_problem *p, double *calib4);
/* Bound all six parameters of camera `cam` to [-threshold, +threshold] for the following solves
 * (ba.cpp:155-162 with threshold = 1e-10); cam < 0 removes the bound. */
int esfm_ba_problem_fix_camera(esfm_ba_problem *p, int cam, double threshold);

/* One-shot solveBA with the optional pieces: calib4 NULL = fixed intrinsics K4_per_cam, else free shared
 * intrinsics (in/out, K4_per_cam ignored); ref_cam < 0 = no reference camera. */
int esfm_ba_solve_ex(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs,
                     const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                     const float *K4_per_cam, double *cams, double *pts,
                     double *calib4, double calib_tolerance, int ref_cam, double ref_threshold,
                     const esfm_ba_options *options, esfm_allreduce_fn allreduce, void *allreduce_user,
                     esfm_ba_summary *summary);

/* ---- multiple-camera mode: one free intrinsics block per camera group ---------------------------
 * The reference's open to-do "multiple-camera mode (different intrinsic elements)".  Camera c belongs to group
 * group_of_cam[c] in [0, n_groups); group g owns a parameter block fx, cx, fy, cy (calib4 + 4 g, doubles), bounded
 * to its start value +- calib_tolerance[g] (each > 0).  The functor is ReprojectErrorTerm_updatecalib with the block
 * of the observation's camera's group.  A group that no observation uses keeps its four values bit for bit.  With
 * n_groups == 1 this is esfm_ba_problem_create_free_calib: the same kernels, launches and summation orders, hence
 * the same bits.  Two solves of the same problem agree in every bit for any n_groups.
 * Errors, reported before anything is written: n_groups < 1, a group index outside [0, n_groups), a tolerance <= 0
 * (ESFM_ERR_INVALID_ARG), a non-finite intrinsic or tolerance (ESFM_ERR_NUMERIC), 6 (n_cam + n_groups) >= 46000.
 * Multi-GPU: every rank passes the same group arrays; a rank need not hold observations of every group; the
 * exchanged sizes are the documented ones with n_cam + n_groups camera-side blocks.
 * Not provided: a mix of fixed and free cameras in one problem (give the cameras to hold a group with a narrow box),
 * tangential distortion terms, k3, fisheye models, and the radial mode in bin/sfm_native's driver.  (Free radial distortion k1, k2
 * per group: esfm_ba_problem_create_radial_groups, below.)
 * In front of the solver the two-view entry points (esfm_find_essential_*, esfm_recover_pose_*, esfm_find_homography_*,
 * esfm_match_guided_*) keep taking ONE K per pair: the host mirrors hand them the keypoints of both images remapped into the
 * pixels of one canonical camera (camera 0), so their pixel thresholds are in canonical pixels in a multi-camera run; the dense
 * stages take K4 per view but one image size for all views. */
int esfm_ba_problem_create_calib_groups(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs,
                                        const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                                        int n_groups, const int32_t *group_of_cam /*n_cam*/, const double *calib4 /*4 n_groups*/,
                                        const double *calib_tolerance /*n_groups, each > 0*/,
                                        const double *cams, const double *pts, esfm_ba_problem **out);
/* new start values and box centres / half widths of every block (problems with free intrinsics, any group count) */
int esfm_ba_problem_set_calib_groups(esfm_ba_problem *p, const double *calib4, const double *calib_tolerance);
int esfm_ba_problem_get_calib_groups(esfm_ba_problem *p, double *calib4 /*4 n_groups*/);
/* 0: fixed intrinsics, else the number of free blocks.  esfm_ba_problem_set_calib / _get_calib serve one-block problems only and
 * return ESFM_ERR_INVALID_ARG on more. */
int esfm_ba_problem_calib_groups(const esfm_ba_problem *p);
/* One-shot, as esfm_ba_solve_ex with the group arrays (calib4 in/out) */
int esfm_ba_solve_groups(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs,
                         const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                         double *cams, double *pts,
                         int n_groups, const int32_t *group_of_cam, double *calib4, const double *calib_tolerance,
                         int ref_cam, double ref_threshold,
                         const esfm_ba_options *options, esfm_allreduce_fn allreduce, void *allreduce_user,
                         esfm_ba_summary *summary);

/* Free radial distortion per camera group: block g is fx, cx, fy, cy, k1, k2.  The model is OpenCV's with p1 = p2 = 0, the one
 * esfm_undistort inverts: with p = R(a) X + t, x = p0/p2, y = p1/p2, r2 = x^2 + y^2 and L = 1 + k1 r2 + k2 r2^2,
 *   r0 = u - (fx x L + cx),   r1 = v - (fy y L + cy).
 * radial2 holds k1, k2 of every group (2 n_groups doubles); they are boxed to their start +- radial_tolerance[g] (each > 0), the four
 * pinhole values to calib4 +- calib_tolerance[g] as above, so a radial problem is always a bounded problem (the constrained loop
 * with the Armijo search).  A radial problem takes the grouped kernels with any group count, one included; a group nobody observes
 * keeps its six values bit for bit; two solves of the same problem agree in every bit.  Every non-radial problem gives the bits it
 * gave before these entry points existed.
 * Errors, before anything is written, as for esfm_ba_problem_create_calib_groups, and: a radial tolerance <= 0
 * (ESFM_ERR_INVALID_ARG), a non-finite coefficient or radial tolerance (ESFM_ERR_NUMERIC).
 * esfm_ba_problem_get / set_calib_groups serve a radial problem too (the four pinhole values; k1, k2 stay as they are); the radial
 * accessors on a problem created without radial distortion return ESFM_ERR_INVALID_ARG. */
int esfm_ba_problem_create_radial_groups(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs,
                                         const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                                         int n_groups, const int32_t *group_of_cam /*n_cam*/, const double *calib4 /*4 n_groups*/,
                                         const double *calib_tolerance /*n_groups, each > 0*/,
                                         const double *radial2 /*2 n_groups*/, const double *radial_tolerance /*n_groups, each > 0*/,
                                         const double *cams, const double *pts, esfm_ba_problem **out);
/* new start values and box centres / half widths of k1, k2 of every block */
int esfm_ba_problem_set_radial_groups(esfm_ba_problem *p, const double *radial2, const double *radial_tolerance);
int esfm_ba_problem_get_radial_groups(esfm_ba_problem *p, double *radial2 /*2 n_groups*/);
/* 0: no free radial distortion, else the number of blocks */
int esfm_ba_problem_radial_groups(const esfm_ba_problem *p);
/* One-shot, as esfm_ba_solve_groups, plus radial2 (in/out) and radial_tolerance */
int esfm_ba_solve_radial_groups(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs,
                                const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                                double *cams, double *pts,
                                int n_groups, const int32_t *group_of_cam, double *calib4, const double *calib_tolerance,
                                double *radial2, const double *radial_tolerance,
                                int ref_cam, double ref_threshold,
                                const esfm_ba_options *options, esfm_allreduce_fn allreduce, void *allreduce_user,
                                esfm_ba_summary *summary);

/* The step-length rule of that line search alone (host arithmetic, no GPU): next trial step after the trial
 * (x_cur, f_cur, g_cur) failed the sufficient-decrease test, given the start point (0, f0, g0) and optionally
 * the trial before; *_valid = 0 marks a sample whose evaluation failed.  [upstream line_search.cc
 * InterpolatingPolynomialMinimizingStepSize, CUBIC] */
double esfm_ba_line_search_next_step(double f0, double g0, double x_prev, double f_prev, double g_prev, int prev_valid,
                                     double x_cur, double f_cur, double g_cur, int cur_valid);

/* Host-only helper (no GPU needed): assigns each point to one of `world`
 * shards so that observation counts balance (greedy over points in index
 * order), writing shard_of_point[n_pt].  Observations follow their point. */
int esfm_ba_shard_points(int n_pt, int n_obs, const int32_t *pt_idx, int world, int32_t *shard_of_point);

/* Host-only (no GPU): the structure-aware plan of the reduced camera system for an observation list -- what esfm_ba_problem_solve
 * builds for itself when the camera count takes the tiled solve.  Block (a, b) of the reduced system is structurally non-zero only
 * if cameras a and b observe a common point (the reference adds one residual block per observation, cpp_code/src/ba.cpp:140-151,
 * and lets DENSE_SCHUR, :201, ignore that).  The cameras are ordered by nested dissection of that co-visibility graph, every
 * supernode padded to whole 64-column tiles; the factorisation visits only the tiles of the symbolic fill.
 *   col_src[k]   original unknown 6 cam + a of permuted column k, -1 for identity padding (nb * 64 entries)
 *   tiles[2 t]   block row / column of tile t of the factor (lower triangle, fill included; block row nb = the right-hand side)
 *   info[0..9]   nb, tiles, longest dependency chain in tile columns, tile columns of the dense path, 1 if the solve would use
 *                the plan (at most half the dense path's tiles or half its dependency chain), 64^3 products, supernodes, workgroups,
 *                co-visible camera blocks (a, b <= a) = what several ranks exchange per LM iteration (36 doubles each), 0
 * col_src / tiles may be NULL (with capacity 0) to size the arrays from info first.  leaf_max <= 0: the library's default. */
int esfm_ba_reduced_plan(int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, int leaf_max,
                         int32_t *col_src, int col_cap, int32_t *tiles, int tile_cap, int32_t *info /*10*/);

/* ---- sparse-cloud statistical outlier removal ------------------------
 * CProceesing::SORFilter (cpp_code/include/cloudprocessing.hpp:24-36, called on the final cloud at
 * cpp_code/test/sfm.cpp:333) = pcl::StatisticalOutlierRemoval with MeanK (50) and StddevMulThresh (2.0):
 * per point the mean distance to its mean_k nearest neighbours (exact search among the finite points, float
 * squared distances, double sum of float square roots in ascending order); then mean and standard deviation of
 * those N numbers; a point is removed iff its mean distance > mean + std_mul * stddev.
 *
 * points: n rows of stride_floats floats with x, y, z first (3 = packed xyz, 8 = pcl::PointXYZRGB as
 * rgb_pointcloud->points stores it).  keep[n]: 1 = the point survives (the order of survivors is the input
 * order, like pcl::Filter::filter); mean_dist[n] (or NULL) receives the per-point mean distances; *threshold the
 * cut.  mean_k in [1, 63].  Host pointers.  Fewer than mean_k + 1 finite points is undefined in PCL; here the
 * neighbours that exist are summed and the sum is still divided by mean_k. */
int esfm_sor_filter(esfm_ctx *ctx, const float *points, int n, int stride_floats, int mean_k, double std_mul,
                    float *mean_dist /*n or NULL*/, uint8_t *keep /*n*/, int32_t *n_keep, double *threshold /*or NULL*/);
/* The k-NN pass alone on device-resident points (what bench.py times); asynchronous on the context's stream. */
int esfm_sor_mean_distances_dev(esfm_ctx *ctx, const float *points_dev, int n, int stride_floats, int mean_k,
                                float *mean_dist_dev /*n*/);

/* ---- two-view triangulation (triangulation part) -----------------------
 * cv::triangulatePoints as MotionEstimator::getDepthFast (cpp_code/src/estimate_motion.cpp:263, once per image pair inside
 * the matching loop, test/sfm.cpp:166) and doTriangulation (:333) call it: proj1 / proj2 are the 3 x 4 CV_32F projection
 * matrices [R | t] (row-major, 12 floats), pts1 / pts2 the correspondences as normalised image points
 * ((u - cx) / fx, (v - cy) / fy: pixel2cam, include/estimate_motion.h:41-46; 2 floats per point), and the result is the
 * 4 x N CV_32F matrix of homogeneous points, stored here point-major: points4d[4 i + 0..3] = X, Y, Z, W.  Each point is
 * the right singular vector of the smallest singular value of the 4 x 4 DLT system (rows x P[2] - P[0], y P[2] - P[1]),
 * evaluated in double like cvTriangulatePoints; it is defined up to sign, which the callers' division by W removes
 * (estimate_motion.cpp:271, :341).  Host pointers. */
int esfm_triangulate_points(esfm_ctx *ctx, const float *proj1, const float *proj2, const float *pts1, const float *pts2, int n,
                            float *points4d /*4*n*/);
/* Batched form for the pair loop: pair p uses proj1[12 p..], proj2[12 p..] and the points
 * [point_offset[p], point_offset[p+1]) of pts1 / pts2 / points4d; one launch for all pairs. */
int esfm_triangulate_pairs(esfm_ctx *ctx, int n_pairs, const float *proj1, const float *proj2, const int32_t *point_offset /*n_pairs+1*/,
                           const float *pts1, const float *pts2, float *points4d);

/* ---- essential-matrix RANSAC and pose recovery --------------------------
 * MotionEstimator::estimate2D2D_E5P_RANSAC (cpp_code/src/estimate_motion.cpp:27-97, once per matched pair at
 * cpp_code/test/sfm.cpp:165) = cv::findEssentialMat(pts1, pts2, K, CV_RANSAC, prob, threshold, mask) (:49) followed by
 * cv::recoverPose(E, pts1, pts2, K, R, t, mask) (:67).
 *
 * esfm_find_essential_mat: pts1 / pts2 are the n matched pixel positions (2 floats each, cv::Point2f), K4 = fx, cx, fy,
 * cy of the float camera matrix (the reference passes frame 1's K for both images, :43-44).  Points are normalised in
 * double, threshold is divided by (fx + fy) / 2, and OpenCV's RANSAC runs with 5 model points, confidence `prob` and at
 * most 1000 iterations on the sample stream of cv::RNG((uint64)-1): each sample goes through the 5-point kernel (up to 10
 * models), each model is scored by the Sampson distance (float error <= (float)threshold^2), a model replaces the best
 * iff it has more inliers (and more than 4), and the iteration count adapts (RANSACUpdateNumIters).  E[9] row-major with
 * unit Frobenius norm, mask[n] = inliers of the winning model, *iterations = iterations the sequential loop runs.
 * Returns ESFM_ERR_NUMERIC when no model is found (n < 5, or no model with at least 5 inliers): OpenCV returns an empty
 * matrix there.  Every model gets a canonical sign (largest-magnitude entry positive) and the models of one sample are
 * tried in ascending order of E[0][0] (OpenCV: cv::solvePoly's root order and its SVD basis' sign, both artefacts); this
 * only decides ties between models of the same sample.
 *
 * The `_pairs` forms batch many image pairs (pair p owns points [point_offset[p], point_offset[p+1]) and K4_per_pair[4 p..]):
 * all hypotheses of a chunk of iterations of all pairs are solved and scored in one launch; status[p] = 1 iff pair p has
 * a model.  Results are those of the per-pair calls. */
int esfm_find_essential_mat(esfm_ctx *ctx, const float *pts1, const float *pts2, int n, const float *K4, double prob,
                            double threshold, double *E /*9*/, uint8_t *mask /*n*/, int32_t *iterations /*or NULL*/);
int esfm_find_essential_pairs(esfm_ctx *ctx, int n_pairs, const int32_t *point_offset /*n_pairs+1*/, const float *pts1,
                              const float *pts2, const float *K4_per_pair, double prob, double threshold,
                              double *E /*9 per pair*/, uint8_t *mask /*per point*/, int32_t *status /*per pair*/,
                              int32_t *iterations /*per pair or NULL*/);
/* cv::recoverPose with distanceThresh = 50: the four poses of decomposeEssentialMat (SVD, W = [0 1 0; -1 0 0; 0 0 1]) in
 * the order (R1, t), (R2, t), (R1, -t), (R2, -t); for each, every point is triangulated in double against [I | 0] and
 * kept iff Z W > 0 and Z / W < 50 in the first camera and 0 < Z < 50 in the second; with `mask` (in/out, or NULL) the
 * tests are AND-ed with it; the pose with the most points wins (first in order on ties).  R[9] row-major, t[3] unit
 * length, *good = its point count. */
int esfm_recover_pose(esfm_ctx *ctx, const double *E, const float *pts1, const float *pts2, int n, const float *K4,
                      double *R, double *t, uint8_t *mask /*n, in/out, or NULL*/, int32_t *good /*or NULL*/);
int esfm_recover_pose_pairs(esfm_ctx *ctx, int n_pairs, const int32_t *point_offset, const float *pts1, const float *pts2,
                            const float *K4_per_pair, const double *E /*9 per pair*/, uint8_t *mask /*in/out or NULL*/,
                            double *R /*9 per pair*/, double *t /*3 per pair*/, int32_t *good /*per pair or NULL*/);
/* cv::solvePnPRansac(pts3d, pts2d, K, dist = 0, rvec, tvec, false, iterationsCount, reprojectionError, confidence, inliers,
 * cv::SOLVEPNP_EPNP) as MotionEstimator::estimate2D3D_P3P_RANSAC calls it (cpp_code/src/estimate_motion.cpp:161-162, once per
 * newly registered frame, cpp_code/test/sfm.cpp:288).  pts3d: n x 3 floats (cv::Point3f), pts2d: n x 2 float pixels, K4 = fx,
 * cx, fy, cy.  RANSAC with 5 model points on the cv::RNG((uint64)-1) sample stream: each sample is solved by EPnP (control
 * points, M'M null space, three beta approximations + 5 Gauss-Newton steps each, absolute orientation, smallest mean
 * reprojection error), scored by the squared pixel distance of the float projection (<= (float)reprojectionError^2), and the
 * iteration count adapts from iterationsCount; then EPnP is run once more on all inliers of the best model.  rvec =
 * cv::Rodrigues(R), tvec; R (or NULL) receives the rotation matrix, inlier_mask[n] (or NULL) the inliers of the best RANSAC
 * model (OpenCV returns their indices), *n_inliers their number.  Fewer than 5 points is ESFM_ERR_UNSUPPORTED (OpenCV switches
 * to P3P at 4); no model with at least 5 inliers is ESFM_ERR_NUMERIC (OpenCV returns false). */
int esfm_solve_pnp_ransac(esfm_ctx *ctx, const float *pts3d, const float *pts2d, int n, const float *K4, int iterations_count,
                          double reprojection_error, double confidence, double *rvec /*3*/, double *tvec /*3*/, double *R /*9 or NULL*/,
                          uint8_t *inlier_mask /*n or NULL*/, int32_t *n_inliers /*or NULL*/, int32_t *iterations /*or NULL*/);
/* The 5-point kernel alone (EMEstimatorCallback::runKernel [upstream five-point.cpp], what cv::findEssentialMat at reference
 * cpp_code/src/estimate_motion.cpp:49-51 runs on every RANSAC sample): n_samples samples of five correspondences in NORMALISED
 * coordinates, q1, q2 [n_samples][5][2] doubles with x2' E x1 = 0.  E_out [n_samples][10][9]: a sample's models (row-major, unit
 * Frobenius norm, largest-magnitude entry positive, ascending E[0][0]); n_models[n_samples] their number (0..10).  stages (or
 * NULL) [n_samples][117]: the intermediate values for stage-by-stage tests -- null-space basis N[4][9], det[11] (lowest degree
 * first), P[3][4], Qp[3][4], R[3][5] of B(z), the monic coefficients cc[10], the root estimates re[10], im[10], the sweeps of
 * the root iteration (-1: no polynomial).  esfm_five_point_models runs essential_setup_kernel's and essential_roots_kernel's
 * code on the GPU; esfm_five_point_models_host runs the host build of the same routines (easysfm_amd/csrc/five_point_core.hpp),
 * no GPU: the two and the CPU restatement agree to the bit (tests/test_five_point_stages.py). */
int esfm_five_point_models(esfm_ctx *ctx, const double *q1, const double *q2, int n_samples, double *E_out, int32_t *n_models,
                           double *stages /*or NULL*/);
int esfm_five_point_models_host(const double *q1, const double *q2, int n_samples, double *E_out, int32_t *n_models,
                                double *stages /*or NULL*/);
/* Host-only (no GPU): the first n_samples 5-index samples RANSAC draws for `count` points (cv::RNG replay). */
int esfm_ransac_sample_stream(int count, int n_samples, int32_t *idx /*5 per sample*/);

/* ---- Homography RANSAC: the planar / panoramic check of two-view verification ------------------------
 * A pair of views related by a pure rotation, or looking at a plane, still gets an essential matrix with many inliers, but its
 * translation is noise.  Such a pair is also explained by a homography; a caller compares the two models' inlier counts
 * (pipeline.match_and_verify_all_pairs(homography_check=True), FeatureMatching::findInitializeFramePair's max_h_inlier_ratio).
 *
 * esfm_find_homography follows cv::findHomography(pts1, pts2, cv::RANSAC, threshold, mask, 2000, confidence) WITHOUT its final
 * Levenberg-Marquardt polish; where the two differ, the rule written here is the authority (parity with OpenCV is not pinned).
 *   - pts1 / pts2: n matched pixel positions (2 floats each).  H[9] row-major maps image 1 to image 2, H[8] = 1.
 *   - RANSAC with 4 model points, at most 2000 iterations, on the sample stream of cv::RNG((uint64)-1).  A sample is four
 *     distinct indices (a repeat is redrawn) that pass the subset check: none of the triples (0,1,2), (1,2,3), (0,2,3), (0,1,3) is
 *     collinear in either image (|cross| <= FLT_EPSILON * (|dx1| + |dy1| + |dx2| + |dy2|), in double), and the products of the two
 *     images' signed triangle areas are negative for none or for all four triples.  A rejected sample is redrawn whole; after
 *     1000 rejections in a row the loop ends where it stands (before its first iteration: no model).
 *   - Minimal solve (f64): Hartley normalisation per image (centroid to the origin, mean distance sqrt 2), the 8 x 9 DLT system,
 *     its null vector by a Householder QR of the transpose, de-normalisation, division by H[8]; no model when
 *     |H[8]| <= DBL_EPSILON * max|H| or an entry is not finite.  Every order of operations: easysfm_amd/csrc/homography_core.hpp.
 *   - Score: the forward transfer error in FLOAT on (float)H: ww = 1.f / (H6 x + H7 y + 1.f), dx = (H0 x + H1 y + H2) ww - x',
 *     dy likewise, err = dx dx + dy dy; inlier iff err <= (float)(threshold * threshold).
 *   - A model replaces the best iff it has more inliers and at least 4; the iteration count adapts (RANSACUpdateNumIters with 4
 *     model points).  mask[n] = the inliers of the winning RANSAC model, *iterations = iterations the sequential loop runs.
 *   - Then H is re-fitted on those inliers: the eigenvector of the smallest eigenvalue of the 9 x 9 normal matrix A'A of their
 *     normalised DLT rows (cyclic Jacobi), summed in one fixed order (256 lanes, lane l the points l, l + 256, .. whose mask is
 *     set, ascending; then a halving tree).  The mask stays the RANSAC mask.  A re-fit without a model leaves the RANSAC winner.
 *   - n = 4: the minimal solve of the four points as given, no subset check, mask all ones, no re-fit, *iterations = 0.
 *   - n < 4 is ESFM_ERR_UNSUPPORTED; no model (no sample passed the check, or no model with 4 inliers) is ESFM_ERR_NUMERIC.
 * esfm_find_homography_pairs batches many pairs (pair p owns points [point_offset[p], point_offset[p+1])): one launch per chunk
 * of iterations of all still-active pairs.  status[p] = 1 iff pair p has a model (a pair with fewer than 4 points has none: no
 * error); H and mask of a pair without a model are zero.  Results are those of the per-pair calls, bit for bit.
 * n_inliers[p] (or NULL) = the correspondences of pair p within the threshold of the RETURNED (re-fitted) H, under the same float
 * error -- not the number of set mask entries.  The mask belongs to a model of four noisy points and RANSAC stops as soon as
 * such a model makes further iterations unlikely to pay, so its count swings with the sample: on planar and rotation-only pairs
 * with 0.3 px noise and a 1 px threshold it was 0.59 .. 0.88 of the correspondences, the returned model's 0.84 .. 0.92 (general
 * pairs: below 0.08 either way).  This count is the planar / panoramic statistic's numerator. */
int esfm_find_homography(esfm_ctx *ctx, const float *pts1, const float *pts2, int n, double threshold, double confidence,
                         double *H /*9*/, uint8_t *mask /*n*/, int32_t *iterations /*or NULL*/);
int esfm_find_homography_pairs(esfm_ctx *ctx, int n_pairs, const int32_t *point_offset /*n_pairs+1*/, const float *pts1,
                               const float *pts2, double threshold, double confidence, double *H /*9 per pair*/,
                               uint8_t *mask /*per point*/, int32_t *status /*per pair*/, int32_t *iterations /*per pair or NULL*/,
                               int32_t *n_inliers /*per pair or NULL*/);
/* The minimal solve alone: n_samples samples of four correspondences in pixels, q1, q2 [n_samples][4][2] doubles.  H_out
 * [n_samples][9] (zeros without a model), has_model[n_samples] 1 / 0.  esfm_homography_models runs homography_solve_kernel's code
 * on the GPU, esfm_homography_models_host the host build of the same header (no GPU): the two and the Python restatement
 * (tests/homography_ref.py) agree to the bit. */
int esfm_homography_models(esfm_ctx *ctx, const double *q1, const double *q2, int n_samples, double *H_out, int32_t *has_model);
int esfm_homography_models_host(const double *q1, const double *q2, int n_samples, double *H_out, int32_t *has_model);
/* Host-only (no GPU): the re-fit solve on the points whose mask is set (mask NULL: all), in the refit kernel's summation order.
 * Fewer than 4 such points or no model: ESFM_ERR_NUMERIC, H zeros. */
int esfm_homography_refit_host(const float *pts1, const float *pts2, int n, const uint8_t *mask /*or NULL*/, double *H /*9*/);
/* Host-only (no GPU): the first n_samples 4-index samples the RANSAC above draws for these `count` correspondences, the subset
 * check included; *redraws (or NULL) = rejected subsets on the way.  ESFM_ERR_NUMERIC when 1000 subsets in a row are rejected. */
int esfm_homography_sample_stream(const float *pts1, const float *pts2, int count, int n_samples, int32_t *idx /*4 per sample*/,
                                  int64_t *redraws /*or NULL*/);

/* ---- Fundamental-matrix RANSAC: the uncalibrated start ------------------------------------------------
 * Two views without a calibration matrix are still related by a fundamental matrix F (x2' F x1 = 0 in pixels), and the F of many pairs
 * taken with one camera pin its focal length down (esfm_focal_cost below; pipeline.run_sfm(auto_focal=...), `bin/sfm ... auto`).
 *
 * esfm_find_fundamental follows cv::findFundamentalMat(pts1, pts2, cv::FM_RANSAC, threshold, confidence); where the two differ, the
 * rule list written here is the authority (parity with OpenCV is not pinned).  Every order of operations:
 * easysfm_amd/csrc/fundamental_core.hpp; the restatement tests/fundamental_ref.py agrees with the host build and the kernels to the bit.
 *   Sampling and iteration
 *   - 7 model points, at most 1000 iterations, on the sample stream of cv::RNG((uint64)-1): seven distinct indices (a repeat is
 *     redrawn).  No subset check.
 *   - n = 7: the models of the seven points as given, *iterations = 0, the mask all ones.  The winner is the model with the most
 *     inliers under the score below, the first in model order on ties.
 *   - n < 7 is ESFM_ERR_UNSUPPORTED; no model with at least 7 inliers (n = 7: no model at all) is ESFM_ERR_NUMERIC.
 *   Minimal solve (f64)
 *   - Hartley normalisation of the seven points per image (centroid to the origin, mean distance sqrt 2); the 7 x 9 system of the rows
 *     (p u, p v, p, q u, q v, q, u, v, 1) of (u, v) -> (p, q); its two-dimensional null space f1, f2 by a Householder QR of the transpose
 *     (the last two columns of the orthogonal factor).
 *   - The cubic det(x f1 + (1 - x) f2) by one written-out expansion; its real roots by a bracketed Newton iteration with a fixed sweep
 *     cap (80) between the Cauchy bound and the cubic's stationary points, using only + - * / sqrt and comparisons (not the 5-point
 *     solver's iteration).
 *   - Vanishing leading coefficient (|c3| <= 1e-12 max|c_i|): the cubic is read as the quadratic of the remaining coefficients (by the
 *     same test as the linear equation, or as nothing); the root at infinity, the model f1 - f2, is dropped.
 *   - Every model is de-normalised, scaled to unit Frobenius norm and given the canonical sign: the entry of largest magnitude (the
 *     first on ties) is positive.  Models are ordered by ascending root.  A model with a non-finite entry is no model.
 *   Score, in float on (float)F
 *   - image 2: a = F0 x + F1 y + F2, b = F3 x + F4 y + F5, c = F6 x + F7 y + F8, d2 = x' a + y' b + c, e2 = d2 d2 / (a a + b b); image 1
 *     the same with F' and the points exchanged; err = max(e1, e2); inlier iff err <= (float)(threshold * threshold).  A NaN (in
 *     either error) is no inlier.
 *   Best model and re-fit
 *   - A model replaces the best iff it has more inliers and at least 7; RANSACUpdateNumIters runs with 7 model points.  mask[n] = the
 *     inliers of the winning RANSAC model, *iterations = iterations the sequential loop runs.
 *   - The re-fit is the normalised 8-point algorithm on the winner's inliers, at least 8 of them: the 9 x 9 normal matrix in the
 *     homography re-fit's summation order (256 lanes, lane l the points l, l + 256, .. ascending, then the halving tree), its smallest
 *     eigenvector by the cyclic Jacobi, rank 2 by zeroing the smallest singular value found by a one-sided Jacobi, de-normalisation,
 *     then the same norm and sign.  The mask stays the RANSAC mask.  A re-fit without a model (or with 7 inliers) leaves the winner.
 * esfm_find_fundamental_pairs batches many pairs like esfm_find_homography_pairs (point_offset, status, iterations as there; a pair
 * with fewer than 7 points: status 0, zeros, no error).  n_inliers[p] (or NULL) is counted under the RETURNED F.
 * Left out: pairs across two cameras (two focal lengths per pair), a free principal point, EXIF. */
int esfm_find_fundamental(esfm_ctx *ctx, const float *pts1, const float *pts2, int n, double threshold, double confidence,
                          double *F /*9*/, uint8_t *mask /*n*/, int32_t *iterations /*or NULL*/);
int esfm_find_fundamental_pairs(esfm_ctx *ctx, int n_pairs, const int32_t *point_offset /*n_pairs+1*/, const float *pts1,
                                const float *pts2, double threshold, double confidence, double *F /*9 per pair*/,
                                uint8_t *mask /*per point*/, int32_t *status /*per pair*/, int32_t *iterations /*per pair or NULL*/,
                                int32_t *n_inliers /*per pair or NULL*/);
/* The minimal solve alone: q1, q2 [n_samples][7][2] doubles in pixels -> F_out [n_samples][3][9] (the models in root order, zeros
 * behind them), n_models[n_samples] 0 .. 3.  On the GPU, and the host build of the same header (no GPU). */
int esfm_fundamental_models(esfm_ctx *ctx, const double *q1, const double *q2, int n_samples, double *F_out, int32_t *n_models);
int esfm_fundamental_models_host(const double *q1, const double *q2, int n_samples, double *F_out, int32_t *n_models);
/* Host-only (no GPU): the 8-point re-fit on the points whose mask is set (mask NULL: all), in the refit kernel's summation order.
 * Fewer than 8 such points or no model: ESFM_ERR_NUMERIC, F zeros. */
int esfm_fundamental_refit_host(const float *pts1, const float *pts2, int n, const uint8_t *mask /*or NULL*/, double *F /*9*/);
/* Host-only (no GPU): the first n_samples 7-index samples the RANSAC above draws for `count` points. */
int esfm_fundamental_sample_stream(int count, int n_samples, int32_t *idx /*7 per sample*/);
/* Focal length from fundamental matrices (Mendonca and Cipolla): with the right K = [f 0 cx; 0 f cy; 0 0 1], K' F K is an essential
 * matrix and its two non-zero singular values are equal.  cost[k] = sum_p w_p (s1 - s2) / (s1 + s2) / sum_p w_p for candidates[k],
 * s1 >= s2 the two largest singular values of K_k' F_p K_k by a one-sided Jacobi in f64; one thread per (candidate, pair), the sums over
 * the pairs in pair order by a fixed tree (256 lanes, lane l the pairs l, l + 256, .., then halving), so the curve is bit-exact
 * against the host twin and the restatement.  The candidates come from the caller (a log grid needs pow).  n_pairs >= 1. */
int esfm_focal_cost(esfm_ctx *ctx, int n_pairs, const double *F /*9 per pair*/, const double *weight /*per pair*/, double cx, double cy,
                    int n_cand, const double *candidates, double *cost_out /*n_cand*/);
int esfm_focal_cost_host(int n_pairs, const double *F /*9 per pair*/, const double *weight /*per pair*/, double cx, double cy, int n_cand,
                         const double *candidates, double *cost_out /*n_cand*/);

/* ---- SURF detection + description (SURF half) ----------------------------
 * FeatureMatching::detectFeaturesSURF (cpp_code/src/feature_matching.cpp:43-58): cv::xfeatures2d::SURF::create(minHessian)
 * ->detect(image, keypoints) then SURF::create()->compute(image, keypoints, descriptors), OpenCV defaults (4 octaves, 3 layers
 * per octave, 64-float descriptors, rotation-invariant).  image: rows x cols x channels uint8, row-major; channels = 3 is BGR
 * as cv::imread delivers it (converted with cvtColor's fixed-point weights), channels = 1 is already gray.  Outputs, strongest
 * first (OpenCV's KeypointGreater order): keypoints[7 k + 0..6] = pt.x, pt.y, size, angle (degrees), response, octave, class_id
 * (sign of the Laplacian); descriptors[64 k ..] unit-length.  At most max_keypoints are returned (OpenCV returns all; pass
 * rows * cols / 4 to be sure).  The box-filter Hessian pyramid, the 3 x 3 x 3 maxima with quadratic refinement, the dominant
 * orientation (cv::fastAtan2 polynomial, 60-degree window in 5-degree steps) and the descriptor (rotated bilinear window,
 * area shrink to 21 x 21, Gaussian-weighted 2 x 2 gradients, 4 x 4 cells) follow OpenCV's surf.cpp operation by operation. */
int esfm_surf_detect_and_compute(esfm_ctx *ctx, const uint8_t *image, int rows, int cols, int channels, double hessian_threshold,
                                 int max_keypoints, float *keypoints /*7 per*/, float *descriptors /*64 per*/, int32_t *n_keypoints);

/*
 * FeatureMatching::detectFeaturesORB (cpp_code/src/feature_matching.cpp:14-41; feature type 'O', sfm.cpp:116):
 * cv::ORB::create(nfeatures)->detect + ->compute with OpenCV's defaults (scale factor 1.2, 8 levels, edge threshold 31,
 * HARRIS_SCORE, patch 31, FAST threshold 20).  image: rows x cols x channels (1 = gray, 3 = BGR) bytes, host.
 * keypoints: 7 floats each -- x, y (level-0 pixels), size, angle (degrees), response (Harris), octave, class_id (-1);
 * descriptors: 32 bytes each (cv::Mat CV_8U, what esfm_match_hamming takes).  Level by level, ordered inside a level by
 * (response descending, y, x); at most max_keypoints are written.  Documented deviation: the 256 intensity tests use this
 * library's own seeded point pairs, not OpenCV's learned rBRIEF table (which ships only inside OpenCV).
 */
int esfm_orb_detect_and_compute(esfm_ctx *ctx, const uint8_t *image, int rows, int cols, int channels, int nfeatures,
                                int max_keypoints, float *keypoints /*7 each*/, uint8_t *descriptors /*32 each*/,
                                int32_t *n_keypoints);

/*
 * SIFT detection + description (feature type 'I'; the Python prototype's SIFT branch, SIFT_create(nfeatures) +
 * detectAndCompute): OpenCV 3.4 xfeatures2d SIFT with its defaults -- 3 layers per octave, contrastThreshold 0.04,
 * edgeThreshold 10, sigma 1.6, an image upsampled x2 first (firstOctave -1), float pyramid.  image: rows x cols x channels
 * (1 = gray, 3 = BGR, converted with cvtColor's fixed-point weights) bytes, host, sides up to 16384.  keypoints: 7 floats each
 * -- x, y (input pixels), size, angle (degrees), response (|contrast|), OpenCV's packed octave (an integer below 2^24, exact in
 * float), class_id (-1); descriptors: 128 floats each with integer values 0..255, as OpenCV 3.x stores them (what
 * esfm_match_l2_f32 takes).  At most max_keypoints are written.
 *
 * Operation by operation (tests/sift_ref/sift_ref.c writes every step down and is bit-identical to this entry point):
 *   base = gray upsampled x2 (INTER_LINEAR, exact) blurred with sqrtf(1.6^2 - 4 * 0.5^2); nOctaves = cvRound(log2(min side of
 *   the base) - 2) + 1; 6 Gaussian layers per octave (GaussianBlur on CV_32F: getGaussianKernel taps from the host's exp(),
 *   BORDER_REFLECT_101 iterated for kernels wider than the image, the row pass summed over the taps in order, the column pass
 *   as w[r] c + sum_k w[r+k] (up_k + down_k)); the next octave starts from every second pixel of layer 3; DoG = layer
 *   differences; candidates |v| > 1 and >= / <= all 26 neighbours, 5 px inside; adjustLocalExtrema (3 x 3 float solve by
 *   partial pivoting, at most 5 steps, contrast and edge tests); a 36-bin orientation histogram per candidate, smoothed
 *   [1 4 6 4 1] / 16, one keypoint per peak >= 0.8 max; the 4 x 4 x 8 descriptor with trilinear splits, the 0.2 clamp and the
 *   512 scale, saturated to bytes.  exp / exp2 / sin / cos are this library's own written-out polynomial routines (double
 *   range reduction and Horner, within 1 ulp of the true value), atan2 is cv::fastAtan2's polynomial.  Keypoints come out in
 *   scan order (octave, layer, row, column, then orientation peak), duplicates (same x, y, size, angle) removed keeping the
 *   first.  Documented deviations from OpenCV: nfeatures > 0 keeps every keypoint whose response is >= the nfeatures-th largest
 *   (ties included) in scan order, where OpenCV's retainBest uses nth_element (its set on ties and its order are
 *   implementation-defined); removeDuplicated keeps the scan order instead of re-sorting; the exp / sin / cos routines are not
 *   OpenCV's, so bit parity with OpenCV binaries is not claimed.  A candidate or keypoint list beyond the internal lists'
 *   capacity (a sixteenth of the interior samples plus 4096; twice that for keypoints) is ESFM_ERR_NUMERIC, never a silent
 *   truncation.
 */
int esfm_sift_detect_and_compute(esfm_ctx *ctx, const uint8_t *image, int rows, int cols, int channels, int nfeatures,
                                 int max_keypoints, float *keypoints /*7 each*/, float *descriptors /*128 each*/,
                                 int32_t *n_keypoints);

/* ---- Image undistortion (undistort part) -------------------------------
 * MotionEstimator::doUnDistort (cpp_code/src/estimate_motion.cpp:431-441): cv::undistort(rgb_image, out, K, distort_coeff), run
 * once per imported frame before feature detection (cpp_code/test/sfm.cpp:97-98).  image / out: rows x cols x channels uint8
 * (1 or 3 interleaved channels), distinct buffers; K4 = fx, cx, fy, cy (no skew; it is also the new camera matrix); dist4 =
 * k1, k2, p1, p2 as DOUBLES -- the values cv::undistort actually sees.  (The reference fills its CV_64F coefficient matrix
 * through at<float>, cpp_code/src/data_io.cpp:118-121, so a distortion file reaches OpenCV as two doubles whose bit patterns
 * are the float pairs (k1, k2) and (p1, p2); the host mirrors reproduce that, this entry point takes whatever doubles result.)
 * Follows OpenCV's algorithm operation by operation: stripes of min(max(1, 4096 / cols), rows) rows with their own new camera
 * matrix (cy - y0) and closed-form 3 x 3 inverse, the normalised x accumulated along the row, the distortion model in double,
 * source coordinates rounded to 1/32 pixel (CV_16SC2 maps), 8-bit bilinear taps with 15-bit fixed-point weights, zero outside
 * the image (INTER_LINEAR, BORDER_CONSTANT). */
int esfm_undistort(esfm_ctx *ctx, const uint8_t *image, int rows, int cols, int channels, const double *K4, const double *dist4,
                   uint8_t *out);

/* ---- Dense reconstruction: plane-sweep depth maps and depth-map fusion ------------------------------
 * The reference README's TODO list: "add multi-view stereo dense reconstruction".  Runs after the final bundle adjustment on the
 * registered poses, the (undistorted) images and the sparse cloud with its track ids.  The classic fronto-parallel plane sweep with
 * windowed NCC (Collins 1996; Gallup et al. 2007) and a geometric-consistency fusion of the depth maps.  Every f32 formula below is
 * written with its operation order; tests/mvs_ref.py restates this text and the GPU reproduces it bit for bit (no contraction of
 * mul + add, correctly rounded division and sqrt, window sums as row-major loops from the top-left tap).
 *
 * Conventions.  Poses: 12 floats per view, row-major [R | t] mapping world to camera (x_cam = R X + t), Frame.pose_cam[:3, :4].
 * K4 = (fx, cx, fy, cy) per view.  Pixel (col x, row y) has its centre at (x, y).  images: n_views x rows x cols x channels u8
 * (3 = BGR, 1 = grey), all views one size; grey values are cvtColor's fixed-point BGR2GRAY (as SURF), used as f32 0..255.
 * Depth is z in the reference camera; 0 = no estimate.  neighbours: n_views x max_neighbours view indices, -1 = none (skipped).
 *
 * Options (esfm_mvs_options_default; every call rejects an out-of-range value with ESFM_ERR_INVALID_ARG and writes nothing):
 *   num_planes D 128 (3..1024), window_radius r 3 (1..7), max_neighbours 4 (1..8), min_shared_points 20 (>= 1), best_k 2
 *   (1..max_neighbours), depth_margin 0.25 (>= 0), max_cost 0.5 (not NaN), min_var 4.0 grey levels^2 (> 0, finite),
 *   fuse_min_views 2 (1..max_neighbours), fuse_reproj_px 1.0 (> 0), fuse_rel_depth 0.01 (> 0).
 *
 * esfm_mvs_plan (host only, no GPU): view selection and depth range.  registered[v] != 0 marks a registered view; obs_offsets
 * [n_views + 1] / obs_points: CSR of the cloud points (indices into xyz) view v observes -- the points whose track id is among
 * the frame's unique_pixel_ids; duplicates count once.  Neighbours of registered view r: every other registered view v scored
 * by |obs(r) n obs(v)|, kept if score >= min_shared_points, the best max_neighbours by score descending, ties to the lower
 * index, padded with -1.  Depth range: z = ((R20 X0 + R21 X1) + R22 X2) + t2 (f32) of the points of obs(r) with z > 0,
 * sorted ascending; fewer than 10 (or no neighbour, or view not registered): (0, 0); otherwise lo = z[floor(0.02 (n - 1))],
 * hi = z[ceil(0.98 (n - 1))], d_min = lo / (1 + depth_margin), d_max = hi * (1 + depth_margin) (f32, 1 + depth_margin first).
 * neighbours out: n_views x max_neighbours; depth_range out: n_views x 2 (d_min, d_max).
 *
 * esfm_mvs_depth_maps: depth and cost, n_views x rows x cols f32 each, for every view with d_min > 0 (others: depth 0,
 * cost +inf).  Rejected: a neighbour index out of range or equal to the view; d_min >= d_max (when d_min > 0; a range must be
 * finite); an image smaller than the window (rows or cols < 2 r + 1).  A source needs only its image and pose.
 *   Planes: in double, step = (1/d_min - 1/d_max) / (D - 1), invd_k = 1/d_max + k step; k = 0 is the farthest.
 *   Homographies, per source s of reference r, in double with explicit scalar loops (sums from 0 over l = 0, 1, 2):
 *   R_sr[i][j] = sum_l Rs[i][l] Rr[j][l]; t_sr[i] = ts[i] - sum_l R_sr[i][l] tr[l]; M = R_sr with M[i][2] += t_sr[i] invd_k;
 *   A[i][j] = sum_l M[i][l] Kr^-1[l][j] with Kr^-1 = [[1/fx, 0, -cx/fx], [0, 1/fy, -cy/fy], [0, 0, 1]];
 *   H[i][j] = sum_l Ks[i][l] A[l][j]; each entry rounded to f32 once.
 *   Warped value of reference pixel (x, y) (f32): w = (h6 x + h7 y) + h8, nu = (h0 x + h1 y) + h2, nv = (h3 x + h4 y) + h5,
 *   u = nu / w, v = nv / w, x0 = floorf(u), fx = u - x0, y0 = floorf(v), fy = v - y0; valid only if w > 0, 0 <= x0,
 *   x0 + 1 < cols, 0 <= y0, y0 + 1 < rows; value = (1 - fy) ((1 - fx) I00 + fx I01) + fy ((1 - fx) I10 + fx I11).
 *   Every window tap of every reference pixel uses this same per-pixel value.
 *   Cost of one source (n = (2r+1)^2 taps, row-major from the top-left tap, sums from 0): mr = (sum ref) / n, ms = (sum src) / n;
 *   cov = sum (ref - mr)(src - ms), vr = sum (ref - mr)^2, vs = sum (src - ms)^2; c = 1 - cov / sqrtf(vr vs).  Invalid if
 *   any tap is invalid, vr < n min_var or vs < n min_var (n min_var in f32).
 *   Aggregation: the v valid source costs sorted ascending, m = min(best_k, v), C_k = (their sum in ascending order) / m;
 *   v = 0: plane invalid.  Winner k* = first k with the smallest valid C_k.  depth = 0 if the reference window leaves the image,
 *   no plane is valid, C_k* > max_cost or k* in {0, D - 1}; otherwise a = C_{k*-1}, b = C_k*, c = C_{k*+1}, den = (a - 2b) + c,
 *   off = den > 0 ? 0.5f (a - c) / den : 0, clamped to [-0.5, 0.5], 0 if a or c is invalid; depth = 1 / ((float)invd_k* +
 *   off (float)step).  cost = C_k*, +inf where no plane is valid.
 *
 * esfm_mvs_fuse: depth (n_views x rows x cols, e.g. from esfm_mvs_depth_maps) to a coloured cloud.  For every view r and pixel
 * (x, y) with d > 0 (f32 throughout): xc = ((x - cx) / fx) d, yc = ((y - cy) / fy) d, zc = d; e = (xc, yc, zc) - t;
 * X[j] = (R[0][j] e0 + R[1][j] e1) + R[2][j] e2.  For each neighbour s (list order, -1 skipped): p = Rs X + ts as
 * ((Rs[i][0] X0 + Rs[i][1] X1) + Rs[i][2] X2) + ts[i]; if p2 > 0: u = fx_s (p0 / p2) + cx_s, v = fy_s (p1 / p2) + cy_s,
 * px = floorf(u + 0.5f), py = floorf(v + 0.5f); if 0 <= px < cols, 0 <= py < rows and d_s = depth_s[py][px] > 0: Y = the
 * back-projection of (px, py) with d_s in s (as X), q = Rr Y + tr (as p), du = (fx (q0 / q2) + cx) - x, dv likewise,
 * consistent if du du + dv dv < fuse_reproj_px fuse_reproj_px and fabsf(q2 - d) < fuse_rel_depth d.  The pixel is kept if at
 * least fuse_min_views neighbours are consistent; its point is (X + Y_1 + Y_2 ...) / (1 + count), summed X first, then the
 * consistent Y in neighbour order, per coordinate; its colour the reference pixel as RGB (grey: a grey triple).  Points are
 * ordered by (view, row, col); xyz / rgb hold n_views rows cols points (3 floats / 3 bytes each), *n_points the number written.
 * Duplicate surface points seen from several views are not removed.
 * Both compute entry points take host pointers; without a usable device they return ESFM_ERR_NO_DEVICE (no CPU fallback). */
typedef struct esfm_mvs_options {
    int32_t num_planes, window_radius, max_neighbours, min_shared_points, best_k;
    float depth_margin, max_cost, min_var;
    int32_t fuse_min_views;
    float fuse_reproj_px, fuse_rel_depth;
} esfm_mvs_options;
void esfm_mvs_options_default(esfm_mvs_options *opt);
int esfm_mvs_plan(int n_views, const uint8_t *registered, const float *poses /*12 each*/, int n_points, const float *xyz /*3 each*/,
                  const int32_t *obs_offsets /*n_views + 1*/, const int32_t *obs_points, const esfm_mvs_options *opt,
                  int32_t *neighbours /*n_views x max_neighbours*/, float *depth_range /*2 each*/);
int esfm_mvs_depth_maps(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4 /*4 each*/,
                        const float *poses /*12 each*/, const int32_t *neighbours, const float *depth_range /*2 each*/,
                        const esfm_mvs_options *opt, float *depth, float *cost);
int esfm_mvs_fuse(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4 /*4 each*/,
                  const float *poses /*12 each*/, const int32_t *neighbours, const float *depth, const esfm_mvs_options *opt,
                  float *xyz, uint8_t *rgb, int32_t *n_points);

/* Dense-cloud merge: per-pixel normals from the depth maps, the fusion that also reports each point's pixel, and a voxel grid
 * that leaves one point per occupied voxel with the views that support it.  tests/merge_ref.py restates the three rules below
 * in numpy; every accumulation across points is an integer sum, so the GPU agrees with it bit for bit whatever the order.
 *
 * esfm_mvs_normals: world normals, n_views x rows x cols x 3 f32, (0, 0, 0) = invalid.  A plane is exactly linear in inverse
 * depth over pixel coordinates, w(x + dx, y + dy) = a dx + b dy + g; the rule fits that function by least squares over a window.
 * Options (esfm_mvs_normal_options_default): normal_radius m 3 (1..7), normal_min_taps 25 (3..(2m+1)^2), normal_rel_step 0.05
 * (> 0, finite).  Pixel (x, y) of view r with d = depth > 0: wc = 1.0f / d (f32).  Taps (dx, dy) over -m..m, row-major from
 * the top-left tap; a tap outside the image is skipped; a tap counts if its depth dt > 0 and fabsf(wt - wc) <=
 * normal_rel_step * wc with wt = 1.0f / dt (both sides f32).  Sums in double, in tap order, each from 0: S1 += 1, Sx += dx,
 * Sy += dy, Sxx += dx dx, Sxy += dx dy, Syy += dy dy, Sw += (double)wt, Sxw += dx (double)wt, Syw += dy (double)wt.  Invalid if
 * S1 < normal_min_taps.  Otherwise, in double with exactly these groupings:
 *   c00 = Syy S1 - Sy Sy, c01 = Sxy S1 - Sy Sx, c02 = Sxy Sy - Syy Sx, det = (Sxx c00 - Sxy c01) + Sx c02,
 *   da = (Sxw c00 - Sxy (Syw S1 - Sy Sw)) + Sx (Syw Sy - Syy Sw),
 *   db = (Sxx (Syw S1 - Sw Sy) - Sxw c01) + Sx (Sxy Sw - Syw Sx),
 *   dg = (Sxx (Syy Sw - Sy Syw) - Sxy (Sxy Sw - Sx Syw)) + Sxw c02.
 * Invalid unless det > 0.  a = da / det, b = db / det, g = dg / det.  Camera normal (fx, cx, fy, cy and x, y as doubles):
 * n0 = a fx, n1 = b fy, n2 = (g + a (cx - x)) + b (cy - y), L = sqrt((n0 n0 + n1 n1) + n2 n2); invalid unless L is finite and
 * > 0; n = -n / L (it faces the camera).  World normal N[j] = (R[0][j] n0 + R[1][j] n1) + R[2][j] n2 with R cast from f32 to
 * double; each component rounded to f32 once.  Arguments as esfm_mvs_fuse takes them (rows, cols 1..16384, at most 2^31 - 256
 * pixels, K4 finite with non-zero focal lengths).
 *
 * esfm_mvs_fuse_ex: esfm_mvs_fuse with one more output, pixel_index (may be NULL; capacity n_views rows cols):
 * (view rows + y) cols + x of each written point.  Points, colours and count are those of esfm_mvs_fuse, bit for bit.
 *
 * esfm_cloud_voxel_merge: n points (0 <= n <= 2^28), xyz f32; rgb u8 (3 each), normals f32 (3 each, finite) and tags int32 (one
 * each, 0..63, e.g. the view) may each be NULL.  voxel_size h f32 (finite, > 0), min_points >= 1, min_tags >= 0.  Outputs of
 * capacity n: out_xyz, and optionally out_rgb, out_normals, out_count (int32 members) and out_tagmask (uint64), plus *n_out.
 * Rejected with ESFM_ERR_INVALID_ARG, nothing written: a tag outside 0..63; min_tags > 0 without tags; an output array
 * requested without its input (out_rgb / rgb, out_normals / normals, out_tagmask / tags); a cell index that would reach 2^21.
 *   A point is valid if its three coordinates are finite; others are ignored.  o_a = the f32 minimum of coordinate a over the
 *   valid points.  Cell c_a = floorf((x_a - o_a) / h) (f32 subtract, correctly rounded f32 divide); floorf is monotone, so
 *   the 2^21 limit is tested with the coordinate maximum.  Key = cz << 42 | cy << 21 | cx.
 *   Member offset in double: u_a = ((double)x_a - (double)o_a) / (double)h - (double)c_a, q_a = llrint(u_a 2^30) (ties to even).
 *   Per voxel with k members, Q_a = sum q_a (int64).  Point: (float)((double)o_a + ((double)c_a + ((double)Q_a / (double)k)
 *   / 2^30) (double)h).  Colour per channel: (sum + k / 2) / k in integers.  Normals: members with a non-zero normal add
 *   llrint((double)n_a 2^20) to int64 M_a; m_a = (double)M_a, L = sqrt((m0 m0 + m1 m1) + m2 m2); output (float)(m_a / L), or
 *   (0, 0, 0) if L is 0.  tagmask = OR of 1 << tag over the members.  A voxel is kept if k >= min_points and
 *   popcount(tagmask) >= min_tags.  Kept voxels come out in ascending key order.  Nothing depends on the order of a voxel's
 *   members.  No valid point: *n_out = 0.
 * All three take host pointers; without a usable device they return ESFM_ERR_NO_DEVICE (no CPU fallback). */
typedef struct esfm_mvs_normal_options {
    int32_t normal_radius, normal_min_taps;
    float normal_rel_step;
} esfm_mvs_normal_options;
void esfm_mvs_normal_options_default(esfm_mvs_normal_options *opt);
int esfm_mvs_normals(esfm_ctx *ctx, int n_views, int rows, int cols, const float *K4 /*4 each*/, const float *poses /*12 each*/,
                     const float *depth, const esfm_mvs_normal_options *opt, float *normals /*3 per pixel*/);
int esfm_mvs_fuse_ex(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4 /*4 each*/,
                     const float *poses /*12 each*/, const int32_t *neighbours, const float *depth, const esfm_mvs_options *opt,
                     float *xyz, uint8_t *rgb, int32_t *pixel_index /*may be NULL*/, int32_t *n_points);
int esfm_cloud_voxel_merge(esfm_ctx *ctx, int n, const float *xyz /*3 each*/, const uint8_t *rgb /*3 each, may be NULL*/,
                           const float *normals /*3 each, may be NULL*/, const int32_t *tags /*may be NULL*/, float voxel_size,
                           int min_points, int min_tags, float *out_xyz, uint8_t *out_rgb, float *out_normals, int32_t *out_count,
                           uint64_t *out_tagmask, int32_t *n_out);

/* ---- Surface reconstruction: TSDF volume and watertight triangle mesh --------------------------------
 * Depth maps (e.g. esfm_mvs_depth_maps masked to the pixels esfm_mvs_fuse_ex kept) are integrated into a truncated signed
 * distance volume, and an indexed triangle mesh is extracted from it by marching tetrahedra on the Kuhn decomposition: a
 * translation-invariant rule, so neighbouring cells agree on every shared face and there are no ambiguity cases.  One voxel
 * is one thread's work and every ordering is by linear index, so nothing depends on scheduling; tests/tsdf_ref.py restates
 * this text in numpy and the GPU reproduces it bit for bit.  Conventions are those of the dense section (poses, K4, depth 0 =
 * none, colour order as esfm_mvs_fuse).  All arithmetic is f32 unless said otherwise, no mul + add contraction, correctly
 * rounded division and sqrtf.
 *
 * Grid (esfm_tsdf_grid): dims (nx, ny, nz) each 2..1024, product at most 2^27; voxel_size h finite and > 0; origin finite.
 * Voxel (i, j, k) has linear index (k ny + j) nx + i and centre X_a = origin_a + ((float)i_a + 0.5f) * h.
 * Options (esfm_tsdf_options_default: trunc 0, min_weight 2): trunc 0 means 4.0f * h, otherwise finite and >= h;
 * min_weight >= 1.
 *
 * esfm_tsdf_integrate: n_views 1..64, images may be NULL (then rgb must be NULL).  Per voxel, the views v = 0 .. n - 1 in that
 * order (a view without a positive depth contributes nothing), S (f32) and W, Wc, colour sums (integers) from 0:
 *   p_i = ((R[i][0] X0 + R[i][1] X1) + R[i][2] X2) + t[i]; skip unless p2 > 0;
 *   u = fx (p0 / p2) + cx, v = fy (p1 / p2) + cy, px = floorf(u + 0.5f), py = floorf(v + 0.5f); skip unless 0 <= px < cols,
 *   0 <= py < rows and d = depth[v][py][px] > 0;
 *   s = d - p2; skip if s < -trunc;  S += fminf(1.0f, s / trunc), W += 1;
 *   with images, if s <= trunc: add the pixel's R, G, B (grey: a grey triple) to the colour sums, Wc += 1.
 * Outputs, one per voxel: tsdf = W > 0 ? S / (float)W : 1.0f; weight = W; rgb = (sum + Wc / 2) / Wc in integers per channel,
 * (0, 0, 0) if Wc is 0.
 *
 * esfm_tsdf_extract: tsdf, weight and rgb (may be NULL) as above, from any source.
 *   A voxel is valid if weight >= min_weight, inside if valid and tsdf < 0.  Cell (i, j, k), i < nx - 1 and so on, has the
 *   eight corner voxels (i + dx, j + dy, k + dz); it is live if all eight are valid.
 *   A live cell splits into six tetrahedra, one per permutation (a, b, c) of the axes in lexicographic order (xyz, xzy, yxz,
 *   yzx, zxy, zyx), with the ordered corners q0 = (0,0,0), q1 = q0 + e_a, q2 = q1 + e_b, q3 = (1,1,1).
 *   Edges: every tetrahedron edge runs from a voxel v to v + delta, delta a non-zero vector of {0,1}^3; v owns it, its
 *   direction id is e = (dx | dy << 1 | dz << 2) - 1 in 0..6.  The edge is used if exactly one end is inside and at least one
 *   cell that holds both ends is live (4 cells for an axis edge, 2 for a face diagonal, 1 for the body diagonal).
 *   Vertices: one per used edge, numbered in ascending (owner linear index, e).  fa = tsdf at the owner, fb at the other end:
 *   tt = fa / (fa - fb); position P_a = Xa_a + tt * ((float)delta_a * h) with Xa the owner's centre; colour per channel
 *   (uint8)floorf((ca + tt * (cb - ca)) + 0.5f), ca and cb as f32.
 *   Gradient at a voxel, per axis, with f+ / f- the tsdf of the axis neighbours that are in the grid and valid:
 *   0.5f * (f+ - f-) if both qualify, f+ - f or f - f- if one does, 0 if none.  g = ga + tt * (gb - ga) per component,
 *   L = sqrtf((g0 g0 + g1 g1) + g2 g2); normal = g / L, or (0, 0, 0) if L is 0 or not finite.  It points to the outside
 *   (towards positive distance: free space).
 *   Triangles: by ascending cell linear index (that of the cell's origin voxel), then tetrahedron 0..5, then as listed, with
 *   local corner indices 0..3 and edges written as corner pairs.  One corner a alone inside or alone outside, the others
 *   b < c < d: (ab, ac, ad).  Two inside a < b, two outside c < d: (ac, ad, bd) and (ac, bd, bc).  None or all four inside:
 *   nothing.  Winding, in integers on lattice coordinates: m_i = the sum of the two corners of edge i, n = (m1 - m0) x
 *   (m2 - m0), s = n_in * (sum of the outside corners) - n_out * (sum of the inside corners); if n . s < 0 the second and
 *   third vertex are swapped (n . s is never 0).  (v1 - v0) x (v2 - v0) then points to the outside.  Where a tsdf value is
 *   exactly 0, tt is 0 or 1 and triangles of zero area occur; they are kept, the topology relies on them.
 *   Capacities: *n_vertices and *n_triangles always receive the needed counts (both below 2^31); if either exceeds
 *   max_vertices / max_triangles no geometry is written and the call returns ESFM_ERR_INVALID_ARG with both counts in the
 *   message.  vertices, normals (may be NULL): 3 f32 each; vertex_rgb (may be NULL, needs rgb): 3 u8; triangles: 3 int32.
 *
 * esfm_mvs_mesh: esfm_tsdf_integrate then esfm_tsdf_extract with the volume staying on the device; the mesh equals the
 * two-step result bit for bit (colours are integrated only if vertex_rgb is requested, which needs images).
 * Rejected with ESFM_ERR_INVALID_ARG, before the device is looked at: a non-finite grid value, dims out of range, more than
 * 2^27 voxels, a trunc that is non-zero and below h or not finite, min_weight < 1, an output requested without its input,
 * a negative capacity.  All three take host pointers; without a usable device they return ESFM_ERR_NO_DEVICE (no CPU
 * fallback). */
typedef struct esfm_tsdf_grid {
    float origin[3];
    float voxel_size;
    int32_t dims[3];
} esfm_tsdf_grid;
typedef struct esfm_tsdf_options {
    float trunc;
    int32_t min_weight;
} esfm_tsdf_options;
void esfm_tsdf_options_default(esfm_tsdf_options *opt);
int esfm_tsdf_integrate(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images /*may be NULL*/,
                        const float *K4 /*4 each*/, const float *poses /*12 each*/, const float *depth, const esfm_tsdf_grid *grid,
                        const esfm_tsdf_options *opt, float *tsdf, int32_t *weight, uint8_t *rgb /*3 each, may be NULL; needs images*/);
int esfm_tsdf_extract(esfm_ctx *ctx, const esfm_tsdf_grid *grid, const float *tsdf, const int32_t *weight,
                      const uint8_t *rgb /*may be NULL*/, const esfm_tsdf_options *opt, int max_vertices, int max_triangles,
                      float *vertices, float *normals /*may be NULL*/, uint8_t *vertex_rgb /*may be NULL; needs rgb*/,
                      int32_t *triangles /*3 each*/, int32_t *n_vertices, int32_t *n_triangles);
int esfm_mvs_mesh(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images /*may be NULL*/,
                  const float *K4 /*4 each*/, const float *poses /*12 each*/, const float *depth, const esfm_tsdf_grid *grid,
                  const esfm_tsdf_options *opt, int max_vertices, int max_triangles, float *vertices, float *normals /*may be NULL*/,
                  uint8_t *vertex_rgb /*may be NULL; needs images*/, int32_t *triangles /*3 each*/, int32_t *n_vertices,
                  int32_t *n_triangles);

/* ---- Mesh clean-up: component filter, Taubin smoothing, face normals ----------------------------------
 * An indexed triangle mesh (e.g. esfm_mvs_mesh's) loses its small connected pieces, is low-pass filtered without shrinking,
 * and gets vertex normals from its faces.  Every step is a rule on sorted key lists with a fixed operation order, so nothing
 * depends on scheduling; tests/mesh_clean_ref.py restates this text in numpy and the GPU reproduces it bit for bit.  All
 * arithmetic is f32, no mul + add contraction, correctly rounded division and sqrtf.
 *
 * Input: V vertices (3 f32 each), vertex_rgb optional (3 u8 each), T triangles (3 int32 each); 0 <= V <= 2^30,
 * 0 <= T <= 2^28.  A triangle index outside 0 .. V - 1 is rejected.  Triangles that repeat an index are legal: the rules
 * below are stated on key lists and so say what happens to them.
 *
 * Components: two vertices are connected if a triangle holds both; label[v] is the smallest vertex index of v's component (a
 * vertex in no triangle is its own component).  A triangle belongs to the component of its first corner; count[c] is the
 * component's number of triangles, largest the maximum count.  A component is kept iff count >= min_component_triangles and
 * 1000 * (int64)count >= (int64)min_component_permille * largest.
 * Compaction: kept vertices and kept triangles keep their ascending order, indices are remapped, colours are carried through;
 * vertex_map / triangle_map (may be NULL) receive the old index of every new vertex / triangle.  The outputs have capacity V
 * and T; *n_out_vertices and *n_out_triangles are always written.  T == 0 or nothing kept: ESFM_OK with 0 and 0.
 *
 * Adjacency, on the output mesh: the multiset of directed keys (a << 32) | b over the six ordered corner pairs (0,1), (1,0),
 * (1,2), (2,1), (2,0), (0,2) of every triangle, without the keys that have a == b.  N(i) is the ascending list of the distinct
 * b with a key (i, b); the multiplicity of (i, b) is the number of triangle sides on the edge {i, b}.  Vertex i is pinned iff
 * some key (i, b) has a multiplicity other than 2 (borders and non-manifold edges).
 *
 * Smoothing (Taubin lambda | mu): passes s = 0 .. 2 smooth_iterations - 1 with w = smooth_lambda on even s, smooth_mu on odd
 * s; every vertex reads the positions p the previous pass left (Jacobi).  k = |N(i)|.  If k == 0, or pin_boundary is set and i
 * is pinned: q_i = p_i.  Otherwise per coordinate a: m = p[n_0]_a, then m += p[n_j]_a for j = 1 .. k - 1 in list order;
 * c = m / (float)k; q_ia = p_ia + w * (c - p_ia).
 *
 * Normals, always recomputed from the output mesh: the face vector of triangle t is e1 = p1 - p0, e2 = p2 - p0,
 * f = (e1_1 e2_2 - e1_2 e2_1, e1_2 e2_0 - e1_0 e2_2, e1_0 e2_1 - e1_1 e2_0), every product rounded.  For vertex i, n is the
 * sequential f32 sum, starting from the first, of f over the keys (i << 32) | (3 t + corner) in ascending key order;
 * L = sqrtf((n0 n0 + n1 n1) + n2 n2); the normal is n / L, or (0, 0, 0) if L is 0 or not finite.  With esfm_tsdf_extract's
 * winding it points to free space as the gradient normals do; a caller who wants those indexes them with vertex_map.
 *
 * Options (esfm_mesh_clean_options_default): min_component_triangles 64 (>= 1), min_component_permille 10 (0..1000),
 * smooth_iterations 5 (0..1000), smooth_lambda 0.5 (finite, in (0, 1]), smooth_mu -0.53 (finite, in [-1.5, 0]), pin_boundary 1
 * (0 or 1).
 *
 * esfm_mesh_components: the labelling alone.  labels: V int32; tri_count (may be NULL): V int32, a component's count at its
 * label vertex and 0 elsewhere; *n_components.
 * esfm_mesh_clean: the whole chain.  out_normals, out_rgb (needs vertex_rgb), vertex_map and triangle_map may be NULL.
 * Rejected with ESFM_ERR_INVALID_ARG, before the device is looked at and with nothing written: an option out of range, a
 * negative count or one above the limits, a triangle index outside 0 .. V - 1, a required pointer that is NULL, out_rgb
 * without vertex_rgb.  Both take host pointers; without a usable device they return ESFM_ERR_NO_DEVICE (no CPU fallback). */
typedef struct esfm_mesh_clean_options {
    int32_t min_component_triangles, min_component_permille, smooth_iterations;
    float smooth_lambda, smooth_mu;
    int32_t pin_boundary;
} esfm_mesh_clean_options;
void esfm_mesh_clean_options_default(esfm_mesh_clean_options *opt);
int esfm_mesh_components(esfm_ctx *ctx, int n_vertices, int n_triangles, const int32_t *triangles /*3 each*/, int32_t *labels /*V*/,
                         int32_t *tri_count /*V, may be NULL*/, int32_t *n_components);
int esfm_mesh_clean(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices /*3 each*/,
                    const uint8_t *vertex_rgb /*3 each, may be NULL*/, const int32_t *triangles /*3 each*/,
                    const esfm_mesh_clean_options *opt, float *out_vertices, float *out_normals /*may be NULL*/,
                    uint8_t *out_rgb /*may be NULL; needs vertex_rgb*/, int32_t *out_triangles, int32_t *vertex_map /*may be NULL*/,
                    int32_t *triangle_map /*may be NULL*/, int32_t *n_out_vertices, int32_t *n_out_triangles);

/* ---- Mesh simplification: grid vertex clustering with quadric placement --------------------------------
 * An indexed triangle mesh (e.g. esfm_mesh_clean's) is reduced by merging all vertices of one cell of a regular grid into one
 * representative, placed where the cell's summed plane quadrics are smallest (Lindstrom's out-of-core simplification).  Every
 * step is a rule on sorted key lists with a fixed operation order, so nothing depends on scheduling; tests/simplify_ref.py
 * restates this text in numpy and the GPU reproduces it bit for bit.  No mul + add contraction anywhere, correctly rounded
 * division and square root; sums are f64, start from +0.0 and add their terms one by one in the stated order.
 *
 * Input: V vertices (3 f32 each), vertex_rgb optional (3 u8 each), T triangles (3 int32 each), with the limits of the clean-up
 * (0 <= V <= 2^30, 0 <= T <= 2^28, indices in 0 .. V - 1, repeated indices legal); origin[3] and cell, f32.
 *
 * Cells: per axis a, i_a = (int)floorf((p_a - origin_a) / cell) in f32.  Every index must lie in 0 .. 2^21 - 1 (a coordinate
 * that is not finite fails this too).  key = (i_0 << 42) | (i_1 << 21) | i_2; the distinct keys in ascending order number the
 * cells 0 .. C - 1, cell_of[v] is vertex v's cell number.  The cell centre is cc_a = origin_a + (i_a + 0.5) * cell in f64 from
 * the f32 inputs.
 *
 * Per-cell sums.  Over the cell's n vertices in ascending vertex index: s_a += (double)p_a - cc_a; m_a = s_a / n.  Colours: the
 * integer sum S per channel, the cell's colour is (2 S + n) / (2 n) in integer division.  Over the cell's triangle corners in
 * ascending 3 t + corner -- the keys (cell_of[vertex] << 32) | (3 t + corner) in ascending order --, with p0, p1, p2 the
 * corners of triangle t in its own order, in f64: e1 = p1 - p0, e2 = p2 - p0,
 * N = (e1_1 e2_2 - e1_2 e2_1, e1_2 e2_0 - e1_0 e2_2, e1_0 e2_1 - e1_1 e2_0), L = sqrt((N_0 N_0 + N_1 N_1) + N_2 N_2).  A corner
 * with L > 0 false adds nothing.  Otherwise D = -((N_0 d_0 + N_1 d_1) + N_2 d_2) with d = p0 - cc, and
 * A_ab += (N_a N_b) / L for ab = 00, 01, 02, 11, 12, 22;  b_a += (N_a D) / L.  This is the area-weighted plane quadric about
 * the cell centre.  A triangle with two or three corners in one cell is added once per corner.
 *
 * Placement: tau = (A_00 + A_11) + A_22.  If use_quadric is 0 or tau > 0 is false, x = m.  Otherwise r = (double)regularisation
 * * tau, M = A + r I, g_a = r m_a - b_a, and (M x = g) by LDL^T without pivoting:
 *   d0 = M_00; l10 = M_01 / d0; l20 = M_02 / d0; d1 = M_11 - l10 M_01; u = M_12 - l20 M_01; l21 = u / d1;
 *   d2 = (M_22 - l20 M_02) - l21 u; y0 = g_0; y1 = g_1 - l10 y0; y2 = (g_2 - l20 y0) - l21 y1;
 *   x_2 = y2 / d2; x_1 = y1 / d1 - l21 x_2; x_0 = (y0 / d0 - l10 x_1) - l20 x_2.
 * If |x_a| <= (double)cell fails for some a (NaN and infinities fail it), x = m.  The representative is (float)(cc + x).
 *
 * Triangles: every corner is remapped through cell_of; a triangle that names a cell twice is dropped.  A survivor is rotated so
 * that its smallest cell number comes first, (c, p, q); it is odd if p > q, even otherwise.  Survivors with the same unordered
 * triple form a group.  A group with more members of one orientation than of the other keeps its lowest-numbered triangle of
 * the majority orientation; a group with equal counts keeps nothing (two opposite faces on the same three vertices: removing
 * both keeps a closed mesh closed).  Kept triangles keep their ascending input order and their input corner order.  Cells in no
 * kept triangle are dropped; the others keep their ascending order and are renumbered.
 *
 * Normals: recomputed on the output mesh by the rule of "Mesh clean-up" (face-vector sums in incidence-key order).
 *
 * Outputs, capacities V and T: out_vertices, out_normals (may be NULL), out_rgb (may be NULL, needs vertex_rgb), out_triangles;
 * vertex_map (may be NULL): V int32, the new vertex of every old vertex or -1; triangle_map (may be NULL): the old index of
 * every new triangle; *n_out_vertices and *n_out_triangles are always written on ESFM_OK.  T == 0 or nothing kept: ESFM_OK with
 * 0 and 0 (vertex_map is all -1).
 *
 * Options (esfm_mesh_simplify_options_default): regularisation 1e-3 (finite, in (0, 1]), use_quadric 1 (0 or 1; 0 places every
 * representative at the cell mean cc + m).
 *
 * Rejected with ESFM_ERR_INVALID_ARG, before the device is looked at and with nothing written: an option out of range, cell not
 * finite or <= 0, an origin that is not finite, a vertex outside the 2^21 cells per axis, a negative count or one above the
 * limits, a triangle index outside 0 .. V - 1, a required pointer that is NULL, out_rgb without vertex_rgb.  The grouping of
 * triangles holds three cell numbers in one 64-bit key: more than 2^21 occupied cells is ESFM_ERR_UNSUPPORTED, with nothing
 * written (use a larger cell).  Host pointers; without a usable device ESFM_ERR_NO_DEVICE (no CPU fallback). */
typedef struct esfm_mesh_simplify_options {
    float regularisation;
    int32_t use_quadric;
} esfm_mesh_simplify_options;
void esfm_mesh_simplify_options_default(esfm_mesh_simplify_options *opt);
int esfm_mesh_simplify(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices /*3 each*/,
                       const uint8_t *vertex_rgb /*3 each, may be NULL*/, const int32_t *triangles /*3 each*/, const float *origin /*3*/,
                       float cell, const esfm_mesh_simplify_options *opt, float *out_vertices, float *out_normals /*may be NULL*/,
                       uint8_t *out_rgb /*may be NULL; needs vertex_rgb*/, int32_t *out_triangles, int32_t *vertex_map /*V, may be NULL*/,
                       int32_t *triangle_map /*may be NULL*/, int32_t *n_out_vertices, int32_t *n_out_triangles);

/* ---- Mesh texturing: per-triangle view choice, z-buffer, atlas bake ---------------------------------------
 * An indexed triangle mesh (e.g. esfm_mesh_simplify's) gets a texture atlas from the photographs: every view rasterises the mesh
 * into a buffer of inverse depths, every triangle chooses the view that sees it largest and unoccluded, and every atlas texel
 * fetches its colour from its triangle's view.  The only combination across threads is an integer maximum, the views are tried in
 * view order and one texel is one thread's work, so nothing depends on scheduling; tests/texture_ref.py restates this text in numpy
 * and the GPU reproduces it bit for bit.  All arithmetic is f32, no mul + add contraction, correctly rounded division and sqrtf;
 * fminf / fmaxf return the other operand where one is NaN.  Conventions are those of the dense section (poses, K4, pixel centres,
 * images n_views x rows x cols x channels u8 with 3 = BGR and 1 = grey; colours come out as RGB, grey as a grey triple).
 *
 * Input: V vertices (3 f32 each, finite), T triangles (3 int32 each, indices in 0 .. V - 1, repeated indices legal), 0 <= V <= 2^30,
 * 0 <= T <= 2^25; n_views 1..64 of rows x cols pixels, both 2..16384; K4 and poses finite, focal lengths not 0.
 *
 * Projection of a world point X into view v: p_i = ((R[i][0] X0 + R[i][1] X1) + R[i][2] X2) + t[i]; u = fx (p0 / p2) + cx,
 * w = fy (p1 / p2) + cy, z = 1.0f / p2 (the inverse depth).  X is in front of v if p2 > 0, |u| <= 2^20 and |w| <= 2^20 (a NaN fails).
 * Its nearest pixel is (floorf(u + 0.5f), floorf(w + 0.5f)), as in esfm_tsdf_integrate.
 *
 * Screen triangle of triangle t in view v: its vertices' (x_k, y_k, z_k) = (u, w, z), k = 0, 1, 2 in the triangle's own order; it
 * exists only if all three are in front.  A triangle with a vertex at p2 <= 0 in a view (or otherwise not in front) is skipped in
 * that view: there it neither occludes nor can be labelled.  area2 = (x1 - x0) (y2 - y0) - (y1 - y0) (x2 - x0).
 *
 * esfm_mesh_texture_views.
 *   Depth buffer of view v, rows x cols uint32, 0 = nothing covers the pixel: each cell is the largest bit pattern (a positive f32
 *   orders like a uint32) of the inverse depths that the screen triangles with area2 != 0 give the pixel.  With s = 1.0f if
 *   area2 > 0, else -1.0f, a triangle gives a value to pixel (px, py) if
 *     fmaxf(ceilf(xmin - 0.5f), 0) <= px <= fminf(floorf(xmax + 0.5f), cols - 1), likewise py with ymin, ymax and rows (xmin =
 *     fminf(fminf(x0, x1), x2) and so on), and for the three edges k, from vertex k to vertex k' = (k + 1) mod 3, with
 *     ex = x_k' - x_k, ey = y_k' - y_k, e_k = ex (py - y_k) - ey (px - x_k):  s e_k >= -0.5f (|ex| + |ey|).
 *   That is coverage widened by half a pixel, because the later look-up is by nearest pixel; both windings occlude.  The value is
 *   b0 = e_1 / area2, b1 = e_2 / area2, b2 = e_0 / area2, z = (b0 z0 + b1 z1) + b2 z2, then z = fminf(fmaxf(z, zmin), zmax) with zmin
 *   and zmax the smallest and largest of z0, z1, z2, so that the half-pixel rim does not extrapolate.
 *   View choice of triangle t: views 0 .. n - 1 in order; best = 0.0f, label = -1.  View v is admissible if
 *     - the screen triangle exists, every vertex has 1 <= x_k <= cols - 2 and 1 <= y_k <= rows - 2, and score = 0.5f |area2| > 0;
 *     - with P0, P1, P2 the world corners, N = (P1 - P0) x (P2 - P0) (products rounded, as the clean-up's face vector; it points
 *       outside by the extractor's convention), G_a = ((P0_a + P1_a) + P2_a) / 3.0f, the camera centre C_j = -((R[0][j] t0 +
 *       R[1][j] t1) + R[2][j] t2), D = C - G, d = (N0 D0 + N1 D1) + N2 D2, |N| = sqrtf((N0 N0 + N1 N1) + N2 N2), |D| likewise:
 *       d > 0 and d >= min_cos * (|N| * |D|);
 *     - each of four test points, the three vertices (x_k, y_k, z_k) and the projection of G (which must be in front), has its
 *       nearest pixel inside the image and z >= (float)buffer[v][py][px] * (1.0f - occlusion_tol), the buffer's bits read as f32.
 *   If v is admissible and score > best: best = score, label = v.  So the label is the admissible view of greatest score (half the
 *   screen area in pixels), the lowest index on a tie, and -1 with score 0 if none is admissible.
 *   Outputs: label [T] int32, score [T] f32 (best), depth_buffers [n_views, rows, cols] uint32 (may be NULL).
 *
 * esfm_mesh_texture_bake.  texels S 4..64, atlas_width A >= 1 squares.  The atlas is W = A S texels wide and
 * H = ceil(ceil(T / 2) / A) S texels high (0 for T = 0), both at most 16384; atlas [H, W, 3] u8 RGB, row 0 first.
 *   Layout: square q = t / 2 has its first texel at column (q % A) S and row (q / A) S.  Texel (i, j) of a square, column i and row
 *   j, has its centre at (i + 0.5, j + 0.5) in the square's texel units and belongs to triangle 2 q if i + j <= S - 1, else to
 *   2 q + 1.  Chart corners, for the triangle's vertices 0, 1, 2: even (0.5, 0.5), (S - 1.5, 0.5), (0.5, S - 1.5); odd
 *   (S - 0.5, S - 0.5), (2.5, S - 0.5), (S - 0.5, 2.5).  With bilinear filtering between texel centres, every texel that has a
 *   non-zero weight for a point inside a chart belongs to that chart's triangle and lies in its square.
 *   uv [T, 3, 2] f32: corner (cx, cy) of a triangle in the square at column X0, row Y0 is (((float)X0 + cx) / (float)W,
 *   ((float)Y0 + cy) / (float)H): normalised, origin at the outer corner of the atlas's first texel, u along a row, v down the rows.
 *   Texel of triangle t >= T: (0, 0, 0).  Otherwise its barycentrics: even b1 = (float)i / (float)(S - 2), b2 = (float)j /
 *   (float)(S - 2); odd b1 = (float)(S - 1 - i) / (float)(S - 3), b2 = (float)(S - 1 - j) / (float)(S - 3); b0 = (1.0f - b1) - b2.
 *   Texels outside the chart extrapolate: that is the gutter fill.
 *   Fallback colour: with vertex_rgb, per channel c = (b0 c0 + b1 c1) + b2 c2 of the three vertex colours as f32,
 *   c = fminf(fmaxf(c, 0.0f), 255.0f), (uint8)floorf(c + 0.5f); without, (128, 128, 128).
 *   label[t] = -1: the fallback colour.  Otherwise X_a = (b0 P0_a + b1 P1_a) + b2 P2_a is projected into view label[t]; if p2 > 0 is
 *   false, the fallback colour; else uc = fminf(fmaxf(u, 0.0f), (float)(cols - 1)), x0 = fminf(floorf(uc), (float)(cols - 2)),
 *   ax = uc - x0, likewise wc, y0, ay with rows, and per channel, with I the image of that view,
 *   c = (1.0f - ay) * ((1.0f - ax) * I[y0][x0] + ax * I[y0][x0 + 1]) + ay * ((1.0f - ax) * I[y0 + 1][x0] + ax * I[y0 + 1][x0 + 1]),
 *   the texel's channel (uint8)floorf(c + 0.5f).
 *   Capacity: *atlas_rows receives H whenever the arguments are otherwise valid; if H > max_atlas_rows nothing else is written and
 *   the call returns ESFM_ERR_INVALID_ARG with H in the message.
 *
 * esfm_mesh_texture_level: seam levelling.  Where neighbouring triangles chose different views the atlas shows a step in colour
 * (exposure, vignetting, small pose errors).  Every (vertex, label) pair gets one additive offset per colour channel such that the
 * views agree at the vertices they share and the offsets vary smoothly inside each view's region: the global adjustment of Waechter,
 * Moehrle and Goesele (2014), restricted to vertex samples.  Steps 2 to 5 are f64, no mul + add contraction, correctly rounded
 * division; no sum depends on thread order, so tests/level_ref.py restates this text and the GPU reproduces it bit for bit.
 *   1. Samples.  Triangle t takes part if label[t] >= 0 and all three of its vertices have p2 > 0 in view label[t].  Corner k of
 *      such a triangle projects its vertex into that view; per RGB channel f is the bake's bilinear c at (u, w) -- the same clamps,
 *      x0, y0, ax, ay and operation order --, kept as f32 and not rounded.  3 channels: BGR as in the bake; 1 channel: the three
 *      colour channels are equal.  Every other triangle gets offsets and samples 0 and contributes nothing.
 *   2. Nodes.  A node is a distinct (vertex, label) among the corners that take part, its key vertex * 64 + label; nodes are numbered
 *      in ascending key order (all corners of a node sample the same pixel position, so a node has one f).  seam(a): the other nodes
 *      with a's vertex (a contiguous run).  smooth(a): the nodes b != a that share a triangle that takes part with a, each once
 *      however many triangles share the edge; a repeated index in a triangle gives no pair.  A seam vertex has two or more nodes.
 *   3. System, per channel: minimise  sum over seam pairs ((g_a + f_a) - (g_b + f_b))^2 + lambda sum over smooth pairs (g_a - g_b)^2
 *      + mu sum g_a^2.  Its normal equations, per node:  (A g)_a = (s + lambda * m) + mu * g_a  with s = sum over b in seam(a) of
 *      (g_a - g_b), m = sum over b in smooth(a) of (g_a - g_b), both in ascending b and starting from 0.0;  rhs_a = sum over b in
 *      seam(a), ascending, of ((double)f_b - (double)f_a), from 0.0;  d_a = ((double)|seam(a)| + lambda * (double)|smooth(a)|) + mu.
 *   4. tree_sum(x[0 .. n)): 0.0 for n = 0; otherwise x is padded with +0.0 to a multiple of 256, in every block of 256, for h = 128,
 *      64, .., 1: x[i] += x[i + h] for i < h, block j's x[0] is element j of the next level, until one value is left.  dot(x, y) is
 *      the tree_sum of the rounded products x_a * y_a, per channel.
 *   5. Jacobi-preconditioned conjugate gradients, the three channels in one loop, each with its own scalars:
 *        g = 0, r = rhs, z = r / d, p = z, rz = dot(r, z), bb = dot(rhs, rhs).  No node, or bb == 0 in every channel: iterations 0,
 *        converged 1.  Otherwise, for k = 1 .. max_iterations (none for 0: iterations 0, converged 0):
 *          q = A p;  pq = dot(p, q);  alpha = rz / pq (0.0 if pq == 0);  g = g + alpha * p;  r = r - alpha * q;  rr = dot(r, r);
 *          if rr <= (tolerance * tolerance) * bb in every channel: iterations = k, converged = 1, stop;
 *          z = r / d;  rz' = dot(r, z);  beta = rz' / rz (0.0 if rz == 0);  p = z + beta * p;  rz = rz'.
 *        Never stopped: iterations = max_iterations, converged = 0.  The count is part of the result.
 *   6. Outputs: offsets [T, 3 corners, 3 RGB] f32 = (float)g of the corner's node, samples (same shape, may be NULL) = f, stats.
 * esfm_mesh_texture_bake_ex is esfm_mesh_texture_bake with offsets [T, 3, 3] (NULL: the same call, bit for bit).  A texel that takes
 * its colour from a view gets, per channel and on the unrounded bilinear c, c = c + ((b0 * o0 + b1 * o1) + b2 * o2) in f32 with its
 * own barycentrics and its triangle's three corner offsets (the gutter extrapolates), c = fminf(fmaxf(c, 0.0f), 255.0f), then
 * (uint8)floorf(c + 0.5f).  Texels with the fallback colour are untouched.
 *
 * Options (esfm_mesh_texture_options_default): min_cos 0.2 (in [0, 1)), occlusion_tol 0.02 (in [0, 1)).
 * (esfm_mesh_texture_level_options_default): lambda 0.1 (finite, > 0), mu 0.001 (finite, > 0), tolerance 1e-4 (in [0, 1)),
 * max_iterations 200 (0..10000).
 * Rejected with ESFM_ERR_INVALID_ARG, before the device is looked at and with nothing written: a vertex, K4 or pose value that is
 * not finite, a focal length of 0, a triangle index outside 0 .. V - 1, a count, n_views, rows or cols out of range, channels other
 * than 1 or 3, texels outside 4..64, atlas_width < 1, an atlas above 16384 texels per side, a label outside -1 .. n_views - 1, an
 * option out of range, an offset that is not finite, a required pointer that is NULL.  Host pointers; without a usable device
 * ESFM_ERR_NO_DEVICE (no CPU fallback). */
typedef struct esfm_mesh_texture_options {
    float min_cos;
    float occlusion_tol;
} esfm_mesh_texture_options;
void esfm_mesh_texture_options_default(esfm_mesh_texture_options *opt);
int esfm_mesh_texture_views(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices /*3 each*/,
                            const int32_t *triangles /*3 each*/, int n_views, int rows, int cols, const float *K4 /*4 each*/,
                            const float *poses /*12 each*/, const esfm_mesh_texture_options *opt, int32_t *label /*T*/,
                            float *score /*T*/, uint32_t *depth_buffers /*n_views x rows x cols, may be NULL*/);
int esfm_mesh_texture_bake(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices /*3 each*/,
                           const uint8_t *vertex_rgb /*3 each, may be NULL*/, const int32_t *triangles /*3 each*/,
                           const int32_t *label /*T*/, int n_views, int rows, int cols, int channels, const uint8_t *images,
                           const float *K4 /*4 each*/, const float *poses /*12 each*/, int texels, int atlas_width,
                           int max_atlas_rows, uint8_t *atlas /*max_atlas_rows x W x 3*/, float *uv /*T x 3 x 2*/,
                           int32_t *atlas_rows);
typedef struct esfm_mesh_texture_level_options {
    double lambda;
    double mu;
    double tolerance;
    int32_t max_iterations;
} esfm_mesh_texture_level_options;
typedef struct esfm_mesh_texture_level_stats {
    int32_t nodes;
    int32_t seam_vertices;
    int32_t iterations;
    int32_t converged;
} esfm_mesh_texture_level_stats;
void esfm_mesh_texture_level_options_default(esfm_mesh_texture_level_options *opt);
int esfm_mesh_texture_level(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices /*3 each*/,
                            const int32_t *triangles /*3 each*/, const int32_t *label /*T*/, int n_views, int rows, int cols,
                            int channels, const uint8_t *images, const float *K4 /*4 each*/, const float *poses /*12 each*/,
                            const esfm_mesh_texture_level_options *opt, float *offsets /*T x 3 x 3*/,
                            float *samples /*T x 3 x 3, may be NULL*/, esfm_mesh_texture_level_stats *stats);
int esfm_mesh_texture_bake_ex(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices /*3 each*/,
                              const uint8_t *vertex_rgb /*3 each, may be NULL*/, const int32_t *triangles /*3 each*/,
                              const int32_t *label /*T*/, int n_views, int rows, int cols, int channels, const uint8_t *images,
                              const float *K4 /*4 each*/, const float *poses /*12 each*/, int texels, int atlas_width,
                              int max_atlas_rows, uint8_t *atlas /*max_atlas_rows x W x 3*/, float *uv /*T x 3 x 2*/,
                              int32_t *atlas_rows, const float *offsets /*T x 3 x 3, may be NULL*/);

/* ---- Mesh rendering: watertight rasteriser, depth, triangle identity, colour ---------------------------------
 * An indexed triangle mesh is drawn into n views: per pixel the triangle that owns it, its depth and its colour from the texture
 * atlas, from vertex colours or plain grey.  The conventions are those of "Mesh texturing": poses, K4, pixel centres at integers,
 * the projection and its `in front` test with the 2^20 bound, f32 with no mul + add contraction, correctly rounded division.  The
 * only combination across threads is an integer maximum, so images, depths and identities do not depend on scheduling;
 * tests/render_ref.py restates this text in numpy and the GPU reproduces it bit for bit.
 *
 * Input: V vertices and T triangles with the texturing section's ranges and checks; optional vertex_rgb [V, 3] u8; optional
 * uv [T, 3, 2] f32 (finite; mesh_texture_bake's) together with atlas [H, W, 3] u8 RGB, H and W 2..16384 -- uv and atlas are both
 * given or both NULL; n_views 1..64 of rows x cols pixels, both 2..16384, with K4 and poses.
 *
 * Screen vertex of a world point in view v: u, w, p2 by the texturing section's projection; sx = (int32)rintf(u * 256.0f),
 * sy = (int32)rintf(w * 256.0f) (1/256-pixel fixed point, ties to even), z = 1.0f / p2.  A triangle takes part in a view only if
 * all three vertices are in front (the texturing section's skip rule; there is no clipping).
 *
 * Coverage, all of it int64 and exact.  With vertices k = 0, 1, 2 in the triangle's own order,
 *   area2 = (sx1 - sx0) (sy2 - sy0) - (sy1 - sy0) (sx2 - sx0);  area2 == 0: the triangle is skipped;  s = the sign of area2 (both
 *   windings are drawn).  For edge k, from vertex k to k' = (k + 1) mod 3: dx = sx_k' - sx_k, dy = sy_k' - sy_k, and at pixel
 *   (px, py)  e_k = dx (256 py - sy_k) - dy (256 px - sx_k).
 *   The pixel is covered if for all three edges  s e_k > 0,  or  s e_k == 0 and the edge owns its boundary:  s dy > 0, or s dy == 0
 *   and s dx < 0.  An edge and its reverse never both own and never both disown, so two triangles that share an edge cover each
 *   pixel on it exactly once: no cracks, no double hits.  Candidate pixels are the integer pixels inside the fixed-point bounding
 *   box, ceil(min / 256) .. floor(max / 256) by floor division, clipped to the image.
 *
 * Depth and identity.  b0 = (float)e_1 / (float)area2, b1 = (float)e_2 / (float)area2, b2 = (float)e_0 / (float)area2 (each int64
 * rounded to f32 once, to nearest even; the signs cancel: the barycentrics of vertices 0, 1, 2);  q_k = b_k z_k;
 * iz = (q0 + q1) + q2.  The pixel's key is (uint64)bits(iz) << 32 | (0xFFFFFFFF - t), skipped if bits(iz) == 0; the buffer keeps
 * the largest key: the nearest surface wins, on equal depth the lowest triangle index.  Key 0 is background.
 *
 * Shading, one pass per pixel from the winning key, with the same b_k, q_k and iz recomputed:  triangle_id = t (-1 background),
 * depth = 1.0f / iz (0 background).  An attribute a is perspective-correct:  ((q0 a0 + q1 a1) + q2 a2) / iz.
 *   With uv: (uu, vv) from the triangle's three corner uvs;  a = uu * (float)W - 0.5f,  c = vv * (float)H - 0.5f;  the bake's
 *   bilinear rule on the atlas as a one-view, three-channel image at (a, c) -- the same clamps, x0, y0, ax, ay and operation order,
 *   channel by channel (the atlas is RGB already) --, the output (uint8)floorf(c + 0.5f).
 *   Without uv but with vertex_rgb: the three vertex colours as f32 per channel, fminf(fmaxf(c, 0.0f), 255.0f), rounded the same way.
 *   With neither: (128, 128, 128).  Background pixels get options.background (three u8, default 0, 0, 0).
 *
 * Outputs: rgb [n_views, rows, cols, 3] u8 RGB, depth [n_views, rows, cols] f32, triangle_id [n_views, rows, cols] int32; each may
 * be NULL, not all three.
 * Rejected with ESFM_ERR_INVALID_ARG, before the device is looked at and with nothing written: what the texturing section rejects
 * of a mesh and of cameras, uv without atlas or atlas without uv, an atlas side outside 2..16384, a texture coordinate that is not
 * finite, options that are NULL, all three outputs NULL.  Host pointers; without a usable device ESFM_ERR_NO_DEVICE (no CPU
 * fallback). */
typedef struct esfm_mesh_render_options {
    uint8_t background[3];
    uint8_t reserved;
} esfm_mesh_render_options;
void esfm_mesh_render_options_default(esfm_mesh_render_options *opt);
int esfm_mesh_render(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices /*3 each*/,
                     const int32_t *triangles /*3 each*/, const uint8_t *vertex_rgb /*3 each, may be NULL*/,
                     const float *uv /*T x 3 x 2, NULL with atlas*/, int atlas_rows, int atlas_cols,
                     const uint8_t *atlas /*atlas_rows x atlas_cols x 3, NULL with uv*/, int n_views, int rows, int cols,
                     const float *K4 /*4 each*/, const float *poses /*12 each*/, const esfm_mesh_render_options *opt,
                     uint8_t *rgb /*may be NULL*/, float *depth /*may be NULL*/, int32_t *triangle_id /*may be NULL*/);

/* ---- Track triangulation: robust multi-view points and a reprojection filter ------------------------------------
 * Re-estimates every sparse-cloud point from ALL the observations of its track and judges it by reprojection error, depth sign
 * and triangulation angle.  Opt-in: nothing else in the library calls it.  One arithmetic (csrc/track_core.hpp: f64, only
 * + - * / sqrt and comparisons, every sum in a fixed order) serves the kernels, the host build (the *_host entry points, no GPU)
 * and the restatement in tests/track_ref.py; the three agree to the bit.
 *
 * Inputs: bundle adjustment's three observation arrays unchanged (cam_idx, pt_idx, obs_uv float32 pixels), K4 = fx, cx, fy, cy
 * floats per camera, and a world -> camera [R | t] per camera as 12 doubles, row-major (Rt[4 r + c]; column 3 is t).  A track is
 * the observations of one point in INPUT order; the arrays need not be grouped.
 *
 * Per observation k:  x = (u - cx) / fx, y = (v - cy) / fy;  centre C_j = -((R0j t0 + R1j t1) + R2j t2);
 *   direction d_j = (R0j x + R1j y) + R2j.  Dot products are (a0 b0 + a1 b1) + a2 b2 throughout.
 * Projection of X:  p_r = ((Rr0 X0 + Rr1 X1) + Rr2 X2) + t_r;  iz = 1 / p_2;  xn = p_0 iz, yn = p_1 iz;
 *   ru = (fx xn + cx) - u, rv = (fy yn + cy) - v, err2 = ru ru + rv rv.  Inlier iff p_2 > 0 and err2 <= thr2 (thr2 =
 *   max_reproj_error_px squared); the cost term is err2 for an inlier and thr2 otherwise (= min(err2, thr2), NaN-free).
 * Hypotheses: the observation pairs (a, b), a < b, in lexicographic order, P = n (n - 1) / 2 of them.  P <= max_hypotheses: all;
 *   else hypothesis h (0 <= h < max_hypotheses) is pair number floor(h P / max_hypotheses) in 64-bit integers.  The point is the
 *   midpoint of the two rays: w = C_a - C_b, aa = d_a.d_a, bb = d_b.d_b, ab = d_a.d_b, dw = d_a.w, ew = d_b.w,
 *   det = aa bb - ab ab, s = (ab ew - bb dw) / det, t = (aa ew - ab dw) / det, X_j = 0.5 ((C_a,j + s d_a,j) + (C_b,j + t d_b,j)).
 *   Void unless det > 1e-12 (aa bb) and s > 0 and t > 0.
 * Rank: (inliers, cost = sum of the cost terms in observation order, hypothesis index) compared as one key: more inliers, then the
 *   lower cost, then the lower index -- a total order, so the reduction over hypotheses does not depend on its shape.
 * Refit: refine_iterations Gauss-Newton steps on the best hypothesis's inliers.  Per inlier in observation order, with a = fx iz,
 *   b = fy iz: Ju_j = a (R0j - xn R2j), Jv_j = b (R1j - yn R2j); A_ij += Ju_i Ju_j + Jv_i Jv_j (i <= j); g_i += Ju_i ru + Jv_i rv.
 *   LDL' in the order 0, 1, 2 without pivoting: d0 = A00; l10 = A01 / d0; l20 = A02 / d0; d1 = A11 - l10 A01; m = A12 - l20 A01;
 *   l21 = m / d1; d2 = (A22 - l20 A02) - l21 m;  y0 = -g0; y1 = -g1 - l10 y0; y2 = (-g2 - l20 y0) - l21 y1;  z_i = y_i / d_i;
 *   e2 = z2; e1 = z1 - l21 e2; e0 = (z0 - l10 e1) - l20 e2;  X += e.  A pivot that is not > 0 or a non-finite new X ends the refit
 *   with the X before that step.  Inliers are then recomputed once; if the refitted point has fewer than the hypothesis had, the
 *   hypothesis point and its inliers stand.
 * Statistics: n_inliers; mse = (sum of the inliers' err2 in observation order) / n_inliers (0 without inliers); min_cos = the
 *   minimum over inlier pairs of e_i.e_j with e_i = (C_i - X) / sqrt((C_i - X).(C_i - X)) componentwise (1 with fewer than two
 *   inliers) -- an exact f64 minimum.
 * Verdict (pt_status): 0 kept; 1 fewer than two observations; 2 no valid hypothesis; 3 n_inliers < min_views; 4 min_cos >
 *   cos_min_angle; 5 a non-finite uv, K4 or Rt value in the track (or, for evaluate, a non-finite point).  The first that applies
 *   in the order 1, 5, 2, 3, 4.  Statuses 0, 3, 4 report the estimated point's inliers and statistics; 1, 2, 5 report obs_inlier 0,
 *   obs_err2 +inf, n_inliers 0, min_cos 1, mse 0.  xyz_out of a point that is not kept is xyz_in's (zeros without xyz_in).
 *
 * Options (esfm_track_options_default): max_reproj_error_px 4.0, min_angle_deg 1.5, min_views 2, max_hypotheses 64,
 * refine_iterations 5.  4 px and 1.5 degrees are the common conventions of incremental SfM; they have NOT been measured on this
 * project's data.  cos_min_angle is what the verdict compares against; _default sets it to cos(min_angle_deg) and a caller who
 * changes the angle sets both (the Python and C++ wrappers do).  Rejected with ESFM_ERR_INVALID_ARG, nothing written: options
 * NULL, a threshold that is not finite and > 0, cos_min_angle NaN, min_views < 2, max_hypotheses outside 1 .. 4096,
 * refine_iterations outside 0 .. 100, an index out of range, a NULL required array.  A track longer than 65 535 observations is
 * ESFM_ERR_UNSUPPORTED.
 *
 * esfm_track_triangulate / esfm_track_evaluate run on the GPU (host pointers; without a usable device no context exists and
 * creating one fails with ESFM_ERR_NO_DEVICE: no CPU fallback).  The tracks are grouped on the device: 64-bit keys
 * (pt_idx << 32 | input index), the radix sort, run heads by the block scan; one wave per track, observations staged in LDS up to
 * ESFM_TRACK_STAGE_CAP (256) per track, longer tracks read the same records from global memory.  esfm_track_evaluate runs no
 * hypotheses and no refit: inliers, statistics and verdict of the given points (status 2 cannot occur) -- the filter after BA.
 * The *_host forms run the same header on the CPU. */
#define ESFM_TRACK_STAGE_CAP 256
#define ESFM_TRACK_MAX_OBS 65535
typedef struct esfm_track_options {
    double max_reproj_error_px;
    double min_angle_deg;
    double cos_min_angle;
    int32_t min_views;
    int32_t max_hypotheses;
    int32_t refine_iterations;
    int32_t reserved;
} esfm_track_options;
void esfm_track_options_default(esfm_track_options *opt);
int esfm_track_triangulate(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx,
                           const float *obs_uv /*2 each*/, const float *K4_per_cam, const double *Rt12_per_cam,
                           const double *xyz_in /*3 n_pt or NULL*/, const esfm_track_options *opt, double *xyz_out /*3 n_pt*/,
                           uint8_t *obs_inlier /*n_obs*/, float *obs_err2 /*n_obs or NULL*/, int32_t *pt_status /*n_pt*/,
                           int32_t *pt_n_inliers /*n_pt*/, double *pt_min_cos /*n_pt or NULL*/, double *pt_mse /*n_pt or NULL*/);
int esfm_track_evaluate(esfm_ctx *ctx, int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx,
                        const float *obs_uv, const float *K4_per_cam, const double *Rt12_per_cam, const double *xyz_in /*3 n_pt*/,
                        const esfm_track_options *opt, uint8_t *obs_inlier, float *obs_err2 /*or NULL*/, int32_t *pt_status,
                        int32_t *pt_n_inliers, double *pt_min_cos /*or NULL*/, double *pt_mse /*or NULL*/);
int esfm_track_triangulate_host(int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                                const float *K4_per_cam, const double *Rt12_per_cam, const double *xyz_in /*or NULL*/,
                                const esfm_track_options *opt, double *xyz_out, uint8_t *obs_inlier, float *obs_err2 /*or NULL*/,
                                int32_t *pt_status, int32_t *pt_n_inliers, double *pt_min_cos /*or NULL*/, double *pt_mse /*or NULL*/);
int esfm_track_evaluate_host(int n_cam, int n_pt, int n_obs, const int32_t *cam_idx, const int32_t *pt_idx, const float *obs_uv,
                             const float *K4_per_cam, const double *Rt12_per_cam, const double *xyz_in,
                             const esfm_track_options *opt, uint8_t *obs_inlier, float *obs_err2 /*or NULL*/, int32_t *pt_status,
                             int32_t *pt_n_inliers, double *pt_min_cos /*or NULL*/, double *pt_mse /*or NULL*/);

/* ---- Track completion: projection search for missing observations -----------------------------------------------
 * Adds observations to tracks: every cloud point is projected into every registered camera that does not observe it yet, and the
 * free keypoint near the projection whose descriptor is nearest to the track's takes the point.  Opt-in: nothing else in the
 * library calls it.  One arithmetic (csrc/complete_core.hpp) serves the kernels, the host build (esfm_track_complete_host, no GPU)
 * and the restatement in tests/complete_ref.py; the three agree to the bit.
 *
 * Inputs: n_cam registered cameras with K4 (fx, cx, fy, cy floats) and Rt (12 doubles) as in "Track triangulation"; their keypoints
 * (2 floats) and descriptor rows back to back with set_row_offset[n_cam + 1], as the guided matcher takes them (L2 of any
 * dim >= 1, or Hamming of 16, 32 or 64 bytes; a device buffer starts on a multiple of 4 bytes); one byte kp_free per keypoint
 * row; n_pt points xyz (double); the existing observations cam_idx, pt_idx, obs_kp (the keypoint index LOCAL to its camera), in
 * any order.
 * Jobs: one job (p, c) for every point p and camera c without an observation of p in the input.
 * Reference rows: the descriptor rows of p's first max_refs observations in input order.  A point without observations has no job.
 * Admissible: keypoint row k of camera c is admissible for (p, c) iff kp_free[k] != 0, the projection has p_2 > 0, and
 *   err2 <= search_radius_px^2 -- p_r, xn, yn, ru, rv, err2 exactly as in "Track triangulation" (f64, no FMA, the same association;
 *   the radius is squared in f64).  A NaN anywhere makes the row inadmissible.  No image size enters; the predicate alone decides
 *   (the kernels' grid only finds the rows to ask it about).
 * Score: d(p, k) = the minimum over the reference rows of the matcher's distance -- sqrtf of the canonical sum for L2, the bit
 *   count as a float for Hamming; a NaN distance is never the minimum.  As in the matcher, a row takes part as a candidate only
 *   with d < FLT_MAX (so neither +inf nor an all-NaN score does).
 * Choice: the two best candidates under ascending (d, k).  The job proposes k0 iff (double)d0 <= max_distance and it has only
 *   one candidate or (double)d0 < ratio * (double)d1.  A lone candidate is accepted on purpose: the window is small and
 *   max_distance is the gate.
 * Conflicts: of the points that propose one keypoint, the lowest (d0, point index) gets it; the others get nothing in that
 *   camera (no second choice).  Implemented as a 64-bit integer minimum over (float bits of d0) << 32 | p: order-free.
 * Output per keypoint row: kp_point (the winning point index, or -1) and kp_dist (d0, or FLT_MAX).  stats (may be NULL), int64[4]:
 *   jobs with at least one admissible row, proposals, proposals lost to a conflict, keypoints assigned.
 * It follows that an assigned observation is an inlier of esfm_track_evaluate at max_reproj_error_px = search_radius_px, that a
 * second call returns nothing once the assignments are applied (kp_free cleared, the observations added), that no keypoint gets
 * two points and no point two keypoints in one camera, and that the results do not depend on the order of execution.
 *
 * Options (esfm_track_complete_options_default): search_radius_px 4.0, max_distance +inf, ratio 0.8, max_refs 8 (1 .. 8,
 * ESFM_TRACK_COMPLETE_MAX_REFS).  These are conventions of incremental SfM (the reprojection threshold of the track options, Lowe's
 * ratio); they have NOT been measured on this project's data.  Rejected with ESFM_ERR_INVALID_ARG, nothing written: options NULL,
 * a NULL required array, a radius that is not finite and > 0, a NaN ratio or max_distance, max_refs outside 1 .. 8, an index out
 * of range, a width < 1 or a Hamming width other than 16, 32, 64, an unknown metric, offsets that do not start at 0 or
 * decrease, a set of more than 2^21 - 1 rows.  2^22 cameras or more, or more than 2^31 - 1 (point, camera) combinations, are
 * ESFM_ERR_UNSUPPORTED.
 *
 * esfm_track_complete takes host pointers, uploads and calls esfm_track_complete_dev.  That form takes the descriptors and the
 * keypoints on the device (everything else on the host) and writes kp_point, kp_dist and stats to device memory, on the
 * context's stream; it waits for the stream once, to size the job list by the number of jobs.  On the device: per camera the box
 * of the free keypoints and a grid of square cells at least 2 search_radius_px wide (at most 1024 per axis), keys
 * camera | cell | row through the radix sort; the jobs by an ordered compaction over n_pt x n_cam (camera not in the track, point
 * in front, window meets the box); sixteen lanes per job walk the at most 3 x 3 cells of the window.  esfm_track_complete_host
 * asks the predicate about every row of every camera on the CPU. */
#define ESFM_TRACK_COMPLETE_MAX_REFS 8
typedef struct esfm_track_complete_options {
    double search_radius_px;
    double max_distance;
    double ratio;
    int32_t max_refs;
    int32_t reserved;
} esfm_track_complete_options;
void esfm_track_complete_options_default(esfm_track_complete_options *opt);
int esfm_track_complete(esfm_ctx *ctx, esfm_metric metric, const void *desc, const float *kp /*2 each*/, const uint8_t *kp_free,
                        const int32_t *set_row_offset /*n_cam + 1*/, int n_cam, int width, const float *K4_per_cam,
                        const double *Rt12_per_cam, int n_pt, const double *xyz /*3 each*/, int n_obs, const int32_t *cam_idx,
                        const int32_t *pt_idx, const int32_t *obs_kp, const esfm_track_complete_options *opt,
                        int32_t *kp_point /*per row*/, float *kp_dist /*per row*/, int64_t *stats /*4, may be NULL*/);
int esfm_track_complete_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const float *kp_dev, const uint8_t *kp_free,
                            const int32_t *set_row_offset, int n_cam, int width, const float *K4_per_cam,
                            const double *Rt12_per_cam, int n_pt, const double *xyz, int n_obs, const int32_t *cam_idx,
                            const int32_t *pt_idx, const int32_t *obs_kp, const esfm_track_complete_options *opt,
                            int32_t *kp_point_dev, float *kp_dist_dev, int64_t *stats_dev /*may be NULL*/);
int esfm_track_complete_host(esfm_metric metric, const void *desc, const float *kp, const uint8_t *kp_free,
                             const int32_t *set_row_offset, int n_cam, int width, const float *K4_per_cam,
                             const double *Rt12_per_cam, int n_pt, const double *xyz, int n_obs, const int32_t *cam_idx,
                             const int32_t *pt_idx, const int32_t *obs_kp, const esfm_track_complete_options *opt,
                             int32_t *kp_point, float *kp_dist, int64_t *stats /*may be NULL*/);

/* ---- Image retrieval: VLAD global descriptors and a k-nearest pair list ------------------------------------------
 * Which images look alike, as an opt-in stage in front of the matcher: one global descriptor per image (VLAD over a k-means
 * codebook trained on the run's own local descriptors, quantised to int8), an all-images similarity table on the i8 matrix cores,
 * the top_k nearest images of each image, and from that table (and an optional window of preceding images) the pair list the
 * match entry points already take.  The reference has no counterpart (its to-do list's "add sequential mode" is the window part).
 * Nothing else in the library calls it.  Every sum across descriptors is an integer sum, so it does not depend on order; the
 * only float arithmetic is per element, in the order stated here.  The kernels and tests/retrieval_ref.py follow this list line
 * by line and agree to the bit.
 *
 * Inputs as esfm_match_pairs: metric, the rows of all sets back to back, set_row_offset[n_sets + 1], width.
 *   Working dimension d: L2: d = width (1 .. 256).  Hamming: d = 8 width (width 1 .. 64 bytes), component
 *   t = (byte[t >> 3] >> (t & 7)) & 1 as 0.0f / 1.0f (numpy: unpackbits(bitorder="little")).
 *   Output dimension D = n_centres d, at most ESFM_RETRIEVAL_MAX_DIM (32768); n_sets at most ESFM_RETRIEVAL_MAX_SETS (8192);
 *   beyond either: ESFM_ERR_UNSUPPORTED.  A non-finite L2 value, or |x| > 16384, is ESFM_ERR_INVALID_ARG (the bound keeps every
 *   int64 sum below 2^62).
 * Distance and assignment: dist(x, m) = acc after acc = 0f; for t ascending: df = x_t - m_t; acc = acc + df df -- all in f32,
 *   multiply and add rounded separately.  assign(x) = the lowest centre index with the smallest dist (centres scanned in ascending
 *   order with a strict <).
 * Fixed point: q(x) = llrint((double)x * 65536.0).
 * Training sample: total = all rows; stride = ceil(total / max_train); the sample is rows 0, stride, 2 stride, ... of the
 *   concatenation; nt their number.  total == 0 is ESFM_ERR_INVALID_ARG.
 * Codebook: centre c starts as sample row floor(c nt / n_centres) (64-bit integers; n_centres > nt gives duplicates, and the tie
 *   rule sends everything to the lower index).  kmeans_iterations times: assign every sample row; count_c and
 *   sum_ct = sum of q(x_t) in int64; a centre with count_c > 0 becomes m_ct = (float)(((double)sum_ct / (double)count_c) / 65536.0),
 *   an empty centre keeps its value.  kmeans_iterations == 0 returns the initialisation.
 * VLAD: per image i, centre c, component t: S = (sum over x in image i with assign(x) = c of q(x_t)) - n_ic q(m_ct) in int64
 *   (n_ic the count); maxS = max |S| over the image's D entries; maxS == 0: b = 0; else
 *   b = sign(S) rint((127.0 * sqrt((double)|S|)) / sqrt((double)maxS)) in f64, rint half-to-even: an int8 in -127 .. 127
 *   (signed-square-root VLAD scaled to its largest entry).  norm2_i = sum of b^2 (at most 32768 * 127^2: an int32).
 * Similarity: dot_ij = sum of b_i b_j in int32 (exact);
 *   score_ij = (double)dot_ij / (sqrt((double)norm2_i) * sqrt((double)norm2_j)), 0 when either norm is 0.
 * Nearest table: nearest[i][0 .. top_k) = the images j != i with norm2_j > 0, ranked by (score_ij descending, j ascending) -- a
 *   total order -- padded with -1; a row with norm2_i == 0 is all -1.
 * Pair list (host): the union of (max(i, j), min(i, j)) over the table's entries >= 0 and of (i, i - w), 1 <= w <= window,
 *   i - w >= 0; ascending by (first, second), without duplicates: the order of the (i, j < i) loop, restricted to the chosen pairs.
 *
 * Options (esfm_retrieval_options_default): n_centres 64 (1 .. 256), kmeans_iterations 10 (0 .. 100), max_train 65536
 * (1 .. 2^24), top_k 10 (0 .. 1024), window 0 (>= 0).  64 centres and 10 nearest images are conventions of VLAD retrieval; they
 * have NOT been tuned on this project's data.  Rejected with ESFM_ERR_INVALID_ARG, nothing written: options NULL or out of range,
 * a NULL required pointer, negative or decreasing offsets, a width outside the ranges above.
 *
 * esfm_retrieval_train writes the codebook (n_centres x d floats).  esfm_retrieval_vlad takes a codebook and writes vlad
 * (n_sets x D int8), norm2 and, for tests, assign (the centre of every row) and sums (S, n_sets x D int64).  esfm_retrieval_rank
 * takes int8 descriptors and writes nearest (n_sets x top_k) and, for tests, dots and scores (n_sets^2 each).
 * esfm_retrieval_pair_list is host code and needs no context; a table entry outside -1 .. n_sets - 1 or equal to its row is
 * ESFM_ERR_INVALID_ARG.  esfm_retrieval_pairs runs the whole chain with the intermediates kept on the device and one read-back
 * of the table; esfm_retrieval_pairs_dev is the same over a resident descriptor buffer and, unlike the other _dev entry points,
 * synchronises (the pair list is built on the host).  With top_k == 0 the list is the window's alone and no device work is done.
 * All pointers but desc_dev are host pointers.  No CPU fallback: without a
 * usable device no context exists. */
#define ESFM_RETRIEVAL_MAX_DIM 32768
#define ESFM_RETRIEVAL_MAX_SETS 8192
typedef struct esfm_retrieval_options {
    int32_t n_centres;
    int32_t kmeans_iterations;
    int32_t max_train;
    int32_t top_k;
    int32_t window;
    int32_t reserved;
} esfm_retrieval_options;
void esfm_retrieval_options_default(esfm_retrieval_options *opt);
int esfm_retrieval_train(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets,
                         int width, const esfm_retrieval_options *opt, float *centres /*n_centres x d*/);
int esfm_retrieval_vlad(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets,
                        int width, int n_centres, const float *centres, int8_t *vlad /*n_sets x D*/, int32_t *norm2 /*n_sets*/,
                        int32_t *assign /*total rows, or NULL*/, int64_t *sums /*n_sets x D, or NULL*/);
int esfm_retrieval_rank(esfm_ctx *ctx, int n_sets, int D, const int8_t *vlad, int top_k, int32_t *nearest /*n_sets x top_k*/,
                        int32_t *dots /*n_sets^2, or NULL*/, double *scores /*n_sets^2, or NULL*/);
int esfm_retrieval_pair_list(int n_sets, int top_k, const int32_t *nearest /*may be NULL when top_k == 0*/, int window,
                             int32_t *pairs /*capacity n_sets (top_k + window), 2 each*/, int32_t *n_pairs);
int esfm_retrieval_pairs(esfm_ctx *ctx, esfm_metric metric, const void *desc_host, const int32_t *set_row_offset, int n_sets,
                         int width, const esfm_retrieval_options *opt, int32_t *pairs /*as esfm_retrieval_pair_list*/,
                         int32_t *n_pairs);
int esfm_retrieval_pairs_dev(esfm_ctx *ctx, esfm_metric metric, const void *desc_dev, const int32_t *set_row_offset, int n_sets,
                             int width, const esfm_retrieval_options *opt, int32_t *pairs, int32_t *n_pairs);
/* Measurement only: with esfm_ctx_set_kernel_timing on, the last esfm_retrieval_pairs / _pairs_dev call's device time per stage in
 * ms[4] (hipEvents on the context's stream): codebook training, assignment + accumulation of all rows, finalise, similarity + ranking. */
int esfm_retrieval_last_stage_ms(esfm_ctx *ctx, double *ms /*4*/);

#ifdef __cplusplus
}
#endif
#endif /* ESFM_H_ */
