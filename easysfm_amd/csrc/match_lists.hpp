// The list kernels behind a 2-NN table (match_lists.hip) and the packed read-back of their output (match_readback.cpp): what the
// plain matcher and the guided matcher both run after their own distance pass.
#pragma once

#include "common.hpp"
#include "pair_desc.hpp"

namespace esfm {

int launch_ratio_compact(hipStream_t st, const PairDesc *pairs, int n_pairs, const int32_t *knn_idx, const float *knn_dist,
                         double ratio, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out);
// pairs: a mirrored table of 2 n_pairs entries (pair n_pairs + p is pair p with query and train swapped), knn_idx / knn_dist the
// 2-NN tables of all of them with their markers.  Pair p keeps query q iff F = knn_idx[2 (out_off[p] + q)] >= 0 and the mirror's
// nearest of row F is q (use_ratio: and ratio_ok on both records); output as launch_ratio_compact's, for the first n_pairs pairs.
int launch_cross_check_compact(hipStream_t st, const PairDesc *pairs, int n_pairs, const int32_t *knn_idx, const float *knn_dist, int use_ratio,
                               double ratio, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out);
int launch_pack_match_lists(hipStream_t st, const long long *tab, const int32_t *n_out, int n_pairs, const int32_t *sq, const int32_t *stn, const float *sd,
                            int32_t *dq, int32_t *dtn, float *dd);
int launch_buffer_checksum(hipStream_t st, const void *buf, size_t bytes, unsigned long long *out);

// The host-pointer forms' device-side output arrays: query_idx / train_idx / distance of n_slots entries in the context's stage_b /
// stage_c / stage_d, n_pairs list lengths in stage_e.
int reserve_match_list_stage(esfm_ctx *ctx, size_t n_slots, int n_pairs);
// ... and the pair-list forms' way back from there (pair p's list at list_off[p]).  Reads the lengths into n_out, then packs the
// lists on the device (scratch: stage_a), reads them back as three dense arrays and places them at list_off[p] of the caller's
// arrays: the transfer is proportional to the matches, not to the slots.  whole_when_dense: when the matches are a quarter of the
// slots or more the three arrays go back as they are instead.  Synchronises.
int read_back_match_lists(esfm_ctx *ctx, int n_pairs, const int64_t *list_off, size_t n_slots, bool whole_when_dense, int32_t *query_idx,
                          int32_t *train_idx, float *distance, int32_t *n_out);

}  // namespace esfm
