// Launchers of the image-retrieval kernels (retrieval_kernels.hip; include/esfm.h "Image retrieval").  Every pointer is a device
// pointer; everything is enqueued on `st`, nothing synchronises.
#pragma once

#include "common.hpp"

namespace esfm {

struct RetrievalShape {
    int metric, width;   // as esfm_match_pairs
    int d, n_centres;    // working dimension; D = n_centres * d
};

// The integer sums are gathered in LDS per workgroup when D int64 entries fit there, else by global atomics (the same result).
constexpr int kRetrievalLdsMaxD = 6144;   // 48 KiB of int64
inline bool retrieval_accumulate_in_lds(int n_centres, int d) { return n_centres * d <= kRetrievalLdsMaxD; }

// *flag (zeroed by the caller) becomes 1 if a value is not finite or exceeds 16384 in magnitude
int launch_retrieval_check_values(hipStream_t st, const float *values, int64_t n, int32_t *flag);
// centre c = sample row floor(c nt / n_centres); sample row s is row s * stride
int launch_retrieval_init(hipStream_t st, const RetrievalShape &sh, const void *desc, int64_t stride, int64_t nt, float *centres);
// assign[s] = the nearest centre of row s * stride, s < n
int launch_retrieval_assign(hipStream_t st, const RetrievalShape &sh, const void *desc, int64_t stride, int64_t n, const float *centres, int32_t *assign);
// sums[set][c][t] += q(x_t), counts[set][c] += 1 over the rows s in [off[set], off[set + 1]) (row s * stride, centre assign[s]); the
// caller zeroes both; longest = the longest set
int launch_retrieval_accumulate(hipStream_t st, const RetrievalShape &sh, const void *desc, const int32_t *off, int n_sets, int64_t longest,
                                int64_t stride, const int32_t *assign, int64_t *sums, int32_t *counts);
// the k-means step: a centre with rows becomes their mean
int launch_retrieval_update(hipStream_t st, const RetrievalShape &sh, const int64_t *sums, const int32_t *counts, float *centres);
// sums becomes S in place; vlad (row pitch `pitch`, zeroed by the caller) and norm2 are written
int launch_retrieval_finalize(hipStream_t st, const RetrievalShape &sh, int n_sets, int64_t *sums, const int32_t *counts, const float *centres,
                              int8_t *vlad, int pitch, int32_t *norm2);
int launch_retrieval_repitch(hipStream_t st, const int8_t *src, int src_pitch, int8_t *dst, int dst_pitch, int rows, int cols);
// dots = V V' of the zero-padded image vp (n16 rows of pitch bytes; n16 a multiple of 16, pitch of 64), n x n of it stored
int launch_retrieval_dots(hipStream_t st, const int8_t *vp, int n16, int pitch, int n, int32_t *dots);
// root[j] = sqrt(norm2_j) (scratch, n doubles); nearest (n x top_k) and, unless NULL, scores (n x n)
int launch_retrieval_rank(hipStream_t st, int n, const int32_t *dots, int top_k, double *root, int32_t *nearest, double *scores);

}  // namespace esfm
