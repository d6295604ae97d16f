// Host side of image retrieval (include/esfm.h "Image retrieval"), free of HIP so that a g++ program under tests/cpp exercises it:
// the option and shape rules, the training sample's arithmetic and the pair list (union, sort, dedup).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/esfm.h"

namespace esfm {
namespace retrieval {

constexpr int kMaxCentres = 256, kMaxIterations = 100, kMaxTrain = 1 << 24, kMaxTopK = 1024;

// NULL when the options are usable, else what is wrong with them
inline const char *options_error(const esfm_retrieval_options *o)
{
    if (!o) return "options are NULL";
    if (o->n_centres < 1 || o->n_centres > kMaxCentres) return "n_centres must be in 1 .. 256";
    if (o->kmeans_iterations < 0 || o->kmeans_iterations > kMaxIterations) return "kmeans_iterations must be in 0 .. 100";
    if (o->max_train < 1 || o->max_train > kMaxTrain) return "max_train must be in 1 .. 2^24";
    if (o->top_k < 0 || o->top_k > kMaxTopK) return "top_k must be in 0 .. 1024";
    if (o->window < 0) return "window must be >= 0";
    return nullptr;
}

// working dimension of a descriptor row, 0 when the width is outside the metric's range
inline int working_dim(int metric, int width)
{
    if (metric == ESFM_L2_F32) return width >= 1 && width <= 256 ? width : 0;
    if (metric == ESFM_HAMMING) return width >= 1 && width <= 64 ? 8 * width : 0;
    return 0;
}

inline const char *offsets_error(const int32_t *off, int n_sets)
{
    if (n_sets < 0) return "n_sets is negative";
    if (!off) return "set_row_offset is NULL";
    if (off[0] < 0) return "set_row_offset is negative";
    for (int s = 0; s < n_sets; ++s) if (off[s + 1] < off[s]) return "set_row_offset decreases";
    return nullptr;
}

// the training sample: rows 0, stride, 2 stride, ... of `total` rows
inline void train_sample(int64_t total, int max_train, int64_t *stride, int64_t *nt)
{
    *stride = (total + max_train - 1) / max_train;
    if (*stride < 1) *stride = 1;
    *nt = (total + *stride - 1) / *stride;
}

// The pair list.  Returns ESFM_OK or ESFM_ERR_INVALID_ARG (*why says what; nothing written then).
inline int pair_list(int n_sets, int top_k, const int32_t *nearest, int window, int32_t *pairs, int32_t *n_pairs, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (n_sets < 0) { *why = "n_sets is negative"; return ESFM_ERR_INVALID_ARG; }
    if (top_k < 0 || top_k > kMaxTopK) { *why = "top_k must be in 0 .. 1024"; return ESFM_ERR_INVALID_ARG; }
    if (window < 0) { *why = "window must be >= 0"; return ESFM_ERR_INVALID_ARG; }
    if (top_k > 0 && n_sets > 0 && !nearest) { *why = "nearest is NULL"; return ESFM_ERR_INVALID_ARG; }
    if (!n_pairs) { *why = "n_pairs is NULL"; return ESFM_ERR_INVALID_ARG; }
    std::vector<uint64_t> keys;
    for (int i = 0; i < n_sets; ++i) {
        for (int k = 0; k < top_k; ++k) {
            const int32_t j = nearest[(size_t)i * (size_t)top_k + (size_t)k];
            if (j < -1 || j >= n_sets || j == i) { *why = "a table entry is outside -1 .. n_sets - 1 or names its own row"; return ESFM_ERR_INVALID_ARG; }
            if (j < 0) continue;
            const uint32_t hi = (uint32_t)(i > j ? i : j), lo = (uint32_t)(i > j ? j : i);
            keys.push_back((uint64_t)hi << 32 | lo);
        }
        const int w_end = window < i ? window : i;
        for (int w = 1; w <= w_end; ++w) keys.push_back((uint64_t)(uint32_t)i << 32 | (uint32_t)(i - w));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (!keys.empty() && !pairs) { *why = "pairs is NULL"; return ESFM_ERR_INVALID_ARG; }
    for (size_t p = 0; p < keys.size(); ++p) {
        pairs[2 * p] = (int32_t)(keys[p] >> 32);
        pairs[2 * p + 1] = (int32_t)(keys[p] & 0xffffffffu);
    }
    *n_pairs = (int32_t)keys.size();
    return ESFM_OK;
}

}  // namespace retrieval
}  // namespace esfm
