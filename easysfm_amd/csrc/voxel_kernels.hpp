// Launch interface between voxel_api.cpp and voxel_kernels.hip / voxel_sort.hip (esfm_cloud_voxel_merge).
#pragma once

#include "common.hpp"

namespace esfm {

constexpr int kVoxelBoundsBlocks = 1024;   // most workgroups of the bounds reduction (one partial each, finished on the host)
constexpr int kVoxelAccWords = 11;         // per-voxel int64 accumulators: Q[3], colour[3], M[3], members, tag mask
constexpr uint64_t kVoxelNoKey = ~0ull;    // sort key of an ignored (non-finite) point: behind every cell key (those stay below 2^63)

struct VoxelBounds {       // one workgroup's partial
    float lo[3], hi[3];
    int32_t n_valid, pad;
};

struct VoxelArgs {
    // input points (rgb, normals, tags may be NULL)
    const float *xyz;
    const uint8_t *rgb;
    const float *normals;
    const int32_t *tags;
    int32_t n, n_valid;    // points; those with finite coordinates (the first n_valid sorted entries)
    float o[3], h;
    // sorted (key, point) pairs
    const uint64_t *keys;
    const int32_t *order;
    int32_t *head_count;   // per 256-entry block: run heads, then their exclusive offset; the total (the voxels) behind them
    // per voxel
    uint64_t *vox_key;
    int64_t *acc;          // kVoxelAccWords each, zero before the accumulation
    int32_t n_vox, min_points, min_tags;
    int32_t *keep_count;   // per 256-voxel block: kept voxels, then their exclusive offset; the total behind them
    // compacted output (out_rgb, out_normals, out_count, out_tagmask may be NULL)
    float *out_xyz;
    uint8_t *out_rgb;
    float *out_normals;
    int32_t *out_count;
    uint64_t *out_tagmask;
};

int launch_voxel_bounds(hipStream_t st, const float *xyz, int n, VoxelBounds *partials, int *n_partials);
int launch_voxel_keys(hipStream_t st, const VoxelArgs &a, uint64_t *keys, int32_t *index);
int launch_voxel_heads(hipStream_t st, const VoxelArgs &a);          // head counts, their scan, the total
int launch_voxel_accumulate(hipStream_t st, const VoxelArgs &a);
int launch_voxel_finalise(hipStream_t st, const VoxelArgs &a);       // keep counts, their scan, the total, the ordered write

// voxel_sort.hip: hipCUB's device radix sort of (64-bit key, point index)
int voxel_sort_scratch_bytes(int n, size_t *bytes, hipStream_t st);
int voxel_sort_pairs(void *tmp, size_t tmp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const int32_t *idx_in, int32_t *idx_out, int n,
                     hipStream_t st);

}  // namespace esfm
