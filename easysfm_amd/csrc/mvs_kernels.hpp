// Launch interface between mvs_api.cpp and mvs_kernels.hip (dense reconstruction: plane sweep and depth-map fusion).
#pragma once

#include "common.hpp"

namespace esfm {

constexpr int kMvsTile = 16;          // output pixels per workgroup side (256 threads, one pixel each)
constexpr int kMvsMaxRadius = 7;
constexpr int kMvsMaxNb = 8;          // max_neighbours
constexpr int kMvsLdsStride = 48;     // LDS row stride of a halo tile: 48 = 16 mod 32, so the two 16-pixel rows of a 32-lane
                                      // ds_read_b32 group fall on disjoint banks; >= 16 + 2 * 7

struct MvsView {            // one reference view of the sweep
    int32_t active;         // has a depth range
    int32_t n_src;          // sources (the non-negative neighbour entries, in list order)
    int32_t src[kMvsMaxNb];
    float step;             // (float) inverse-depth step
    int32_t pad;
    int64_t h_off;          // first float of this view's homographies: [n_src][D][9]
    int64_t invd_off;       // first float of this view's (float) invd_k: [D]
};

struct MvsSweepArgs {
    const uint8_t *gray;    // n_views x rows x cols
    const MvsView *views;   // n_views
    const float *H;
    const float *invd;
    float *depth, *cost;    // n_views x rows x cols
    int32_t rows, cols, D, best_k, tiles_x;
    int32_t max_src;        // the most sources any view has: the dynamic LDS holds that many halo tiles
    float min_var_n, max_cost;   // n * min_var (f32), max_cost
};

struct MvsCam {             // a view of the fusion
    float K[4];             // fx, cx, fy, cy
    float P[12];            // [R | t] row-major
    int32_t nb[kMvsMaxNb];  // neighbours, -1 = none
};

struct MvsFuseArgs {
    const uint8_t *images;  // n_views x rows x cols x channels
    const MvsCam *cams;
    const float *depth;     // n_views x rows x cols
    float *stage_xyz;       // per pixel (3 floats)
    uint8_t *stage_rgb;     // per pixel (3 bytes)
    uint8_t *keep;          // per pixel
    int32_t *block_count;   // per 256-pixel block, then its exclusive offset
    float *xyz;             // compacted output
    uint8_t *rgb;
    int32_t *pixel_index;   // (view rows + y) cols + x of each compacted point; NULL = not wanted (esfm_mvs_fuse)
    int32_t *n_points;
    int64_t n_px;           // n_views x rows x cols
    int32_t rows, cols, channels, n_nb, min_views;
    float reproj2, rel_depth;
};

int launch_mvs_sweep(hipStream_t st, const MvsSweepArgs &a, int radius, int n_views);
int launch_mvs_fuse(hipStream_t st, const MvsFuseArgs &a);

struct MvsNormalArgs {
    const float *depth;     // n_views x rows x cols
    const MvsCam *cams;     // K and P are read
    float *normals;         // n_views x rows x cols x 3
    int32_t rows, cols, tiles_x, radius, min_taps;
    float rel_step;
};
int launch_mvs_normals(hipStream_t st, const MvsNormalArgs &a, int n_views);   // mvs_normals.hip

}  // namespace esfm
