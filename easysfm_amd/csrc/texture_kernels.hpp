// Launch interface between texture_api.cpp and texture_kernels.hip (esfm_mesh_texture_views, esfm_mesh_texture_bake).
#pragma once

#include "common.hpp"
#include "texture_check.hpp"

namespace esfm {

struct TextureViewsArgs {
    const float *vertices;       // V x 3, finite (checked on the host)
    const int32_t *tri;          // T x 3, every index in 0 .. V - 1 (checked on the host)
    const TextureCam *cams;      // n
    float4 *proj;                // n x V: (u, w, z, 1) of a vertex in front of the view, (0, 0, 0, 0) otherwise
    uint32_t *buffers;           // n x rows x cols, zero before the rasterisation
    uint32_t *list;              // n x T: the (view, triangle) pairs whose box holds more than kTextureSmallBox pixels, in any order
    uint32_t *count;             // their number, zero before the rasterisation
    int32_t *label;              // T
    float *score;                // T
    int32_t V, T, n, rows, cols;
    float min_cos, keep;         // keep = 1.0f - occlusion_tol
};

struct TextureBakeArgs {
    const float *vertices;
    const uint8_t *rgb;          // V x 3, may be NULL
    const int32_t *tri;
    const int32_t *label;        // T, every value in -1 .. n - 1 (checked on the host)
    const TextureCam *cams;
    const uint8_t *images;       // n x rows x cols x channels
    uint8_t *atlas;              // H x W x 3
    const float *offsets;        // T x 3 corners x 3 channels, finite (checked on the host); NULL: the plain bake
    int32_t T, rows, cols, channels, S, A, H;   // W = A S
};

int launch_texture_project(hipStream_t st, const TextureViewsArgs &a);     // proj
int launch_texture_rasterise(hipStream_t st, const TextureViewsArgs &a);   // buffers: a lane per pair, then a wave per listed pair
int launch_texture_choose(hipStream_t st, const TextureViewsArgs &a);      // label, score
int launch_texture_bake(hipStream_t st, const TextureBakeArgs &a);         // atlas

}  // namespace esfm
