// Launch interface between render_api.cpp and render_kernels.hip (esfm_mesh_render).
#pragma once

#include "common.hpp"
#include "render_check.hpp"

namespace esfm {

struct RenderArgs {
    const float *vertices;       // V x 3, finite (checked on the host)
    const int32_t *tri;          // T x 3, every index in 0 .. V - 1 (checked on the host)
    const uint8_t *rgb;          // V x 3, may be NULL
    const float *uv;             // T x 3 x 2, finite (checked on the host); NULL exactly when atlas is
    const uint8_t *atlas;        // H x W x 3 RGB
    const TextureCam *cams;      // n
    int4 *proj;                  // n x V: (sx, sy, bits(z), 1) of a vertex in front of the view, (0, 0, 0, 0) otherwise
    unsigned long long *keys;    // n x rows x cols, zero before the rasterisation
    uint32_t *list;              // n x T: the (view, triangle) pairs whose box holds more than kRenderSmallBox pixels, in any order
    uint32_t *count;             // their number, zero before the rasterisation
    uint8_t *out_rgb;            // n x rows x cols x 3, may be NULL
    float *out_depth;            // n x rows x cols, may be NULL
    int32_t *out_id;             // n x rows x cols, may be NULL
    int32_t V, T, n, rows, cols, H, W;
    uint8_t background[3];
};

int launch_render_project(hipStream_t st, const RenderArgs &a);     // proj
int launch_render_rasterise(hipStream_t st, const RenderArgs &a);   // keys: a lane per pair, then a wave per listed pair
int launch_render_shade(hipStream_t st, const RenderArgs &a);       // out_rgb, out_depth, out_id

}  // namespace esfm
