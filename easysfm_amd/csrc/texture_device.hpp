// Device pieces that texture_kernels.hip and level_kernels.hip share (include/esfm.h, "Mesh texturing"): the projection of a world
// point and the bilinear fetch of the bake, each f32 expression in the header's order.
#pragma once

#include "texture_kernels.hpp"

namespace esfm {

// u, w, p2 of a world point; true if it is in front of the view
__device__ inline bool texture_project(const TextureCam &c, float X0, float X1, float X2, float &u, float &w, float &p2)
{
    const float p0 = ((c.P[0] * X0 + c.P[1] * X1) + c.P[2] * X2) + c.P[3];
    const float p1 = ((c.P[4] * X0 + c.P[5] * X1) + c.P[6] * X2) + c.P[7];
    p2 = ((c.P[8] * X0 + c.P[9] * X1) + c.P[10] * X2) + c.P[11];
    u = c.K[0] * (p0 / p2) + c.K[1];
    w = c.K[2] * (p1 / p2) + c.K[3];
    return p2 > 0.f && fabsf(u) <= 1048576.f && fabsf(w) <= 1048576.f;
}

// The four pixels around (u, w) in one view's image and their weights.
struct TextureTaps {
    const uint8_t *I;            // the pixel (x0, y0)
    int64_t right, down;
    float ax, ay;
};

__device__ inline TextureTaps texture_taps(const uint8_t *images, int label, int rows, int cols, int channels, float u, float w)
{
    const float uc = fminf(fmaxf(u, 0.0f), (float)(cols - 1)), wc = fminf(fmaxf(w, 0.0f), (float)(rows - 1));
    const float x0 = fminf(floorf(uc), (float)(cols - 2)), y0 = fminf(floorf(wc), (float)(rows - 2));
    TextureTaps s;
    s.ax = uc - x0; s.ay = wc - y0;
    s.I = images + (((int64_t)label * rows + (int)y0) * cols + (int)x0) * channels;
    s.right = channels; s.down = (int64_t)cols * channels;
    return s;
}

// The unrounded bilinear value of image channel ch.
__device__ inline float texture_fetch(const TextureTaps &s, int ch)
{
    return (1.0f - s.ay) * ((1.0f - s.ax) * (float)s.I[ch] + s.ax * (float)s.I[s.right + ch]) +
           s.ay * ((1.0f - s.ax) * (float)s.I[s.down + ch] + s.ax * (float)s.I[s.down + s.right + ch]);
}

}  // namespace esfm
