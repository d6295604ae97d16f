// Kernels of the mesh texturing (include/esfm.h, "Mesh texturing"): the projection of every vertex into every view, the
// rasterisation of every (view, triangle) pair into the view's buffer of inverse depths, the per-triangle view choice and the
// per-texel bake.  The only combination across threads is atomicMax on a uint32 (a positive f32 orders like its bit pattern), so
// the buffers do not depend on the order in which the pairs arrive; the list of large boxes is filled in arrival order, which the
// maximum does not see.  Every f32 expression is the header's, in its order (the build has no mul + add contraction).
#include "block_scan.hpp"         // blocks_of, LAUNCH_OK
#include "texture_device.hpp"     // texture_project, texture_taps, texture_fetch

namespace esfm {

__global__ __launch_bounds__(256) void texture_project_kernel(TextureViewsArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)a.n * a.V) return;
    const int v = (int)(k / a.V);
    const int64_t i = k % a.V;
    float u, w, p2;
    const bool front = texture_project(a.cams[v], a.vertices[3 * i], a.vertices[3 * i + 1], a.vertices[3 * i + 2], u, w, p2);
    a.proj[k] = front ? make_float4(u, w, 1.0f / p2, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The screen triangle of one (view, triangle) pair and its box.
struct TextureTri {
    float x[3], y[3], z[3], area2;
    int bx0, bx1, by0, by1;   // an empty box has bx1 < bx0 or by1 < by0
    bool exists;              // all three vertices in front
};

__device__ inline TextureTri texture_screen(const TextureViewsArgs &a, int v, int64_t t)
{
    TextureTri s;
    s.exists = true;
    for (int k = 0; k < 3; ++k) {
        const float4 p = a.proj[(int64_t)v * a.V + a.tri[3 * t + k]];
        s.x[k] = p.x; s.y[k] = p.y; s.z[k] = p.z;
        s.exists = s.exists && p.w != 0.f;
    }
    s.area2 = (s.x[1] - s.x[0]) * (s.y[2] - s.y[0]) - (s.y[1] - s.y[0]) * (s.x[2] - s.x[0]);
    s.bx0 = (int)fmaxf(ceilf(fminf(fminf(s.x[0], s.x[1]), s.x[2]) - 0.5f), 0.f);
    s.bx1 = (int)fminf(floorf(fmaxf(fmaxf(s.x[0], s.x[1]), s.x[2]) + 0.5f), (float)(a.cols - 1));
    s.by0 = (int)fmaxf(ceilf(fminf(fminf(s.y[0], s.y[1]), s.y[2]) - 0.5f), 0.f);
    s.by1 = (int)fminf(floorf(fmaxf(fmaxf(s.y[0], s.y[1]), s.y[2]) + 0.5f), (float)(a.rows - 1));
    return s;
}

// One pixel of the pair's box, 0 <= px < cols and 0 <= py < rows: the coverage test and the maximum.
__device__ inline void texture_pixel(const TextureTri &s, uint32_t *buffer, int cols, int px, int py)
{
    const float fx = (float)px, fy = (float)py, sign = s.area2 > 0.f ? 1.f : -1.f;
    float e[3];
    bool inside = true;
    for (int k = 0; k < 3; ++k) {
        const int k1 = k == 2 ? 0 : k + 1;
        const float ex = s.x[k1] - s.x[k], ey = s.y[k1] - s.y[k];
        e[k] = ex * (fy - s.y[k]) - ey * (fx - s.x[k]);
        inside = inside && sign * e[k] >= -0.5f * (fabsf(ex) + fabsf(ey));
    }
    if (!inside) return;
    const float b0 = e[1] / s.area2, b1 = e[2] / s.area2, b2 = e[0] / s.area2;
    float z = (b0 * s.z[0] + b1 * s.z[1]) + b2 * s.z[2];
    z = fminf(fmaxf(z, fminf(fminf(s.z[0], s.z[1]), s.z[2])), fmaxf(fmaxf(s.z[0], s.z[1]), s.z[2]));
    atomicMax(buffer + (int64_t)py * cols + px, __float_as_uint(z));
}

// A lane per pair: a box of at most kTextureSmallBox pixels is walked here, a larger one is listed for the wave-per-pair kernel.
__global__ __launch_bounds__(256) void texture_raster_small_kernel(TextureViewsArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)a.n * a.T) return;
    const int v = (int)(k / a.T);
    const TextureTri s = texture_screen(a, v, k % a.T);
    if (!s.exists || s.area2 == 0.f || s.bx1 < s.bx0 || s.by1 < s.by0) return;
    const int bw = s.bx1 - s.bx0 + 1, bh = s.by1 - s.by0 + 1;
    if ((int64_t)bw * bh > kTextureSmallBox) {
        a.list[atomicAdd(a.count, 1u)] = (uint32_t)k;      // (at most n T entries: one per pair)
        return;
    }
    uint32_t *buffer = a.buffers + (int64_t)v * a.rows * a.cols;
    for (int py = s.by0; py <= s.by1; ++py)
        for (int px = s.bx0; px <= s.bx1; ++px) texture_pixel(s, buffer, a.cols, px, py);
}

// A wave per listed pair, its 64 lanes striding over the box's pixels in row-major order.
__global__ __launch_bounds__(256) void texture_raster_large_kernel(TextureViewsArgs a)
{
    const uint32_t waves = gridDim.x * 4u, lane = threadIdx.x & 63u, listed = *a.count;
    for (uint32_t entry = blockIdx.x * 4u + (threadIdx.x >> 6); entry < listed; entry += waves) {
        const int64_t k = a.list[entry];
        const int v = (int)(k / a.T);
        const TextureTri s = texture_screen(a, v, k % a.T);
        const int bw = s.bx1 - s.bx0 + 1;
        const int64_t pixels = (int64_t)bw * (s.by1 - s.by0 + 1);
        uint32_t *buffer = a.buffers + (int64_t)v * a.rows * a.cols;
        for (int64_t i = lane; i < pixels; i += 64) texture_pixel(s, buffer, a.cols, s.bx0 + (int)(i % bw), s.by0 + (int)(i / bw));
    }
}

// true if the point's nearest pixel lies in the image and the buffer there does not hold something nearer
__device__ inline bool texture_visible(const uint32_t *buffer, int rows, int cols, float u, float w, float z, float keep)
{
    const float px = floorf(u + 0.5f), py = floorf(w + 0.5f);
    if (!(px >= 0.f && px < (float)cols && py >= 0.f && py < (float)rows)) return false;
    return z >= __uint_as_float(buffer[(int64_t)(int)py * cols + (int)px]) * keep;
}

__global__ __launch_bounds__(256) void texture_choose_kernel(TextureViewsArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    float P[3][3];
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) P[k][c] = a.vertices[3 * (int64_t)a.tri[3 * t + k] + c];
    const float e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    const float N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float lN = sqrtf((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
    float G[3];
    for (int c = 0; c < 3; ++c) G[c] = ((P[0][c] + P[1][c]) + P[2][c]) / 3.0f;
    float best = 0.f;
    int label = -1;
    for (int v = 0; v < a.n; ++v) {
        const TextureTri s = texture_screen(a, v, t);
        const float score = 0.5f * fabsf(s.area2);
        bool ok = s.exists && score > 0.f;
        for (int k = 0; k < 3; ++k)
            ok = ok && s.x[k] >= 1.f && s.x[k] <= (float)(a.cols - 2) && s.y[k] >= 1.f && s.y[k] <= (float)(a.rows - 2);
        if (!ok) continue;
        const TextureCam &c = a.cams[v];
        float D[3];
        for (int j = 0; j < 3; ++j) D[j] = -((c.P[j] * c.P[3] + c.P[4 + j] * c.P[7]) + c.P[8 + j] * c.P[11]) - G[j];
        const float d = (N[0] * D[0] + N[1] * D[1]) + N[2] * D[2], lD = sqrtf((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
        if (!(d > 0.f && d >= a.min_cos * (lN * lD))) continue;
        float gu, gw, gp2;
        if (!texture_project(c, G[0], G[1], G[2], gu, gw, gp2)) continue;
        const uint32_t *buffer = a.buffers + (int64_t)v * a.rows * a.cols;
        ok = texture_visible(buffer, a.rows, a.cols, gu, gw, 1.0f / gp2, a.keep);
        for (int k = 0; k < 3; ++k) ok = ok && texture_visible(buffer, a.rows, a.cols, s.x[k], s.y[k], s.z[k], a.keep);
        if (ok && score > best) { best = score; label = v; }
    }
    a.label[t] = label;
    a.score[t] = best;
}

// One thread per texel, numbered square by square (S S consecutive threads fill one square), so a wave covers whole squares or whole
// rows of one: its image reads stay inside the two triangles' footprints instead of running along an atlas row over many charts.
// kOffsets: the levelled bake of esfm_mesh_texture_bake_ex, a variant of its own so that the plain one keeps its code.
template <bool kOffsets>
__global__ __launch_bounds__(256) void texture_bake_kernel(TextureBakeArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int W = a.A * a.S, SS = a.S * a.S;
    if (k >= (int64_t)a.H * W) return;
    const int64_t q = k / SS;
    const int r = (int)(k % SS), j = r / a.S, i = r % a.S;
    const bool odd = i + j > a.S - 1;
    const int64_t t = 2 * q + (odd ? 1 : 0);
    uint8_t *out = a.atlas + 3 * (((q / a.A) * a.S + j) * W + (q % a.A) * a.S + i);
    if (t >= a.T) { out[0] = 0; out[1] = 0; out[2] = 0; return; }
    const float b1 = odd ? (float)(a.S - 1 - i) / (float)(a.S - 3) : (float)i / (float)(a.S - 2);
    const float b2 = odd ? (float)(a.S - 1 - j) / (float)(a.S - 3) : (float)j / (float)(a.S - 2);
    const float b0 = (1.0f - b1) - b2;
    const int32_t i0 = a.tri[3 * t], i1 = a.tri[3 * t + 1], i2 = a.tri[3 * t + 2];
    const int label = a.label[t];
    if (label >= 0) {
        float X[3];
        for (int c = 0; c < 3; ++c) X[c] = (b0 * a.vertices[3 * (int64_t)i0 + c] + b1 * a.vertices[3 * (int64_t)i1 + c]) + b2 * a.vertices[3 * (int64_t)i2 + c];
        float u, w, p2;
        texture_project(a.cams[label], X[0], X[1], X[2], u, w, p2);
        if (p2 > 0.f) {
            const TextureTaps taps = texture_taps(a.images, label, a.rows, a.cols, a.channels, u, w);
            for (int c = 0; c < 3; ++c) {
                float v = texture_fetch(taps, a.channels == 3 ? 2 - c : 0);
                if constexpr (kOffsets) {
                    const float *o = a.offsets + 9 * t + c;          // the three corners' offsets of this channel
                    v = v + ((b0 * o[0] + b1 * o[3]) + b2 * o[6]);
                    v = fminf(fmaxf(v, 0.0f), 255.0f);
                }
                out[c] = (uint8_t)floorf(v + 0.5f);
            }
            return;
        }
    }
    for (int c = 0; c < 3; ++c) {
        float v = 128.f;
        if (a.rgb) {
            v = (b0 * (float)a.rgb[3 * (int64_t)i0 + c] + b1 * (float)a.rgb[3 * (int64_t)i1 + c]) + b2 * (float)a.rgb[3 * (int64_t)i2 + c];
            v = floorf(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f);
        }
        out[c] = (uint8_t)v;
    }
}

int launch_texture_project(hipStream_t st, const TextureViewsArgs &a)
{
    hipLaunchKernelGGL(texture_project_kernel, dim3(blocks_of((int64_t)a.n * a.V)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_texture_rasterise(hipStream_t st, const TextureViewsArgs &a)
{
    const int64_t pairs = (int64_t)a.n * a.T;
    hipLaunchKernelGGL(texture_raster_small_kernel, dim3(blocks_of(pairs)), dim3(256), 0, st, a);
    LAUNCH_OK();
    // the number of listed pairs stays on the device: a fixed grid of at most 1024 workgroups (4096 waves) strides over the list
    const int64_t groups = (pairs + 3) / 4;
    hipLaunchKernelGGL(texture_raster_large_kernel, dim3((unsigned)(groups < 1024 ? groups : 1024)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_texture_choose(hipStream_t st, const TextureViewsArgs &a)
{
    hipLaunchKernelGGL(texture_choose_kernel, dim3(blocks_of(a.T)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_texture_bake(hipStream_t st, const TextureBakeArgs &a)
{
    if (a.offsets) hipLaunchKernelGGL(texture_bake_kernel<true>, dim3(blocks_of((int64_t)a.H * a.A * a.S)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(texture_bake_kernel<false>, dim3(blocks_of((int64_t)a.H * a.A * a.S)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
