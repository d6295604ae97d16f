// Kernels of the mesh rendering (include/esfm.h, "Mesh rendering"): the projection of every vertex into every view as a screen
// vertex in 1/256-pixel fixed point, the rasterisation of every (view, triangle) pair into the view's buffer of 64-bit keys
// (inverse depth above, triangle below) and the per-pixel shading from the winning key.  Coverage is exact int64 arithmetic with
// a top-left style ownership rule, so two triangles that share an edge cover each pixel on it exactly once.  The only combination
// across threads is atomicMax on an unsigned 64-bit key, so the buffers do not depend on the order in which the pairs arrive; the
// list of large boxes is filled in arrival order, which the maximum does not see.  Every f32 expression is the header's, in its
// order (the build has no mul + add contraction).
#include "block_scan.hpp"         // blocks_of, LAUNCH_OK
#include "render_kernels.hpp"
#include "texture_device.hpp"     // texture_project, texture_taps, texture_fetch

namespace esfm {

__global__ __launch_bounds__(256) void render_project_kernel(RenderArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)a.n * a.V) return;
    const int v = (int)(k / a.V);
    const int64_t i = k % a.V;
    float u, w, p2;
    const bool front = texture_project(a.cams[v], a.vertices[3 * i], a.vertices[3 * i + 1], a.vertices[3 * i + 2], u, w, p2);
    // |u|, |w| <= 2^20 in front: the products are exact and below 2^28
    a.proj[k] = front ? make_int4((int32_t)rintf(u * 256.0f), (int32_t)rintf(w * 256.0f), (int32_t)__float_as_uint(1.0f / p2), 1) : make_int4(0, 0, 0, 0);
}

// The screen triangle of one (view, triangle) pair and its box.
struct RenderTri {
    int32_t sx[3], sy[3];
    float z[3];
    int64_t area2;
    int bx0, bx1, by0, by1;   // an empty box has bx1 < bx0 or by1 < by0
    bool exists;              // all three vertices in front
};

__device__ inline RenderTri render_screen(const RenderArgs &a, int v, int64_t t)
{
    RenderTri s;
    s.exists = true;
    for (int k = 0; k < 3; ++k) {
        const int4 p = a.proj[(int64_t)v * a.V + a.tri[3 * t + k]];
        s.sx[k] = p.x; s.sy[k] = p.y; s.z[k] = __uint_as_float((uint32_t)p.z);
        s.exists = s.exists && p.w != 0;
    }
    s.area2 = (int64_t)(s.sx[1] - s.sx[0]) * (s.sy[2] - s.sy[0]) - (int64_t)(s.sy[1] - s.sy[0]) * (s.sx[2] - s.sx[0]);
    // the integer pixels inside the fixed-point box: ceil(min / 256) .. floor(max / 256), by floor division
    s.bx0 = max((min(min(s.sx[0], s.sx[1]), s.sx[2]) + 255) >> 8, 0);
    s.bx1 = min(max(max(s.sx[0], s.sx[1]), s.sx[2]) >> 8, a.cols - 1);
    s.by0 = max((min(min(s.sy[0], s.sy[1]), s.sy[2]) + 255) >> 8, 0);
    s.by1 = min(max(max(s.sy[0], s.sy[1]), s.sy[2]) >> 8, a.rows - 1);
    return s;
}

// One pixel against a triangle with area2 != 0: true if covered, then q[k] = b_k z_k and iz = (q0 + q1) + q2.
__device__ inline bool render_cover(const RenderTri &s, int px, int py, float q[3], float &iz)
{
    const int64_t X = 256 * (int64_t)px, Y = 256 * (int64_t)py;
    const bool pos = s.area2 > 0;
    int64_t e[3];
    for (int k = 0; k < 3; ++k) {
        const int k1 = k == 2 ? 0 : k + 1;
        const int64_t dx = s.sx[k1] - s.sx[k], dy = s.sy[k1] - s.sy[k];
        e[k] = dx * (Y - s.sy[k]) - dy * (X - s.sx[k]);
        const int64_t se = pos ? e[k] : -e[k], sdx = pos ? dx : -dx, sdy = pos ? dy : -dy;
        const bool owns = sdy > 0 || (sdy == 0 && sdx < 0);
        if (!(se > 0 || (se == 0 && owns))) return false;
    }
    const float fa = (float)s.area2;
    const float b0 = (float)e[1] / fa, b1 = (float)e[2] / fa, b2 = (float)e[0] / fa;
    q[0] = b0 * s.z[0]; q[1] = b1 * s.z[1]; q[2] = b2 * s.z[2];
    iz = (q[0] + q[1]) + q[2];
    return true;
}

// One pixel of the pair's box, 0 <= px < cols and 0 <= py < rows: the coverage test and the maximum.
__device__ inline void render_pixel(const RenderTri &s, unsigned long long *keys, int cols, uint32_t t, int px, int py)
{
    float q[3], iz;
    if (!render_cover(s, px, py, q, iz)) return;
    const uint32_t bits = __float_as_uint(iz);
    if (bits == 0u) return;
    atomicMax(keys + (int64_t)py * cols + px, ((unsigned long long)bits << 32) | (0xFFFFFFFFu - t));
}

// A lane per pair: a box of at most kRenderSmallBox pixels is walked here, a larger one is listed for the wave-per-pair kernel.
__global__ __launch_bounds__(256) void render_raster_small_kernel(RenderArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)a.n * a.T) return;
    const int v = (int)(k / a.T);
    const int64_t t = k % a.T;
    const RenderTri s = render_screen(a, v, t);
    if (!s.exists || s.area2 == 0 || s.bx1 < s.bx0 || s.by1 < s.by0) return;
    const int bw = s.bx1 - s.bx0 + 1, bh = s.by1 - s.by0 + 1;
    if ((int64_t)bw * bh > kRenderSmallBox) {
        a.list[atomicAdd(a.count, 1u)] = (uint32_t)k;      // (at most n T entries: one per pair)
        return;
    }
    unsigned long long *keys = a.keys + (int64_t)v * a.rows * a.cols;
    for (int py = s.by0; py <= s.by1; ++py)
        for (int px = s.bx0; px <= s.bx1; ++px) render_pixel(s, keys, a.cols, (uint32_t)t, px, py);
}

// A wave per listed pair, its 64 lanes striding over the box's pixels in row-major order.
__global__ __launch_bounds__(256) void render_raster_large_kernel(RenderArgs a)
{
    const uint32_t waves = gridDim.x * 4u, lane = threadIdx.x & 63u, listed = *a.count;
    for (uint32_t entry = blockIdx.x * 4u + (threadIdx.x >> 6); entry < listed; entry += waves) {
        const int64_t k = a.list[entry];
        const int v = (int)(k / a.T);
        const int64_t t = k % a.T;
        const RenderTri s = render_screen(a, v, t);
        const int bw = s.bx1 - s.bx0 + 1, bh = s.by1 - s.by0 + 1;
        unsigned long long *keys = a.keys + (int64_t)v * a.rows * a.cols;
        // pixel lane, lane + 64, .. of the box: one division per pair, then (x, y) advances by 64 = step_y bw + step_x
        const int step_y = 64 / bw, step_x = 64 % bw;
        for (int x = (int)lane % bw, y = (int)lane / bw; y < bh; ) {
            render_pixel(s, keys, a.cols, (uint32_t)t, s.bx0 + x, s.by0 + y);
            x += step_x; y += step_y;
            if (x >= bw) { x -= bw; ++y; }
        }
    }
}

// One thread per pixel, consecutive threads along a row: the winning key's triangle is covered again for its q_k and iz.
__global__ __launch_bounds__(256) void render_shade_kernel(RenderArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x, per_view = (int64_t)a.rows * a.cols;
    if (k >= a.n * per_view) return;
    const unsigned long long key = a.keys[k];
    int32_t id = -1;
    float depth = 0.f;
    uint8_t c[3] = {a.background[0], a.background[1], a.background[2]};
    if (key != 0ull) {
        const int v = (int)(k / per_view);
        const int64_t r = k % per_view;
        const int64_t t = 0xFFFFFFFFu - (uint32_t)key;
        const RenderTri s = render_screen(a, v, t);
        float q[3], iz;
        render_cover(s, (int)(r % a.cols), (int)(r / a.cols), q, iz);
        id = (int32_t)t;
        depth = 1.0f / iz;
        if (a.out_rgb) {
            if (a.uv) {
                const float *g = a.uv + 6 * t;
                const float uu = ((q[0] * g[0] + q[1] * g[2]) + q[2] * g[4]) / iz, vv = ((q[0] * g[1] + q[1] * g[3]) + q[2] * g[5]) / iz;
                const TextureTaps taps = texture_taps(a.atlas, 0, a.H, a.W, 3, uu * (float)a.W - 0.5f, vv * (float)a.H - 0.5f);
                for (int ch = 0; ch < 3; ++ch) c[ch] = (uint8_t)floorf(texture_fetch(taps, ch) + 0.5f);
            } else if (a.rgb) {
                const uint8_t *c0 = a.rgb + 3 * (int64_t)a.tri[3 * t], *c1 = a.rgb + 3 * (int64_t)a.tri[3 * t + 1], *c2 = a.rgb + 3 * (int64_t)a.tri[3 * t + 2];
                for (int ch = 0; ch < 3; ++ch) {
                    const float x = ((q[0] * (float)c0[ch] + q[1] * (float)c1[ch]) + q[2] * (float)c2[ch]) / iz;
                    c[ch] = (uint8_t)floorf(fminf(fmaxf(x, 0.0f), 255.0f) + 0.5f);
                }
            } else {
                c[0] = c[1] = c[2] = 128;
            }
        }
    }
    if (a.out_rgb) { a.out_rgb[3 * k] = c[0]; a.out_rgb[3 * k + 1] = c[1]; a.out_rgb[3 * k + 2] = c[2]; }
    if (a.out_depth) a.out_depth[k] = depth;
    if (a.out_id) a.out_id[k] = id;
}

int launch_render_project(hipStream_t st, const RenderArgs &a)
{
    hipLaunchKernelGGL(render_project_kernel, dim3(blocks_of((int64_t)a.n * a.V)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_render_rasterise(hipStream_t st, const RenderArgs &a)
{
    const int64_t pairs = (int64_t)a.n * a.T;
    hipLaunchKernelGGL(render_raster_small_kernel, dim3(blocks_of(pairs)), dim3(256), 0, st, a);
    LAUNCH_OK();
    // the number of listed pairs stays on the device: a fixed grid of at most 1024 workgroups (4096 waves) strides over the list
    const int64_t groups = (pairs + 3) / 4;
    hipLaunchKernelGGL(render_raster_large_kernel, dim3((unsigned)(groups < 1024 ? groups : 1024)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_render_shade(hipStream_t st, const RenderArgs &a)
{
    hipLaunchKernelGGL(render_shade_kernel, dim3(blocks_of((int64_t)a.n * a.rows * a.cols)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
