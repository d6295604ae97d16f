// Dense reconstruction kernels (include/esfm.h, "Dense reconstruction"): the fronto-parallel plane sweep with windowed NCC and
// the geometric-consistency fusion of depth maps.  Every f32 operation follows the header's text in its stated order; the
// Makefile's -ffp-contract=off keeps mul + add unfused, and HIP's default division and sqrtf are correctly rounded.
// tests/mvs_ref.py restates both and the output is compared bit for bit.
#include <cmath>

#include "block_scan.hpp"
#include "mvs_kernels.hpp"

namespace esfm {

// ---- plane sweep ---------------------------------------------------------------------------------------------------------
// One workgroup = 16 x 16 output pixels of one reference view, one thread per pixel.  The reference halo tile and its window
// statistics (mean, variance) are computed once.  For every plane, the (16 + 2r)^2 warped values of every source go to LDS (a
// pixel's warped value is shared by all windows that contain it), then each thread scores its window against each source,
// keeps the best_k smallest costs in a sorted register list, and updates its running winner with the costs at k* - 1 and
// k* + 1.  No cost volume leaves the workgroup.
template <int R>
__global__ __launch_bounds__(256) void mvs_sweep_kernel(MvsSweepArgs a)
{
    constexpr int W = kMvsTile + 2 * R;              // halo tile side
    constexpr int N = (2 * R + 1) * (2 * R + 1);     // taps per window
    constexpr int S = kMvsLdsStride;
    __shared__ float ref_t[W * S];
    extern __shared__ float src_lds[];               // a.max_src tiles of W x S: sized by the sources the views have, not by kMvsMaxNb

    const int view = blockIdx.y;
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int tx0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * kMvsTile, ty0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * kMvsTile;
    const int x = tx0 + lx, y = ty0 + ly, rows = a.rows, cols = a.cols, D = a.D;
    const size_t plane = (size_t)rows * cols;
    const bool in_img = x < cols && y < rows;
    const size_t out = (size_t)view * plane + (size_t)y * cols + x;
    const MvsView *V = a.views + view;
    if (!V->active) {                                // (uniform over the workgroup)
        if (in_img) { a.depth[out] = 0.f; a.cost[out] = INFINITY; }
        return;
    }
    const int n_src = V->n_src;

    // reference halo (positions outside the image only feed windows that leave it)
    const uint8_t *g_ref = a.gray + (size_t)view * plane;
    for (int i = tid; i < W * W; i += 256) {
        const int hy = i / W, hx = i - hy * W, gx = tx0 - R + hx, gy = ty0 - R + hy;
        ref_t[hy * S + hx] = (gx >= 0 && gy >= 0 && gx < cols && gy < rows) ? (float)g_ref[(size_t)gy * cols + gx] : 0.f;
    }
    __syncthreads();
    const bool win_ok = in_img && x >= R && y >= R && x + R < cols && y + R < rows;
    float mr = 0.f, vr = 0.f;
    {
        float s = 0.f;
#pragma unroll
        for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
            for (int dx = 0; dx <= 2 * R; ++dx) s += ref_t[(ly + dy) * S + lx + dx];
        mr = s / (float)N;
#pragma unroll
        for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
            for (int dx = 0; dx <= 2 * R; ++dx) { const float d = ref_t[(ly + dy) * S + lx + dx] - mr; vr += d * d; }
    }
    const bool ref_ok = win_ok && !(vr < a.min_var_n);   // vr < n min_var invalidates every source

    float best = INFINITY, c_prev = INFINITY, c_lo = INFINITY, c_hi = INFINITY;
    int best_k = -1;
    for (int k = 0; k < D; ++k) {
        __syncthreads();                             // the previous plane's readers are done with the source tiles
        for (int si = 0; si < n_src; ++si) {
            const float *h = a.H + V->h_off + ((size_t)si * D + k) * 9;
            const float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7], h8 = h[8];
            const uint8_t *g = a.gray + (size_t)V->src[si] * plane;
            float *dst = src_lds + si * (W * S);
            for (int i = tid; i < W * W; i += 256) {
                const int hy = i / W, hx = i - hy * W;
                const float px = (float)(tx0 - R + hx), py = (float)(ty0 - R + hy);
                const float w = (h6 * px + h7 * py) + h8;
                const float nu = (h0 * px + h1 * py) + h2;
                const float nv = (h3 * px + h4 * py) + h5;
                float val = -1.f;                    // invalid sample (valid values are >= 0)
                if (w > 0.f) {
                    const float u = nu / w, v = nv / w;
                    const float x0 = floorf(u), y0 = floorf(v);
                    if (x0 >= 0.f && x0 + 1.f < (float)cols && y0 >= 0.f && y0 + 1.f < (float)rows) {
                        const float fx = u - x0, fy = v - y0;
                        const uint8_t *p = g + (size_t)(int)y0 * cols + (int)x0;
                        const float i00 = (float)p[0], i01 = (float)p[1], i10 = (float)p[cols], i11 = (float)p[cols + 1];
                        val = (1.f - fy) * ((1.f - fx) * i00 + fx * i01) + fy * ((1.f - fx) * i10 + fx * i11);
                    }
                }
                dst[hy * S + hx] = val;
            }
        }
        __syncthreads();
        float top[kMvsMaxNb];                        // the smallest valid costs, ascending
#pragma unroll
        for (int j = 0; j < kMvsMaxNb; ++j) top[j] = INFINITY;
        int n_valid = 0;
        if (ref_ok) {
            for (int si = 0; si < n_src; ++si) {
                const float *t = src_lds + si * (W * S);
                float s = 0.f;
                bool bad = false;
#pragma unroll
                for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
                    for (int dx = 0; dx <= 2 * R; ++dx) { const float v = t[(ly + dy) * S + lx + dx]; bad |= v < 0.f; s += v; }
                if (bad) continue;
                const float ms = s / (float)N;
                float cov = 0.f, vs = 0.f;
#pragma unroll
                for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
                    for (int dx = 0; dx <= 2 * R; ++dx) {
                        const int o = (ly + dy) * S + lx + dx;
                        const float dr = ref_t[o] - mr, ds = t[o] - ms;
                        cov += dr * ds;
                        vs += ds * ds;
                    }
                if (vs < a.min_var_n) continue;
                float c = 1.f - cov / sqrtf(vr * vs);
#pragma unroll
                for (int j = 0; j < kMvsMaxNb; ++j) { const float lo = fminf(top[j], c); c = fmaxf(top[j], c); top[j] = lo; }
                ++n_valid;
            }
        }
        float ck = INFINITY;
        if (n_valid > 0) {
            const int m = n_valid < a.best_k ? n_valid : a.best_k;
            float sum = top[0];
#pragma unroll
            for (int j = 1; j < kMvsMaxNb; ++j) if (j < m) sum += top[j];
            ck = sum / (float)m;
        }
        if (best_k >= 0 && best_k == k - 1) c_hi = ck;
        if (ck < best) { best = ck; best_k = k; c_lo = c_prev; c_hi = INFINITY; }
        c_prev = ck;
    }
    if (!in_img) return;
    float depth = 0.f;
    if (best_k > 0 && best_k < D - 1 && !(best > a.max_cost)) {
        float off = 0.f;
        if (c_lo != INFINITY && c_hi != INFINITY) {
            const float den = (c_lo - 2.f * best) + c_hi;
            if (den > 0.f) off = fminf(fmaxf(0.5f * (c_lo - c_hi) / den, -0.5f), 0.5f);
        }
        depth = 1.f / (a.invd[V->invd_off + best_k] + off * V->step);
    }
    a.depth[out] = depth;
    a.cost[out] = best;
}

// ---- fusion --------------------------------------------------------------------------------------------------------------
__device__ inline void mvs_backproject(const MvsCam &c, float x, float y, float d, float X[3])
{
    const float e0 = ((x - c.K[1]) / c.K[0]) * d - c.P[3];
    const float e1 = ((y - c.K[3]) / c.K[2]) * d - c.P[7];
    const float e2 = d - c.P[11];
#pragma unroll
    for (int j = 0; j < 3; ++j) X[j] = (c.P[j] * e0 + c.P[4 + j] * e1) + c.P[8 + j] * e2;
}

__device__ inline void mvs_to_camera(const MvsCam &c, const float X[3], float p[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = ((c.P[4 * i] * X[0] + c.P[4 * i + 1] * X[1]) + c.P[4 * i + 2] * X[2]) + c.P[4 * i + 3];
}

// One thread per (view, pixel): the consistency test against every neighbour, the fused point and its colour in a per-pixel
// slot, and the keep flag; every 256-pixel block counts its kept pixels for the ordered compaction.
__global__ __launch_bounds__(256) void mvs_fuse_kernel(MvsFuseArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (idx < a.n_px) {
        const int64_t plane = (int64_t)a.rows * a.cols;
        const int view = (int)(idx / plane);
        const int64_t pix = idx - (int64_t)view * plane;
        const int y = (int)(pix / a.cols), x = (int)(pix - (int64_t)y * a.cols);
        const float d = a.depth[idx];
        if (d > 0.f) {
            const MvsCam &c = a.cams[view];
            const float fx = (float)x, fy = (float)y;
            float X[3], sum[3];
            mvs_backproject(c, fx, fy, d, X);
            sum[0] = X[0]; sum[1] = X[1]; sum[2] = X[2];
            int count = 0;
            for (int j = 0; j < a.n_nb; ++j) {
                const int s = c.nb[j];
                if (s < 0) continue;
                const MvsCam &cs = a.cams[s];
                float p[3];
                mvs_to_camera(cs, X, p);
                if (!(p[2] > 0.f)) continue;
                const float u = cs.K[0] * (p[0] / p[2]) + cs.K[1], v = cs.K[2] * (p[1] / p[2]) + cs.K[3];
                const float px = floorf(u + 0.5f), py = floorf(v + 0.5f);
                if (!(px >= 0.f && px < (float)a.cols && py >= 0.f && py < (float)a.rows)) continue;
                const float ds = a.depth[(int64_t)s * plane + (int64_t)(int)py * a.cols + (int)px];
                if (!(ds > 0.f)) continue;
                float Y[3], q[3];
                mvs_backproject(cs, px, py, ds, Y);
                mvs_to_camera(c, Y, q);
                const float du = (c.K[0] * (q[0] / q[2]) + c.K[1]) - fx, dv = (c.K[2] * (q[1] / q[2]) + c.K[3]) - fy;
                if (du * du + dv * dv < a.reproj2 && fabsf(q[2] - d) < a.rel_depth * d) {
                    sum[0] += Y[0]; sum[1] += Y[1]; sum[2] += Y[2];
                    ++count;
                }
            }
            if (count >= a.min_views) {
                keep = true;
                const float n = (float)(1 + count);
                a.stage_xyz[3 * idx] = sum[0] / n; a.stage_xyz[3 * idx + 1] = sum[1] / n; a.stage_xyz[3 * idx + 2] = sum[2] / n;
                const uint8_t *px = a.images + idx * a.channels;
                uint8_t *o = a.stage_rgb + 3 * idx;
                if (a.channels == 3) { o[0] = px[2]; o[1] = px[1]; o[2] = px[0]; }
                else { o[0] = px[0]; o[1] = px[0]; o[2] = px[0]; }
            }
        }
        a.keep[idx] = keep ? 1 : 0;
    }
    const int n = __syncthreads_count(keep);
    if (threadIdx.x == 0) a.block_count[blockIdx.x] = n;
}

// The ordered write: a kept pixel goes to its block's offset plus the kept pixels before it in the block.
__global__ __launch_bounds__(256) void mvs_fuse_write_kernel(MvsFuseArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool k = idx < a.n_px && a.keep[idx];
    const int incl = block_inclusive_count(k);
    if (!k) return;
    const int64_t dst = (int64_t)a.block_count[blockIdx.x] + incl - 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.xyz[3 * dst + c] = a.stage_xyz[3 * idx + c]; a.rgb[3 * dst + c] = a.stage_rgb[3 * idx + c]; }
    if (a.pixel_index) a.pixel_index[dst] = (int32_t)idx;      // (n_px < 2^31: check_views)
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
int launch_mvs_sweep(hipStream_t st, const MvsSweepArgs &a, int radius, int n_views)
{
    const int tiles_y = (a.rows + kMvsTile - 1) / kMvsTile;
    const dim3 grid((unsigned)(a.tiles_x * tiles_y), (unsigned)n_views);
    if (a.max_src < 0 || a.max_src > kMvsMaxNb) { set_error("%d sources per view", a.max_src); return ESFM_ERR_INVALID_ARG; }
    const size_t lds = sizeof(float) * (size_t)a.max_src * (kMvsTile + 2 * radius) * kMvsLdsStride;   // the source tiles
    switch (radius) {
    case 1: hipLaunchKernelGGL(mvs_sweep_kernel<1>, grid, dim3(256), lds, st, a); break;
    case 2: hipLaunchKernelGGL(mvs_sweep_kernel<2>, grid, dim3(256), lds, st, a); break;
    case 3: hipLaunchKernelGGL(mvs_sweep_kernel<3>, grid, dim3(256), lds, st, a); break;
    case 4: hipLaunchKernelGGL(mvs_sweep_kernel<4>, grid, dim3(256), lds, st, a); break;
    case 5: hipLaunchKernelGGL(mvs_sweep_kernel<5>, grid, dim3(256), lds, st, a); break;
    case 6: hipLaunchKernelGGL(mvs_sweep_kernel<6>, grid, dim3(256), lds, st, a); break;
    case 7: hipLaunchKernelGGL(mvs_sweep_kernel<7>, grid, dim3(256), lds, st, a); break;
    default: set_error("window radius %d is outside 1..7", radius); return ESFM_ERR_INVALID_ARG;
    }
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_mvs_fuse(hipStream_t st, const MvsFuseArgs &a)
{
    const int n_blocks = (int)((a.n_px + 255) / 256);
    hipLaunchKernelGGL(mvs_fuse_kernel, dim3((unsigned)n_blocks), dim3(256), 0, st, a);
    LAUNCH_OK();
    if (int rc = launch_block_offsets_scan(st, a.block_count, n_blocks, a.n_points)) return rc;
    hipLaunchKernelGGL(mvs_fuse_write_kernel, dim3((unsigned)n_blocks), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
