// Per-pixel world normals from depth maps (include/esfm.h, "Dense-cloud merge", esfm_mvs_normals): a least-squares fit of the
// linear function a plane is in inverse depth over pixel coordinates.  Every operation follows the header's text in its stated
// order and grouping (-ffp-contract=off; HIP's default f32 / f64 division and f64 sqrt are correctly rounded);
// tests/merge_ref.py restates it and the output is compared bit for bit.
#include <cmath>

#include "mvs_kernels.hpp"

namespace esfm {

// One workgroup = 16 x 16 pixels of one view, one thread per pixel.  The halo tile holds wt = 1.0f / dt of every pixel the
// windows touch (one division per pixel, not per tap); -1 marks a tap that cannot count (outside the image, or no depth).
__global__ __launch_bounds__(256) void mvs_normals_kernel(MvsNormalArgs a)
{
    constexpr int S = kMvsLdsStride;
    __shared__ float w_t[(kMvsTile + 2 * kMvsMaxRadius) * S];

    const int view = blockIdx.y, m = a.radius, W = kMvsTile + 2 * m;
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int tx0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * kMvsTile, ty0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * kMvsTile;
    const int x = tx0 + lx, y = ty0 + ly, rows = a.rows, cols = a.cols;
    const size_t plane = (size_t)rows * cols;
    const float *g_d = a.depth + (size_t)view * plane;
    for (int i = tid; i < W * W; i += 256) {
        const int hy = i / W, hx = i - hy * W, gx = tx0 - m + hx, gy = ty0 - m + hy;
        float wt = -1.f;
        if (gx >= 0 && gy >= 0 && gx < cols && gy < rows) {
            const float dt = g_d[(size_t)gy * cols + gx];
            if (dt > 0.f) wt = 1.0f / dt;
        }
        w_t[hy * S + hx] = wt;
    }
    __syncthreads();
    if (x >= cols || y >= rows) return;

    float N[3] = {0.f, 0.f, 0.f};
    const float wc = w_t[(ly + m) * S + lx + m];
    if (wc >= 0.f) {
        const float tol = a.rel_step * wc;
        double S1 = 0, Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0, Sw = 0, Sxw = 0, Syw = 0;
        for (int dy = -m; dy <= m; ++dy)
            for (int dx = -m; dx <= m; ++dx) {
                const float wt = w_t[(ly + m + dy) * S + lx + m + dx];
                if (!(wt >= 0.f && fabsf(wt - wc) <= tol)) continue;
                const double fx = (double)dx, fy = (double)dy, w = (double)wt;
                S1 += 1.0; Sx += fx; Sy += fy; Sxx += fx * fx; Sxy += fx * fy; Syy += fy * fy;
                Sw += w; Sxw += fx * w; Syw += fy * w;
            }
        if (!(S1 < (double)a.min_taps)) {
            const double c00 = Syy * S1 - Sy * Sy, c01 = Sxy * S1 - Sy * Sx, c02 = Sxy * Sy - Syy * Sx;
            const double det = (Sxx * c00 - Sxy * c01) + Sx * c02;
            const double da = (Sxw * c00 - Sxy * (Syw * S1 - Sy * Sw)) + Sx * (Syw * Sy - Syy * Sw);
            const double db = (Sxx * (Syw * S1 - Sw * Sy) - Sxw * c01) + Sx * (Sxy * Sw - Syw * Sx);
            const double dg = (Sxx * (Syy * Sw - Sy * Syw) - Sxy * (Sxy * Sw - Sx * Syw)) + Sxw * c02;
            if (det > 0.0) {
                const MvsCam &c = a.cams[view];
                const double ca = da / det, cb = db / det, cg = dg / det;
                const double n0 = ca * (double)c.K[0], n1 = cb * (double)c.K[2];
                const double n2 = (cg + ca * ((double)c.K[1] - (double)x)) + cb * ((double)c.K[3] - (double)y);
                const double L = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
                if (L > 0.0 && L < (double)INFINITY) {
                    const double u0 = -n0 / L, u1 = -n1 / L, u2 = -n2 / L;
#pragma unroll
                    for (int j = 0; j < 3; ++j) N[j] = (float)(((double)c.P[j] * u0 + (double)c.P[4 + j] * u1) + (double)c.P[8 + j] * u2);
                }
            }
        }
    }
    float *o = a.normals + 3 * ((size_t)view * plane + (size_t)y * cols + x);
    o[0] = N[0]; o[1] = N[1]; o[2] = N[2];
}

int launch_mvs_normals(hipStream_t st, const MvsNormalArgs &a, int n_views)
{
    if (a.radius < 1 || a.radius > kMvsMaxRadius) { set_error("normal radius %d is outside 1..7", a.radius); return ESFM_ERR_INVALID_ARG; }
    const int tiles_y = (a.rows + kMvsTile - 1) / kMvsTile;
    hipLaunchKernelGGL(mvs_normals_kernel, dim3((unsigned)(a.tiles_x * tiles_y), (unsigned)n_views), dim3(256), 0, st, a);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

}  // namespace esfm
