// SIFT detector + 128-float descriptor for gfx950 (MI355X): the device side of esfm_sift_detect_and_compute, the
// replacement for cv::xfeatures2d::SIFT_create(nfeatures)->detectAndCompute (the Python prototype's SIFT branch).  The
// arithmetic follows tests/sift_ref/sift_ref.c, which writes the rules down operation by operation: every float expression
// keeps its order (no FMA contraction), every histogram bin is summed by one lane in sample order, exp / exp2 / sin / cos
// are the written-out routines below (same constants as sift_ref.c), and atan2 is cv::fastAtan2 (feature_math.hpp), so the
// result is bit-identical to the CPU restatement.
//
//   sift_upsample_kernel     gray bytes -> x2 INTER_LINEAR float base image
//   sift_blur_rows_kernel    horizontal Gaussian pass (taps summed in order, iterative BORDER_REFLECT_101)
//   sift_blur_cols_kernel    vertical pass in the symmetric form, and the DoG layer against the previous Gaussian layer
//   sift_downsample_kernel   every second pixel of layer 3 starts the next octave
//   sift_extrema_kernel      26-neighbour extremum test + adjustLocalExtrema, one thread per DoG sample of layers 1..3
//   sift_orient_kernel       one wave per candidate: 36-bin orientation histogram (lane = bin), smoothing, peaks
//   sift_describe_kernel     one workgroup per keypoint: samples staged in LDS in order, lane = bin of the 6 x 6 x 10 histogram
#include "sift_kernels.hpp"
#include "feature_math.hpp"

#include <float.h>
#include <math.h>

#include <algorithm>

namespace esfm {

// ---- the written-out math routines (identical in sift_ref.c)
__device__ __forceinline__ double sift_exp_core(double r)
{
    double p = 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p;
}

__device__ __forceinline__ float sift_exp(float x)
{
    const double xd = x;
    const double n = rint(xd * 1.4426950408889634);
    const double r = xd - n * 0.6931471805599453;
    return (float)(sift_exp_core(r) * ldexp(1.0, (int)n));
}

__device__ __forceinline__ float sift_exp2(float x)
{
    const double xd = x;
    const double n = rint(xd);
    const double r = (xd - n) * 0.6931471805599453;
    return (float)(sift_exp_core(r) * ldexp(1.0, (int)n));
}

__device__ __forceinline__ double sift_sin_core(double r)
{
    const double z = r * r;
    double p = -1.0 / 1307674368000.0;
    p = p * z + 1.0 / 6227020800.0;
    p = p * z - 1.0 / 39916800.0;
    p = p * z + 1.0 / 362880.0;
    p = p * z - 1.0 / 5040.0;
    p = p * z + 1.0 / 120.0;
    p = p * z - 1.0 / 6.0;
    p = p * z;
    return r + r * p;
}

__device__ __forceinline__ double sift_cos_core(double r)
{
    const double z = r * r;
    double p = 1.0 / 20922789888000.0;
    p = p * z - 1.0 / 87178291200.0;
    p = p * z + 1.0 / 479001600.0;
    p = p * z - 1.0 / 3628800.0;
    p = p * z + 1.0 / 40320.0;
    p = p * z - 1.0 / 720.0;
    p = p * z + 1.0 / 24.0;
    p = p * z - 0.5;
    p = p * z;
    return 1.0 + p;
}

__device__ __forceinline__ double sift_quadrant(float x, int *q)
{
    const double xd = x;
    const double k = rint(xd * 0.6366197723675814);
    *q = ((int)k) & 3;
    return (xd - k * 1.5707963267948966) - k * 6.123233995736766e-17;
}

__device__ __forceinline__ float sift_sin(float x)
{
    int q;
    const double r = sift_quadrant(x, &q);
    const double v = (q & 1) ? sift_cos_core(r) : sift_sin_core(r);
    return (float)((q & 2) ? -v : v);
}

__device__ __forceinline__ float sift_cos(float x)
{
    int q;
    const double r = sift_quadrant(x, &q);
    const double v = (q & 1) ? sift_sin_core(r) : sift_cos_core(r);
    return (float)(((q + 1) & 2) ? -v : v);
}

// cv::borderInterpolate(p, len, BORDER_REFLECT_101), iterated for kernels wider than the image
__device__ __forceinline__ int border101(int p, int len)
{
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : len - 1 - (p - len) - 1;
    return p;
}

// ---- pyramid
__global__ __launch_bounds__(256) void sift_upsample_kernel(const uint8_t *__restrict__ gray, int rows, int cols, float *__restrict__ out)
{
    const int C2 = 2 * cols;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)2 * rows * C2) return;
    const int y = (int)(i / C2), x = (int)(i % C2);
    const int k = x >> 1, kx = (x & 1) ? (k + 1 < cols ? k + 1 : cols - 1) : (k > 0 ? k - 1 : 0);
    const int ky = y >> 1, kb = (y & 1) ? (ky + 1 < rows ? ky + 1 : rows - 1) : (ky > 0 ? ky - 1 : 0);
    float h[2];
    const int yy[2] = {ky, kb};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float a = gray[(size_t)yy[t] * cols + k], b = gray[(size_t)yy[t] * cols + kx];
        h[t] = (x & 1) ? a * 0.75f + b * 0.25f : b * 0.25f + a * 0.75f;
    }
    out[i] = (y & 1) ? h[0] * 0.75f + h[1] * 0.25f : h[1] * 0.25f + h[0] * 0.75f;
}

__global__ __launch_bounds__(256) void sift_blur_rows_kernel(const float *__restrict__ src, float *__restrict__ tmp, int rows, int cols, SiftTaps T)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= cols) return;
    const int r = T.n / 2;
    const float *row = src + (size_t)y * cols;
    float s = 0.f;
    if (x >= r && x + r < cols) {
        for (int k = 0; k < T.n; ++k) s += T.w[k] * row[x + k - r];
    } else {
        for (int k = 0; k < T.n; ++k) s += T.w[k] * row[border101(x + k - r, cols)];
    }
    tmp[(size_t)y * cols + x] = s;
}

__global__ __launch_bounds__(256) void sift_blur_cols_kernel(const float *__restrict__ tmp, float *__restrict__ dst, const float *__restrict__ prev,
                                                            float *__restrict__ dog, int rows, int cols, SiftTaps T)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= cols) return;
    const int r = T.n / 2;
    const size_t p = (size_t)y * cols + x;
    float s = T.w[r] * tmp[p];
    if (y >= r && y + r < rows) {
        for (int k = 1; k <= r; ++k) s += T.w[r + k] * (tmp[p - (size_t)k * cols] + tmp[p + (size_t)k * cols]);
    } else {
        for (int k = 1; k <= r; ++k) s += T.w[r + k] * (tmp[(size_t)border101(y - k, rows) * cols + x] + tmp[(size_t)border101(y + k, rows) * cols + x]);
    }
    dst[p] = s;
    if (dog) dog[p] = s - prev[p];
}

__global__ __launch_bounds__(256) void sift_downsample_kernel(const float *__restrict__ src, int src_cols, float *__restrict__ dst, int rows, int cols)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * cols) return;
    const int y = (int)(i / cols), x = (int)(i % cols);
    dst[i] = src[(size_t)(2 * y) * src_cols + 2 * x];
}

// ---- extrema + adjustLocalExtrema
#define AT(m, rr, cc) ((m)[(size_t)(rr) * cols + (cc)])

__device__ void sift_solve3(float A[3][3], float b[3], float x[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int k = i;
#pragma unroll
        for (int j = i + 1; j < 3; ++j) if (fabsf(A[j][i]) > fabsf(A[k][i])) k = j;
        if (fabsf(A[k][i]) < FLT_EPSILON * 10) { x[0] = x[1] = x[2] = 0.f; return; }
        if (k != i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) if (j >= i) { const float t = A[i][j]; A[i][j] = A[k][j]; A[k][j] = t; }
            const float t = b[i]; b[i] = b[k]; b[k] = t;
        }
        const float d = -1.f / A[i][i];
#pragma unroll
        for (int j = i + 1; j < 3; ++j) {
            const float alpha = A[j][i] * d;
#pragma unroll
            for (int k2 = i + 1; k2 < 3; ++k2) A[j][k2] += alpha * A[i][k2];
            b[j] += alpha * b[i];
        }
        A[i][i] = -d;
    }
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        float s = b[i];
#pragma unroll
        for (int k = i + 1; k < 3; ++k) s -= A[i][k] * b[k];
        b[i] = s * A[i][i];
    }
    x[0] = b[0]; x[1] = b[1]; x[2] = b[2];
}

__global__ __launch_bounds__(256) void sift_extrema_kernel(const float *__restrict__ dog, int rows, int cols, int o, SiftKp *__restrict__ cand,
                                                          int32_t *__restrict__ counters, int cand_cap)
{
    const int h = rows - 2 * kSiftBorder, w = cols - 2 * kSiftBorder;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)kSiftLayers * h * w) return;
    const int i = (int)(t / ((int64_t)h * w)) + 1;
    const int rem = (int)(t % ((int64_t)h * w));
    const int r0 = rem / w + kSiftBorder, c0 = rem % w + kSiftBorder;
    const size_t plane = (size_t)rows * cols;
    {
        const float *img = dog + plane * i;
        const float val = AT(img, r0, c0);
        if (!(fabsf(val) > 1.f)) return;
        bool ext = true;
        for (int dl = -1; dl <= 1; ++dl) {
            const float *m = img + (ptrdiff_t)plane * dl;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dl == 0 && dy == 0 && dx == 0) continue;
                    const float u = AT(m, r0 + dy, c0 + dx);
                    ext = ext && (val > 0 ? val >= u : val <= u);
                }
        }
        if (!ext) return;
    }
    const float img_scale = 1.f / 255, deriv_scale = img_scale * 0.5f, second_deriv_scale = img_scale, cross_deriv_scale = img_scale * 0.25f;
    int layer = i, r = r0, c = c0;
    float xi = 0, xr = 0, xc = 0;
    int it = 0;
    for (; it < 5; ++it) {
        const float *img = dog + plane * layer, *prev = img - plane, *next = img + plane;
        float dD[3] = {(AT(img, r, c + 1) - AT(img, r, c - 1)) * deriv_scale, (AT(img, r + 1, c) - AT(img, r - 1, c)) * deriv_scale,
                       (AT(next, r, c) - AT(prev, r, c)) * deriv_scale};
        const float v2 = AT(img, r, c) * 2.f;
        const float dxx = (AT(img, r, c + 1) + AT(img, r, c - 1) - v2) * second_deriv_scale;
        const float dyy = (AT(img, r + 1, c) + AT(img, r - 1, c) - v2) * second_deriv_scale;
        const float dss = (AT(next, r, c) + AT(prev, r, c) - v2) * second_deriv_scale;
        const float dxy = (AT(img, r + 1, c + 1) - AT(img, r + 1, c - 1) - AT(img, r - 1, c + 1) + AT(img, r - 1, c - 1)) * cross_deriv_scale;
        const float dxs = (AT(next, r, c + 1) - AT(next, r, c - 1) - AT(prev, r, c + 1) + AT(prev, r, c - 1)) * cross_deriv_scale;
        const float dys = (AT(next, r + 1, c) - AT(next, r - 1, c) - AT(prev, r + 1, c) + AT(prev, r - 1, c)) * cross_deriv_scale;
        float H[3][3] = {{dxx, dxy, dxs}, {dxy, dyy, dys}, {dxs, dys, dss}}, X[3];
        sift_solve3(H, dD, X);
        xi = -X[2]; xr = -X[1]; xc = -X[0];
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
        const float big = (float)(INT32_MAX / 3);
        if (fabsf(xi) > big || fabsf(xr) > big || fabsf(xc) > big) return;
        c += (int)rintf(xc); r += (int)rintf(xr); layer += (int)rintf(xi);
        if (layer < 1 || layer > kSiftLayers || c < kSiftBorder || c >= cols - kSiftBorder || r < kSiftBorder || r >= rows - kSiftBorder) return;
    }
    if (it >= 5) return;
    float contr;
    {
        const float *img = dog + plane * layer, *prev = img - plane, *next = img + plane;
        const float dD0 = (AT(img, r, c + 1) - AT(img, r, c - 1)) * deriv_scale, dD1 = (AT(img, r + 1, c) - AT(img, r - 1, c)) * deriv_scale,
                    dD2 = (AT(next, r, c) - AT(prev, r, c)) * deriv_scale;
        const float tt = dD0 * xc + dD1 * xr + dD2 * xi;
        contr = AT(img, r, c) * img_scale + tt * 0.5f;
        if (fabsf(contr) * kSiftLayers < 0.04f) return;
        const float v2 = AT(img, r, c) * 2.f;
        const float dxx = (AT(img, r, c + 1) + AT(img, r, c - 1) - v2) * second_deriv_scale;
        const float dyy = (AT(img, r + 1, c) + AT(img, r - 1, c) - v2) * second_deriv_scale;
        const float dxy = (AT(img, r + 1, c + 1) - AT(img, r + 1, c - 1) - AT(img, r - 1, c + 1) + AT(img, r - 1, c - 1)) * cross_deriv_scale;
        const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
        if (det <= 0 || tr * tr * 10.f >= 121.f * det) return;
    }
    SiftKp k;
    const float p2 = (float)(1 << o);
    k.xo = (float)c + xc; k.yo = (float)r + xr;
    k.x = k.xo * p2; k.y = k.yo * p2;
    k.octave = o + (layer << 8) + ((int)rint(((double)xi + 0.5) * 255) << 16);
    k.scl = 1.6f * sift_exp2(((float)layer + xi) / (float)kSiftLayers);
    k.size = k.scl * p2 * 2.f;
    k.response = fabsf(contr);
    k.angle = 0.f;
    k.o = o; k.layer = layer; k.r = r; k.c = c; k.pad = 0;
    k.key = (((int64_t)(o * 4 + i) * 65536 + r0) * 65536 + c0);
    const int slot = atomicAdd(&counters[0], 1);
    if (slot < cand_cap) cand[slot] = k;
}

// ---- orientation: one wave per candidate, lane b < 36 owns bin b
__global__ __launch_bounds__(256) void sift_orient_kernel(SiftPyr P, const float *__restrict__ pyr, const SiftKp *__restrict__ cand,
                                                         int32_t *__restrict__ counters, int cand_cap, SiftKp *__restrict__ kps, int kp_cap)
{
    const int lane = threadIdx.x & 63;
    const int n_cand = min(counters[0], cand_cap);
    for (int ci = blockIdx.x * 4 + (threadIdx.x >> 6); ci < n_cand; ci += gridDim.x * 4) {
        const SiftKp cd = cand[ci];
        const int rows = P.oct[cd.o].rows, cols = P.oct[cd.o].cols;
        const float *img = pyr + P.oct[cd.o].g_off + (int64_t)cd.layer * rows * cols;
        const float scl = cd.scl;
        const int radius = (int)rintf(4.5f * scl), side = 2 * radius + 1, total = side * side;
        const float sigma = 1.5f * scl, expf_scale = -1.f / (2.f * sigma * sigma);
        float acc = 0.f;
        for (int base = 0; base < total; base += 64) {
            const int s = base + lane;
            int bin = -1;
            float val = 0.f;
            if (s < total) {
                const int i = s / side - radius, j = s % side - radius;
                const int y = cd.r + i, x = cd.c + j;
                if (y > 0 && y < rows - 1 && x > 0 && x < cols - 1) {
                    const float dx = AT(img, y, x + 1) - AT(img, y, x - 1), dy = AT(img, y - 1, x) - AT(img, y + 1, x);
                    const float w = sift_exp((float)(i * i + j * j) * expf_scale);
                    const float ori = fast_atan2(dy, dx), mag = sqrtf(dx * dx + dy * dy);
                    bin = (int)rintf((kSiftOriBins / 360.f) * ori);
                    if (bin >= kSiftOriBins) bin -= kSiftOriBins;
                    if (bin < 0) bin += kSiftOriBins;
                    val = w * mag;
                }
            }
            const int cnt = min(64, total - base);
            for (int t = 0; t < cnt; ++t) {
                const int bt = __shfl(bin, t);
                const float vt = __shfl(val, t);
                if (bt == lane) acc += vt;
            }
        }
        const int b = lane < kSiftOriBins ? lane : 0;
        const float tm2 = __shfl(acc, (b + kSiftOriBins - 2) % kSiftOriBins), tp2 = __shfl(acc, (b + 2) % kSiftOriBins);
        const float tm1 = __shfl(acc, (b + kSiftOriBins - 1) % kSiftOriBins), tp1 = __shfl(acc, (b + 1) % kSiftOriBins);
        const float t0 = __shfl(acc, b);
        const float hist = (tm2 + tp2) * (1.f / 16.f) + (tm1 + tp1) * (4.f / 16.f) + t0 * (6.f / 16.f);
        float omax = lane < kSiftOriBins ? hist : -1.f;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) omax = fmaxf(omax, __shfl_xor(omax, off));
        const float mag_thr = omax * 0.8f;
        const float hl = __shfl(hist, (b + kSiftOriBins - 1) % kSiftOriBins), hr = __shfl(hist, (b + 1) % kSiftOriBins);
        if (lane < kSiftOriBins && hist > hl && hist > hr && hist >= mag_thr) {
            float bin = (float)lane + 0.5f * (hl - hr) / (hl - 2 * hist + hr);
            bin = bin < 0 ? kSiftOriBins + bin : bin >= kSiftOriBins ? bin - kSiftOriBins : bin;
            SiftKp k = cd;
            k.angle = 360.f - (360.f / kSiftOriBins) * bin;
            if (fabsf(k.angle - 360.f) < FLT_EPSILON) k.angle = 0.f;
            k.key = cd.key * 64 + lane;
            const int slot = atomicAdd(&counters[1], 1);
            if (slot < kp_cap) kps[slot] = k;
        }
    }
}

// ---- descriptor: one workgroup per keypoint
__global__ __launch_bounds__(kSiftDescThreads) void sift_describe_kernel(SiftPyr P, const float *__restrict__ pyr, const SiftKp *__restrict__ kps,
                                                                         float *__restrict__ desc)
{
    constexpr int d = 4, n = 8, NT = kSiftDescThreads;
    __shared__ float s_rb[NT], s_cb[NT], s_ob[NT], s_mag[NT];
    __shared__ int s_cell[NT];      // (r0 + 1) | (c0 + 1) << 8 | o0 << 16
    __shared__ int s_wcnt[NT / 64];
    __shared__ float s_hist[(d + 2) * (d + 2) * (n + 2)], s_v[d * d * n], s_scale[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SiftKp k = kps[blockIdx.x];
    const int rows = P.oct[k.o].rows, cols = P.oct[k.o].cols;
    const float *img = pyr + P.oct[k.o].g_off + (int64_t)k.layer * rows * cols;
    float ori = 360.f - k.angle;
    if (fabsf(ori - 360.f) < FLT_EPSILON) ori = 0.f;
    const int ptx = (int)rintf(k.xo), pty = (int)rintf(k.yo);
    float cos_t = sift_cos(ori * (float)(3.14159265358979323846 / 180)), sin_t = sift_sin(ori * (float)(3.14159265358979323846 / 180));
    const float bins_per_rad = n / 360.f, exp_scale = -1.f / (d * d * 0.5f), hist_width = 3.f * k.scl;
    int radius = (int)rintf(hist_width * 1.4142135623730951f * (d + 1) * 0.5f);
    const int diag = (int)sqrt((double)cols * cols + (double)rows * rows);
    radius = min(radius, diag);
    cos_t /= hist_width; sin_t /= hist_width;
    const int side = 2 * radius + 1, total = side * side;
    // the bin this thread owns
    const int my_r = tid / ((d + 2) * (n + 2)), my_c = (tid / (n + 2)) % (d + 2), my_o = tid % (n + 2);
    float acc = 0.f;
    for (int base = 0; base < total; base += NT) {
        const int s = base + tid;
        bool ok = false;
        float rbin = 0, cbin = 0, obin = 0, mag = 0;
        int r0 = 0, c0 = 0, o0 = 0;
        if (s < total) {
            const int i = s / side - radius, j = s % side - radius;
            const float c_rot = (float)j * cos_t - (float)i * sin_t, r_rot = (float)j * sin_t + (float)i * cos_t;
            rbin = r_rot + (float)(d / 2) - 0.5f; cbin = c_rot + (float)(d / 2) - 0.5f;
            const int r = pty + i, c = ptx + j;
            ok = rbin > -1 && rbin < d && cbin > -1 && cbin < d && r > 0 && r < rows - 1 && c > 0 && c < cols - 1;
            if (ok) {
                const float dx = AT(img, r, c + 1) - AT(img, r, c - 1), dy = AT(img, r - 1, c) - AT(img, r + 1, c);
                const float W = sift_exp((c_rot * c_rot + r_rot * r_rot) * exp_scale);
                const float Ori = fast_atan2(dy, dx), Mag = sqrtf(dx * dx + dy * dy);
                obin = (Ori - ori) * bins_per_rad;
                mag = Mag * W;
                r0 = (int)floorf(rbin); c0 = (int)floorf(cbin); o0 = (int)floorf(obin);
                rbin -= (float)r0; cbin -= (float)c0; obin -= (float)o0;
                if (o0 < 0) o0 += n;
                if (o0 >= n) o0 -= n;
            }
        }
        // order-preserving compaction of this chunk's samples into LDS
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = 0, n_ok = 0;
        for (int w = 0; w < NT / 64; ++w) { if (w < wave) off += s_wcnt[w]; n_ok += s_wcnt[w]; }
        if (ok) {
            const int pos = off + __popcll(m & ((1ull << lane) - 1));
            s_rb[pos] = rbin; s_cb[pos] = cbin; s_ob[pos] = obin; s_mag[pos] = mag;
            s_cell[pos] = (r0 + 1) | ((c0 + 1) << 8) | (o0 << 16);
        }
        __syncthreads();
        if (tid < (d + 2) * (d + 2) * (n + 2)) {
            for (int q = 0; q < n_ok; ++q) {
                const int cell = s_cell[q];
                const unsigned dr = (unsigned)(my_r - (cell & 255)), dc = (unsigned)(my_c - ((cell >> 8) & 255)), dq = (unsigned)(my_o - (cell >> 16));
                if (dr <= 1 && dc <= 1 && dq <= 1) {
                    const float mg = s_mag[q];
                    const float v_r1 = mg * s_rb[q], v_r0 = mg - v_r1;
                    const float vr = dr ? v_r1 : v_r0;
                    const float vc1 = vr * s_cb[q], vc0 = vr - vc1;
                    const float vc = dc ? vc1 : vc0;
                    const float vo1 = vc * s_ob[q], vo0 = vc - vo1;
                    acc += dq ? vo1 : vo0;
                }
            }
        }
        __syncthreads();
    }
    if (tid < (d + 2) * (d + 2) * (n + 2)) s_hist[tid] = acc;
    __syncthreads();
    if (tid < d * d * n) {
        const int i = tid / (d * n), j = (tid / n) % d, q = tid % n;
        const int idx = ((i + 1) * (d + 2) + (j + 1)) * (n + 2);
        s_v[tid] = q == 0 ? s_hist[idx] + s_hist[idx + n] : q == 1 ? s_hist[idx + 1] + s_hist[idx + n + 1] : s_hist[idx + q];
    }
    __syncthreads();
    if (tid == 0) {
        float nrm2 = 0;
        for (int q = 0; q < d * d * n; ++q) nrm2 += s_v[q] * s_v[q];
        const float thr = sqrtf(nrm2) * 0.2f;
        nrm2 = 0;
        for (int q = 0; q < d * d * n; ++q) { const float val = s_v[q] < thr ? s_v[q] : thr; nrm2 += val * val; }
        const float sq = sqrtf(nrm2);
        s_scale[0] = thr;
        s_scale[1] = 512.f / (sq > FLT_EPSILON ? sq : FLT_EPSILON);
    }
    __syncthreads();
    if (tid < d * d * n) {
        const float val = s_v[tid] < s_scale[0] ? s_v[tid] : s_scale[0];
        const int iv = (int)rintf(val * s_scale[1]);
        desc[(size_t)blockIdx.x * (d * d * n) + tid] = (float)(iv < 0 ? 0 : iv > 255 ? 255 : iv);
    }
}

#undef AT

// ---- launches
int launch_sift_upsample(hipStream_t st, const uint8_t *gray, int rows, int cols, float *out)
{
    const int64_t n = (int64_t)4 * rows * cols;
    hipLaunchKernelGGL(sift_upsample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gray, rows, cols, out);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_sift_blur(hipStream_t st, const float *src, float *tmp, float *dst, const float *prev, float *dog, int rows, int cols, const SiftTaps &taps)
{
    const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)rows);
    hipLaunchKernelGGL(sift_blur_rows_kernel, grid, dim3(256), 0, st, src, tmp, rows, cols, taps);
    ESFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sift_blur_cols_kernel, grid, dim3(256), 0, st, (const float *)tmp, dst, prev, dog, rows, cols, taps);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_sift_downsample(hipStream_t st, const float *src, int src_cols, float *dst, int rows, int cols)
{
    const int64_t n = (int64_t)rows * cols;
    hipLaunchKernelGGL(sift_downsample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, src_cols, dst, rows, cols);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_sift_extrema(hipStream_t st, const SiftPyr &pyr, const float *pyr_buf, int o, SiftKp *cand, int32_t *counters, int cand_cap)
{
    const int rows = pyr.oct[o].rows, cols = pyr.oct[o].cols;
    if (rows <= 2 * kSiftBorder || cols <= 2 * kSiftBorder) return ESFM_OK;
    const int64_t n = (int64_t)kSiftLayers * (rows - 2 * kSiftBorder) * (cols - 2 * kSiftBorder);
    hipLaunchKernelGGL(sift_extrema_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pyr_buf + pyr.oct[o].dog_off, rows, cols, o, cand,
                       counters, cand_cap);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_sift_orient(hipStream_t st, const SiftPyr &pyr, const float *pyr_buf, const SiftKp *cand, int32_t *counters, int cand_cap, SiftKp *kps,
                       int kp_cap)
{
    const int blocks = std::min(1024, std::max(1, (cand_cap + 3) / 4));
    hipLaunchKernelGGL(sift_orient_kernel, dim3(blocks), dim3(256), 0, st, pyr, pyr_buf, cand, counters, cand_cap, kps, kp_cap);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_sift_describe(hipStream_t st, const SiftPyr &pyr, const float *pyr_buf, const SiftKp *kps, int n_kp, float *desc)
{
    if (n_kp <= 0) return ESFM_OK;
    hipLaunchKernelGGL(sift_describe_kernel, dim3(n_kp), dim3(kSiftDescThreads), 0, st, pyr, pyr_buf, kps, desc);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

}  // namespace esfm
