// Homography RANSAC for gfx950 (MI355X): the device side of the planar / panoramic check of two-view verification (include/esfm.h
// "Homography RANSAC").  The split is the essential matrix's (ransac_kernels.hip): the host replays the sample stream and the
// sequential best-model bookkeeping, every hypothesis of a chunk of iterations of every pair is solved and scored concurrently.
//
//   homography_solve_kernel   one thread per (pair, iteration): Hartley normalisation, 8 x 9 DLT, Householder null vector (f64)
//   homography_score_kernel   one workgroup per (pair, iteration): inlier count under the FLOAT forward transfer error
//   homography_mask_kernel    one workgroup per pair: inlier mask of the winning model
//   homography_refit_kernel   one workgroup per pair: normal matrix of the inliers in a fixed summation order, Jacobi eigenvector
//
// The arithmetic is homography_core.hpp (host + device, restated to the letter by tests/homography_ref.py); the kernels below only
// decide which lane runs which piece of it.  Inlier counts are integer sums and the refit's f64 sums follow one fixed order (lane l
// adds its points ascending, then a halving tree over the 256 lanes), so nothing depends on scheduling; there are no float atomics.
#include "homography_kernels.hpp"
#include "homography_core.hpp"

namespace esfm {

constexpr int kSolveLanes = 64;
constexpr int kRefitLanes = homog::kRefitLanes;

__global__ __launch_bounds__(kSolveLanes) void homography_solve_kernel(const HomogPair *__restrict__ pairs, int n_pairs, const float2 *__restrict__ p1,
                                                                       const float2 *__restrict__ p2, const int32_t *__restrict__ samples, int chunk,
                                                                       double *__restrict__ models, int32_t *__restrict__ has_model)
{
    const int g = blockIdx.x * kSolveLanes + threadIdx.x;
    if (g >= n_pairs * chunk) return;
    const HomogPair pr = pairs[g / chunk];
    const int32_t *id = samples + 4 * (size_t)g;
    if (!pr.active || id[0] < 0) { has_model[g] = 0; return; }
    double q1[8], q2[8], H[9];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float2 a = p1[pr.first + id[k]], b = p2[pr.first + id[k]];
        q1[2 * k] = (double)a.x; q1[2 * k + 1] = (double)a.y; q2[2 * k] = (double)b.x; q2[2 * k + 1] = (double)b.y;
    }
    const bool ok = homog::homography_from_4(q1, q2, H);
#pragma unroll
    for (int k = 0; k < 9; ++k) models[9 * (size_t)g + k] = H[k];
    has_model[g] = ok ? 1 : 0;
}

// the same for samples given directly (esfm_homography_models: the solver alone, q[16 g ..] = q1[8], q2[8])
__global__ __launch_bounds__(kSolveLanes) void homography_solve_samples_kernel(const double *__restrict__ q, int n, double *__restrict__ models,
                                                                               int32_t *__restrict__ has_model)
{
    const int g = blockIdx.x * kSolveLanes + threadIdx.x;
    if (g >= n) return;
    double q1[8], q2[8], H[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) { q1[k] = q[16 * (size_t)g + k]; q2[k] = q[16 * (size_t)g + 8 + k]; }
    const bool ok = homog::homography_from_4(q1, q2, H);
#pragma unroll
    for (int k = 0; k < 9; ++k) models[9 * (size_t)g + k] = H[k];
    has_model[g] = ok ? 1 : 0;
}

// one workgroup per (pair, iteration): counts[g] = inliers of its model (0 without one)
__global__ __launch_bounds__(256) void homography_score_kernel(const HomogPair *__restrict__ pairs, const float2 *__restrict__ p1, const float2 *__restrict__ p2,
                                                               int chunk, const double *__restrict__ models, const int32_t *__restrict__ has_model,
                                                               int32_t *__restrict__ counts)
{
    __shared__ int red[4];
    const int g = blockIdx.x;
    if (__builtin_amdgcn_readfirstlane(has_model[g]) <= 0) { if (threadIdx.x == 0) counts[g] = 0; return; }
    const HomogPair pr = pairs[g / chunk];
    float Hf[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Hf[k] = (float)models[9 * (size_t)g + k];
    int c = 0;
    for (int i = threadIdx.x; i < pr.count; i += 256) {
        const float2 a = p1[pr.first + i], b = p2[pr.first + i];
        c += homog::transfer_inlier(Hf, a.x, a.y, b.x, b.y, pr.thresh_sq) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[g] = red[0] + red[1] + red[2] + red[3];
}

// one workgroup per pair: inlier mask of its best model (best[9 * pair])
__global__ __launch_bounds__(256) void homography_mask_kernel(const HomogPair *__restrict__ pairs, const float2 *__restrict__ p1, const float2 *__restrict__ p2,
                                                              const double *__restrict__ best, uint8_t *__restrict__ mask)
{
    const HomogPair pr = pairs[blockIdx.x];
    float Hf[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Hf[k] = (float)best[9 * (size_t)blockIdx.x + k];
    for (int i = threadIdx.x; i < pr.count; i += 256) {
        const float2 a = p1[pr.first + i], b = p2[pr.first + i];
        mask[pr.first + i] = homog::transfer_inlier(Hf, a.x, a.y, b.x, b.y, pr.thresh_sq) ? 1 : 0;
    }
}

// the halving tree over the 256 lanes' partials of K sums at once: sh[a][l] += sh[a][l + stride], stride 128, 64 .. 1; every lane
// returns with the totals readable in sh[a][0]
template <int K>
__device__ __forceinline__ void tree_fold(double (*sh)[kRefitLanes], int l)
{
    __syncthreads();
#pragma unroll 1
    for (int stride = kRefitLanes / 2; stride > 0; stride >>= 1) {
        if (l < stride) {
#pragma unroll
            for (int a = 0; a < K; ++a) sh[a][l] += sh[a][l + stride];
        }
        __syncthreads();
    }
}

// one workgroup of 256 lanes per pair: lane l adds the pair's points l, l + 256, .. whose mask is set, ascending -- first the
// coordinate sums, then the distances from the centroids, then the 45 upper entries of A'A -- and each set of 256 partials is folded
// by the halving tree; lane 0 then runs the re-fit solve
__global__ __launch_bounds__(kRefitLanes) void homography_refit_kernel(const HomogPair *__restrict__ pairs, const float2 *__restrict__ p1, const float2 *__restrict__ p2,
                                                                       const uint8_t *__restrict__ mask, double *__restrict__ refit, int32_t *__restrict__ ok)
{
    __shared__ double sh[9][kRefitLanes];
    __shared__ double sA[81], sV[81], sG[45];
    __shared__ int s_cnt;
    const HomogPair pr = pairs[blockIdx.x];
    if (!pr.active) return;                                 // (uniform over the workgroup)
    const int l = threadIdx.x;
    if (l == 0) s_cnt = 0;
    __syncthreads();
    {
        double sx = 0.0, sy = 0.0, sX = 0.0, sY = 0.0;
        int c = 0;
        for (int i = l; i < pr.count; i += kRefitLanes) {
            if (!mask[pr.first + i]) continue;
            const float2 a = p1[pr.first + i], b = p2[pr.first + i];
            sx += (double)a.x; sy += (double)a.y; sX += (double)b.x; sY += (double)b.y; ++c;
        }
        sh[0][l] = sx; sh[1][l] = sy; sh[2][l] = sX; sh[3][l] = sY;
        if (c) atomicAdd(&s_cnt, c);                        // (an integer sum: order-free)
    }
    tree_fold<4>(sh, l);
    const int cnt = s_cnt;
    if (cnt < 4) {
        if (l < 9) refit[9 * (size_t)blockIdx.x + l] = 0.0;
        if (l == 0) ok[blockIdx.x] = 0;
        return;
    }
    const double nn = (double)cnt;
    homog::Norm t1 = homog::norm_from_sums(sh[0][0], sh[1][0], nn), t2 = homog::norm_from_sums(sh[2][0], sh[3][0], nn);
    __syncthreads();
    {
        double d1 = 0.0, d2 = 0.0;
        for (int i = l; i < pr.count; i += kRefitLanes) {
            if (!mask[pr.first + i]) continue;
            const float2 a = p1[pr.first + i], b = p2[pr.first + i];
            d1 += homog::centred_distance(t1, (double)a.x, (double)a.y);
            d2 += homog::centred_distance(t2, (double)b.x, (double)b.y);
        }
        sh[0][l] = d1; sh[1][l] = d2;
    }
    tree_fold<2>(sh, l);
    homog::norm_set_scale(t1, sh[0][0], nn); homog::norm_set_scale(t2, sh[1][0], nn);
    __syncthreads();
    double g[45];
#pragma unroll
    for (int a = 0; a < 45; ++a) g[a] = 0.0;
    for (int i = l; i < pr.count; i += kRefitLanes) {
        if (!mask[pr.first + i]) continue;
        const float2 a = p1[pr.first + i], b = p2[pr.first + i];
        double r0[9], r1[9];
        homog::dlt_rows(t1, t2, (double)a.x, (double)a.y, (double)b.x, (double)b.y, r0, r1);
        homog::normal_accumulate(r0, r1, g);
    }
#pragma unroll
    for (int b = 0; b < 5; ++b) {                           // nine sums per pass through the 18 KB of partials
#pragma unroll
        for (int a = 0; a < 9; ++a) sh[a][l] = g[9 * b + a];
        tree_fold<9>(sh, l);
        if (l < 9) sG[9 * b + l] = sh[l][0];
        __syncthreads();
    }
    if (l == 0) {
        double H[9];
        const bool good = homog::homography_from_normal(sG, t1, t2, sA, sV, H);
        for (int k = 0; k < 9; ++k) refit[9 * (size_t)blockIdx.x + k] = H[k];
        ok[blockIdx.x] = good ? 1 : 0;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
int launch_homography_chunk(hipStream_t st, const HomogPair *pairs, int n_pairs, const float *p1, const float *p2, const int32_t *samples, int chunk,
                            double *models, int32_t *has_model, int32_t *counts, esfm_ctx *timing_ctx)
{
    const int n = n_pairs * chunk;
    if (n <= 0) return ESFM_OK;
    KernelTimer tm(timing_ctx, ESFM_K_RANSAC);
    hipLaunchKernelGGL(homography_solve_kernel, dim3((n + kSolveLanes - 1) / kSolveLanes), dim3(kSolveLanes), 0, st, pairs, n_pairs,
                       reinterpret_cast<const float2 *>(p1), reinterpret_cast<const float2 *>(p2), samples, chunk, models, has_model);
    ESFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(homography_score_kernel, dim3(n), dim3(256), 0, st, pairs, reinterpret_cast<const float2 *>(p1), reinterpret_cast<const float2 *>(p2),
                       chunk, models, has_model, counts);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_homography_score(hipStream_t st, const HomogPair *pairs, int n_pairs, const float *p1, const float *p2, int chunk, const double *models,
                            const int32_t *has_model, int32_t *counts)
{
    const int n = n_pairs * chunk;
    if (n <= 0) return ESFM_OK;
    hipLaunchKernelGGL(homography_score_kernel, dim3(n), dim3(256), 0, st, pairs, reinterpret_cast<const float2 *>(p1), reinterpret_cast<const float2 *>(p2),
                       chunk, models, has_model, counts);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_homography_solve_samples(hipStream_t st, const double *q, int n, double *models, int32_t *has_model)
{
    if (n <= 0) return ESFM_OK;
    hipLaunchKernelGGL(homography_solve_samples_kernel, dim3((n + kSolveLanes - 1) / kSolveLanes), dim3(kSolveLanes), 0, st, q, n, models, has_model);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_homography_mask(hipStream_t st, const HomogPair *pairs, int n_pairs, const float *p1, const float *p2, const double *best, uint8_t *mask)
{
    if (n_pairs <= 0) return ESFM_OK;
    hipLaunchKernelGGL(homography_mask_kernel, dim3(n_pairs), dim3(256), 0, st, pairs, reinterpret_cast<const float2 *>(p1),
                       reinterpret_cast<const float2 *>(p2), best, mask);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_homography_refit(hipStream_t st, const HomogPair *pairs, int n_pairs, const float *p1, const float *p2, const uint8_t *mask, double *refit,
                            int32_t *ok)
{
    if (n_pairs <= 0) return ESFM_OK;
    hipLaunchKernelGGL(homography_refit_kernel, dim3(n_pairs), dim3(kRefitLanes), 0, st, pairs, reinterpret_cast<const float2 *>(p1),
                       reinterpret_cast<const float2 *>(p2), mask, refit, ok);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

}  // namespace esfm
