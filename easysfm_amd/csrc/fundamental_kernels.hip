// Fundamental-matrix RANSAC and the focal-length cost for gfx950 (MI355X): the device side of the uncalibrated start (include/esfm.h
// "Fundamental-matrix RANSAC").  The split is the homography's (homography_kernels.hip): the host replays the sample stream and the
// sequential best-model bookkeeping, every hypothesis of a chunk of iterations of every pair is solved and scored concurrently.
//
//   fundamental_solve_kernel   one thread per (pair, iteration): Hartley normalisation, 7 x 9 system, Householder null space, the
//                              cubic's real roots by bracketed Newton, up to three models (f64)
//   fundamental_score_kernel   one workgroup per (pair, iteration): inlier counts of its models under the FLOAT epipolar error
//   fundamental_mask_kernel    one workgroup per pair: inlier mask of the winning model
//   fundamental_refit_kernel   one workgroup per pair: normal matrix of the inliers in a fixed summation order, Jacobi eigenvector, rank 2
//   focal_term_kernel          one thread per (candidate, pair): w_p (s1 - s2) / (s1 + s2) of K' F_p K
//   focal_reduce_kernel        one workgroup per candidate: the sums over the pairs in pair order by the fixed tree
//
// The arithmetic is fundamental_core.hpp (host + device, restated by tests/fundamental_ref.py); the kernels below only decide which lane
// runs which piece of it.  Inlier counts are integer sums and the f64 sums follow one fixed order (lane l adds its items ascending, then
// a halving tree over the 256 lanes), so nothing depends on scheduling; there are no float atomics.
#include "fundamental_kernels.hpp"
#include "fundamental_core.hpp"

namespace esfm {

constexpr int kFmSolveLanes = 64;      // (the homography solve's launch bounds: the 7 x 9 system in f64 is its 8 x 9 with one row fewer)
constexpr int kFmLanes = homog::kRefitLanes;

__global__ __launch_bounds__(kFmSolveLanes) void fundamental_solve_kernel(const FundPair *__restrict__ pairs, int n_pairs, const float2 *__restrict__ p1,
                                                                          const float2 *__restrict__ p2, const int32_t *__restrict__ samples, int chunk,
                                                                          double *__restrict__ models, int32_t *__restrict__ n_models)
{
    const int g = blockIdx.x * kFmSolveLanes + threadIdx.x;
    if (g >= n_pairs * chunk) return;
    const FundPair pr = pairs[g / chunk];
    const int32_t *id = samples + 7 * (size_t)g;
    if (!pr.active || id[0] < 0) { n_models[g] = 0; return; }
    double q1[14], q2[14], F[27];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float2 a = p1[pr.first + id[k]], b = p2[pr.first + id[k]];
        q1[2 * k] = (double)a.x; q1[2 * k + 1] = (double)a.y; q2[2 * k] = (double)b.x; q2[2 * k + 1] = (double)b.y;
    }
    const int n = fundm::fundamental_from_7(q1, q2, F);
#pragma unroll
    for (int k = 0; k < 27; ++k) models[27 * (size_t)g + k] = F[k];
    n_models[g] = n;
}

// the same for samples given directly (esfm_fundamental_models: the solver alone, q[28 g ..] = q1[14], q2[14])
__global__ __launch_bounds__(kFmSolveLanes) void fundamental_solve_samples_kernel(const double *__restrict__ q, int n, double *__restrict__ models,
                                                                                  int32_t *__restrict__ n_models)
{
    const int g = blockIdx.x * kFmSolveLanes + threadIdx.x;
    if (g >= n) return;
    double q1[14], q2[14], F[27];
#pragma unroll
    for (int k = 0; k < 14; ++k) { q1[k] = q[28 * (size_t)g + k]; q2[k] = q[28 * (size_t)g + 14 + k]; }
    const int nm = fundm::fundamental_from_7(q1, q2, F);
#pragma unroll
    for (int k = 0; k < 27; ++k) models[27 * (size_t)g + k] = F[k];
    n_models[g] = nm;
}

// one workgroup per (pair, iteration): counts[3 g + m] = inliers of its model m (0 behind the last one); every point is read once
__global__ __launch_bounds__(256) void fundamental_score_kernel(const FundPair *__restrict__ pairs, const float2 *__restrict__ p1, const float2 *__restrict__ p2,
                                                                int chunk, const double *__restrict__ models, const int32_t *__restrict__ n_models,
                                                                int32_t *__restrict__ counts)
{
    __shared__ int red[3][4];
    const int g = blockIdx.x;
    const int nm = __builtin_amdgcn_readfirstlane(n_models[g]);
    if (nm <= 0) { if (threadIdx.x < 3) counts[3 * (size_t)g + threadIdx.x] = 0; return; }
    const FundPair pr = pairs[g / chunk];
    float Ff[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) Ff[k] = (float)models[27 * (size_t)g + k];
    int c[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < pr.count; i += 256) {
        const float2 a = p1[pr.first + i], b = p2[pr.first + i];
#pragma unroll
        for (int m = 0; m < 3; ++m)
            if (m < nm) c[m] += fundm::epipolar_inlier(Ff + 9 * m, a.x, a.y, b.x, b.y, pr.thresh_sq) ? 1 : 0;
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[m] += __shfl_xor(c[m], o);
        if ((threadIdx.x & 63) == 0) red[m][threadIdx.x >> 6] = c[m];
    }
    __syncthreads();
    if (threadIdx.x < 3) counts[3 * (size_t)g + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

// one workgroup per pair: inlier mask of its best model (best[9 * pair])
__global__ __launch_bounds__(256) void fundamental_mask_kernel(const FundPair *__restrict__ pairs, const float2 *__restrict__ p1, const float2 *__restrict__ p2,
                                                               const double *__restrict__ best, uint8_t *__restrict__ mask)
{
    const FundPair pr = pairs[blockIdx.x];
    float Ff[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ff[k] = (float)best[9 * (size_t)blockIdx.x + k];
    for (int i = threadIdx.x; i < pr.count; i += 256) {
        const float2 a = p1[pr.first + i], b = p2[pr.first + i];
        mask[pr.first + i] = fundm::epipolar_inlier(Ff, a.x, a.y, b.x, b.y, pr.thresh_sq) ? 1 : 0;
    }
}

// the halving tree over the 256 lanes' partials of K sums at once (homography_kernels.hip's)
template <int K>
__device__ __forceinline__ void fm_tree_fold(double (*sh)[kFmLanes], int l)
{
    __syncthreads();
#pragma unroll 1
    for (int stride = kFmLanes / 2; stride > 0; stride >>= 1) {
        if (l < stride) {
#pragma unroll
            for (int a = 0; a < K; ++a) sh[a][l] += sh[a][l + stride];
        }
        __syncthreads();
    }
}

// one workgroup of 256 lanes per pair, the homography re-fit's order of sums: lane l adds the pair's points l, l + 256, .. whose mask is
// set, ascending -- the coordinate sums, the distances from the centroids, the 45 upper entries of the normal matrix -- each set of
// 256 partials folded by the halving tree; lane 0 then runs the re-fit solve
__global__ __launch_bounds__(kFmLanes) void fundamental_refit_kernel(const FundPair *__restrict__ pairs, const float2 *__restrict__ p1, const float2 *__restrict__ p2,
                                                                     const uint8_t *__restrict__ mask, double *__restrict__ refit, int32_t *__restrict__ ok)
{
    __shared__ double sh[9][kFmLanes];
    __shared__ double sA[81], sV[81], sG[45];
    __shared__ int s_cnt;
    const FundPair pr = pairs[blockIdx.x];
    if (!pr.active) return;                                 // (uniform over the workgroup)
    const int l = threadIdx.x;
    if (l == 0) s_cnt = 0;
    __syncthreads();
    {
        double sx = 0.0, sy = 0.0, sX = 0.0, sY = 0.0;
        int c = 0;
        for (int i = l; i < pr.count; i += kFmLanes) {
            if (!mask[pr.first + i]) continue;
            const float2 a = p1[pr.first + i], b = p2[pr.first + i];
            sx += (double)a.x; sy += (double)a.y; sX += (double)b.x; sY += (double)b.y; ++c;
        }
        sh[0][l] = sx; sh[1][l] = sy; sh[2][l] = sX; sh[3][l] = sY;
        if (c) atomicAdd(&s_cnt, c);                        // (an integer sum: order-free)
    }
    fm_tree_fold<4>(sh, l);
    const int cnt = s_cnt;
    if (cnt < 8) {
        if (l < 9) refit[9 * (size_t)blockIdx.x + l] = 0.0;
        if (l == 0) ok[blockIdx.x] = 0;
        return;
    }
    const double nn = (double)cnt;
    homog::Norm t1 = homog::norm_from_sums(sh[0][0], sh[1][0], nn), t2 = homog::norm_from_sums(sh[2][0], sh[3][0], nn);
    __syncthreads();
    {
        double d1 = 0.0, d2 = 0.0;
        for (int i = l; i < pr.count; i += kFmLanes) {
            if (!mask[pr.first + i]) continue;
            const float2 a = p1[pr.first + i], b = p2[pr.first + i];
            d1 += homog::centred_distance(t1, (double)a.x, (double)a.y);
            d2 += homog::centred_distance(t2, (double)b.x, (double)b.y);
        }
        sh[0][l] = d1; sh[1][l] = d2;
    }
    fm_tree_fold<2>(sh, l);
    homog::norm_set_scale(t1, sh[0][0], nn); homog::norm_set_scale(t2, sh[1][0], nn);
    __syncthreads();
    double g[45];
#pragma unroll
    for (int a = 0; a < 45; ++a) g[a] = 0.0;
    for (int i = l; i < pr.count; i += kFmLanes) {
        if (!mask[pr.first + i]) continue;
        const float2 a = p1[pr.first + i], b = p2[pr.first + i];
        double r[9];
        fundm::fm_row(t1, t2, (double)a.x, (double)a.y, (double)b.x, (double)b.y, r);
        fundm::normal_accumulate(r, g);
    }
#pragma unroll
    for (int b = 0; b < 5; ++b) {                           // nine sums per pass through the 18 KB of partials
#pragma unroll
        for (int a = 0; a < 9; ++a) sh[a][l] = g[9 * b + a];
        fm_tree_fold<9>(sh, l);
        if (l < 9) sG[9 * b + l] = sh[l][0];
        __syncthreads();
    }
    if (l == 0) {
        double F[9];
        const bool good = fundm::fundamental_from_normal(sG, t1, t2, sA, sV, F);
        for (int k = 0; k < 9; ++k) refit[9 * (size_t)blockIdx.x + k] = F[k];
        ok[blockIdx.x] = good ? 1 : 0;
    }
}

// one thread per (candidate, pair): terms[n_pairs k + p]
__global__ __launch_bounds__(64) void focal_term_kernel(int n_pairs, const double *__restrict__ F, const double *__restrict__ weight, double cx, double cy,
                                                        int n_cand, const double *__restrict__ cand, double *__restrict__ terms)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= n_cand * n_pairs) return;
    const int k = g / n_pairs, p = g - k * n_pairs;
    double Fp[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Fp[i] = F[9 * (size_t)p + i];
    terms[g] = weight[p] * fundm::focal_term(Fp, cand[k], cx, cy);
}

// one workgroup per candidate: lane l adds the pairs l, l + 256, .. ascending, then the halving tree; cost = sum of terms / sum of weights
__global__ __launch_bounds__(kFmLanes) void focal_reduce_kernel(int n_pairs, const double *__restrict__ weight, const double *__restrict__ terms,
                                                                double *__restrict__ cost)
{
    __shared__ double sh[2][kFmLanes];
    const int l = threadIdx.x, k = blockIdx.x;
    double num = 0.0, den = 0.0;
    for (int p = l; p < n_pairs; p += kFmLanes) { num += terms[(size_t)n_pairs * k + p]; den += weight[p]; }
    sh[0][l] = num; sh[1][l] = den;
    fm_tree_fold<2>(sh, l);
    if (l == 0) cost[k] = sh[0][0] / sh[1][0];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
int launch_fundamental_chunk(hipStream_t st, const FundPair *pairs, int n_pairs, const float *p1, const float *p2, const int32_t *samples, int chunk,
                             double *models, int32_t *n_models, int32_t *counts, esfm_ctx *timing_ctx)
{
    const int n = n_pairs * chunk;
    if (n <= 0) return ESFM_OK;
    KernelTimer tm(timing_ctx, ESFM_K_RANSAC);
    hipLaunchKernelGGL(fundamental_solve_kernel, dim3((n + kFmSolveLanes - 1) / kFmSolveLanes), dim3(kFmSolveLanes), 0, st, pairs, n_pairs,
                       reinterpret_cast<const float2 *>(p1), reinterpret_cast<const float2 *>(p2), samples, chunk, models, n_models);
    ESFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fundamental_score_kernel, dim3(n), dim3(256), 0, st, pairs, reinterpret_cast<const float2 *>(p1), reinterpret_cast<const float2 *>(p2),
                       chunk, models, n_models, counts);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_fundamental_score(hipStream_t st, const FundPair *pairs, int n_pairs, const float *p1, const float *p2, int chunk, const double *models,
                             const int32_t *n_models, int32_t *counts)
{
    const int n = n_pairs * chunk;
    if (n <= 0) return ESFM_OK;
    hipLaunchKernelGGL(fundamental_score_kernel, dim3(n), dim3(256), 0, st, pairs, reinterpret_cast<const float2 *>(p1), reinterpret_cast<const float2 *>(p2),
                       chunk, models, n_models, counts);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_fundamental_solve_samples(hipStream_t st, const double *q, int n, double *models, int32_t *n_models)
{
    if (n <= 0) return ESFM_OK;
    hipLaunchKernelGGL(fundamental_solve_samples_kernel, dim3((n + kFmSolveLanes - 1) / kFmSolveLanes), dim3(kFmSolveLanes), 0, st, q, n, models, n_models);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_fundamental_mask(hipStream_t st, const FundPair *pairs, int n_pairs, const float *p1, const float *p2, const double *best, uint8_t *mask)
{
    if (n_pairs <= 0) return ESFM_OK;
    hipLaunchKernelGGL(fundamental_mask_kernel, dim3(n_pairs), dim3(256), 0, st, pairs, reinterpret_cast<const float2 *>(p1),
                       reinterpret_cast<const float2 *>(p2), best, mask);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_fundamental_refit(hipStream_t st, const FundPair *pairs, int n_pairs, const float *p1, const float *p2, const uint8_t *mask, double *refit,
                             int32_t *ok)
{
    if (n_pairs <= 0) return ESFM_OK;
    hipLaunchKernelGGL(fundamental_refit_kernel, dim3(n_pairs), dim3(kFmLanes), 0, st, pairs, reinterpret_cast<const float2 *>(p1),
                       reinterpret_cast<const float2 *>(p2), mask, refit, ok);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_focal_cost(hipStream_t st, int n_pairs, const double *F, const double *weight, double cx, double cy, int n_cand, const double *cand,
                      double *terms, double *cost)
{
    const int n = n_pairs * n_cand;
    if (n <= 0) return ESFM_OK;
    hipLaunchKernelGGL(focal_term_kernel, dim3((n + 63) / 64), dim3(64), 0, st, n_pairs, F, weight, cx, cy, n_cand, cand, terms);
    ESFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(focal_reduce_kernel, dim3(n_cand), dim3(kFmLanes), 0, st, n_pairs, weight, terms, cost);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

}  // namespace esfm
