// Kernels of image retrieval (include/esfm.h "Image retrieval": the rule list they follow line by line).
//   assignment   VALU f32 in the stated order per (row, centre): the matrix cores sum in another order, so they are not used here.
//                One thread per row; 16 centres at a time in LDS, their 16 running sums in registers, the block's rows staged
//                transposed 16 components at a time; the best centre is carried across the centre tiles in ascending order.
//   accumulation integer atomics only: per workgroup in LDS where D int64 entries fit, global otherwise (identical results).
//   finalise     integer maximum, per-element f64 quantisation, integer norm.
//   similarity   V V' on v_mfma_i32_16x16x64_i8, one wave per 16 x 16 tile, operands zero-padded to 16 rows / 64 columns.
//   ranking      one wave per row selects top_k times by the total order (score descending, index ascending).
#include <climits>

#include "block_scan.hpp"
#include "retrieval_kernels.hpp"

namespace esfm {
namespace {

constexpr int kRows = 256;   // rows of a workgroup of the assignment (one per thread)
constexpr int kCT = 16;      // centres per tile
constexpr int kTC = 16;      // components staged per step
constexpr int kAccRows = 1024;   // rows of one accumulation workgroup

typedef int v4i __attribute__((ext_vector_type(4)));

// component t of row `row` as the working f32 value
__device__ __forceinline__ float component(const void *desc, int metric, int width, int64_t row, int t)
{
    if (metric == ESFM_L2_F32) return static_cast<const float *>(desc)[row * width + t];
    const unsigned b = static_cast<const unsigned char *>(desc)[row * width + (t >> 3)];
    return (float)((b >> (t & 7)) & 1u);
}

__device__ __forceinline__ long long fixed_point(float x) { return llrint((double)x * 65536.0); }

__global__ __launch_bounds__(256) void retrieval_check_kernel(const float *__restrict__ v, int64_t n, int32_t *flag)
{
    bool bad = false;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) bad = bad || !(fabsf(v[e]) <= 16384.0f);
    if (bad) *flag = 1;
}

__global__ __launch_bounds__(256) void retrieval_init_kernel(const void *__restrict__ desc, RetrievalShape sh, int64_t stride, int64_t nt, float *centres)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= sh.n_centres * sh.d) return;
    const int c = e / sh.d, t = e - c * sh.d;
    const int64_t s = (int64_t)c * nt / sh.n_centres;
    centres[e] = component(desc, sh.metric, sh.width, s * stride, t);
}

__global__ __launch_bounds__(256) void retrieval_assign_kernel(const void *__restrict__ desc, RetrievalShape sh, int64_t stride, int64_t n,
                                                               const float *__restrict__ centres, int32_t *__restrict__ assign)
{
    extern __shared__ float lds[];
    float *ms = lds;                  // [d][kCT]: component-major, so a thread's 16 centres are contiguous
    float *xs = lds + sh.d * kCT;     // [kTC][kRows + 1]
    const int tid = threadIdx.x, d = sh.d;
    const int64_t s0 = (int64_t)blockIdx.x * kRows;
    float best = 0.0f;
    int best_c = 0;
    for (int c0 = 0; c0 < sh.n_centres; c0 += kCT) {
        __syncthreads();              // the last tile's reads of ms are done
        for (int e = tid; e < d * kCT; e += 256) {
            const int k = e / d, t = e - k * d;
            ms[t * kCT + k] = c0 + k < sh.n_centres ? centres[(c0 + k) * d + t] : 0.0f;
        }
        float acc[kCT];
#pragma unroll
        for (int k = 0; k < kCT; ++k) acc[k] = 0.0f;
        for (int t0 = 0; t0 < d; t0 += kTC) {
            __syncthreads();          // ms is staged; the last step's reads of xs are done
            for (int e = tid; e < kRows * kTC; e += 256) {
                const int r = e / kTC, tt = e - r * kTC;
                float v = 0.0f;
                if (s0 + r < n && t0 + tt < d) v = component(desc, sh.metric, sh.width, (s0 + r) * stride, t0 + tt);
                xs[tt * (kRows + 1) + r] = v;
            }
            __syncthreads();
            const int tn = d - t0 < kTC ? d - t0 : kTC;
            for (int tt = 0; tt < tn; ++tt) {
                const float x = xs[tt * (kRows + 1) + tid];
                const float *m = ms + (t0 + tt) * kCT;
#pragma unroll
                for (int k = 0; k < kCT; ++k) {
                    const float df = x - m[k];
                    acc[k] = acc[k] + df * df;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kCT; ++k)
            if (c0 + k < sh.n_centres && (c0 + k == 0 || acc[k] < best)) { best = acc[k]; best_c = c0 + k; }
    }
    if (s0 + tid < n) assign[s0 + tid] = best_c;
}

__global__ __launch_bounds__(256) void retrieval_accumulate_kernel(const void *__restrict__ desc, RetrievalShape sh, const int32_t *__restrict__ off,
                                                                   int64_t stride, const int32_t *__restrict__ assign, unsigned long long *sums,
                                                                   unsigned int *counts, int use_lds)
{
    extern __shared__ unsigned long long acc[];   // use_lds: D sums, then n_centres counts
    const int set = blockIdx.y, tid = threadIdx.x, d = sh.d, D = sh.n_centres * sh.d;
    const int64_t first = off[set], n = (int64_t)off[set + 1] - first, r0 = (int64_t)blockIdx.x * kAccRows;
    if (r0 >= n) return;              // the whole workgroup leaves together
    const int64_t r1 = r0 + kAccRows < n ? r0 + kAccRows : n;
    unsigned int *cnt = reinterpret_cast<unsigned int *>(acc + D);
    if (use_lds) {
        for (int e = tid; e < D; e += 256) acc[e] = 0ull;
        for (int e = tid; e < sh.n_centres; e += 256) cnt[e] = 0u;
        __syncthreads();
    }
    unsigned long long *g_sums = sums + (size_t)set * D;
    unsigned int *g_cnt = counts + (size_t)set * sh.n_centres;
    const int wave = tid >> 6, lane = tid & 63;
    for (int64_t r = r0 + wave; r < r1; r += 4) {
        const int64_t s = first + r;
        const int c = assign[s];
        for (int t = lane; t < d; t += 64) {
            const long long q = fixed_point(component(desc, sh.metric, sh.width, s * stride, t));
            if (!q) continue;
            if (use_lds) atomicAdd(&acc[c * d + t], (unsigned long long)q);
            else atomicAdd(&g_sums[c * d + t], (unsigned long long)q);
        }
        if (lane == 0) {
            if (use_lds) atomicAdd(&cnt[c], 1u);
            else atomicAdd(&g_cnt[c], 1u);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int e = tid; e < D; e += 256) if (acc[e]) atomicAdd(&g_sums[e], acc[e]);
        for (int e = tid; e < sh.n_centres; e += 256) if (cnt[e]) atomicAdd(&g_cnt[e], cnt[e]);
    }
}

__global__ __launch_bounds__(256) void retrieval_update_kernel(RetrievalShape sh, const int64_t *__restrict__ sums, const int32_t *__restrict__ counts, float *centres)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= sh.n_centres * sh.d) return;
    const int32_t n = counts[e / sh.d];
    if (n > 0) centres[e] = (float)(((double)sums[e] / (double)n) / 65536.0);
}

// one workgroup per image
__global__ __launch_bounds__(256) void retrieval_finalize_kernel(RetrievalShape sh, int64_t *sums, const int32_t *__restrict__ counts,
                                                                 const float *__restrict__ centres, int8_t *vlad, int pitch, int32_t *norm2)
{
    __shared__ unsigned long long red_max[256];
    __shared__ int red_sum[256];
    const int set = blockIdx.x, tid = threadIdx.x, d = sh.d, D = sh.n_centres * sh.d;
    int64_t *S = sums + (size_t)set * D;
    unsigned long long mx = 0ull;
    for (int e = tid; e < D; e += 256) {
        const long long v = S[e] - (long long)counts[(size_t)set * sh.n_centres + e / d] * fixed_point(centres[e]);
        S[e] = v;
        const unsigned long long a = v < 0 ? (unsigned long long)(-v) : (unsigned long long)v;
        mx = a > mx ? a : mx;
    }
    red_max[tid] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && red_max[tid + w] > red_max[tid]) red_max[tid] = red_max[tid + w];
        __syncthreads();
    }
    const unsigned long long max_s = red_max[0];
    const double root_max = sqrt((double)max_s);
    int sum = 0;
    for (int e = tid; e < D; e += 256) {
        const long long v = S[e];
        int b = 0;
        if (max_s) {
            const unsigned long long a = v < 0 ? (unsigned long long)(-v) : (unsigned long long)v;
            const int m = (int)rint((127.0 * sqrt((double)a)) / root_max);
            b = v < 0 ? -m : m;
        }
        vlad[(size_t)set * pitch + e] = (int8_t)b;
        sum += b * b;
    }
    red_sum[tid] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red_sum[tid] += red_sum[tid + w];
        __syncthreads();
    }
    if (tid == 0) norm2[set] = red_sum[0];
}

__global__ __launch_bounds__(256) void retrieval_repitch_kernel(const int8_t *__restrict__ src, int src_pitch, int8_t *__restrict__ dst, int dst_pitch, int rows, int cols)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)rows * cols) return;
    const int r = (int)(e / cols), c = (int)(e - (int64_t)r * cols);
    dst[(size_t)r * dst_pitch + c] = src[(size_t)r * src_pitch + c];
}

// One wave per 16 x 16 tile of V V'.  Lane l holds 16 consecutive k of row (l & 15) of each operand, the same k on both sides,
// so the sum over k is complete whatever the instruction's order inside a step; the result has column (l & 15) -- the B row --
// on the lane and row 4 (l >> 4) + r -- the A row -- in register r.
__global__ __launch_bounds__(256) void retrieval_dots_kernel(const int8_t *__restrict__ vp, int n16, int pitch, int n, int32_t *__restrict__ dots)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ti = blockIdx.y, tj = blockIdx.x * 4 + wave;
    if (tj * 16 >= n16) return;
    const int8_t *a = vp + (size_t)(ti * 16 + (lane & 15)) * pitch + 16 * (lane >> 4);
    const int8_t *b = vp + (size_t)(tj * 16 + (lane & 15)) * pitch + 16 * (lane >> 4);
    v4i acc = {0, 0, 0, 0};
    for (int k = 0; k < pitch; k += 64) {
        const v4i av = *reinterpret_cast<const v4i *>(a + k), bv = *reinterpret_cast<const v4i *>(b + k);
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, acc, 0, 0, 0);
    }
    const int j = tj * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = ti * 16 + 4 * (lane >> 4) + r;
        if (i < n && j < n) dots[(size_t)i * n + j] = acc[r];
    }
}

__global__ __launch_bounds__(256) void retrieval_roots_kernel(const int32_t *__restrict__ dots, int n, double *root)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) root[j] = sqrt((double)dots[(size_t)j * n + j]);
}

__device__ __forceinline__ double score_of(int32_t dot, double ri, double rj) { return ri > 0.0 && rj > 0.0 ? (double)dot / (ri * rj) : 0.0; }

// one wave per row
__global__ __launch_bounds__(256) void retrieval_rank_kernel(const int32_t *__restrict__ dots, int n, int top_k, const double *__restrict__ root,
                                                             int32_t *__restrict__ nearest, double *__restrict__ scores)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    if (i >= n) return;
    const int32_t *row = dots + (size_t)i * n;
    const double ri = root[i];
    if (scores) for (int j = lane; j < n; j += 64) scores[(size_t)i * n + j] = score_of(row[j], ri, root[j]);
    bool done = !(ri > 0.0);
    double prev_s = 0.0;
    int prev_j = -1;
    for (int r = 0; r < top_k; ++r) {
        double bs = 0.0;
        int bj = INT_MAX;
        if (!done) {
            for (int j = lane; j < n; j += 64) {
                const double rj = root[j];
                if (j == i || !(rj > 0.0)) continue;
                const double s = (double)row[j] / (ri * rj);
                if (r > 0 && !(s < prev_s || (s == prev_s && j > prev_j))) continue;   // selected already
                if (bj == INT_MAX || s > bs || (s == bs && j < bj)) { bs = s; bj = j; }
            }
            for (int w = 32; w > 0; w >>= 1) {
                const double os = __shfl_xor(bs, w);
                const int oj = __shfl_xor(bj, w);
                if (oj != INT_MAX && (bj == INT_MAX || os > bs || (os == bs && oj < bj))) { bs = os; bj = oj; }
            }
            if (bj == INT_MAX) done = true;
        }
        if (lane == 0) nearest[(size_t)i * top_k + r] = done ? -1 : bj;
        prev_s = bs; prev_j = bj;
    }
}

}  // namespace

int launch_retrieval_check_values(hipStream_t st, const float *values, int64_t n, int32_t *flag)
{
    if (n <= 0) return ESFM_OK;
    const unsigned blocks = blocks_of(n) < 2048u ? blocks_of(n) : 2048u;
    hipLaunchKernelGGL(retrieval_check_kernel, dim3(blocks), dim3(256), 0, st, values, n, flag);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_retrieval_init(hipStream_t st, const RetrievalShape &sh, const void *desc, int64_t stride, int64_t nt, float *centres)
{
    hipLaunchKernelGGL(retrieval_init_kernel, dim3(blocks_of((int64_t)sh.n_centres * sh.d)), dim3(256), 0, st, desc, sh, stride, nt, centres);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_retrieval_assign(hipStream_t st, const RetrievalShape &sh, const void *desc, int64_t stride, int64_t n, const float *centres, int32_t *assign)
{
    if (n <= 0) return ESFM_OK;
    const size_t lds = sizeof(float) * ((size_t)sh.d * kCT + (size_t)kTC * (kRows + 1));   // at most 49 KiB (d = 512)
    hipLaunchKernelGGL(retrieval_assign_kernel, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(256), lds, st, desc, sh, stride, n, centres, assign);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_retrieval_accumulate(hipStream_t st, const RetrievalShape &sh, const void *desc, const int32_t *off, int n_sets, int64_t longest,
                                int64_t stride, const int32_t *assign, int64_t *sums, int32_t *counts)
{
    if (n_sets <= 0 || longest <= 0) return ESFM_OK;
    const int use_lds = retrieval_accumulate_in_lds(sh.n_centres, sh.d) ? 1 : 0;
    const size_t lds = use_lds ? sizeof(unsigned long long) * (size_t)sh.n_centres * sh.d + sizeof(unsigned int) * (size_t)sh.n_centres : 0;
    hipLaunchKernelGGL(retrieval_accumulate_kernel, dim3((unsigned)((longest + kAccRows - 1) / kAccRows), (unsigned)n_sets), dim3(256), lds, st, desc, sh,
                       off, stride, assign, reinterpret_cast<unsigned long long *>(sums), reinterpret_cast<unsigned int *>(counts), use_lds);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_retrieval_update(hipStream_t st, const RetrievalShape &sh, const int64_t *sums, const int32_t *counts, float *centres)
{
    hipLaunchKernelGGL(retrieval_update_kernel, dim3(blocks_of((int64_t)sh.n_centres * sh.d)), dim3(256), 0, st, sh, sums, counts, centres);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_retrieval_finalize(hipStream_t st, const RetrievalShape &sh, int n_sets, int64_t *sums, const int32_t *counts, const float *centres,
                              int8_t *vlad, int pitch, int32_t *norm2)
{
    if (n_sets <= 0) return ESFM_OK;
    hipLaunchKernelGGL(retrieval_finalize_kernel, dim3((unsigned)n_sets), dim3(256), 0, st, sh, sums, counts, centres, vlad, pitch, norm2);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_retrieval_repitch(hipStream_t st, const int8_t *src, int src_pitch, int8_t *dst, int dst_pitch, int rows, int cols)
{
    if (rows <= 0 || cols <= 0) return ESFM_OK;
    hipLaunchKernelGGL(retrieval_repitch_kernel, dim3(blocks_of((int64_t)rows * cols)), dim3(256), 0, st, src, src_pitch, dst, dst_pitch, rows, cols);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_retrieval_dots(hipStream_t st, const int8_t *vp, int n16, int pitch, int n, int32_t *dots)
{
    if (n <= 0) return ESFM_OK;
    const unsigned tiles = (unsigned)(n16 / 16);
    hipLaunchKernelGGL(retrieval_dots_kernel, dim3((tiles + 3) / 4, tiles), dim3(256), 0, st, vp, n16, pitch, n, dots);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_retrieval_rank(hipStream_t st, int n, const int32_t *dots, int top_k, double *root, int32_t *nearest, double *scores)
{
    if (n <= 0) return ESFM_OK;
    hipLaunchKernelGGL(retrieval_roots_kernel, dim3(blocks_of(n)), dim3(256), 0, st, dots, n, root);
    LAUNCH_OK();
    if (top_k <= 0 && !scores) return ESFM_OK;
    hipLaunchKernelGGL(retrieval_rank_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, dots, n, top_k, root, nearest, scores);
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
