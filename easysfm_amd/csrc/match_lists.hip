// The list kernels behind every 2-NN table (behind every row of DESIGN.md section 4.4, and the guided matcher's filters): ratio test +
// ordered compaction, cross-check join, the packing of match lists for the read-back, and the prepared buffer's fingerprint.
#include "match_lists.hpp"
#include "match_device.hpp"

#include <float.h>

namespace esfm {

// ---------------------------------------------------------------------------------------------
// The ratio test + compaction as a launch of its own (ratio_compact_pair, match_device.hpp): one workgroup per pair.  The 64-float L2 path does
// it inside l2_finish_kernel; this serves Hamming and the other L2 passes.
constexpr int kRatioThreads = 1024;     // 4096 queries per sweep of the workgroup: one round of loads for a 4096-row set
__global__ __launch_bounds__(kRatioThreads) void ratio_compact_kernel(const PairDesc *__restrict__ pairs, const int32_t *__restrict__ knn_idx,
                                                                      const float *__restrict__ knn_dist, double ratio,
                                                                      int32_t *__restrict__ query_idx, int32_t *__restrict__ train_idx,
                                                                      float *__restrict__ distance, int32_t *__restrict__ n_out)
{
    __shared__ int s_wave[kRatioThreads / 64];
    __shared__ int s_base;
    const PairDesc pd = pairs[blockIdx.x];
    ratio_compact_pair<kRatioThreads, 4>(pd, knn_idx, knn_dist, ratio, query_idx, train_idx, distance, n_out + blockIdx.x, s_wave, &s_base);
}

// ---------------------------------------------------------------------------------------------
// Cross-check (strict mutual nearest neighbour) + ordered compaction: one workgroup per FORWARD pair p of a mirrored plan whose pair
// n_pairs + p is p with query and train swapped, both 2-NN tables written by one knn pass with their markers (-2 screened, -3 proved).
// Query q of pair p, F = its forward slot 0, is kept iff F >= 0 and the mirror's slot 0 at row F is q -- plus, use_ratio, ratio_ok on
// both records.  The forward records are read as ratio_compact_pair reads them (kCrossPer consecutive queries per thread); the mirror
// record of F is a gather from the mirror pair's slice (nt x 16 B: a few tens of KB that stay in L2).  Output as ratio_compact_pair's:
// pair p's survivors query-ascending at out_off[p], the count in n_out[p], the distance the forward d0.
constexpr int kCrossThreads = 1024, kCrossPer = 4;
__global__ __launch_bounds__(kCrossThreads) void cross_check_compact_kernel(const PairDesc *__restrict__ pairs, int n_pairs,
                                                                            const int32_t *__restrict__ knn_idx, const float *__restrict__ knn_dist,
                                                                            int use_ratio, double ratio, int32_t *__restrict__ query_idx,
                                                                            int32_t *__restrict__ train_idx, float *__restrict__ distance,
                                                                            int32_t *__restrict__ n_out)
{
    __shared__ int s_wave[kCrossThreads / 64];
    __shared__ int s_base;
    const PairDesc pd = pairs[blockIdx.x], pm = pairs[n_pairs + blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int2 *fi = reinterpret_cast<const int2 *>(knn_idx) + pd.out_off, *mi = reinterpret_cast<const int2 *>(knn_idx) + pm.out_off;
    const float2 *fd = reinterpret_cast<const float2 *>(knn_dist) + pd.out_off, *md = reinterpret_cast<const float2 *>(knn_dist) + pm.out_off;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int q0 = 0; q0 < pd.nq; q0 += kCrossThreads * kCrossPer) {
        const int qa = q0 + tid * kCrossPer;
        int2 iv[kCrossPer]; float2 dv[kCrossPer];
#pragma unroll
        for (int u = 0; u < kCrossPer; ++u) { const int q = min(qa + u, pd.nq - 1); iv[u] = fi[q]; dv[u] = fd[q]; }
        bool pass[kCrossPer];
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < kCrossPer; ++u) {
            const int f = iv[u].x;
            // (unsigned) f < pm.nq: a forward index is a row of the train set, the mirror's query set -- checked, not assumed
            bool keep = qa + u < pd.nq && (unsigned)f < (unsigned)pm.nq && (!use_ratio || ratio_ok(f, iv[u].y, dv[u].x, dv[u].y, ratio));
            if (keep) {
                const int2 r = mi[f];
                keep = r.x == qa + u;
                if (keep && use_ratio) { const float2 rd = md[f]; keep = ratio_ok(r.x, r.y, rd.x, rd.y, ratio); }
            }
            pass[u] = keep;
            cnt += keep ? 1 : 0;
        }
        // exclusive scan of cnt over the workgroup (as ratio_compact_pair)
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        size_t o = (size_t)pd.out_off + off + (incl - cnt);
#pragma unroll
        for (int u = 0; u < kCrossPer; ++u) {
            if (pass[u]) { query_idx[o] = qa + u; train_idx[o] = iv[u].x; distance[o] = dv[u].x; ++o; }
        }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < kCrossThreads / 64; ++w) t += s_wave[w]; s_base += t; }
        __syncthreads();
    }
    if (tid == 0) n_out[blockIdx.x] = s_base;
}

// ---------------------------------------------------------------------------------------------
// Fingerprint of a resident descriptor buffer (esfm_ctx_set_prepared_check): a position-keyed 64-bit sum over its 4-byte words --
// integer addition, so the order in which the waves arrive does not matter.  One word of `out` is added to (zeroed by the caller).
__global__ __launch_bounds__(256) void buffer_checksum_kernel(const uint32_t *__restrict__ p, long long n_words, unsigned long long *__restrict__ out)
{
    unsigned long long h = 0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (long long)gridDim.x * 256) {
        unsigned long long x = ((unsigned long long)p[i] << 32 | (unsigned long long)(uint32_t)i) ^ ((unsigned long long)(i >> 32) << 17);
        x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;      // (murmur3's finaliser)
        h += x;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) h += __shfl_xor(h, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, h);
}

// esfm_match_pairs (host pointers): the pairs' match lists, each at its own offset in three sum(nq)-long arrays, packed back to
// back so that the read-back moves the matches and not the gaps.  tab: per pair {source offset, packed offset} (int64) and count.
__global__ __launch_bounds__(256) void pack_match_lists_kernel(const long long *__restrict__ tab, const int32_t *__restrict__ n_out, int n_pairs,
                                                               const int32_t *__restrict__ sq, const int32_t *__restrict__ stn, const float *__restrict__ sd,
                                                               int32_t *__restrict__ dq, int32_t *__restrict__ dtn, float *__restrict__ dd)
{
    for (int p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const long long so = tab[2 * (size_t)p], dof = tab[2 * (size_t)p + 1];
        const int n = n_out[p];
        for (int e = threadIdx.x; e < n; e += 256) { dq[dof + e] = sq[so + e]; dtn[dof + e] = stn[so + e]; dd[dof + e] = sd[so + e]; }
    }
}

int launch_pack_match_lists(hipStream_t st, const long long *tab, const int32_t *n_out, int n_pairs, const int32_t *sq, const int32_t *stn, const float *sd,
                            int32_t *dq, int32_t *dtn, float *dd)
{
    if (n_pairs <= 0) return ESFM_OK;
    hipLaunchKernelGGL(pack_match_lists_kernel, dim3(std::min(n_pairs, 4096)), dim3(256), 0, st, tab, n_out, n_pairs, sq, stn, sd, dq, dtn, dd);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_buffer_checksum(hipStream_t st, const void *buf, size_t bytes, unsigned long long *out)
{
    ESFM_HIP_TRY(hipMemsetAsync(out, 0, sizeof(unsigned long long), st));
    const long long n_words = (long long)(bytes / 4);
    if (n_words <= 0) return ESFM_OK;
    const int grid = (int)std::min<long long>((n_words + 255) / 256, 2048);
    hipLaunchKernelGGL(buffer_checksum_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(buf), n_words, out);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_ratio_compact(hipStream_t st, const PairDesc *pairs, int n_pairs, const int32_t *knn_idx, const float *knn_dist,
                         double ratio, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    if (n_pairs <= 0) return ESFM_OK;
    hipLaunchKernelGGL(ratio_compact_kernel, dim3(n_pairs), dim3(kRatioThreads), 0, st, pairs, knn_idx, knn_dist, ratio, query_idx,
                       train_idx, distance, n_out);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_cross_check_compact(hipStream_t st, const PairDesc *pairs, int n_pairs, const int32_t *knn_idx, const float *knn_dist, int use_ratio,
                               double ratio, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    if (n_pairs <= 0) return ESFM_OK;
    hipLaunchKernelGGL(cross_check_compact_kernel, dim3(n_pairs), dim3(kCrossThreads), 0, st, pairs, n_pairs, knn_idx, knn_dist, use_ratio, ratio,
                       query_idx, train_idx, distance, n_out);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

}  // namespace esfm
