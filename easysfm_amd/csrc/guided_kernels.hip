// Epipolar-guided matching (include/esfm.h "Epipolar-guided matching"): for every query row the two nearest train rows among those
// that pass the essential-matrix RANSAC's inlier test against it.  DESIGN.md section "Epipolar-guided matching" has the layout and
// what bounds the kernel.
#include <cfloat>
#include <cmath>
#include <cstdlib>

#include "guided_kernels.hpp"
#include "match_device.hpp"   // find_pair_by_block, l2sqr_canonical: the plain matcher's own

namespace esfm {

namespace {

typedef unsigned long long u64;

constexpr int kThreads = kGuidedQueryBlock;
constexpr int kTile = 256;          // rows of the streamed set whose records sit in LDS at a time
constexpr int kChunk = 16;          // rows between two looks at the queue's fill
constexpr int kQueueCap = 8192;     // admissible (lane, row) entries waiting for their descriptor distance
static_assert(kQueueCap >= 2 * kThreads * kChunk, "a chunk's pushes must fit behind the drain threshold");
constexpr u64 kEmpty = ~0ull;

// A row in the role it plays in the predicate, once per (pair, row): the query role's (Ex0, Ex1, Ex2, Ex0^2 + Ex1^2), the train
// role's (x2, y2, Et0^2, Et1^2).  The normalisation is ransac_kernels.hip's normalise_pt.
__device__ __forceinline__ double4 guided_record(const GuidedGeom &g, float2 p, bool train_role)
{
    const double x = ((double)p.x - g.cx) / g.fx, y = ((double)p.y - g.cy) / g.fy;
    if (train_role) {
        const double Et0 = g.E[0] * x + g.E[3] * y + g.E[6], Et1 = g.E[1] * x + g.E[4] * y + g.E[7];
        return make_double4(x, y, Et0 * Et0, Et1 * Et1);
    }
    const double Ex0 = g.E[0] * x + g.E[1] * y + g.E[2], Ex1 = g.E[3] * x + g.E[4] * y + g.E[5], Ex2 = g.E[6] * x + g.E[7] * y + g.E[8];
    return make_double4(Ex0, Ex1, Ex2, Ex0 * Ex0 + Ex1 * Ex1);
}

// sampson_inlier (ransac_kernels.hip) on the two records: the same operations on the same operands in the same order, whichever
// of the two rows the calling lane owns.  A NaN anywhere compares false.
__device__ __forceinline__ bool guided_admissible_divide(double p, double den, float tsq)
{
    const float err = (float)(p / den);
    return err <= tsq;
}
// The verdict without the division for the rows that are far from the cut -- all but a relative band of 1.2e-7 around it.  With
// p = v * v and den as the definition rounds them, r = fl(p / den) is within 2^-53 relative of p / den and lo = fl(den * t_in),
// hi = fl(den * t_out) within 2^-53 of their products while those are normal numbers (lo >= 1e-290; an overflow to +inf makes no
// false claim).  t_in = tsq (1 - 1e-12): p < lo  =>  r < tsq  =>  (float) r <= tsq.  t_out = nextafterf(tsq) (1 + 1e-12):
// p > hi  =>  r > nextafterf(tsq)  =>  (float) r > tsq.  Everything else -- the band, NaN, a zero or denormal product -- takes the
// defined expression.  `exact` (ESFM_GUIDED_DIVIDE=1, a measurement switch) sends every row there.
__device__ __forceinline__ bool guided_admissible(const double4 q, const double4 t, const GuidedGeom &g, bool exact)
{
    const double v = t.x * q.x + t.y * q.y + q.z;
    const double p = v * v, den = q.w + t.z + t.w;
    const double lo = den * g.t_in, hi = den * g.t_out;
    const bool decided = !exact && lo >= 1e-290 && (p < lo || p > hi);
    if (__builtin_expect(decided, 1)) return p < lo;
    return guided_admissible_divide(p, den, g.tsq);
}

enum { kL2Vec = 0, kL2Scalar = 1, kHamming = 2 };

// the plain matcher's distance of two rows of the descriptor buffer (width: floats or bytes)
template <int MODE>
__device__ __forceinline__ float guided_distance(const void *__restrict__ desc, int width, size_t qrow, size_t trow)
{
    if (MODE == kHamming) {
        const uint32_t *a = static_cast<const uint32_t *>(desc) + qrow * (size_t)(width >> 2), *b = static_cast<const uint32_t *>(desc) + trow * (size_t)(width >> 2);
        int d = 0;
        for (int w = 0; w < (width >> 2); ++w) d += __popc(a[w] ^ b[w]);
        return (float)d;
    }
    const float *a = static_cast<const float *>(desc) + qrow * (size_t)width, *b = static_cast<const float *>(desc) + trow * (size_t)width;
    return sqrtf(l2sqr_canonical<MODE == kL2Vec>(a, b, width));
}

// One workgroup per (pair, block of 256 own rows), a lane per own row.  The other set streams through LDS as records, 256 rows
// at a time; every lane evaluates the predicate of its row against each record (an LDS broadcast).  An admissible (lane, row) is
// pushed on an LDS queue; when the queue could overflow in the next 16 rows -- and at the end -- the workgroup computes the queued
// descriptor distances densely, an entry per thread, and folds each into its lane's two best keys by LDS atomic minima:
//   old = min-exchange(best0, key); min(best1, max(old, key))
// Every key but the smallest leaves best0 exactly once, so best1 ends as the second smallest whatever the order of arrival: the
// table is a function of the inputs alone.  key = distance bits << 32 | row: the (distance, index) order with ties to the lower row.
template <int MODE>
__global__ __launch_bounds__(kThreads) void guided_knn2_kernel(const void *__restrict__ desc, int width, const float2 *__restrict__ kp,
                                                               const PairDesc *__restrict__ pairs, int n_tab, int n_fwd,
                                                               const GuidedGeom *__restrict__ geom, int32_t *__restrict__ knn_idx,
                                                               float *__restrict__ knn_dist, int32_t *__restrict__ n_adm, bool exact)
{
    __shared__ double4 s_rec[kTile];
    __shared__ uint32_t s_queue[kQueueCap];
    __shared__ u64 s_b0[kThreads], s_b1[kThreads];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int g = find_pair_by_block(pairs, n_tab, (int)blockIdx.x);
    const PairDesc pd = pairs[g];
    const bool rev = g >= n_fwd;          // own rows: the forward pair's TRAIN set, in the predicate's train role
    const GuidedGeom gm = geom[rev ? g - n_fwd : g];
    const int q0 = ((int)blockIdx.x - pd.blk_off) * kThreads, q = q0 + tid;
    const bool valid = q < pd.nq;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double4 own = valid ? guided_record(gm, kp[(size_t)pd.q_row0 + q], rev) : make_double4(nan, nan, nan, nan);
    s_b0[tid] = kEmpty; s_b1[tid] = kEmpty;
    if (tid == 0) s_cnt = 0;
    int nadm = 0;

    auto drain = [&](int n) {             // (called by the whole workgroup, n uniform, every push visible)
        for (int e = tid; e < n; e += kThreads) {
            const uint32_t ent = s_queue[e];
            const int ql = (int)(ent >> 21), t = (int)(ent & 0x1FFFFFu);
            const float d = guided_distance<MODE>(desc, width, (size_t)pd.q_row0 + q0 + ql, (size_t)pd.t_row0 + t);
            if (d < FLT_MAX) {            // the oracle's strict `d < d1` on an empty slot: FLT_MAX, +inf and NaN are never neighbours
                const u64 key = ((u64)__float_as_uint(d) << 32) | (u64)(uint32_t)t;
                const u64 old = atomicMin(&s_b0[ql], key);
                atomicMin(&s_b1[ql], old > key ? old : key);
            }
        }
        __syncthreads();
        if (tid == 0) s_cnt = 0;
        __syncthreads();
    };

    for (int t0 = 0; t0 < pd.nt; t0 += kTile) {
        const int tn = min(kTile, pd.nt - t0);
        __syncthreads();                  // the previous tile's readers are done
        if (tid < tn) s_rec[tid] = guided_record(gm, kp[(size_t)pd.t_row0 + t0 + tid], !rev);
        for (int j0 = 0; j0 < tn; j0 += kChunk) {
            __syncthreads();
            const int cnt = s_cnt;
            __syncthreads();
            if (cnt > kQueueCap - kThreads * kChunk) drain(cnt);
            const int je = min(j0 + kChunk, tn);
            for (int j = j0; j < je; ++j) {
                const double4 r = s_rec[j];
                const bool adm = rev ? guided_admissible(r, own, gm, exact) : guided_admissible(own, r, gm, exact);
                if (adm) {
                    ++nadm;
                    const int slot = atomicAdd(&s_cnt, 1);
                    s_queue[slot] = ((uint32_t)tid << 21) | (uint32_t)(t0 + j);
                }
            }
        }
    }
    __syncthreads();
    drain(s_cnt);
    if (valid) {
        const u64 b0 = s_b0[tid], b1 = s_b1[tid];
        const size_t o = 2 * ((size_t)pd.out_off + q);
        knn_idx[o] = b0 == kEmpty ? -1 : (int32_t)(uint32_t)b0;
        knn_idx[o + 1] = b1 == kEmpty ? -1 : (int32_t)(uint32_t)b1;
        knn_dist[o] = b0 == kEmpty ? FLT_MAX : __uint_as_float((uint32_t)(b0 >> 32));
        knn_dist[o + 1] = b1 == kEmpty ? FLT_MAX : __uint_as_float((uint32_t)(b1 >> 32));
        if (n_adm) n_adm[(size_t)pd.out_off + q] = nadm;
    }
}

}  // namespace

void guided_set_threshold(GuidedGeom &g, double max_epipolar_px)
{
    const double t = max_epipolar_px / ((g.fx + g.fy) / 2.0);   // as the RANSAC's threshold (ransac_api.cpp fill_pairs)
    g.tsq = (float)(t * t);
    g.t_in = (double)g.tsq * (1.0 - 1e-12);
    g.t_out = (double)nextafterf(g.tsq, INFINITY) * (1.0 + 1e-12);
    g.pad = 0;
}

int launch_guided_knn2(hipStream_t st, esfm_metric metric, int width, const void *desc, const float *kp, const PairDesc *pairs, int n_tab,
                       int n_fwd, const GuidedGeom *geom, int n_blocks, int32_t *knn_idx, float *knn_dist, int32_t *n_adm)
{
    if (n_blocks <= 0 || n_tab <= 0) return ESFM_OK;
    const float2 *kp2 = reinterpret_cast<const float2 *>(kp);
    static const bool exact = [] { const char *e = getenv("ESFM_GUIDED_DIVIDE"); return e && atoi(e) != 0; }();
    if (metric == ESFM_HAMMING)
        hipLaunchKernelGGL(guided_knn2_kernel<kHamming>, dim3(n_blocks), dim3(kThreads), 0, st, desc, width, kp2, pairs, n_tab, n_fwd, geom, knn_idx, knn_dist, n_adm, exact);
    else if (width % 4 == 0 && (reinterpret_cast<uintptr_t>(desc) & 15) == 0)
        hipLaunchKernelGGL(guided_knn2_kernel<kL2Vec>, dim3(n_blocks), dim3(kThreads), 0, st, desc, width, kp2, pairs, n_tab, n_fwd, geom, knn_idx, knn_dist, n_adm, exact);
    else
        hipLaunchKernelGGL(guided_knn2_kernel<kL2Scalar>, dim3(n_blocks), dim3(kThreads), 0, st, desc, width, kp2, pairs, n_tab, n_fwd, geom, knn_idx, knn_dist, n_adm, exact);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

}  // namespace esfm
