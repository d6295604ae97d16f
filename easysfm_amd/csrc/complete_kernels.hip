// Track completion for gfx950 (MI355X): the device side of include/esfm.h "Track completion".
//
//   complete_box_kernel     one workgroup per camera: the box of its keypoints that take part (free; finite) and the camera's grid
//   complete_keys_kernel    one thread per keypoint row: key = camera | cell | row local to the camera (camera field n_cam: no part)
//   (mesh_sort_keys)        the radix sort the mesh code wraps: a cell's keypoints come out adjacent, a cell row's cells too
//   CompleteIsJob           the ordered compaction of block_scan.hpp over the n_pt x n_cam combinations: camera not in the track,
//                           point in front, window meets the camera's box
//   complete_jobs_kernel    ... its write half: point << 32 | camera
//   complete_search_kernel  sixteen lanes per job: the cell rows of the window by two binary searches each, the exact predicate per
//                           keypoint, the canonical distances to the point's reference rows, a two-best fold, the claim
//   complete_decode_kernel  one thread per keypoint row: the claim as kp_point / kp_dist
//   complete_stats_kernel   one thread: the counters as stats
//
// The arithmetic is complete_core.hpp (host + device, restated by tests/complete_ref.py); the kernels only decide which lane runs
// which piece.  Everything that crosses threads is an integer: the two-best fold is a total order over (distance, row), a claim is
// a 64-bit atomicMin over (distance bits, point index), the counters are integer adds.  No float atomics, no waits across workgroups.
#include "complete_kernels.hpp"
#include "block_scan.hpp"
#include "match_device.hpp"
#include "mesh_kernels.hpp"

namespace esfm {

using complete::Best2;
using complete::CamGrid;
using complete::Pixel;

constexpr int kLanesPerJob = 16, kJobsPerBlock = 256 / kLanesPerJob;

// ---- grid ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void complete_box_kernel(CompleteArgs a)
{
    __shared__ float s_box[4][4];
    __shared__ int32_t s_n[4];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t r0 = a.row_off[c], r1 = a.row_off[c + 1];
    float x0 = FLT_MAX, y0 = FLT_MAX, x1 = -FLT_MAX, y1 = -FLT_MAX;
    int32_t n = 0;
    for (int32_t r = r0 + tid; r < r1; r += 256) {
        const float u = a.kp[2 * (size_t)r], v = a.kp[2 * (size_t)r + 1];
        if (!complete::takes_part(a.kp_free[r], u, v, a.opt)) continue;
        ++n;
        if (complete::finite_f(u) && complete::finite_f(v)) { x0 = fminf(x0, u); x1 = fmaxf(x1, u); y0 = fminf(y0, v); y1 = fmaxf(y1, v); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = fminf(x0, __shfl_xor(x0, o)); y0 = fminf(y0, __shfl_xor(y0, o));
        x1 = fmaxf(x1, __shfl_xor(x1, o)); y1 = fmaxf(y1, __shfl_xor(y1, o));
        n += __shfl_xor(n, o);
    }
    if (lane == 0) { s_box[wave][0] = x0; s_box[wave][1] = y0; s_box[wave][2] = x1; s_box[wave][3] = y1; s_n[wave] = n; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            x0 = fminf(x0, s_box[w][0]); y0 = fminf(y0, s_box[w][1]); x1 = fmaxf(x1, s_box[w][2]); y1 = fmaxf(y1, s_box[w][3]);
            n += s_n[w];
        }
        a.grid[c] = complete::make_grid(x0, y0, x1, y1, n, a.opt);
    }
}

__global__ __launch_bounds__(256) void complete_keys_kernel(CompleteArgs a)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_rows) return;
    int lo = 0, hi = a.n_cam - 1;                       // the last camera whose first row is <= r (cameras without rows are passed over)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.row_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int c = lo;
    const float u = a.kp[2 * (size_t)r], v = a.kp[2 * (size_t)r + 1];
    uint64_t key = complete::grid_key(a.n_cam, 0, 0);
    if (complete::takes_part(a.kp_free[r], u, v, a.opt))
        key = complete::grid_key(c, complete::keypoint_cell(a.grid[c], u, v, a.opt), (int32_t)(r - a.row_off[c]));
    a.keys[r] = key;
}

// ---- jobs ----------------------------------------------------------------------------------------------------------------------
// combination i = point * n_cam + camera
struct CompleteIsJob {
    CompleteArgs a;
    __device__ bool operator()(int64_t i) const
    {
        if (i >= complete_combinations(a)) return false;
        const int32_t i32 = (int32_t)i;                     // (the host admits at most 2^31 - 1 combinations: a 32-bit division)
        const int32_t p = i32 / a.n_cam, c = i32 - p * a.n_cam;
        const CamGrid &g = a.grid[c];
        if (g.n <= 0) return false;
        const int32_t first = a.pt_first[p], n = a.pt_first[p + 1] - first;
        if (n == 0) return false;
        for (int32_t k = 0; k < n; ++k) if (a.obs_cam[first + k] == c) return false;
        const Pixel q = complete::project_pixel(a.Rt + 12 * (size_t)c, a.K4 + 4 * (size_t)c, a.xyz + 3 * (size_t)p);
        return complete::job_possible(g, q, a.opt);
    }
};

__global__ __launch_bounds__(256) void complete_jobs_kernel(CompleteArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool job = CompleteIsJob{a}(i);
    const int incl = block_inclusive_count(job);
    if (!job) return;
    const int32_t p = (int32_t)i / a.n_cam, c = (int32_t)i - p * a.n_cam;
    a.jobs[a.job_blocks[blockIdx.x] + incl - 1] = (uint64_t)(uint32_t)p << 32 | (uint64_t)(uint32_t)c;
}

// ---- search --------------------------------------------------------------------------------------------------------------------
template <int METRIC>
__device__ __forceinline__ float row_distance(const void *desc, int width, int32_t ra, int32_t rb)
{
    if (METRIC == ESFM_L2_F32) {
        const float *d = static_cast<const float *>(desc);
        return sqrt_rn_f32(l2sqr_canonical<false>(d + (size_t)ra * width, d + (size_t)rb * width, width));
    }
    const uint32_t *d = static_cast<const uint32_t *>(desc);
    const int words = width >> 2;
    const uint32_t *x = d + (size_t)ra * words, *y = d + (size_t)rb * words;
    int c = 0;
    for (int j = 0; j < words; ++j) c += __popc(x[j] ^ y[j]);
    return (float)c;
}

__device__ __forceinline__ Best2 group_best(Best2 b)
{
#pragma unroll
    for (int o = kLanesPerJob / 2; o > 0; o >>= 1) {
        Best2 q;
        q.d0 = __shfl_xor(b.d0, o); q.d1 = __shfl_xor(b.d1, o); q.k0 = __shfl_xor(b.k0, o); q.k1 = __shfl_xor(b.k1, o);
        complete::merge(b, q);
    }
    return b;
}

// Sixteen lanes per job; the lanes of a job take the keypoints of a cell row sixteen at a time, as many rounds as the row needs.
template <int METRIC>
__global__ __launch_bounds__(256) void complete_search_kernel(CompleteArgs a, int32_t n_jobs)
{
    const int tid = threadIdx.x, sub = tid & (kLanesPerJob - 1);
    const int64_t j = (int64_t)blockIdx.x * kJobsPerBlock + (tid / kLanesPerJob);
    const bool live = j < n_jobs;
    Best2 best = complete::empty_best();
    bool any_adm = false;
    int32_t p = 0, c = 0, row0 = 0;
    if (live) {
        const uint64_t job = a.jobs[j];
        p = (int32_t)(job >> 32); c = (int32_t)(uint32_t)job;
        row0 = a.row_off[c];
        const CamGrid g = a.grid[c];
        const Pixel q = complete::project_pixel(a.Rt + 12 * (size_t)c, a.K4 + 4 * (size_t)c, a.xyz + 3 * (size_t)p);
        const complete::Window w = complete::window_cells(g, q, a.opt);
        const int32_t first = a.pt_first[p];
        const int32_t n_all = a.pt_first[p + 1] - first, n_ref = n_all < a.opt.max_refs ? n_all : a.opt.max_refs;
        for (int32_t cy = w.cy0; cy <= w.cy1; ++cy) {
            const uint64_t k_lo = complete::grid_key(c, cy * g.nx + w.cx0, 0);
            const uint64_t k_hi = complete::grid_key(c, cy * g.nx + w.cx1, 0) + (1ull << complete::kRowBits);
            const int64_t lo = lower_bound(a.sorted, a.n_rows, k_lo), hi = lower_bound(a.sorted, a.n_rows, k_hi);
            for (int64_t s = lo + sub; s < hi; s += kLanesPerJob) {
                const int32_t k = (int32_t)(a.sorted[s] & ((1ull << complete::kRowBits) - 1));
                const size_t r = (size_t)row0 + (size_t)k;
                if (!complete::admissible(q, a.kp[2 * r], a.kp[2 * r + 1], a.opt.thr2)) continue;
                any_adm = true;
                float d = NAN;
                for (int32_t t = 0; t < n_ref; ++t) d = complete::min_score(d, row_distance<METRIC>(a.desc, a.width, a.obs_row[first + t], (int32_t)r));
                if (complete::is_candidate(d)) complete::insert(best, d, k);
            }
        }
    }
    best = group_best(best);
#pragma unroll
    for (int o = kLanesPerJob / 2; o > 0; o >>= 1) any_adm = __shfl_xor((int)any_adm, o) || any_adm;
    const bool lead = live && sub == 0;
    const bool prop = lead && complete::proposes(best, a.opt);
    if (prop) atomicMin(a.claim + (size_t)row0 + (size_t)best.k0, (unsigned long long)complete::claim_key(best.d0, p));
    const int n_adm = __syncthreads_count(lead && any_adm);
    const int n_prop = __syncthreads_count(prop);
    if (tid == 0) {
        if (n_adm) atomicAdd(a.counters + 0, (unsigned long long)n_adm);
        if (n_prop) atomicAdd(a.counters + 1, (unsigned long long)n_prop);
    }
}

// ---- results -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void complete_decode_kernel(CompleteArgs a)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool won = false;
    if (r < a.n_rows) {
        const uint64_t key = a.claim[r];
        won = key != complete::kNoClaim;
        a.kp_point[r] = won ? (int32_t)(uint32_t)key : -1;
        a.kp_dist[r] = won ? complete::bits_float((uint32_t)(key >> 32)) : FLT_MAX;
    }
    const int n = __syncthreads_count(won);
    if (threadIdx.x == 0 && n) atomicAdd(a.counters + 3, (unsigned long long)n);
}

__global__ void complete_stats_kernel(CompleteArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    a.stats[0] = (int64_t)a.counters[0]; a.stats[1] = (int64_t)a.counters[1];
    a.stats[2] = (int64_t)(a.counters[1] - a.counters[3]);      // every assigned keypoint has exactly one winner
    a.stats[3] = (int64_t)a.counters[3];
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
int launch_complete_grid(hipStream_t st, const CompleteArgs &a, void *sort_tmp, size_t sort_bytes)
{
    hipLaunchKernelGGL(complete_box_kernel, dim3((unsigned)a.n_cam), dim3(256), 0, st, a);
    LAUNCH_OK();
    hipLaunchKernelGGL(complete_keys_kernel, dim3(blocks_of(a.n_rows)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return mesh_sort_keys(sort_tmp, sort_bytes, a.keys, const_cast<uint64_t *>(a.sorted), a.n_rows, complete_key_bits(a.n_cam), st);
}

int launch_complete_job_count(hipStream_t st, const CompleteArgs &a)
{
    return launch_flag_offsets(st, complete_combinations(a), CompleteIsJob{a}, a.job_blocks);
}

int launch_complete_jobs(hipStream_t st, const CompleteArgs &a)
{
    hipLaunchKernelGGL(complete_jobs_kernel, dim3(blocks_of(complete_combinations(a))), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_complete_search(hipStream_t st, const CompleteArgs &a, int32_t n_jobs)
{
    const unsigned nb = (unsigned)((n_jobs + kJobsPerBlock - 1) / kJobsPerBlock);
    if (a.metric == ESFM_L2_F32) hipLaunchKernelGGL(complete_search_kernel<ESFM_L2_F32>, dim3(nb), dim3(256), 0, st, a, n_jobs);
    else hipLaunchKernelGGL(complete_search_kernel<ESFM_HAMMING>, dim3(nb), dim3(256), 0, st, a, n_jobs);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_complete_decode(hipStream_t st, const CompleteArgs &a)
{
    if (a.n_rows > 0) {
        hipLaunchKernelGGL(complete_decode_kernel, dim3(blocks_of(a.n_rows)), dim3(256), 0, st, a);
        LAUNCH_OK();
    }
    if (a.stats) {
        hipLaunchKernelGGL(complete_stats_kernel, dim3(1), dim3(64), 0, st, a);
        LAUNCH_OK();
    }
    return ESFM_OK;
}

}  // namespace esfm
