// Track triangulation for gfx950 (MI355X): the device side of include/esfm.h "Track triangulation".
//
//   track_keys_kernel       one thread per observation: key = pt_idx << 32 | input index
//   (mesh_sort_keys)        the radix sort the mesh code wraps; a track's observations come out adjacent and in input order
//   TrackIsHead             run heads through block_scan.hpp's ordered compaction: track t starts at sorted position track_first[t]
//   track_defaults_kernel   one thread per point: the outputs of a point no track names (status 1)
//   track_solve_kernel      one wave per track
//
// The arithmetic is track_core.hpp (host + device, restated to the letter by tests/track_ref.py); the kernel only decides which lane
// runs which piece of it.  A wave stages its track once as 64-byte records -- in LDS up to track::kStageCap observations (16 KB per
// one-wave workgroup, ten workgroups in a CU's 160 KB), else in its slice of a global array -- and then:
//   lanes take hypotheses h = lane, lane + 64 ..; each scores its hypothesis over all observations in observation order; the best
//     rank is folded across the wave by a butterfly of cross-lane shuffles (track::better is a total order: any shape gives the same);
//   every lane runs the refit's sums redundantly in observation order (the LDS reads are broadcasts), so no lane waits for another's
//     result and no value crosses lanes;
//   lanes take observations for the final inlier flags and unit vectors, and rows of the pair-cosine minimum, an exact f64 minimum.
// Inlier counts are integer sums.  No float atomics, no waits across workgroups.
#include "track_kernels.hpp"
#include "block_scan.hpp"
#include "mesh_kernels.hpp"

namespace esfm {

using track::Obs;
using track::Rank;

constexpr int kWave = 64;

__global__ __launch_bounds__(256) void track_keys_kernel(TrackArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_obs) return;
    a.keys[i] = (uint64_t)(uint32_t)a.pt_idx[i] << 32 | (uint64_t)i;
}

// a sorted key whose point differs from its predecessor's
struct TrackIsHead {
    TrackArgs a;
    __device__ bool operator()(int64_t i) const
    {
        if (i >= a.n_obs) return false;
        return i == 0 || (a.sorted[i - 1] >> 32) != (a.sorted[i] >> 32);
    }
};

// one thread per sorted key and one more: the heads' positions in track order, n_obs behind the last
__global__ __launch_bounds__(256) void track_heads_kernel(TrackArgs a, int n_blocks)
{
    const int64_t n = a.n_obs, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool head = TrackIsHead{a}(i);
    const int incl = block_inclusive_count(head);
    if (i > n) return;
    if (i == n) { a.track_first[a.head_blocks[n_blocks]] = (int32_t)n; return; }
    if (head) a.track_first[a.head_blocks[blockIdx.x] + incl - 1] = (int32_t)i;
}

__device__ __forceinline__ void write_point(const TrackArgs &a, int32_t p, int status, int n_inliers, double min_cos, double mse, const double *X)
{
    a.pt_status[p] = status; a.pt_n_inliers[p] = n_inliers;
    if (a.pt_min_cos) a.pt_min_cos[p] = min_cos;
    if (a.pt_mse) a.pt_mse[p] = mse;
    if (a.xyz_out) {
        const bool kept = status == track::kKept;
#pragma unroll
        for (int j = 0; j < 3; ++j) a.xyz_out[3 * (size_t)p + j] = kept ? X[j] : (a.xyz_in ? a.xyz_in[3 * (size_t)p + j] : 0.0);
    }
}

__global__ __launch_bounds__(256) void track_defaults_kernel(TrackArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n_pt) return;
    const double zero[3] = {0.0, 0.0, 0.0};
    write_point(a, (int32_t)p, track::kTooFew, 0, 1.0, 0.0, zero);
}

__device__ __forceinline__ Rank wave_best(Rank r)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        Rank q;
        q.inliers = __shfl_xor(r.inliers, o); q.cost = __shfl_xor(r.cost, o); q.h = __shfl_xor(r.h, o);
        if (track::better(q, r)) r = q;
    }
    return r;
}

__device__ __forceinline__ int wave_sum(int c)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
    return c;
}

// the track from its staged records on: every lane of the wave calls with the same arguments
__device__ __forceinline__ void solve_staged(const TrackArgs &a, Obs *rec, int n, int first, int32_t p, int lane)
{
    const track::Options &o = a.opt;
    double X[3] = {0.0, 0.0, 0.0};
    if (a.evaluate) {
#pragma unroll
        for (int j = 0; j < 3; ++j) X[j] = a.xyz_in[3 * (size_t)p + j];
    } else {
        Rank best = track::void_rank();
        const int H = track::hypothesis_count(n, o.max_hypotheses);
        for (int h = lane; h < H; h += kWave) {
            double Xh[3];
            const Rank rk = track::hypothesis_rank(rec, n, a.Rt, a.K4, o, h, Xh);
            if (track::better(rk, best)) best = rk;
        }
        best = wave_best(best);
        if (best.inliers < 0) {
            for (int k = lane; k < n; k += kWave) {
                const uint32_t idx = (uint32_t)a.sorted[first + k];
                a.obs_inlier[idx] = 0;
                if (a.obs_err2) a.obs_err2[idx] = INFINITY;
            }
            if (lane == 0) write_point(a, p, track::kNoHypothesis, 0, 1.0, 0.0, X);
            return;
        }
        int pa, pb;
        track::pair_from_number(track::hypothesis_pair(best.h, n, o.max_hypotheses), n, pa, pb);
        double Xh[3];
        track::hypothesis_point(rec[pa], rec[pb], Xh);
        for (int k = lane; k < n; k += kWave) rec[k].flags = track::project_obs(rec[k], a.Rt, a.K4, Xh, o.thr2).inlier ? 1 : 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 3; ++j) X[j] = Xh[j];
        track::refit(rec, n, a.Rt, a.K4, o, X);
        int c = 0;
        for (int k = lane; k < n; k += kWave) c += track::project_obs(rec[k], a.Rt, a.K4, X, o.thr2).inlier ? 1 : 0;
        if (wave_sum(c) < best.inliers) {
#pragma unroll
            for (int j = 0; j < 3; ++j) X[j] = Xh[j];
        }
        __syncthreads();
    }
    int c = 0;
    for (int k = lane; k < n; k += kWave) {
        track::finish_obs(rec[k], a.Rt, a.K4, X, o.thr2);
        const uint32_t idx = (uint32_t)a.sorted[first + k];
        a.obs_inlier[idx] = (uint8_t)(rec[k].flags & 1);
        if (a.obs_err2) a.obs_err2[idx] = track::err2_out(rec[k].C[0]);
        c += rec[k].flags & 1;
    }
    const int n_inliers = wave_sum(c);
    __syncthreads();
    double m = 1.0;
    for (int i = lane; i < n; i += kWave) m = track::min_cos_row(rec, n, i, m);
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) { const double q = __shfl_xor(m, s); m = q < m ? q : m; }
    if (lane == 0) {
        const double mse = track::inlier_mse(rec, n, n_inliers);
        const int status = track::verdict(n_inliers, m, o);
        write_point(a, p, status, n_inliers, m, mse, X);
    }
}

// One wave per track.  Every branch on n, on the staging's finiteness and on the ranks is uniform over the wave.
__global__ __launch_bounds__(kWave) void track_solve_kernel(TrackArgs a, int n_blocks)
{
    __shared__ Obs stage[track::kStageCap];
    const int n_tracks = a.head_blocks[n_blocks];
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_tracks) return;
    const int first = a.track_first[t], n = a.track_first[t + 1] - first;
    const int32_t p = (int32_t)(a.sorted[first] >> 32);
    const double zero[3] = {0.0, 0.0, 0.0};
    Obs *rec = n <= track::kStageCap ? stage : a.long_rec + first;
    bool ok = true;
    if (a.evaluate) {
#pragma unroll
        for (int j = 0; j < 3; ++j) ok = ok && track::finite_d(a.xyz_in[3 * (size_t)p + j]);
    }
    if (n >= 2) {
        for (int k = lane; k < n; k += kWave) {
            const uint32_t idx = (uint32_t)a.sorted[first + k];
            const int32_t cam = a.cam_idx[idx];
            Obs ob;
            ok = track::make_obs(a.Rt + 12 * (size_t)cam, a.K4 + 4 * (size_t)cam, a.uv[2 * (size_t)idx], a.uv[2 * (size_t)idx + 1], cam, ob) && ok;
            rec[k] = ob;
        }
    }
    ok = __all(ok);
    __syncthreads();
    if (n < 2 || !ok) {
        for (int k = lane; k < n; k += kWave) {
            const uint32_t idx = (uint32_t)a.sorted[first + k];
            a.obs_inlier[idx] = 0;
            if (a.obs_err2) a.obs_err2[idx] = INFINITY;
        }
        if (lane == 0) write_point(a, p, n < 2 ? track::kTooFew : track::kNonFinite, 0, 1.0, 0.0, zero);
        return;
    }
    if (n <= track::kStageCap) solve_staged(a, stage, n, first, p, lane);   // (two calls: the compiler sees which memory `rec` is)
    else solve_staged(a, a.long_rec + first, n, first, p, lane);
}

int launch_track_defaults(hipStream_t st, const TrackArgs &a)
{
    hipLaunchKernelGGL(track_defaults_kernel, dim3(blocks_of(a.n_pt)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_track_solve(hipStream_t st, const TrackArgs &a, void *sort_tmp, size_t sort_bytes)
{
    const int64_t n = a.n_obs;
    hipLaunchKernelGGL(track_keys_kernel, dim3(blocks_of(n)), dim3(256), 0, st, a);
    LAUNCH_OK();
    if (int rc = mesh_sort_keys(sort_tmp, sort_bytes, a.keys, const_cast<uint64_t *>(a.sorted), n, track_key_bits(a.n_pt), st)) return rc;
    if (int rc = launch_flag_offsets(st, n, TrackIsHead{a}, a.head_blocks)) return rc;
    hipLaunchKernelGGL(track_heads_kernel, dim3(blocks_of(n + 1)), dim3(256), 0, st, a, (int)blocks_of(n));
    LAUNCH_OK();
    if (int rc = launch_track_defaults(st, a)) return rc;
    // one workgroup per possible track: a workgroup beyond the number of run heads returns at once
    const int64_t max_tracks = n < a.n_pt ? n : (int64_t)a.n_pt;
    hipLaunchKernelGGL(track_solve_kernel, dim3((unsigned)max_tracks), dim3(kWave), 0, st, a, (int)blocks_of(n));
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
