// Kernels of the seam levelling (include/esfm.h, "Mesh texturing", esfm_mesh_texture_level): the node table from the sorted corner
// keys, the samples, and the Jacobi-preconditioned conjugate gradients over all three channels.  The smoothness neighbours are a
// CSR built by the clean-up's adjacency kernels (mesh_kernels.hip) over the corner -> node table, read as a mesh whose vertices
// are the nodes.  Every sum runs in a stated order -- a node's neighbours in ascending node order, a dot product as the header's
// tree_sum: 256 products per workgroup halved in LDS, the block sums halved again by one workgroup -- and the only atomic is an
// integer count, so the result does not depend on scheduling; tests/level_ref.py restates the rule and the output is compared bit
// for bit (-ffp-contract=off; HIP's f64 division is correctly rounded).  Nothing waits for another workgroup: every hand-over is
// the end of a launch.  Vectors are stored channel by channel, so a wave's 64 nodes read 512 contiguous bytes per channel.
#include "block_scan.hpp"
#include "level_kernels.hpp"
#include "texture_device.hpp"     // texture_project, texture_taps, texture_fetch

namespace esfm {

// One level of tree_sum for K sums at once: every thread of the workgroup brings K values (+0.0 where it has no element), thread 0
// leaves with the K block sums.  x[i] += x[i + h] for h = 128 .. 1, as the header writes it.
template <int K>
__device__ inline void level_block_sums(double (&v)[K])
{
    __shared__ double sh[K][256];
    const int i = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][i] = v[k];
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
        if (i < h) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k][i] += sh[k][i + h];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sh[k][0];
}

// ---- node table ------------------------------------------------------------------------------------------------------------
// A triangle takes part if it is labelled and its three vertices have p2 > 0 in its view; the key of a corner that does not is
// V * 64: behind every other key, and no node's.
__global__ __launch_bounds__(256) void level_corner_keys_kernel(LevelArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    const int label = a.label[t];
    const int64_t i[3] = {a.tri[3 * t], a.tri[3 * t + 1], a.tri[3 * t + 2]};
    bool part = label >= 0;
    if (part) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float u, w, p2;
            texture_project(a.cams[label], a.vertices[3 * i[k]], a.vertices[3 * i[k] + 1], a.vertices[3 * i[k] + 2], u, w, p2);
            part = part && p2 > 0.f;
        }
    }
    const uint64_t none = (uint64_t)a.V << 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.corner_keys[3 * t + k] = part ? (uint64_t)i[k] << 6 | (uint64_t)label : none;
}

// A run head of the 3 T sorted corner keys that is a node's.
struct LevelIsHead {
    LevelArgs a;
    __device__ bool operator()(int64_t i) const
    {
        if (i >= 3 * (int64_t)a.T) return false;
        const uint64_t key = a.sorted[i];
        return key < (uint64_t)a.V << 6 && (i == 0 || a.sorted[i - 1] != key);
    }
};

__global__ __launch_bounds__(256) void level_node_keys_kernel(LevelArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool head = LevelIsHead{a}(i);
    const int incl = block_inclusive_count(head);
    if (head) a.node_keys[a.head_blocks[blockIdx.x] + incl - 1] = a.sorted[i];
}

// One thread per node: its sample in the three channels, the run of nodes of its vertex, and the count of seam vertices (at the
// first node of a run of two or more).
__global__ __launch_bounds__(256) void level_nodes_kernel(LevelArgs a)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool seam_vertex = false;
    if (n < a.N) {
        const uint64_t key = a.node_keys[n];
        const int64_t vertex = (int64_t)(key >> 6);
        const int label = (int)(key & 63u);
        float u, w, p2;
        texture_project(a.cams[label], a.vertices[3 * vertex], a.vertices[3 * vertex + 1], a.vertices[3 * vertex + 2], u, w, p2);
        const TextureTaps taps = texture_taps(a.images, label, a.rows, a.cols, a.channels, u, w);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.f[c * a.stride + n] = texture_fetch(taps, a.channels == 3 ? 2 - c : 0);
        const int32_t first = (int32_t)lower_bound(a.node_keys, a.N, (uint64_t)vertex << 6);
        const int32_t last = (int32_t)lower_bound(a.node_keys, a.N, (uint64_t)(vertex + 1) << 6);
        a.seam_first[n] = first;
        a.seam_last[n] = last;
        seam_vertex = first == n && last - first >= 2;
    }
    const int count = __syncthreads_count(seam_vertex);
    if (threadIdx.x == 0 && count) atomicAdd(a.counters, count);
}

__global__ __launch_bounds__(256) void level_corner_node_kernel(LevelArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;       // 3 t + corner
    if (j >= 3 * (int64_t)a.T) return;
    const uint64_t key = a.corner_keys[j];
    a.corner_node[j] = key < (uint64_t)a.V << 6 ? (int32_t)lower_bound(a.node_keys, a.N, key) : 0;
}

// ---- the scalars -----------------------------------------------------------------------------------------------------------
// The upper levels of tree_sum over m block sums, in place, by one workgroup of 256: every thread returns the sum.
__device__ inline double level_upper_sum(double *x, int64_t m)
{
    __shared__ double sh[256];
    const int i = threadIdx.x;
    while (m > 1) {
        const int64_t blocks = (m + 255) / 256;
        for (int64_t b = 0; b < blocks; ++b) {
            sh[i] = 256 * b + i < m ? x[256 * b + i] : 0.0;
            __syncthreads();
#pragma unroll
            for (int h = 128; h >= 1; h >>= 1) {
                if (i < h) sh[i] += sh[i + h];
                __syncthreads();
            }
            if (i == 0) x[b] = sh[0];                             // (b <= 256 b: nothing unread is overwritten)
            __syncthreads();
        }
        m = blocks;
    }
    __syncthreads();
    return x[0];
}

enum LevelPhase { kPhaseStart = 0, kPhaseAlpha = 1, kPhaseBeta = 2 };

// start: rz = sum a, bb = sum b.  alpha: pq = sum a, alpha = rz / pq.  beta: rr = sum a, rz' = sum b, beta = rz' / rz, rz = rz'.
__global__ __launch_bounds__(256) void level_scalars_kernel(LevelArgs a, int phase)
{
    const int64_t m = ((int64_t)a.N + 255) / 256;
    for (int c = 0; c < 3; ++c) {
        const double sa = level_upper_sum(a.part_a + c * a.partials, m);
        const double sb = phase == kPhaseAlpha ? 0.0 : level_upper_sum(a.part_b + c * a.partials, m);
        if (threadIdx.x != 0) continue;
        double *s = a.scalars;
        if (phase == kPhaseStart) {
            s[kLevelRz + c] = sa;
            s[kLevelBb + c] = sb;
        } else if (phase == kPhaseAlpha) {
            s[kLevelAlpha + c] = sa == 0.0 ? 0.0 : s[kLevelRz + c] / sa;
        } else {
            const double rz = s[kLevelRz + c];
            s[kLevelRr + c] = sa;
            s[kLevelBeta + c] = rz == 0.0 ? 0.0 : sb / rz;
            s[kLevelRz + c] = sb;
        }
    }
}

// ---- the iteration ---------------------------------------------------------------------------------------------------------
// d, g = 0, r = rhs, p = z = r / d; the block sums of r z and of rhs rhs.
__global__ __launch_bounds__(256) void level_start_kernel(LevelArgs a)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n < a.N) {
        const int32_t first = a.seam_first[n], last = a.seam_last[n];
        float fa[3];
        double rhs[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 3; ++c) fa[c] = a.f[c * a.stride + n];
        for (int32_t b = first; b < last; ++b) {
            if (b == n) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) rhs[c] += (double)a.f[c * a.stride + b] - (double)fa[c];
        }
        const double d = ((double)(last - first - 1) + a.lambda * (double)(a.row_start[n + 1] - a.row_start[n])) + a.mu;
        a.d[n] = d;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double z = rhs[c] / d;
            a.g[c * a.stride + n] = 0.0;
            a.r[c * a.stride + n] = rhs[c];
            a.p[c * a.stride + n] = z;
            sums[c] = rhs[c] * z;
            sums[3 + c] = rhs[c] * rhs[c];
        }
    }
    level_block_sums<6>(sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.part_a[c * a.partials + blockIdx.x] = sums[c];
            a.part_b[c * a.partials + blockIdx.x] = sums[3 + c];
        }
    }
}

// q = A p and the block sums of p q.  (1 + seam + smooth) x 24 bytes of p in through the caches, 24 bytes out.
__global__ __launch_bounds__(256) void level_apply_kernel(LevelArgs a)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double sums[3] = {0.0, 0.0, 0.0};
    if (n < a.N) {
        double pa[3], s[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 3; ++c) pa[c] = a.p[c * a.stride + n];
        const int32_t first = a.seam_first[n], last = a.seam_last[n];
        for (int32_t b = first; b < last; ++b) {
            if (b == n) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += pa[c] - a.p[c * a.stride + b];
        }
        const int32_t j1 = a.row_start[n + 1];
        for (int32_t j = a.row_start[n]; j < j1; ++j) {
            const int64_t b = a.col[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] += pa[c] - a.p[c * a.stride + b];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double q = (s[c] + a.lambda * m[c]) + a.mu * pa[c];
            a.q[c * a.stride + n] = q;
            sums[c] = pa[c] * q;
        }
    }
    level_block_sums<3>(sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.part_a[c * a.partials + blockIdx.x] = sums[c];
    }
}

// g = g + alpha p, r = r - alpha q; the block sums of r r and, with z = r / d, of r z.
__global__ __launch_bounds__(256) void level_update_kernel(LevelArgs a)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n < a.N) {
        const double d = a.d[n];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double alpha = a.scalars[kLevelAlpha + c];
            const int64_t at = c * a.stride + n;
            a.g[at] = a.g[at] + alpha * a.p[at];
            const double r = a.r[at] - alpha * a.q[at];
            a.r[at] = r;
            sums[c] = r * r;
            sums[3 + c] = r * (r / d);
        }
    }
    level_block_sums<6>(sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.part_a[c * a.partials + blockIdx.x] = sums[c];
            a.part_b[c * a.partials + blockIdx.x] = sums[3 + c];
        }
    }
}

// p = z + beta p with z = r / d (the quotient the update summed: the same operands give the same bits)
__global__ __launch_bounds__(256) void level_direction_kernel(LevelArgs a)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    const double d = a.d[n];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t at = c * a.stride + n;
        a.p[at] = a.r[at] / d + a.scalars[kLevelBeta + c] * a.p[at];
    }
}

__global__ __launch_bounds__(256) void level_outputs_kernel(LevelArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;       // 3 t + corner
    if (j >= 3 * (int64_t)a.T) return;
    const bool part = a.corner_keys[j] < (uint64_t)a.V << 6;
    const int64_t n = a.corner_node[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.offsets[3 * j + c] = part ? (float)a.g[c * a.stride + n] : 0.f;
        a.samples[3 * j + c] = part ? a.f[c * a.stride + n] : 0.f;
    }
}

// ---- launches --------------------------------------------------------------------------------------------------------------
int launch_level_corner_keys(hipStream_t st, const LevelArgs &a)
{
    hipLaunchKernelGGL(level_corner_keys_kernel, dim3(blocks_of(a.T)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_level_node_keys(hipStream_t st, const LevelArgs &a)
{
    const int64_t n = 3 * (int64_t)a.T;
    if (int rc = launch_flag_offsets(st, n, LevelIsHead{a}, a.head_blocks)) return rc;
    hipLaunchKernelGGL(level_node_keys_kernel, dim3(blocks_of(n)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_level_nodes(hipStream_t st, const LevelArgs &a)
{
    hipLaunchKernelGGL(level_nodes_kernel, dim3(blocks_of(a.N)), dim3(256), 0, st, a);
    LAUNCH_OK();
    hipLaunchKernelGGL(level_corner_node_kernel, dim3(blocks_of(3 * (int64_t)a.T)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_level_start(hipStream_t st, const LevelArgs &a)
{
    hipLaunchKernelGGL(level_start_kernel, dim3(blocks_of(a.N)), dim3(256), 0, st, a);
    LAUNCH_OK();
    hipLaunchKernelGGL(level_scalars_kernel, dim3(1), dim3(256), 0, st, a, (int)kPhaseStart);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_level_step(hipStream_t st, const LevelArgs &a)
{
    hipLaunchKernelGGL(level_apply_kernel, dim3(blocks_of(a.N)), dim3(256), 0, st, a);
    LAUNCH_OK();
    hipLaunchKernelGGL(level_scalars_kernel, dim3(1), dim3(256), 0, st, a, (int)kPhaseAlpha);
    LAUNCH_OK();
    hipLaunchKernelGGL(level_update_kernel, dim3(blocks_of(a.N)), dim3(256), 0, st, a);
    LAUNCH_OK();
    hipLaunchKernelGGL(level_scalars_kernel, dim3(1), dim3(256), 0, st, a, (int)kPhaseBeta);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_level_direction(hipStream_t st, const LevelArgs &a)
{
    hipLaunchKernelGGL(level_direction_kernel, dim3(blocks_of(a.N)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_level_outputs(hipStream_t st, const LevelArgs &a)
{
    hipLaunchKernelGGL(level_outputs_kernel, dim3(blocks_of(3 * (int64_t)a.T)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
