// Mesh clean-up (include/esfm.h, "Mesh clean-up"): connected components by a lock-free union-find, the filtered and ordered
// compaction, the adjacency of the output mesh from its sorted directed keys (mesh_sort.hip sorts them), the Jacobi smoothing
// passes and the face-vector sums in incidence order.  Every float sum runs over a sorted list in list order and every count is
// an integer atomic, so the result does not depend on scheduling; tests/mesh_clean_ref.py restates the rule and the output is
// compared bit for bit (-ffp-contract=off; HIP's default f32 division and sqrtf are correctly rounded).
#include <cmath>

#include "block_scan.hpp"
#include "mesh_kernels.hpp"

namespace esfm {

// ---- components ----------------------------------------------------------------------------------------------------------
// A forest over the vertices in which a parent is always SMALLER than its child: a root is only ever linked under a smaller
// root, by a compare-and-swap on the larger root's own word, and path halving replaces a parent by a grandparent.  So a word
// only decreases, a vertex that has stopped being a root never becomes one again, and the root of the final tree is the
// component's smallest vertex whatever order the triangles arrive in.  Every access inside the launches that change the forest
// is an agent-scope relaxed atomic (the L2s of the XCDs are not coherent for plain accesses within a kernel).  A stale value is
// an older ancestor, still an ancestor; a failed compare-and-swap is another lane's success and walks on from the new parent.
// Nothing waits for another lane: no flag, no barrier across workgroups.
__device__ inline int32_t uf_load(int32_t *parent, int32_t x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int32_t uf_find(int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = uf_load(parent, x);
        if (p == x) return x;
        const int32_t g = uf_load(parent, p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // x is no root: nobody swaps on its word
        x = g;                                                    // (g < x: the walk ends)
    }
}

__device__ inline void uf_union(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }         // a is the larger root: it goes under b
        int32_t expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

__global__ __launch_bounds__(256) void mesh_init_kernel(MeshLabelArgs a)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < a.V) { a.parent[v] = (int32_t)v; a.tri_count[v] = 0; }
}

__global__ __launch_bounds__(256) void mesh_hook_kernel(MeshLabelArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    const int32_t i0 = a.tri[3 * t], i1 = a.tri[3 * t + 1], i2 = a.tri[3 * t + 2];
    uf_union(a.parent, i0, i1);
    uf_union(a.parent, i0, i2);
}

// A launch of its own: the forest is final, every walk ends at the component's minimum (halving goes on shortening the paths
// the other lanes walk, hence the atomics here too).
__global__ __launch_bounds__(256) void mesh_flatten_kernel(MeshLabelArgs a)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool root = false;
    if (v < a.V) {
        const int32_t r = uf_find(a.parent, (int32_t)v);
        a.label[v] = r;
        root = r == v;
    }
    const int n = __syncthreads_count(root);
    if (threadIdx.x == 0 && n) atomicAdd(a.stats + 1, n);
}

// count[label of the first corner] += 1.  Neighbouring triangles nearly always share their label, so a wave folds equal labels
// first (the lowest live lane names a label, the lanes that hold it are counted with one ballot) and issues one integer atomic
// per distinct label.
__global__ __launch_bounds__(256) void mesh_count_kernel(MeshLabelArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = t < a.T;
    const int32_t c = valid ? a.label[a.tri[3 * t]] : -1;
    unsigned long long live = __ballot(valid);
    while (live) {                                                // (wave-uniform)
        const int leader = __ffsll((long long)live) - 1;
        const int32_t named = __shfl(c, leader);
        const unsigned long long same = __ballot(valid && c == named);
        if (lane == leader) atomicAdd(a.tri_count + named, __popcll(same));
        live &= ~same;
    }
}

__global__ __launch_bounds__(256) void mesh_largest_kernel(MeshLabelArgs a)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t m = v < a.V ? a.tri_count[v] : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(a.stats, m);
}

int launch_mesh_labels(hipStream_t st, const MeshLabelArgs &a)
{
    ESFM_HIP_TRY(hipMemsetAsync(a.stats, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(mesh_init_kernel, dim3(blocks_of(a.V)), dim3(256), 0, st, a);
    LAUNCH_OK();
    if (a.T > 0) {
        hipLaunchKernelGGL(mesh_hook_kernel, dim3(blocks_of(a.T)), dim3(256), 0, st, a);
        LAUNCH_OK();
    }
    hipLaunchKernelGGL(mesh_flatten_kernel, dim3(blocks_of(a.V)), dim3(256), 0, st, a);
    LAUNCH_OK();
    if (a.T > 0) {
        hipLaunchKernelGGL(mesh_count_kernel, dim3(blocks_of(a.T)), dim3(256), 0, st, a);
        LAUNCH_OK();
        hipLaunchKernelGGL(mesh_largest_kernel, dim3(blocks_of(a.V)), dim3(256), 0, st, a);
        LAUNCH_OK();
    }
    return ESFM_OK;
}

// ---- filter and ordered compaction -----------------------------------------------------------------------------------------
__device__ inline bool mesh_component_kept(const MeshCompactArgs &a, int32_t c)
{
    const int64_t n = a.tri_count[c];
    return n >= a.min_triangles && 1000 * n >= (int64_t)a.min_permille * a.stats[0];
}
struct MeshVertexKept {
    MeshCompactArgs a;
    __device__ bool operator()(int64_t v) const { return v < a.V && mesh_component_kept(a, a.label[v]); }
};
struct MeshTriangleKept {
    MeshCompactArgs a;
    __device__ bool operator()(int64_t t) const { return t < a.T && mesh_component_kept(a, a.label[a.tri[3 * t]]); }
};

__global__ __launch_bounds__(256) void mesh_write_vertices_kernel(MeshCompactArgs a)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = MeshVertexKept{a}(v);
    const int incl = block_inclusive_count(keep);
    if (!keep) return;
    const int64_t dst = (int64_t)a.vertex_blocks[blockIdx.x] + incl - 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out_vertices[3 * dst + c] = a.vertices[3 * v + c];
    if (a.out_rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out_rgb[3 * dst + c] = a.rgb[3 * v + c];
    }
    if (a.vertex_map) a.vertex_map[dst] = (int32_t)v;
    a.remap[v] = (int32_t)dst;
}

// (a kept triangle's corners are connected to its first one: all three have a new index)
__global__ __launch_bounds__(256) void mesh_write_triangles_kernel(MeshCompactArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = MeshTriangleKept{a}(t);
    const int incl = block_inclusive_count(keep);
    if (!keep) return;
    const int64_t dst = (int64_t)a.triangle_blocks[blockIdx.x] + incl - 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out_tri[3 * dst + c] = a.remap[a.tri[3 * t + c]];
    if (a.triangle_map) a.triangle_map[dst] = (int32_t)t;
}

int launch_mesh_compact(hipStream_t st, const MeshCompactArgs &a)
{
    if (int rc = launch_flag_offsets(st, a.V, MeshVertexKept{a}, a.vertex_blocks)) return rc;
    if (int rc = launch_flag_offsets(st, a.T, MeshTriangleKept{a}, a.triangle_blocks)) return rc;
    hipLaunchKernelGGL(mesh_write_vertices_kernel, dim3(blocks_of(a.V)), dim3(256), 0, st, a);
    LAUNCH_OK();
    hipLaunchKernelGGL(mesh_write_triangles_kernel, dim3(blocks_of(a.T)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

// ---- adjacency -------------------------------------------------------------------------------------------------------------
// A key with a == b is written as (V << 32): behind every other key, and no row's.
__global__ __launch_bounds__(256) void mesh_edge_keys_kernel(MeshGraphArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    const uint64_t i[3] = {(uint64_t)a.tri[3 * t], (uint64_t)a.tri[3 * t + 1], (uint64_t)a.tri[3 * t + 2]};
    const uint64_t none = (uint64_t)a.V << 32;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint64_t p = i[c], q = i[(c + 1) % 3];
        a.keys[6 * t + 2 * c] = p == q ? none : p << 32 | q;
        a.keys[6 * t + 2 * c + 1] = p == q ? none : q << 32 | p;
    }
}

// A run head of the 6 T sorted keys that names a row.
struct MeshIsHead {
    MeshGraphArgs a;
    __device__ bool operator()(int64_t i) const
    {
        if (i >= 6 * (int64_t)a.T) return false;
        const uint64_t key = a.sorted[i];
        return (int64_t)(key >> 32) < a.V && (i == 0 || a.sorted[i - 1] != key);
    }
};

// One thread per sorted key and one more: the number of run heads before each key (so the first key of a row names the row's
// first column), the column of each head, and a row's pinned byte wherever a run is not exactly two keys long.
__global__ __launch_bounds__(256) void mesh_columns_kernel(MeshGraphArgs a, int n_blocks)
{
    const int64_t n = 6 * (int64_t)a.T, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool head = MeshIsHead{a}(i);
    const int incl = block_inclusive_count(head);
    if (i > n) return;
    if (i == n) { a.head_rank[n] = a.head_blocks[n_blocks]; return; }
    const int32_t rank = a.head_blocks[blockIdx.x] + incl - (head ? 1 : 0);
    a.head_rank[i] = rank;
    if (!head) return;
    const uint64_t key = a.sorted[i];
    a.col[rank] = (int32_t)(key & 0xFFFFFFFFull);
    const bool two = i + 1 < n && a.sorted[i + 1] == key && (i + 2 >= n || a.sorted[i + 2] != key);
    if (!two) a.pinned[key >> 32] = 1;
}

__global__ __launch_bounds__(256) void mesh_rows_kernel(const uint64_t *sorted, int64_t n, const int32_t *rank, int32_t V, int32_t *start)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v > V) return;
    const int64_t j = lower_bound(sorted, n, (uint64_t)v << 32);
    start[v] = rank ? rank[j] : (int32_t)j;
}

int mesh_build_adjacency(hipStream_t st, const MeshGraphArgs &a, void *sort_tmp, size_t sort_bytes)
{
    const int64_t n = 6 * (int64_t)a.T;
    hipLaunchKernelGGL(mesh_edge_keys_kernel, dim3(blocks_of(a.T)), dim3(256), 0, st, a);
    LAUNCH_OK();
    if (int rc = mesh_sort_keys(sort_tmp, sort_bytes, a.keys, const_cast<uint64_t *>(a.sorted), n, mesh_key_bits(a.V), st)) return rc;
    ESFM_HIP_TRY(hipMemsetAsync(a.pinned, 0, (size_t)a.V, st));
    if (int rc = launch_flag_offsets(st, n, MeshIsHead{a}, a.head_blocks)) return rc;
    hipLaunchKernelGGL(mesh_columns_kernel, dim3(blocks_of(n + 1)), dim3(256), 0, st, a, (int)blocks_of(n));
    LAUNCH_OK();
    hipLaunchKernelGGL(mesh_rows_kernel, dim3(blocks_of((int64_t)a.V + 1)), dim3(256), 0, st, a.sorted, n, (const int32_t *)a.head_rank, a.V, a.row_start);
    LAUNCH_OK();
    return ESFM_OK;
}

// ---- smoothing -------------------------------------------------------------------------------------------------------------
// One thread per vertex and pass: (1 + k) x 12 bytes in through the caches, 12 bytes out; the neighbours in list order.
__global__ __launch_bounds__(256) void mesh_smooth_kernel(MeshGraphArgs a, const float *p, float *q, float w, int pin_boundary)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.V) return;
    const int32_t r0 = a.row_start[i], k = a.row_start[i + 1] - r0;
    float x[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
    if (k > 0 && !(pin_boundary && a.pinned[i])) {
        const int64_t n0 = a.col[r0];
        float m[3] = {p[3 * n0], p[3 * n0 + 1], p[3 * n0 + 2]};
        for (int32_t j = 1; j < k; ++j) {
            const int64_t nj = a.col[r0 + j];
            m[0] += p[3 * nj]; m[1] += p[3 * nj + 1]; m[2] += p[3 * nj + 2];
        }
        const float kf = (float)k;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float centre = m[c] / kf;
            x[c] = x[c] + w * (centre - x[c]);
        }
    }
    q[3 * i] = x[0]; q[3 * i + 1] = x[1]; q[3 * i + 2] = x[2];
}

int launch_mesh_smooth(hipStream_t st, const MeshGraphArgs &a, const float *p, float *q, float w, int pin_boundary)
{
    hipLaunchKernelGGL(mesh_smooth_kernel, dim3(blocks_of(a.V)), dim3(256), 0, st, a, p, q, w, pin_boundary);
    LAUNCH_OK();
    return ESFM_OK;
}

// ---- normals ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_incidence_keys_kernel(MeshGraphArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;       // 3 t + corner
    if (j >= 3 * (int64_t)a.T) return;
    a.keys[j] = (uint64_t)a.tri[j] << 32 | (uint64_t)j;
}

__global__ __launch_bounds__(256) void mesh_faces_kernel(MeshGraphArgs a, const float *p)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    const int64_t i0 = a.tri[3 * t], i1 = a.tri[3 * t + 1], i2 = a.tri[3 * t + 2];
    float e1[3], e2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { e1[c] = p[3 * i1 + c] - p[3 * i0 + c]; e2[c] = p[3 * i2 + c] - p[3 * i0 + c]; }
    a.face[3 * t] = e1[1] * e2[2] - e1[2] * e2[1];
    a.face[3 * t + 1] = e1[2] * e2[0] - e1[0] * e2[2];
    a.face[3 * t + 2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// One thread per vertex over its run of sorted incidence keys: the inverted index fixes the order of the sum.
__global__ __launch_bounds__(256) void mesh_normals_kernel(MeshGraphArgs a, float *normals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.V) return;
    const int32_t j0 = a.inc_start[i], j1 = a.inc_start[i + 1];
    float n[3] = {0.f, 0.f, 0.f};
    for (int32_t j = j0; j < j1; ++j) {
        const int64_t t = (int64_t)(a.sorted[j] & 0xFFFFFFFFull) / 3;
        const float f[3] = {a.face[3 * t], a.face[3 * t + 1], a.face[3 * t + 2]};
        if (j == j0) { n[0] = f[0]; n[1] = f[1]; n[2] = f[2]; }
        else { n[0] += f[0]; n[1] += f[1]; n[2] += f[2]; }
    }
    const float L = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool ok = L > 0.f && isfinite(L);
    normals[3 * i] = ok ? n[0] / L : 0.f;
    normals[3 * i + 1] = ok ? n[1] / L : 0.f;
    normals[3 * i + 2] = ok ? n[2] / L : 0.f;
}

int mesh_build_normals(hipStream_t st, const MeshGraphArgs &a, void *sort_tmp, size_t sort_bytes, const float *p, float *normals)
{
    const int64_t n = 3 * (int64_t)a.T;
    hipLaunchKernelGGL(mesh_incidence_keys_kernel, dim3(blocks_of(n)), dim3(256), 0, st, a);
    LAUNCH_OK();
    if (int rc = mesh_sort_keys(sort_tmp, sort_bytes, a.keys, const_cast<uint64_t *>(a.sorted), n, mesh_key_bits(a.V), st)) return rc;
    hipLaunchKernelGGL(mesh_faces_kernel, dim3(blocks_of(a.T)), dim3(256), 0, st, a, p);
    LAUNCH_OK();
    hipLaunchKernelGGL(mesh_rows_kernel, dim3(blocks_of((int64_t)a.V + 1)), dim3(256), 0, st, a.sorted, n, (const int32_t *)nullptr, a.V, a.inc_start);
    LAUNCH_OK();
    hipLaunchKernelGGL(mesh_normals_kernel, dim3(blocks_of(a.V)), dim3(256), 0, st, a, normals);
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
