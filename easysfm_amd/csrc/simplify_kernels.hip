// Mesh simplification (include/esfm.h, "Mesh simplification"): vertex clustering on a regular grid with the representative placed
// by the cell's summed plane quadrics.  Cell keys -> sorted (key, vertex) pairs -> run heads -> cell numbers; the per-cell kernel
// walks its vertex run and its run of sorted (cell, 3 t + corner) keys in list order with f64 accumulators and solves the 3 x 3
// system; triangles on the same three cells vote by orientation over their sorted grouping keys; kept triangles and the cells
// they name are compacted in order.  Every float sum runs over a sorted list in list order inside one thread and there is no
// atomic, so the result does not depend on scheduling; tests/simplify_ref.py restates the rule and the output is compared bit
// for bit (-ffp-contract=off; HIP's default f32 / f64 division and f64 sqrt are correctly rounded).
#include <cmath>

#include "block_scan.hpp"
#include "simplify_kernels.hpp"

namespace esfm {

constexpr uint64_t kNoGroup = ~0ull;          // grouping key of a triangle that names a cell twice: behind every other key

// ---- cells -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void simplify_cell_keys_kernel(SimplifyArgs a)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= a.V) return;
    uint64_t key = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                 // (the host has checked 0 <= index <= 2^21 - 1 with this expression)
        const uint64_t i = (uint64_t)(int64_t)simplify_cell_coordinate(a.vertices[3 * v + c], a.origin[c], a.cell);
        key = key << 21 | (i & (uint64_t)kSimplifyMaxIndex);
    }
    a.key_in[v] = key;
    a.val_in[v] = (int32_t)v;
}

struct SimplifyIsCellHead {
    SimplifyArgs a;
    __device__ bool operator()(int64_t i) const { return i < a.V && (i == 0 || a.key_out[i - 1] != a.key_out[i]); }
};

// One thread per sorted vertex: the run heads up to and including it number its cell (position 0 is a head, so the number is
// never negative); a head also records where its run starts and its key, the last position closes the last run.
__global__ __launch_bounds__(256) void simplify_cell_numbers_kernel(SimplifyArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool head = SimplifyIsCellHead{a}(i);
    const int incl = block_inclusive_count(head);
    if (i >= a.V) return;
    const int32_t cell = a.cell_blocks[blockIdx.x] + incl - 1;
    a.cell_of[a.val_out[i]] = cell;
    if (head) { a.cell_start[cell] = (int32_t)i; a.cell_key[cell] = a.key_out[i]; }
    if (i == a.V - 1) a.cell_start[cell + 1] = a.V;
}

int launch_simplify_cell_keys(hipStream_t st, const SimplifyArgs &a)
{
    hipLaunchKernelGGL(simplify_cell_keys_kernel, dim3(blocks_of(a.V)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_simplify_cells(hipStream_t st, const SimplifyArgs &a)
{
    if (int rc = launch_flag_offsets(st, a.V, SimplifyIsCellHead{a}, a.cell_blocks)) return rc;
    hipLaunchKernelGGL(simplify_cell_numbers_kernel, dim3(blocks_of(a.V)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

// ---- per-cell sums and placement -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void simplify_corner_keys_kernel(SimplifyArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;       // 3 t + corner
    if (j >= 3 * (int64_t)a.T) return;
    a.key_in[j] = (uint64_t)a.cell_of[a.tri[j]] << 32 | (uint64_t)j;
}

// One thread per cell; a run is never split across lanes, the order is the rule.  All arithmetic is f64 in the header's order:
// twelve accumulators (three of the mean, six of A, three of b) and the elimination stay in registers.
__global__ __launch_bounds__(256) void simplify_place_kernel(SimplifyArgs a, const int32_t *n_cells)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= *n_cells) return;
    const uint64_t key = a.cell_key[c];
    const double cell = (double)a.cell;
    double cc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) cc[k] = (double)a.origin[k] + ((double)(int64_t)(key >> (21 * (2 - k)) & (uint64_t)kSimplifyMaxIndex) + 0.5) * cell;

    // the mean offset and the colour over the cell's vertices in ascending vertex index
    const int32_t i0 = a.cell_start[c], i1 = a.cell_start[c + 1];
    double s[3] = {0.0, 0.0, 0.0};
    uint64_t col[3] = {0, 0, 0};
    for (int32_t i = i0; i < i1; ++i) {
        const int64_t v = a.val_out[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = s[k] + ((double)a.vertices[3 * v + k] - cc[k]);
        if (a.rep_rgb) {
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] += a.rgb[3 * v + k];
        }
    }
    const double n = (double)(i1 - i0);
    const double m[3] = {s[0] / n, s[1] / n, s[2] / n};
    if (a.rep_rgb) {
        const uint64_t cnt = (uint64_t)(i1 - i0);
#pragma unroll
        for (int k = 0; k < 3; ++k) a.rep_rgb[3 * c + k] = (uint8_t)((2 * col[k] + cnt) / (2 * cnt));
    }

    // the area-weighted plane quadric about the cell centre over the cell's corners in ascending 3 t + corner
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    const int64_t n_keys = 3 * (int64_t)a.T;
    const int64_t j0 = lower_bound(a.key_out, n_keys, (uint64_t)c << 32), j1 = lower_bound(a.key_out, n_keys, (uint64_t)(c + 1) << 32);
    for (int64_t j = j0; j < j1; ++j) {
        const int64_t t = (int64_t)(a.key_out[j] & 0xFFFFFFFFull) / 3;
        const int64_t v0 = a.tri[3 * t], v1 = a.tri[3 * t + 1], v2 = a.tri[3 * t + 2];
        double p0[3], e1[3], e2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p0[k] = (double)a.vertices[3 * v0 + k];
            e1[k] = (double)a.vertices[3 * v1 + k] - p0[k];
            e2[k] = (double)a.vertices[3 * v2 + k] - p0[k];
        }
        const double N0 = e1[1] * e2[2] - e1[2] * e2[1], N1 = e1[2] * e2[0] - e1[0] * e2[2], N2 = e1[0] * e2[1] - e1[1] * e2[0];
        const double L = sqrt((N0 * N0 + N1 * N1) + N2 * N2);
        if (!(L > 0.0)) continue;
        const double D = -((N0 * (p0[0] - cc[0]) + N1 * (p0[1] - cc[1])) + N2 * (p0[2] - cc[2]));
        A00 = A00 + N0 * N0 / L; A01 = A01 + N0 * N1 / L; A02 = A02 + N0 * N2 / L;
        A11 = A11 + N1 * N1 / L; A12 = A12 + N1 * N2 / L; A22 = A22 + N2 * N2 / L;
        b0 = b0 + N0 * D / L; b1 = b1 + N1 * D / L; b2 = b2 + N2 * D / L;
    }

    // (A + r I) x = r m - b by LDL^T without pivoting
    double x[3] = {m[0], m[1], m[2]};
    const double tau = (A00 + A11) + A22;
    if (a.use_quadric && tau > 0.0) {
        const double r = (double)a.regularisation * tau;
        const double M00 = A00 + r, M11 = A11 + r, M22 = A22 + r;
        const double g0 = r * m[0] - b0, g1 = r * m[1] - b1, g2 = r * m[2] - b2;
        const double d0 = M00;
        const double l10 = A01 / d0, l20 = A02 / d0;
        const double d1 = M11 - l10 * A01;
        const double u = A12 - l20 * A01;
        const double l21 = u / d1;
        const double d2 = (M22 - l20 * A02) - l21 * u;
        const double y0 = g0;
        const double y1 = g1 - l10 * y0;
        const double y2 = (g2 - l20 * y0) - l21 * y1;
        const double x2 = y2 / d2;
        const double x1 = y1 / d1 - l21 * x2;
        const double x0 = (y0 / d0 - l10 * x1) - l20 * x2;
        if (fabs(x0) <= cell && fabs(x1) <= cell && fabs(x2) <= cell) { x[0] = x0; x[1] = x1; x[2] = x2; }   // (NaN and inf fail)
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) a.rep[3 * c + k] = (float)(cc[k] + x[k]);
}

int launch_simplify_corner_keys(hipStream_t st, const SimplifyArgs &a)
{
    hipLaunchKernelGGL(simplify_corner_keys_kernel, dim3(blocks_of(3 * (int64_t)a.T)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

// (the number of cells stays on the device: the grid covers V, threads beyond the count leave)
int launch_simplify_place(hipStream_t st, const SimplifyArgs &a)
{
    hipLaunchKernelGGL(simplify_place_kernel, dim3(blocks_of(a.V)), dim3(256), 0, st, a, (const int32_t *)(a.cell_blocks + blocks_of(a.V)));
    LAUNCH_OK();
    return ESFM_OK;
}

// ---- triangles -------------------------------------------------------------------------------------------------------------
// The grouping key of a triangle on three distinct cells is its sorted cell triple, 21 bits each (the caller refuses the result
// when a cell number needs more); the value is 2 t + (the rotation that puts the smallest cell first has its second cell above
// its third), so the stable sort keeps a group's triangles in ascending t with their orientation beside them.
__global__ __launch_bounds__(256) void simplify_group_keys_kernel(SimplifyArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    const uint64_t c0 = (uint64_t)a.cell_of[a.tri[3 * t]], c1 = (uint64_t)a.cell_of[a.tri[3 * t + 1]], c2 = (uint64_t)a.cell_of[a.tri[3 * t + 2]];
    uint64_t key = kNoGroup;
    int32_t odd = 0;
    if (c0 != c1 && c1 != c2 && c0 != c2) {
        uint64_t lo = c0, p = c1, q = c2;                            // (lo, p, q): the rotation with the smallest first
        if (c1 < c0 && c1 < c2) { lo = c1; p = c2; q = c0; }
        else if (c2 < c0 && c2 < c1) { lo = c2; p = c0; q = c1; }
        odd = p > q;
        key = lo << 42 | (odd ? q : p) << 21 | (odd ? p : q);
    }
    a.key_in[t] = key;
    a.val_in[t] = (int32_t)(2 * t) | odd;
}

// One thread per run head of the sorted grouping keys: the majority orientation's first triangle stays, a tie keeps nothing.
__global__ __launch_bounds__(256) void simplify_vote_kernel(SimplifyArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.T) return;
    const uint64_t key = a.key_out[i];
    if (key == kNoGroup || (i > 0 && a.key_out[i - 1] == key)) return;
    int32_t count[2] = {0, 0}, first[2] = {-1, -1};
    for (int64_t j = i; j < a.T && a.key_out[j] == key; ++j) {
        const int32_t val = a.val_out[j], o = val & 1;
        if (count[o]++ == 0) first[o] = val >> 1;
    }
    if (count[0] == count[1]) return;
    const int64_t t = first[count[1] > count[0] ? 1 : 0];
    a.keep[t] = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.used[a.cell_of[a.tri[3 * t + k]]] = 1;   // (several threads may store the same 1)
}

int launch_simplify_group_keys(hipStream_t st, const SimplifyArgs &a)
{
    hipLaunchKernelGGL(simplify_group_keys_kernel, dim3(blocks_of(a.T)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_simplify_vote(hipStream_t st, const SimplifyArgs &a)
{
    ESFM_HIP_TRY(hipMemsetAsync(a.keep, 0, (size_t)a.T, st));
    ESFM_HIP_TRY(hipMemsetAsync(a.used, 0, (size_t)a.V, st));
    hipLaunchKernelGGL(simplify_vote_kernel, dim3(blocks_of(a.T)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

// ---- ordered compaction ------------------------------------------------------------------------------------------------------
// (used[] is zero from the cell count on, so the cell kernels run over V without knowing the count)
struct SimplifyCellUsed {
    SimplifyArgs a;
    __device__ bool operator()(int64_t c) const { return c < a.V && a.used[c]; }
};
struct SimplifyTriangleKept {
    SimplifyArgs a;
    __device__ bool operator()(int64_t t) const { return t < a.T && a.keep[t]; }
};

__global__ __launch_bounds__(256) void simplify_write_vertices_kernel(SimplifyArgs a)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = SimplifyCellUsed{a}(c);
    const int incl = block_inclusive_count(keep);
    if (!keep) return;
    const int64_t dst = (int64_t)a.used_blocks[blockIdx.x] + incl - 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out_vertices[3 * dst + k] = a.rep[3 * c + k];
    if (a.out_rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.out_rgb[3 * dst + k] = a.rep_rgb[3 * c + k];
    }
    a.new_of_cell[c] = (int32_t)dst;
}

// (a kept triangle's three cells are used: all three have an output vertex)
__global__ __launch_bounds__(256) void simplify_write_triangles_kernel(SimplifyArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = SimplifyTriangleKept{a}(t);
    const int incl = block_inclusive_count(keep);
    if (!keep) return;
    const int64_t dst = (int64_t)a.tri_blocks[blockIdx.x] + incl - 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out_tri[3 * dst + k] = a.new_of_cell[a.cell_of[a.tri[3 * t + k]]];
    if (a.triangle_map) a.triangle_map[dst] = (int32_t)t;
}

__global__ __launch_bounds__(256) void simplify_vertex_map_kernel(SimplifyArgs a)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= a.V) return;
    const int32_t c = a.cell_of[v];
    a.vertex_map[v] = a.used[c] ? a.new_of_cell[c] : -1;
}

int launch_simplify_compact(hipStream_t st, const SimplifyArgs &a)
{
    const unsigned vb = blocks_of(a.V), tb = blocks_of(a.T);
    if (int rc = launch_flag_offsets(st, a.V, SimplifyCellUsed{a}, a.used_blocks)) return rc;
    if (int rc = launch_flag_offsets(st, a.T, SimplifyTriangleKept{a}, a.tri_blocks)) return rc;
    hipLaunchKernelGGL(simplify_write_vertices_kernel, dim3(vb), dim3(256), 0, st, a);
    LAUNCH_OK();
    hipLaunchKernelGGL(simplify_write_triangles_kernel, dim3(tb), dim3(256), 0, st, a);
    LAUNCH_OK();
    if (a.vertex_map) {
        hipLaunchKernelGGL(simplify_vertex_map_kernel, dim3(vb), dim3(256), 0, st, a);
        LAUNCH_OK();
    }
    return ESFM_OK;
}

}  // namespace esfm
