// Surface reconstruction (include/esfm.h, "Surface reconstruction"): depth maps into a truncated signed distance volume, and an
// indexed triangle mesh out of it by marching tetrahedra on the Kuhn decomposition.  One thread owns one voxel in every kernel
// and every ordering is by linear index, so nothing depends on scheduling; tests/tsdf_ref.py restates the rules and the output
// is compared bit for bit (-ffp-contract=off; HIP's default f32 division and sqrtf are correctly rounded).
#include <cmath>

#include "block_scan.hpp"
#include "tsdf_kernels.hpp"

namespace esfm {

__device__ inline void tsdf_voxel_of(const TsdfVolume &g, int idx, int &i, int &j, int &k)
{
    const int row = idx / g.nx;
    i = idx - row * g.nx;
    k = row / g.ny;
    j = row - k * g.ny;
}

__device__ inline float tsdf_centre(const TsdfVolume &g, int axis, int i) { return g.origin[axis] + ((float)i + 0.5f) * g.h; }

// ---- integration ---------------------------------------------------------------------------------------------------------
// One thread per voxel, x fastest across lanes (neighbouring lanes gather neighbouring depth pixels); the view loop runs inside
// the thread in view order, the cameras of all views sit in LDS (every lane reads the same word: a broadcast).
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(TsdfIntegrateArgs a)
{
    __shared__ TsdfCam s_cam[kTsdfMaxViews];
    {
        const int32_t *src = reinterpret_cast<const int32_t *>(a.cams);
        int32_t *dst = reinterpret_cast<int32_t *>(s_cam);
        const int words = a.n_cams * (int)(sizeof(TsdfCam) / sizeof(int32_t));
        for (int w = threadIdx.x; w < words; w += 256) dst[w] = src[w];
    }
    __syncthreads();
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    if (idx >= a.vol.n) return;
    int i, j, k;
    tsdf_voxel_of(a.vol, idx, i, j, k);
    const float X0 = tsdf_centre(a.vol, 0, i), X1 = tsdf_centre(a.vol, 1, j), X2 = tsdf_centre(a.vol, 2, k);
    const int64_t plane = (int64_t)a.rows * a.cols;
    float S = 0.f;
    int32_t W = 0, Wc = 0, sum[3] = {0, 0, 0};
    for (int v = 0; v < a.n_cams; ++v) {
        const TsdfCam &c = s_cam[v];
        const float p2 = ((c.P[8] * X0 + c.P[9] * X1) + c.P[10] * X2) + c.P[11];
        if (!(p2 > 0.f)) continue;
        const float p0 = ((c.P[0] * X0 + c.P[1] * X1) + c.P[2] * X2) + c.P[3];
        const float p1 = ((c.P[4] * X0 + c.P[5] * X1) + c.P[6] * X2) + c.P[7];
        const float u = c.K[0] * (p0 / p2) + c.K[1], w = c.K[2] * (p1 / p2) + c.K[3];
        const float px = floorf(u + 0.5f), py = floorf(w + 0.5f);
        if (!(px >= 0.f && px < (float)a.cols && py >= 0.f && py < (float)a.rows)) continue;
        const int64_t pix = (int64_t)c.view * plane + (int64_t)(int)py * a.cols + (int)px;
        const float d = a.depth[pix];
        if (!(d > 0.f)) continue;
        const float s = d - p2;
        if (s < -a.trunc) continue;
        S += fminf(1.0f, s / a.trunc);
        ++W;
        if (a.images && s <= a.trunc) {
            const uint8_t *q = a.images + pix * a.channels;
            if (a.channels == 3) { sum[0] += q[2]; sum[1] += q[1]; sum[2] += q[0]; }
            else { sum[0] += q[0]; sum[1] += q[0]; sum[2] += q[0]; }
            ++Wc;
        }
    }
    a.vol.tsdf[idx] = W > 0 ? S / (float)W : 1.0f;
    a.vol.weight[idx] = W;
    if (a.vol.rgb) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a.vol.rgb[3 * (int64_t)idx + ch] = Wc > 0 ? (uint8_t)((sum[ch] + Wc / 2) / Wc) : (uint8_t)0;
    }
}

// ---- the tetrahedron table -----------------------------------------------------------------------------------------------
// Corner c of a cell is the voxel at offset (c & 1, c >> 1 & 1, c >> 2).  Tetrahedron t of the Kuhn decomposition, one per
// permutation (a, b, c) of the axes in lexicographic order, has the ordered corners 0, e_a, e_a + e_b, 7.  For every inside mask
// of its four corners (bit l = local corner l inside): the triangles, each as three edges lo | hi << 2 of local corners lo < hi,
// wound by the header's integer rule so that (v1 - v0) x (v2 - v0) points to the outside.
struct TetTable {
    uint8_t corner[6][4];
    uint8_t n_tri[6][16];
    uint8_t edge[6][16][6];
};

constexpr TetTable make_tet_table()
{
    TetTable T{};
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int t = 0; t < 6; ++t) {
        const int q[4] = {0, 1 << perm[t][0], (1 << perm[t][0]) | (1 << perm[t][1]), 7};
        for (int l = 0; l < 4; ++l) T.corner[t][l] = (uint8_t)q[l];
        for (int m = 1; m < 15; ++m) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, n_in = 0, n_out = 0;
            int s_in[3] = {0, 0, 0}, s_out[3] = {0, 0, 0};
            for (int l = 0; l < 4; ++l) {
                const bool inside = (m >> l) & 1;
                if (inside) in[n_in++] = l; else out[n_out++] = l;
                for (int x = 0; x < 3; ++x) (inside ? s_in : s_out)[x] += (q[l] >> x) & 1;
            }
            int tri[2][3][2] = {};
            int n_tri = 1;
            if (n_in == 2) {                                   // a < b inside, c < d outside: (ac, ad, bd), (ac, bd, bc)
                const int A = in[0], B = in[1], Cc = out[0], D = out[1];
                const int first[3][2] = {{A, Cc}, {A, D}, {B, D}}, second[3][2] = {{A, Cc}, {B, D}, {B, Cc}};
                for (int e = 0; e < 3; ++e)
                    for (int x = 0; x < 2; ++x) { tri[0][e][x] = first[e][x]; tri[1][e][x] = second[e][x]; }
                n_tri = 2;
            } else {                                           // a alone on its side, the others b < c < d: (ab, ac, ad)
                const int A = n_in == 1 ? in[0] : out[0];
                const int *rest = n_in == 1 ? out : in;
                for (int e = 0; e < 3; ++e) { tri[0][e][0] = A; tri[0][e][1] = rest[e]; }
            }
            int s[3] = {0, 0, 0};
            for (int x = 0; x < 3; ++x) s[x] = n_in * s_out[x] - n_out * s_in[x];
            T.n_tri[t][m] = (uint8_t)n_tri;
            for (int r = 0; r < n_tri; ++r) {
                int mid[3][3] = {};
                for (int e = 0; e < 3; ++e)
                    for (int x = 0; x < 3; ++x) mid[e][x] = ((q[tri[r][e][0]] >> x) & 1) + ((q[tri[r][e][1]] >> x) & 1);
                int u[3] = {0, 0, 0}, w[3] = {0, 0, 0};
                for (int x = 0; x < 3; ++x) { u[x] = mid[1][x] - mid[0][x]; w[x] = mid[2][x] - mid[0][x]; }
                const int n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
                const bool swap = n[0] * s[0] + n[1] * s[1] + n[2] * s[2] < 0;
                for (int e = 0; e < 3; ++e) {
                    const int from = e == 0 ? 0 : (swap ? 3 - e : e);
                    const int c0 = tri[r][from][0], c1 = tri[r][from][1];
                    const int lo = c0 < c1 ? c0 : c1, hi = c0 < c1 ? c1 : c0;
                    T.edge[t][m][3 * r + e] = (uint8_t)(lo | hi << 2);
                }
            }
        }
    }
    return T;
}

__constant__ TetTable kTet = make_tet_table();

// ---- classification ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_state_kernel(TsdfExtractArgs a)
{
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    if (idx >= a.vol.n) return;
    const bool valid = a.vol.weight[idx] >= a.min_weight;
    a.state[idx] = (uint8_t)((valid ? 1 : 0) | (valid && a.vol.tsdf[idx] < 0.f ? 2 : 0));
}

// bits of the 27-neighbourhood validity word (bit (dz + 1) 9 + (dy + 1) 3 + dx + 1) that are the corners of the cell whose
// origin is the voxel plus (ox, oy, oz), each in {-1, 0}
constexpr uint32_t tsdf_cell_bits(int ox, int oy, int oz)
{
    uint32_t m = 0;
    for (int d = 0; d < 8; ++d) m |= 1u << ((oz + (d >> 2 & 1) + 1) * 9 + (oy + (d >> 1 & 1) + 1) * 3 + (ox + (d & 1) + 1));
    return m;
}

// The sum of `v` over the 256 threads of the workgroup, in thread 0 (every thread calls; v < 2^23).
__device__ inline int block_sum_to_zero(int v)
{
    __shared__ int32_t per_wave[4];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) per_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return per_wave[0] + per_wave[1] + per_wave[2] + per_wave[3];
}

// The sum of `v` over the threads of the 256-thread workgroup below this one (every thread calls).
__device__ inline int block_exclusive_sum(int v)
{
    __shared__ int32_t per_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) per_wave[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += per_wave[w];
    return before + incl - v;
}

// Per voxel: the used-edge mask of the 7 edges it owns and the triangle count of the cell it is the origin of; per 256-voxel
// block their sums.  An edge v -> v + delta is used if exactly one end is inside and a cell that holds both ends is live: a
// gather over the 27 neighbours' state bytes.
__global__ __launch_bounds__(256) void tsdf_classify_kernel(TsdfExtractArgs a)
{
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    int n_vert = 0, n_tri = 0;
    if (idx < a.vol.n) {
        int i, j, k;
        tsdf_voxel_of(a.vol, idx, i, j, k);
        uint32_t valid = 0, inside = 0;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int x = i + dx, y = j + dy, z = k + dz;
                    if (x < 0 || x >= a.vol.nx || y < 0 || y >= a.vol.ny || z < 0 || z >= a.vol.nz) continue;
                    const uint32_t s = a.state[idx + (dz * a.vol.ny + dy) * a.vol.nx + dx];
                    if (s & 1) valid |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1);
                    if (dx >= 0 && dy >= 0 && dz >= 0 && (s & 2)) inside |= 1u << (dx | dy << 1 | dz << 2);
                }
        uint32_t live = 0;                                     // bit (ox + 1) | (oy + 1) << 1 | (oz + 1) << 2
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t need = tsdf_cell_bits((c & 1) - 1, (c >> 1 & 1) - 1, (c >> 2 & 1) - 1);
            if ((valid & need) == need) live |= 1u << c;
        }
        uint32_t mask = 0;
#pragma unroll
        for (int delta = 1; delta < 8; ++delta) {
            uint32_t cells = 0;                                // the cells that hold both ends: offset 0 along every axis of delta
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if ((c & delta) == delta) cells |= 1u << c;
            if (((inside ^ (inside >> delta)) & 1) && (live & cells)) mask |= 1u << (delta - 1);
        }
        if (live & 0x80u) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                uint32_t m = 0;
#pragma unroll
                for (int l = 0; l < 4; ++l) m |= ((inside >> kTet.corner[t][l]) & 1) << l;
                n_tri += kTet.n_tri[t][m];
            }
        }
        n_vert = __popc(mask);
        a.edge_mask[idx] = (uint8_t)mask;
        a.tri_count[idx] = (uint8_t)n_tri;
    }
    const int both = block_sum_to_zero(n_vert | n_tri << 12);  // (at most 256 x 7 vertices: below 2^12)
    if (threadIdx.x == 0) { a.block_vertices[blockIdx.x] = both & 0xFFF; a.block_triangles[blockIdx.x] = both >> 12; }
}

// ---- vertices ------------------------------------------------------------------------------------------------------------
__device__ inline void tsdf_gradient(const TsdfExtractArgs &a, int idx, int i, int j, int k, float g[3])
{
    const int at[3] = {i, j, k}, dim[3] = {a.vol.nx, a.vol.ny, a.vol.nz}, step[3] = {1, a.vol.nx, a.vol.nx * a.vol.ny};
    const float f = a.vol.tsdf[idx];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const bool lo = at[x] > 0 && (a.state[idx - step[x]] & 1), hi = at[x] + 1 < dim[x] && (a.state[idx + step[x]] & 1);
        const float fm = lo ? a.vol.tsdf[idx - step[x]] : 0.f, fp = hi ? a.vol.tsdf[idx + step[x]] : 0.f;
        g[x] = lo && hi ? 0.5f * (fp - fm) : hi ? fp - f : lo ? f - fm : 0.f;
    }
}

// One vertex per used edge, numbered by (owner, e): the block's offset plus the used edges of the voxels before this one.
__global__ __launch_bounds__(256) void tsdf_vertices_kernel(TsdfExtractArgs a)
{
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    const uint32_t mask = idx < a.vol.n ? a.edge_mask[idx] : 0u;
    const int first = a.block_vertices[blockIdx.x] + block_exclusive_sum(__popc(mask));
    if (idx >= a.vol.n) return;
    a.vertex_base[idx] = first;
    if (!mask) return;
    int i, j, k;
    tsdf_voxel_of(a.vol, idx, i, j, k);
    const float Xa[3] = {tsdf_centre(a.vol, 0, i), tsdf_centre(a.vol, 1, j), tsdf_centre(a.vol, 2, k)};
    const float fa = a.vol.tsdf[idx];
    float ga[3];
    if (a.normals) tsdf_gradient(a, idx, i, j, k, ga);
    int64_t dst = first;
    for (int e = 0; e < 7; ++e) {
        if (!((mask >> e) & 1)) continue;
        const int dx = (e + 1) & 1, dy = (e + 1) >> 1 & 1, dz = (e + 1) >> 2;
        const int other = idx + (dz * a.vol.ny + dy) * a.vol.nx + dx;      // in the grid: a live cell holds both ends
        const float fb = a.vol.tsdf[other];
        const float tt = fa / (fa - fb);
        a.vertices[3 * dst] = Xa[0] + tt * ((float)dx * a.vol.h);
        a.vertices[3 * dst + 1] = Xa[1] + tt * ((float)dy * a.vol.h);
        a.vertices[3 * dst + 2] = Xa[2] + tt * ((float)dz * a.vol.h);
        if (a.vertex_rgb) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float ca = (float)a.vol.rgb[3 * (int64_t)idx + ch], cb = (float)a.vol.rgb[3 * (int64_t)other + ch];
                a.vertex_rgb[3 * dst + ch] = (uint8_t)floorf((ca + tt * (cb - ca)) + 0.5f);
            }
        }
        if (a.normals) {
            float gb[3], g[3];
            tsdf_gradient(a, other, i + dx, j + dy, k + dz, gb);
#pragma unroll
            for (int x = 0; x < 3; ++x) g[x] = ga[x] + tt * (gb[x] - ga[x]);
            const float L = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
            const bool ok = L > 0.f && isfinite(L);
#pragma unroll
            for (int x = 0; x < 3; ++x) a.normals[3 * dst + x] = ok ? g[x] / L : 0.f;
        }
        ++dst;
    }
}

// ---- triangles -----------------------------------------------------------------------------------------------------------
// By cell, tetrahedron and the table's order; a vertex id is the owner's base plus its used edges below this one.
__global__ __launch_bounds__(256) void tsdf_triangles_kernel(TsdfExtractArgs a)
{
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    const int count = idx < a.vol.n ? a.tri_count[idx] : 0;
    int64_t dst = a.block_triangles[blockIdx.x] + block_exclusive_sum(count);
    if (!count) return;
    int at[8];                                                 // (count > 0: the cell is live, its eight corners are in the grid)
    uint32_t inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        at[c] = idx + ((c >> 2) * a.vol.ny + (c >> 1 & 1)) * a.vol.nx + (c & 1);
        inside |= (uint32_t)(a.state[at[c]] >> 1 & 1) << c;
    }
    for (int t = 0; t < 6; ++t) {
        uint32_t m = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l) m |= ((inside >> kTet.corner[t][l]) & 1) << l;
        const int n = kTet.n_tri[t][m];
        for (int e = 0; e < 3 * n; ++e) {
            const int code = kTet.edge[t][m][e];
            const int lo = kTet.corner[t][code & 3], hi = kTet.corner[t][code >> 2];
            const int owner = at[lo], dir = (hi - lo) - 1;    // (the corners ascend bitwise: hi - lo is the offset delta)
            a.triangles[3 * dst + e] = a.vertex_base[owner] + __popc(a.edge_mask[owner] & ((1u << dir) - 1u));
        }
        dst += n;
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
int launch_tsdf_integrate(hipStream_t st, const TsdfIntegrateArgs &a)
{
    if (a.n_cams < 0 || a.n_cams > kTsdfMaxViews) { set_error("%d views to integrate", a.n_cams); return ESFM_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((a.vol.n + 255) / 256)), dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

int launch_tsdf_classify(hipStream_t st, const TsdfExtractArgs &a)
{
    const dim3 grid((unsigned)a.n_blocks);
    hipLaunchKernelGGL(tsdf_state_kernel, grid, dim3(256), 0, st, a);
    LAUNCH_OK();
    hipLaunchKernelGGL(tsdf_classify_kernel, grid, dim3(256), 0, st, a);
    LAUNCH_OK();
    if (int rc = launch_block_offsets_scan(st, a.block_vertices, a.n_blocks, a.block_vertices + a.n_blocks)) return rc;
    return launch_block_offsets_scan(st, a.block_triangles, a.n_blocks, a.block_triangles + a.n_blocks);
}

int launch_tsdf_mesh(hipStream_t st, const TsdfExtractArgs &a)
{
    const dim3 grid((unsigned)a.n_blocks);
    hipLaunchKernelGGL(tsdf_vertices_kernel, grid, dim3(256), 0, st, a);
    LAUNCH_OK();
    hipLaunchKernelGGL(tsdf_triangles_kernel, grid, dim3(256), 0, st, a);
    LAUNCH_OK();
    return ESFM_OK;
}

}  // namespace esfm
