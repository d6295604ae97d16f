// C-ABI entry points of the mesh simplification (include/esfm.h, "Mesh simplification"): esfm_mesh_simplify.  Host side: the
// argument checks on the caller's arrays and the scratch layout (simplify_check.hpp), uploads, launches, the one read-back of the
// three counts, the normals through the clean-up's launchers, and the copy of the mesh.  The work runs in simplify_kernels.hip;
// tests/simplify_ref.py restates the rule.
#include "mesh_kernels.hpp"
#include "simplify_kernels.hpp"
#include "voxel_kernels.hpp"   // voxel_sort_pairs

extern "C" {

void esfm_mesh_simplify_options_default(esfm_mesh_simplify_options *opt)
{
    if (!opt) return;
    opt->regularisation = 1e-3f;
    opt->use_quadric = 1;
}

int esfm_mesh_simplify(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices, const uint8_t *vertex_rgb, const int32_t *triangles,
                       const float *origin, float cell, const esfm_mesh_simplify_options *opt, float *out_vertices, float *out_normals,
                       uint8_t *out_rgb, int32_t *out_triangles, int32_t *vertex_map, int32_t *triangle_map, int32_t *n_out_vertices,
                       int32_t *n_out_triangles)
{
    if (int rc = esfm::simplify_check_args(n_vertices, n_triangles, vertices, vertex_rgb, triangles, origin, cell, opt, out_vertices, out_rgb,
                                           out_triangles, n_out_vertices, n_out_triangles)) return rc;
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(ctx)) return rc;
    if (n_vertices == 0 || n_triangles == 0) {
        *n_out_vertices = 0; *n_out_triangles = 0;
        if (vertex_map) for (int v = 0; v < n_vertices; ++v) vertex_map[v] = -1;
        return ESFM_OK;
    }
    hipStream_t st = ctx->stream;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, vb = (V + 255) / 256, tb = (T + 255) / 256;

    // the corner keys' high word is a cell number below V; the pair sorts run over all 64 bits (voxel_sort.hip's entry point)
    const int corner_bits = esfm::mesh_key_bits(n_vertices);
    size_t pair_b = 0, corner_b = 0;
    if (int rc = esfm::voxel_sort_scratch_bytes((int)(V > T ? V : T), &pair_b, st)) return rc;
    if (int rc = esfm::mesh_sort_scratch_bytes(3 * (int64_t)T, corner_bits, &corner_b, st)) return rc;
    const size_t sort_b = pair_b > corner_b ? pair_b : corner_b;
    const esfm::SimplifyLayout l = esfm::simplify_layout(V, T, out_rgb != nullptr, out_normals != nullptr, vertex_map != nullptr, triangle_map != nullptr, sort_b);
    if (int rc = ctx->stage_a.reserve(l.a_bytes)) return rc;
    if (int rc = ctx->stage_b.reserve(l.b_bytes)) return rc;
    if (int rc = ctx->stage_c.reserve(l.c_bytes)) return rc;
    if (int rc = ctx->stage_d.reserve(l.d_bytes)) return rc;
    uint8_t *p_a = ctx->stage_a.as<uint8_t>(), *p_b = ctx->stage_b.as<uint8_t>(), *p_c = ctx->stage_c.as<uint8_t>(), *p_d = ctx->stage_d.as<uint8_t>();
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.vertices, vertices, sizeof(float) * 3 * V, st));
    if (out_rgb) ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.rgb, vertex_rgb, 3 * V, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.tri, triangles, sizeof(int32_t) * 3 * T, st));

    esfm::SimplifyArgs a;
    memset(&a, 0, sizeof(a));
    a.vertices = reinterpret_cast<const float *>(p_a + l.vertices);
    a.rgb = out_rgb ? p_a + l.rgb : nullptr;
    a.tri = reinterpret_cast<const int32_t *>(p_a + l.tri);
    a.V = n_vertices; a.T = n_triangles;
    a.origin[0] = origin[0]; a.origin[1] = origin[1]; a.origin[2] = origin[2];
    a.cell = cell; a.regularisation = opt->regularisation; a.use_quadric = opt->use_quadric;
    uint64_t *key_in = reinterpret_cast<uint64_t *>(p_b + l.key_in), *key_out = reinterpret_cast<uint64_t *>(p_b + l.key_out);
    int32_t *val_in = reinterpret_cast<int32_t *>(p_b + l.val_in), *val_out = reinterpret_cast<int32_t *>(p_b + l.val_out);
    void *d_sort = p_b + l.sort;
    a.key_in = key_in; a.key_out = key_out; a.val_in = val_in; a.val_out = val_out;
    a.cell_blocks = reinterpret_cast<int32_t *>(p_a + l.cell_blocks);
    a.cell_of = reinterpret_cast<int32_t *>(p_a + l.cell_of);
    a.cell_start = reinterpret_cast<int32_t *>(p_a + l.cell_start);
    a.cell_key = reinterpret_cast<uint64_t *>(p_a + l.cell_key);
    a.rep = reinterpret_cast<float *>(p_a + l.rep);
    a.rep_rgb = out_rgb ? p_a + l.rep_rgb : nullptr;
    a.keep = p_a + l.keep;
    a.used = p_a + l.used;
    a.used_blocks = reinterpret_cast<int32_t *>(p_a + l.used_blocks);
    a.tri_blocks = reinterpret_cast<int32_t *>(p_a + l.tri_blocks);
    a.new_of_cell = reinterpret_cast<int32_t *>(p_a + l.new_of_cell);
    a.out_vertices = reinterpret_cast<float *>(p_d + l.out_vertices);
    a.out_rgb = out_rgb ? p_d + l.out_rgb : nullptr;
    a.out_tri = reinterpret_cast<int32_t *>(p_d + l.out_tri);
    a.vertex_map = vertex_map ? reinterpret_cast<int32_t *>(p_d + l.vertex_map) : nullptr;
    a.triangle_map = triangle_map ? reinterpret_cast<int32_t *>(p_d + l.triangle_map) : nullptr;

    if (int rc = esfm::launch_simplify_cell_keys(st, a)) return rc;
    if (int rc = esfm::voxel_sort_pairs(d_sort, sort_b, key_in, key_out, val_in, val_out, n_vertices, st)) return rc;
    if (int rc = esfm::launch_simplify_cells(st, a)) return rc;
    if (int rc = esfm::launch_simplify_corner_keys(st, a)) return rc;
    if (int rc = esfm::mesh_sort_keys(d_sort, sort_b, key_in, key_out, 3 * (int64_t)T, corner_bits, st)) return rc;
    if (int rc = esfm::launch_simplify_place(st, a)) return rc;
    if (int rc = esfm::launch_simplify_group_keys(st, a)) return rc;
    if (int rc = esfm::voxel_sort_pairs(d_sort, sort_b, key_in, key_out, val_in, val_out, n_triangles, st)) return rc;
    if (int rc = esfm::launch_simplify_vote(st, a)) return rc;
    if (int rc = esfm::launch_simplify_compact(st, a)) return rc;

    int32_t nc = 0, nv = 0, nt = 0;
    ESFM_HIP_TRY(esfm::copy_d2h(&nc, a.cell_blocks + vb, sizeof(int32_t), st));
    ESFM_HIP_TRY(esfm::copy_d2h(&nv, a.used_blocks + vb, sizeof(int32_t), st));
    ESFM_HIP_TRY(esfm::copy_d2h(&nt, a.tri_blocks + tb, sizeof(int32_t), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    if (nc > esfm::kSimplifyMaxCells) {     // (the grouping keys were cut to 21 bits per cell number: nothing of this run is handed out)
        esfm::set_error("mesh simplify: %d cells are occupied, the grouping key holds 2^21; use a larger cell", nc);
        return ESFM_ERR_UNSUPPORTED;
    }
    if (nc < 1 || nv < 0 || nv > nc || nt < 0 || nt > n_triangles || (nv == 0) != (nt == 0)) {
        esfm::set_error("mesh simplify: %d cells, %d of them and %d of %d triangles kept", nc, nv, nt, n_triangles);
        return ESFM_ERR_NUMERIC;
    }
    const size_t Vo = (size_t)nv, To = (size_t)nt;
    float *d_normals = reinterpret_cast<float *>(p_d + l.out_normals);
    if (out_normals && nt > 0) {
        esfm::MeshGraphArgs g;
        memset(&g, 0, sizeof(g));
        g.tri = a.out_tri; g.V = nv; g.T = nt;
        g.keys = key_in; g.sorted = key_out;
        g.inc_start = reinterpret_cast<int32_t *>(p_c + l.inc_start);
        g.face = reinterpret_cast<float *>(p_c + l.face);
        if (int rc = esfm::mesh_build_normals(st, g, d_sort, sort_b, a.out_vertices, d_normals)) return rc;
    }
    if (nt > 0) {
        ESFM_HIP_TRY(esfm::copy_d2h(out_vertices, a.out_vertices, sizeof(float) * 3 * Vo, st));
        if (out_normals) ESFM_HIP_TRY(esfm::copy_d2h(out_normals, d_normals, sizeof(float) * 3 * Vo, st));
        if (out_rgb) ESFM_HIP_TRY(esfm::copy_d2h(out_rgb, a.out_rgb, 3 * Vo, st));
        ESFM_HIP_TRY(esfm::copy_d2h(out_triangles, a.out_tri, sizeof(int32_t) * 3 * To, st));
        if (triangle_map) ESFM_HIP_TRY(esfm::copy_d2h(triangle_map, a.triangle_map, sizeof(int32_t) * To, st));
    }
    if (vertex_map) ESFM_HIP_TRY(esfm::copy_d2h(vertex_map, a.vertex_map, sizeof(int32_t) * V, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    *n_out_vertices = nv; *n_out_triangles = nt;
    return ESFM_OK;
}

}  // extern "C"
