// C-ABI entry points of the mesh clean-up (include/esfm.h, "Mesh clean-up"): esfm_mesh_components and esfm_mesh_clean.  Host
// side: argument checks (the triangle indices on the caller's copy), buffer layout, uploads, launches, the one read-back of the
// two kept counts, and the copy of the mesh.  The work runs in mesh_kernels.hip, the two sorts in mesh_sort.hip;
// tests/mesh_clean_ref.py restates the rules.
#include <cmath>

#include "mesh_kernels.hpp"

namespace {

size_t al(size_t b) { return (b + 255) / 256 * 256; }

int check_mesh(int V, int T, const int32_t *triangles)
{
    ESFM_REQUIRE(V >= 0 && V <= (1 << 30), "n_vertices must be 0..2^30");
    ESFM_REQUIRE(T >= 0 && T <= (1 << 28), "n_triangles must be 0..2^28");
    ESFM_REQUIRE(T == 0 || triangles, "NULL argument");
    for (size_t i = 0; i < 3 * (size_t)T; ++i) ESFM_REQUIRE(triangles[i] >= 0 && triangles[i] < V, "a triangle index is outside 0..n_vertices-1");
    return ESFM_OK;
}

int check_options(const esfm_mesh_clean_options *o)
{
    ESFM_REQUIRE(o, "options are NULL");
    ESFM_REQUIRE(o->min_component_triangles >= 1, "min_component_triangles must be >= 1");
    ESFM_REQUIRE(o->min_component_permille >= 0 && o->min_component_permille <= 1000, "min_component_permille must be 0..1000");
    ESFM_REQUIRE(o->smooth_iterations >= 0 && o->smooth_iterations <= 1000, "smooth_iterations must be 0..1000");
    ESFM_REQUIRE(std::isfinite(o->smooth_lambda) && o->smooth_lambda > 0.f && o->smooth_lambda <= 1.f, "smooth_lambda must be finite and in (0, 1]");
    ESFM_REQUIRE(std::isfinite(o->smooth_mu) && o->smooth_mu >= -1.5f && o->smooth_mu <= 0.f, "smooth_mu must be finite and in [-1.5, 0]");
    ESFM_REQUIRE(o->pin_boundary == 0 || o->pin_boundary == 1, "pin_boundary must be 0 or 1");
    return ESFM_OK;
}

int check_ctx(esfm_ctx *ctx)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    return esfm::set_device(ctx);
}

int bit_width(uint32_t x) { int n = 0; while (x) { ++n; x >>= 1; } return n; }

// the labelling's device arrays behind `head` bytes of stage_a: triangles | parent | label | tri_count | stats
int place_labels(esfm_ctx *ctx, size_t head, size_t tail, int V, int T, const int32_t *triangles, esfm::MeshLabelArgs *a)
{
    const size_t tri_b = al(sizeof(int32_t) * 3 * (size_t)T), v_b = al(sizeof(int32_t) * (size_t)V);
    if (int rc = ctx->stage_a.reserve(head + tri_b + 3 * v_b + 256 + tail)) return rc;
    uint8_t *p = ctx->stage_a.as<uint8_t>() + head;
    a->tri = reinterpret_cast<const int32_t *>(p);
    a->parent = reinterpret_cast<int32_t *>(p + tri_b);
    a->label = reinterpret_cast<int32_t *>(p + tri_b + v_b);
    a->tri_count = reinterpret_cast<int32_t *>(p + tri_b + 2 * v_b);
    a->stats = reinterpret_cast<int32_t *>(p + tri_b + 3 * v_b);
    a->V = V; a->T = T;
    if (T) ESFM_HIP_TRY(esfm::copy_h2d(p, triangles, sizeof(int32_t) * 3 * (size_t)T, ctx->stream));
    return ESFM_OK;
}

}  // namespace

extern "C" {

void esfm_mesh_clean_options_default(esfm_mesh_clean_options *opt)
{
    if (!opt) return;
    opt->min_component_triangles = 64;
    opt->min_component_permille = 10;
    opt->smooth_iterations = 5;
    opt->smooth_lambda = 0.5f;
    opt->smooth_mu = -0.53f;
    opt->pin_boundary = 1;
}

int esfm_mesh_components(esfm_ctx *ctx, int n_vertices, int n_triangles, const int32_t *triangles, int32_t *labels, int32_t *tri_count,
                         int32_t *n_components)
{
    if (int rc = check_mesh(n_vertices, n_triangles, triangles)) return rc;
    ESFM_REQUIRE(n_components && (n_vertices == 0 || labels), "NULL argument");
    if (int rc = check_ctx(ctx)) return rc;
    if (n_vertices == 0) { *n_components = 0; return ESFM_OK; }
    hipStream_t st = ctx->stream;
    esfm::MeshLabelArgs a;
    if (int rc = place_labels(ctx, 0, 0, n_vertices, n_triangles, triangles, &a)) return rc;
    if (int rc = esfm::launch_mesh_labels(st, a)) return rc;
    const size_t V = (size_t)n_vertices;
    int32_t stats[2] = {0, 0};
    ESFM_HIP_TRY(esfm::copy_d2h(labels, a.label, sizeof(int32_t) * V, st));
    if (tri_count) ESFM_HIP_TRY(esfm::copy_d2h(tri_count, a.tri_count, sizeof(int32_t) * V, st));
    ESFM_HIP_TRY(esfm::copy_d2h(stats, a.stats, sizeof(stats), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    *n_components = stats[1];
    return ESFM_OK;
}

int esfm_mesh_clean(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices, const uint8_t *vertex_rgb, const int32_t *triangles,
                    const esfm_mesh_clean_options *opt, float *out_vertices, float *out_normals, uint8_t *out_rgb, int32_t *out_triangles,
                    int32_t *vertex_map, int32_t *triangle_map, int32_t *n_out_vertices, int32_t *n_out_triangles)
{
    if (int rc = check_options(opt)) return rc;
    ESFM_REQUIRE(n_out_vertices && n_out_triangles, "NULL argument");
    ESFM_REQUIRE(n_vertices <= 0 || (vertices && out_vertices), "NULL argument");
    ESFM_REQUIRE(n_triangles <= 0 || out_triangles, "NULL argument");
    ESFM_REQUIRE(!out_rgb || vertex_rgb, "an output array is requested without its input");
    if (int rc = check_mesh(n_vertices, n_triangles, triangles)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    *n_out_vertices = 0; *n_out_triangles = 0;
    if (n_vertices == 0 || n_triangles == 0) return ESFM_OK;
    hipStream_t st = ctx->stream;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, vb = (V + 255) / 256, tb = (T + 255) / 256;

    // stage_a: vertices | colours, then the labelling's arrays, then remap | vertex block counts | triangle block counts
    const size_t vtx_b = al(sizeof(float) * 3 * V), col_b = out_rgb ? al(3 * V) : 0, map_b = al(sizeof(int32_t) * V),
                 vcnt_b = al(sizeof(int32_t) * (vb + 1)), tcnt_b = al(sizeof(int32_t) * (tb + 1));
    esfm::MeshLabelArgs lab;
    if (int rc = place_labels(ctx, vtx_b + col_b, map_b + vcnt_b + tcnt_b, n_vertices, n_triangles, triangles, &lab)) return rc;
    uint8_t *p_a = ctx->stage_a.as<uint8_t>();
    ESFM_HIP_TRY(esfm::copy_h2d(p_a, vertices, sizeof(float) * 3 * V, st));
    if (out_rgb) ESFM_HIP_TRY(esfm::copy_h2d(p_a + vtx_b, vertex_rgb, 3 * V, st));
    if (int rc = esfm::launch_mesh_labels(st, lab)) return rc;

    // stage_d: positions (two buffers) | normals | colours | triangles | vertex_map | triangle_map
    const size_t nrm_b = out_normals ? vtx_b : 0, otri_b = al(sizeof(int32_t) * 3 * T), vmap_b = vertex_map ? map_b : 0,
                 tmap_b = triangle_map ? al(sizeof(int32_t) * T) : 0;
    if (int rc = ctx->stage_d.reserve(2 * vtx_b + nrm_b + col_b + otri_b + vmap_b + tmap_b)) return rc;
    uint8_t *p_d = ctx->stage_d.as<uint8_t>();
    float *pos[2] = {reinterpret_cast<float *>(p_d), reinterpret_cast<float *>(p_d + vtx_b)};
    float *d_normals = reinterpret_cast<float *>(p_d + 2 * vtx_b);
    esfm::MeshCompactArgs c;
    memset(&c, 0, sizeof(c));
    c.tri = lab.tri; c.label = lab.label; c.tri_count = lab.tri_count; c.stats = lab.stats;
    c.vertices = reinterpret_cast<const float *>(p_a);
    c.rgb = out_rgb ? p_a + vtx_b : nullptr;
    c.V = n_vertices; c.T = n_triangles;
    c.min_triangles = opt->min_component_triangles; c.min_permille = opt->min_component_permille;
    uint8_t *p_tail = reinterpret_cast<uint8_t *>(lab.stats) + 256;
    c.remap = reinterpret_cast<int32_t *>(p_tail);
    c.vertex_blocks = reinterpret_cast<int32_t *>(p_tail + map_b);
    c.triangle_blocks = reinterpret_cast<int32_t *>(p_tail + map_b + vcnt_b);
    c.out_vertices = pos[0];
    c.out_rgb = out_rgb ? p_d + 2 * vtx_b + nrm_b : nullptr;
    c.out_tri = reinterpret_cast<int32_t *>(p_d + 2 * vtx_b + nrm_b + col_b);
    c.vertex_map = vertex_map ? reinterpret_cast<int32_t *>(p_d + 2 * vtx_b + nrm_b + col_b + otri_b) : nullptr;
    c.triangle_map = triangle_map ? reinterpret_cast<int32_t *>(p_d + 2 * vtx_b + nrm_b + col_b + otri_b + vmap_b) : nullptr;
    if (int rc = esfm::launch_mesh_compact(st, c)) return rc;
    int32_t nv = 0, nt = 0;
    ESFM_HIP_TRY(esfm::copy_d2h(&nv, c.vertex_blocks + vb, sizeof(int32_t), st));
    ESFM_HIP_TRY(esfm::copy_d2h(&nt, c.triangle_blocks + tb, sizeof(int32_t), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    if (nv < 0 || nv > n_vertices || nt < 0 || nt > n_triangles || (nv == 0) != (nt == 0)) {
        esfm::set_error("mesh clean: %d of %d vertices and %d of %d triangles kept", nv, n_vertices, nt, n_triangles);
        return ESFM_ERR_NUMERIC;
    }
    if (nt == 0) return ESFM_OK;
    const size_t Vo = (size_t)nv, To = (size_t)nt;

    // stage_b: keys | sorted keys | run heads before each key | head block counts | sort scratch;  stage_c: columns | row starts |
    // incidence starts | face vectors | pinned bytes
    const int end_bit = 32 + bit_width((uint32_t)nv);
    const int64_t n_keys = 6 * (int64_t)To;
    const size_t kb = ((size_t)n_keys + 255) / 256;
    size_t sort_b = 0;
    if (int rc = esfm::mesh_sort_scratch_bytes(n_keys, end_bit, &sort_b, st)) return rc;
    const size_t key_b = al(sizeof(uint64_t) * (size_t)n_keys), rank_b = al(sizeof(int32_t) * ((size_t)n_keys + 1)), kcnt_b = al(sizeof(int32_t) * (kb + 1));
    if (int rc = ctx->stage_b.reserve(2 * key_b + rank_b + kcnt_b + sort_b)) return rc;
    uint8_t *p_b = ctx->stage_b.as<uint8_t>();
    const size_t ncol_b = al(sizeof(int32_t) * (size_t)n_keys), row_b = al(sizeof(int32_t) * (Vo + 1)), face_b = al(sizeof(float) * 3 * To);
    if (int rc = ctx->stage_c.reserve(ncol_b + 2 * row_b + face_b + al(Vo))) return rc;
    uint8_t *p_c = ctx->stage_c.as<uint8_t>();
    esfm::MeshGraphArgs g;
    memset(&g, 0, sizeof(g));
    g.tri = c.out_tri; g.V = nv; g.T = nt;
    g.keys = reinterpret_cast<uint64_t *>(p_b);
    g.sorted = reinterpret_cast<const uint64_t *>(p_b + key_b);
    g.head_rank = reinterpret_cast<int32_t *>(p_b + 2 * key_b);
    g.head_blocks = reinterpret_cast<int32_t *>(p_b + 2 * key_b + rank_b);
    void *d_sort = p_b + 2 * key_b + rank_b + kcnt_b;
    g.col = reinterpret_cast<int32_t *>(p_c);
    g.row_start = reinterpret_cast<int32_t *>(p_c + ncol_b);
    g.inc_start = reinterpret_cast<int32_t *>(p_c + ncol_b + row_b);
    g.face = reinterpret_cast<float *>(p_c + ncol_b + 2 * row_b);
    g.pinned = p_c + ncol_b + 2 * row_b + face_b;

    int cur = 0;
    if (opt->smooth_iterations > 0) {
        if (int rc = esfm::launch_mesh_edge_keys(st, g)) return rc;
        if (int rc = esfm::mesh_sort_keys(d_sort, sort_b, g.keys, const_cast<uint64_t *>(g.sorted), n_keys, end_bit, st)) return rc;
        if (int rc = esfm::launch_mesh_adjacency(st, g)) return rc;
        for (int s = 0; s < 2 * opt->smooth_iterations; ++s, cur ^= 1)
            if (int rc = esfm::launch_mesh_smooth(st, g, pos[cur], pos[cur ^ 1], s % 2 == 0 ? opt->smooth_lambda : opt->smooth_mu, opt->pin_boundary)) return rc;
    }
    if (out_normals) {
        if (int rc = esfm::launch_mesh_incidence_keys(st, g)) return rc;
        if (int rc = esfm::mesh_sort_keys(d_sort, sort_b, g.keys, const_cast<uint64_t *>(g.sorted), 3 * (int64_t)To, end_bit, st)) return rc;
        if (int rc = esfm::launch_mesh_normals(st, g, pos[cur], d_normals)) return rc;
    }
    ESFM_HIP_TRY(esfm::copy_d2h(out_vertices, pos[cur], sizeof(float) * 3 * Vo, st));
    if (out_normals) ESFM_HIP_TRY(esfm::copy_d2h(out_normals, d_normals, sizeof(float) * 3 * Vo, st));
    if (out_rgb) ESFM_HIP_TRY(esfm::copy_d2h(out_rgb, c.out_rgb, 3 * Vo, st));
    ESFM_HIP_TRY(esfm::copy_d2h(out_triangles, c.out_tri, sizeof(int32_t) * 3 * To, st));
    if (vertex_map) ESFM_HIP_TRY(esfm::copy_d2h(vertex_map, c.vertex_map, sizeof(int32_t) * Vo, st));
    if (triangle_map) ESFM_HIP_TRY(esfm::copy_d2h(triangle_map, c.triangle_map, sizeof(int32_t) * To, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    *n_out_vertices = nv; *n_out_triangles = nt;
    return ESFM_OK;
}

}  // extern "C"
