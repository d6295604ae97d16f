// C-ABI entry points of the mesh clean-up (include/esfm.h, "Mesh clean-up"): esfm_mesh_components and esfm_mesh_clean.  Host
// side: argument checks (the triangle indices on the caller's copy), buffer layout, uploads, launches, the one read-back of the
// two kept counts, and the copy of the mesh.  The work runs in mesh_kernels.hip, the two sorts in mesh_sort.hip;
// tests/mesh_clean_ref.py restates the rules.
#include <cmath>

#include "mesh_check.hpp"
#include "mesh_kernels.hpp"

namespace {

using esfm::check_mesh;

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

// the labelling's device arrays in stage_a, behind whatever the caller has carved before them: triangles | parent | label |
// tri_count | stats
struct LabelLayout { size_t tri, parent, label, tri_count, stats; };

LabelLayout carve_labels(esfm::ScratchCarver *at, size_t V, size_t T)
{
    LabelLayout l;
    l.tri = at->take(sizeof(int32_t) * 3 * T);
    l.parent = at->take(sizeof(int32_t) * V);
    l.label = at->take(sizeof(int32_t) * V);
    l.tri_count = at->take(sizeof(int32_t) * V);
    l.stats = at->take(sizeof(int32_t) * 2);
    return l;
}

// (stage_a is reserved) points the arguments at the arrays and uploads the triangles
int place_labels(esfm_ctx *ctx, const LabelLayout &l, int V, int T, const int32_t *triangles, esfm::MeshLabelArgs *a)
{
    uint8_t *p = ctx->stage_a.as<uint8_t>();
    a->tri = reinterpret_cast<const int32_t *>(p + l.tri);
    a->parent = reinterpret_cast<int32_t *>(p + l.parent);
    a->label = reinterpret_cast<int32_t *>(p + l.label);
    a->tri_count = reinterpret_cast<int32_t *>(p + l.tri_count);
    a->stats = reinterpret_cast<int32_t *>(p + l.stats);
    a->V = V; a->T = T;
    if (T) ESFM_HIP_TRY(esfm::copy_h2d(p + l.tri, triangles, sizeof(int32_t) * 3 * (size_t)T, ctx->stream));
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
    esfm::ScratchCarver in;
    const LabelLayout l = carve_labels(&in, (size_t)n_vertices, (size_t)n_triangles);
    if (int rc = ctx->stage_a.reserve(in.at)) return rc;
    esfm::MeshLabelArgs a;
    if (int rc = place_labels(ctx, l, n_vertices, n_triangles, triangles, &a)) return rc;
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
    esfm::ScratchCarver in;
    const size_t in_vertices = in.take(sizeof(float) * 3 * V), in_rgb = in.take(out_rgb ? 3 * V : 0);
    const LabelLayout labels_at = carve_labels(&in, V, T);
    const size_t remap = in.take(sizeof(int32_t) * V), vertex_blocks = in.take(sizeof(int32_t) * (vb + 1)),
                 triangle_blocks = in.take(sizeof(int32_t) * (tb + 1));
    if (int rc = ctx->stage_a.reserve(in.at)) return rc;
    esfm::MeshLabelArgs lab;
    if (int rc = place_labels(ctx, labels_at, n_vertices, n_triangles, triangles, &lab)) return rc;
    uint8_t *p_a = ctx->stage_a.as<uint8_t>();
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + in_vertices, vertices, sizeof(float) * 3 * V, st));
    if (out_rgb) ESFM_HIP_TRY(esfm::copy_h2d(p_a + in_rgb, vertex_rgb, 3 * V, st));
    if (int rc = esfm::launch_mesh_labels(st, lab)) return rc;

    // stage_d: positions (two buffers) | normals | colours | triangles | vertex_map | triangle_map
    esfm::ScratchCarver out;
    const size_t pos0 = out.take(sizeof(float) * 3 * V), pos1 = out.take(sizeof(float) * 3 * V),
                 o_normals = out.take(out_normals ? sizeof(float) * 3 * V : 0), o_rgb = out.take(out_rgb ? 3 * V : 0),
                 o_tri = out.take(sizeof(int32_t) * 3 * T), o_vmap = out.take(vertex_map ? sizeof(int32_t) * V : 0),
                 o_tmap = out.take(triangle_map ? sizeof(int32_t) * T : 0);
    if (int rc = ctx->stage_d.reserve(out.at)) return rc;
    uint8_t *p_d = ctx->stage_d.as<uint8_t>();
    float *pos[2] = {reinterpret_cast<float *>(p_d + pos0), reinterpret_cast<float *>(p_d + pos1)};
    float *d_normals = reinterpret_cast<float *>(p_d + o_normals);
    esfm::MeshCompactArgs c;
    memset(&c, 0, sizeof(c));
    c.tri = lab.tri; c.label = lab.label; c.tri_count = lab.tri_count; c.stats = lab.stats;
    c.vertices = reinterpret_cast<const float *>(p_a + in_vertices);
    c.rgb = out_rgb ? p_a + in_rgb : nullptr;
    c.V = n_vertices; c.T = n_triangles;
    c.min_triangles = opt->min_component_triangles; c.min_permille = opt->min_component_permille;
    c.remap = reinterpret_cast<int32_t *>(p_a + remap);
    c.vertex_blocks = reinterpret_cast<int32_t *>(p_a + vertex_blocks);
    c.triangle_blocks = reinterpret_cast<int32_t *>(p_a + triangle_blocks);
    c.out_vertices = pos[0];
    c.out_rgb = out_rgb ? p_d + o_rgb : nullptr;
    c.out_tri = reinterpret_cast<int32_t *>(p_d + o_tri);
    c.vertex_map = vertex_map ? reinterpret_cast<int32_t *>(p_d + o_vmap) : nullptr;
    c.triangle_map = triangle_map ? reinterpret_cast<int32_t *>(p_d + o_tmap) : nullptr;
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
    const size_t n_keys = 6 * To;
    size_t sort_b = 0;
    if (int rc = esfm::mesh_sort_scratch_bytes((int64_t)n_keys, esfm::mesh_key_bits(nv), &sort_b, st)) return rc;
    esfm::ScratchCarver sorting, graph;
    const size_t keys = sorting.take(sizeof(uint64_t) * n_keys), sorted = sorting.take(sizeof(uint64_t) * n_keys),
                 head_rank = sorting.take(sizeof(int32_t) * (n_keys + 1)), head_blocks = sorting.take(sizeof(int32_t) * ((n_keys + 255) / 256 + 1)),
                 sort = sorting.take(sort_b);
    if (int rc = ctx->stage_b.reserve(sorting.at)) return rc;
    uint8_t *p_b = ctx->stage_b.as<uint8_t>();
    const size_t col = graph.take(sizeof(int32_t) * n_keys), row_start = graph.take(sizeof(int32_t) * (Vo + 1)),
                 inc_start = graph.take(sizeof(int32_t) * (Vo + 1)), face = graph.take(sizeof(float) * 3 * To), pinned = graph.take(Vo);
    if (int rc = ctx->stage_c.reserve(graph.at)) return rc;
    uint8_t *p_c = ctx->stage_c.as<uint8_t>();
    esfm::MeshGraphArgs g;
    memset(&g, 0, sizeof(g));
    g.tri = c.out_tri; g.V = nv; g.T = nt;
    g.keys = reinterpret_cast<uint64_t *>(p_b + keys);
    g.sorted = reinterpret_cast<const uint64_t *>(p_b + sorted);
    g.head_rank = reinterpret_cast<int32_t *>(p_b + head_rank);
    g.head_blocks = reinterpret_cast<int32_t *>(p_b + head_blocks);
    void *d_sort = p_b + sort;
    g.col = reinterpret_cast<int32_t *>(p_c + col);
    g.row_start = reinterpret_cast<int32_t *>(p_c + row_start);
    g.inc_start = reinterpret_cast<int32_t *>(p_c + inc_start);
    g.face = reinterpret_cast<float *>(p_c + face);
    g.pinned = p_c + pinned;

    int cur = 0;
    if (opt->smooth_iterations > 0) {
        if (int rc = esfm::mesh_build_adjacency(st, g, d_sort, sort_b)) return rc;
        for (int s = 0; s < 2 * opt->smooth_iterations; ++s, cur ^= 1)
            if (int rc = esfm::launch_mesh_smooth(st, g, pos[cur], pos[cur ^ 1], s % 2 == 0 ? opt->smooth_lambda : opt->smooth_mu, opt->pin_boundary)) return rc;
    }
    if (out_normals)
        if (int rc = esfm::mesh_build_normals(st, g, d_sort, sort_b, pos[cur], d_normals)) return rc;
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
