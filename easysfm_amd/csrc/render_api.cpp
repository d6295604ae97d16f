// C-ABI entry point of the mesh rendering (include/esfm.h, "Mesh rendering"): esfm_mesh_render.  Host side: the argument checks on
// the caller's arrays and the scratch layout (render_check.hpp), uploads, launches and the copies back.  The work runs in
// render_kernels.hip; tests/render_ref.py restates the rule.
#include "render_kernels.hpp"

extern "C" {

void esfm_mesh_render_options_default(esfm_mesh_render_options *opt)
{
    if (!opt) return;
    opt->background[0] = opt->background[1] = opt->background[2] = 0;
    opt->reserved = 0;
}

int esfm_mesh_render(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices, const int32_t *triangles, const uint8_t *vertex_rgb,
                     const float *uv, int atlas_rows, int atlas_cols, const uint8_t *atlas, int n_views, int rows, int cols, const float *K4,
                     const float *poses, const esfm_mesh_render_options *opt, uint8_t *rgb, float *depth, int32_t *triangle_id)
{
    if (int rc = esfm::render_check_args(n_vertices, n_triangles, vertices, triangles, uv, atlas_rows, atlas_cols, atlas, n_views, rows, cols, K4, poses, opt,
                                         rgb, depth, triangle_id)) return rc;
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, n = (size_t)n_views, pixels = (size_t)rows * cols;
    const size_t atlas_bytes = atlas ? (size_t)atlas_rows * atlas_cols * 3 : 0;
    const esfm::RenderLayout l = esfm::render_layout(V, T, n, pixels, vertex_rgb != nullptr, atlas_bytes, rgb != nullptr, depth != nullptr, triangle_id != nullptr);
    if (int rc = ctx->stage_a.reserve(l.a_bytes)) return rc;
    if (int rc = ctx->stage_b.reserve(l.b_bytes)) return rc;
    if (int rc = ctx->stage_c.reserve(l.c_bytes)) return rc;
    if (int rc = ctx->stage_d.reserve(l.d_bytes)) return rc;
    if (int rc = ctx->pin(sizeof(esfm::TextureCam) * n)) return rc;
    uint8_t *p_a = ctx->stage_a.as<uint8_t>(), *p_b = ctx->stage_b.as<uint8_t>(), *p_c = ctx->stage_c.as<uint8_t>(), *p_d = ctx->stage_d.as<uint8_t>();
    esfm::TextureCam *cams = static_cast<esfm::TextureCam *>(ctx->pinned);
    for (int v = 0; v < n_views; ++v) {
        memcpy(cams[v].K, K4 + 4 * v, sizeof(float) * 4);
        memcpy(cams[v].P, poses + 12 * v, sizeof(float) * 12);
    }
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.vertices, vertices, sizeof(float) * 3 * V, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.tri, triangles, sizeof(int32_t) * 3 * T, st));
    if (vertex_rgb) ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.rgb, vertex_rgb, 3 * V, st));
    if (atlas) {
        ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.uv, uv, sizeof(float) * 6 * T, st));
        ESFM_HIP_TRY(esfm::copy_h2d(p_c + l.atlas, atlas, atlas_bytes, st));
    }
    ESFM_HIP_TRY(hipMemcpyAsync(p_a + l.cams, ctx->pinned, sizeof(esfm::TextureCam) * n, hipMemcpyHostToDevice, st));
    ESFM_HIP_TRY(hipMemsetAsync(p_b + l.keys, 0, sizeof(uint64_t) * n * pixels, st));
    ESFM_HIP_TRY(hipMemsetAsync(p_b + l.count, 0, sizeof(uint32_t), st));

    esfm::RenderArgs a;
    memset(&a, 0, sizeof(a));
    a.vertices = reinterpret_cast<const float *>(p_a + l.vertices);
    a.tri = reinterpret_cast<const int32_t *>(p_a + l.tri);
    a.rgb = vertex_rgb ? p_a + l.rgb : nullptr;
    a.uv = atlas ? reinterpret_cast<const float *>(p_a + l.uv) : nullptr;
    a.atlas = atlas ? p_c + l.atlas : nullptr;
    a.cams = reinterpret_cast<const esfm::TextureCam *>(p_a + l.cams);
    a.proj = reinterpret_cast<int4 *>(p_b + l.proj);
    a.keys = reinterpret_cast<unsigned long long *>(p_b + l.keys);
    a.list = reinterpret_cast<uint32_t *>(p_b + l.list);
    a.count = reinterpret_cast<uint32_t *>(p_b + l.count);
    a.out_rgb = rgb ? p_d + l.out_rgb : nullptr;
    a.out_depth = depth ? reinterpret_cast<float *>(p_d + l.out_depth) : nullptr;
    a.out_id = triangle_id ? reinterpret_cast<int32_t *>(p_d + l.out_id) : nullptr;
    a.V = n_vertices; a.T = n_triangles; a.n = n_views; a.rows = rows; a.cols = cols; a.H = atlas_rows; a.W = atlas_cols;
    memcpy(a.background, opt->background, 3);

    if (n_triangles > 0) {                                               // (then V > 0: the indices were checked)
        if (int rc = esfm::launch_render_project(st, a)) return rc;
        if (int rc = esfm::launch_render_rasterise(st, a)) return rc;
    }
    if (int rc = esfm::launch_render_shade(st, a)) return rc;
    // the outputs are written only once everything has run: into the context's own buffers first
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    if (rgb) ESFM_HIP_TRY(esfm::copy_d2h(rgb, a.out_rgb, 3 * n * pixels, st));
    if (depth) ESFM_HIP_TRY(esfm::copy_d2h(depth, a.out_depth, sizeof(float) * n * pixels, st));
    if (triangle_id) ESFM_HIP_TRY(esfm::copy_d2h(triangle_id, a.out_id, sizeof(int32_t) * n * pixels, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

}  // extern "C"
