// C-ABI entry points of the mesh texturing (include/esfm.h, "Mesh texturing"): esfm_mesh_texture_views, esfm_mesh_texture_bake and
// esfm_mesh_texture_bake_ex (the bake with the seam levelling's offsets; level_api.cpp computes them).  Host side: the argument checks on the caller's arrays, the atlas layout with its uv corners and the
// scratch layout (texture_check.hpp), uploads, launches and the copies back.  The work runs in texture_kernels.hip;
// tests/texture_ref.py restates the rule.
#include "level_check.hpp"
#include "texture_kernels.hpp"

namespace {

void fill_cams(esfm::TextureCam *cams, int n, const float *K4, const float *poses)
{
    for (int v = 0; v < n; ++v) {
        memcpy(cams[v].K, K4 + 4 * v, sizeof(float) * 4);
        memcpy(cams[v].P, poses + 12 * v, sizeof(float) * 12);
    }
}

}  // namespace

extern "C" {

void esfm_mesh_texture_options_default(esfm_mesh_texture_options *opt)
{
    if (!opt) return;
    opt->min_cos = 0.2f;
    opt->occlusion_tol = 0.02f;
}

int esfm_mesh_texture_views(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices, const int32_t *triangles, int n_views, int rows,
                            int cols, const float *K4, const float *poses, const esfm_mesh_texture_options *opt, int32_t *label, float *score,
                            uint32_t *depth_buffers)
{
    if (int rc = esfm::texture_check_views_args(n_vertices, n_triangles, vertices, triangles, n_views, rows, cols, K4, poses, opt, label, score)) return rc;
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(ctx)) return rc;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, n = (size_t)n_views, pixels = (size_t)rows * cols;
    if (n_triangles == 0) {
        if (depth_buffers) memset(depth_buffers, 0, sizeof(uint32_t) * n * pixels);
        return ESFM_OK;
    }
    hipStream_t st = ctx->stream;
    const esfm::TextureLayout l = esfm::texture_layout(V, T, n, false, pixels, 0, 0);
    if (int rc = ctx->stage_a.reserve(l.a_bytes)) return rc;
    if (int rc = ctx->stage_b.reserve(l.b_bytes)) return rc;
    if (int rc = ctx->pin(sizeof(esfm::TextureCam) * n)) return rc;
    uint8_t *p_a = ctx->stage_a.as<uint8_t>(), *p_b = ctx->stage_b.as<uint8_t>();
    fill_cams(static_cast<esfm::TextureCam *>(ctx->pinned), n_views, K4, poses);
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.vertices, vertices, sizeof(float) * 3 * V, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.tri, triangles, sizeof(int32_t) * 3 * T, st));
    ESFM_HIP_TRY(hipMemcpyAsync(p_a + l.cams, ctx->pinned, sizeof(esfm::TextureCam) * n, hipMemcpyHostToDevice, st));
    ESFM_HIP_TRY(hipMemsetAsync(p_b + l.buffers, 0, sizeof(uint32_t) * n * pixels, st));
    ESFM_HIP_TRY(hipMemsetAsync(p_b + l.count, 0, sizeof(uint32_t), st));

    esfm::TextureViewsArgs a;
    memset(&a, 0, sizeof(a));
    a.vertices = reinterpret_cast<const float *>(p_a + l.vertices);
    a.tri = reinterpret_cast<const int32_t *>(p_a + l.tri);
    a.cams = reinterpret_cast<const esfm::TextureCam *>(p_a + l.cams);
    a.proj = reinterpret_cast<float4 *>(p_b + l.proj);
    a.buffers = reinterpret_cast<uint32_t *>(p_b + l.buffers);
    a.list = reinterpret_cast<uint32_t *>(p_b + l.list);
    a.count = reinterpret_cast<uint32_t *>(p_b + l.count);
    a.label = reinterpret_cast<int32_t *>(p_a + l.label);
    a.score = reinterpret_cast<float *>(p_a + l.score);
    a.V = n_vertices; a.T = n_triangles; a.n = n_views; a.rows = rows; a.cols = cols;
    a.min_cos = opt->min_cos; a.keep = 1.0f - opt->occlusion_tol;

    if (int rc = esfm::launch_texture_project(st, a)) return rc;
    if (int rc = esfm::launch_texture_rasterise(st, a)) return rc;
    if (int rc = esfm::launch_texture_choose(st, a)) return rc;
    // the outputs are written only once everything has run: into the context's own buffers first
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    ESFM_HIP_TRY(esfm::copy_d2h(label, a.label, sizeof(int32_t) * T, st));
    ESFM_HIP_TRY(esfm::copy_d2h(score, a.score, sizeof(float) * T, st));
    if (depth_buffers) ESFM_HIP_TRY(esfm::copy_d2h(depth_buffers, a.buffers, sizeof(uint32_t) * n * pixels, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

int esfm_mesh_texture_bake(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices, const uint8_t *vertex_rgb, const int32_t *triangles,
                           const int32_t *label, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4,
                           const float *poses, int texels, int atlas_width, int max_atlas_rows, uint8_t *atlas, float *uv, int32_t *atlas_rows)
{
    return esfm_mesh_texture_bake_ex(ctx, n_vertices, n_triangles, vertices, vertex_rgb, triangles, label, n_views, rows, cols, channels, images, K4, poses,
                                     texels, atlas_width, max_atlas_rows, atlas, uv, atlas_rows, nullptr);
}

// offsets == NULL: the plain bake (the kernel's variant without offsets, nothing more uploaded)
int esfm_mesh_texture_bake_ex(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices, const uint8_t *vertex_rgb, const int32_t *triangles,
                              const int32_t *label, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4,
                              const float *poses, int texels, int atlas_width, int max_atlas_rows, uint8_t *atlas, float *uv, int32_t *atlas_rows,
                              const float *offsets)
{
    int H = 0;
    if (int rc = esfm::texture_check_bake_args(n_vertices, n_triangles, vertices, triangles, label, n_views, rows, cols, channels, images, K4, poses, texels,
                                               atlas_width, max_atlas_rows, atlas, uv, atlas_rows, &H)) return rc;
    if (int rc = esfm::level_check_offsets(n_triangles, offsets)) return rc;
    *atlas_rows = H;
    if (H > max_atlas_rows) {
        esfm::set_error("esfm_mesh_texture_bake: the atlas needs %d rows of %d texels, the buffer holds %d", H, atlas_width * texels, max_atlas_rows);
        return ESFM_ERR_INVALID_ARG;
    }
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(ctx)) return rc;
    if (n_triangles == 0) return ESFM_OK;
    hipStream_t st = ctx->stream;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, n = (size_t)n_views;
    const size_t image_bytes = n * rows * cols * channels, atlas_bytes = (size_t)H * atlas_width * texels * 3;
    const esfm::TextureLayout l = esfm::texture_layout(V, T, n, vertex_rgb != nullptr, 0, image_bytes, atlas_bytes);
    if (int rc = ctx->stage_a.reserve(l.a_bytes)) return rc;
    if (int rc = ctx->stage_c.reserve(l.c_bytes)) return rc;
    if (int rc = ctx->stage_d.reserve(l.d_bytes)) return rc;
    if (offsets) { if (int rc = ctx->stage_b.reserve(sizeof(float) * 9 * T)) return rc; }
    if (int rc = ctx->pin(sizeof(esfm::TextureCam) * n)) return rc;
    uint8_t *p_a = ctx->stage_a.as<uint8_t>(), *p_c = ctx->stage_c.as<uint8_t>(), *p_d = ctx->stage_d.as<uint8_t>();
    fill_cams(static_cast<esfm::TextureCam *>(ctx->pinned), n_views, K4, poses);
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.vertices, vertices, sizeof(float) * 3 * V, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.tri, triangles, sizeof(int32_t) * 3 * T, st));
    if (vertex_rgb) ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.rgb, vertex_rgb, 3 * V, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.label, label, sizeof(int32_t) * T, st));
    ESFM_HIP_TRY(hipMemcpyAsync(p_a + l.cams, ctx->pinned, sizeof(esfm::TextureCam) * n, hipMemcpyHostToDevice, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_c + l.images, images, image_bytes, st));

    esfm::TextureBakeArgs a;
    memset(&a, 0, sizeof(a));
    a.vertices = reinterpret_cast<const float *>(p_a + l.vertices);
    a.rgb = vertex_rgb ? p_a + l.rgb : nullptr;
    a.tri = reinterpret_cast<const int32_t *>(p_a + l.tri);
    a.label = reinterpret_cast<const int32_t *>(p_a + l.label);
    a.cams = reinterpret_cast<const esfm::TextureCam *>(p_a + l.cams);
    a.images = p_c + l.images;
    a.atlas = p_d + l.atlas;
    if (offsets) {                                                     // stage_b: the bake's only use of it
        ESFM_HIP_TRY(esfm::copy_h2d(ctx->stage_b.ptr, offsets, sizeof(float) * 9 * T, st));
        a.offsets = ctx->stage_b.as<float>();
    }
    a.T = n_triangles; a.rows = rows; a.cols = cols; a.channels = channels; a.S = texels; a.A = atlas_width; a.H = H;
    if (int rc = esfm::launch_texture_bake(st, a)) return rc;
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    ESFM_HIP_TRY(esfm::copy_d2h(atlas, a.atlas, atlas_bytes, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    esfm::texture_uv(n_triangles, texels, atlas_width, H, uv);
    return ESFM_OK;
}

}  // extern "C"
