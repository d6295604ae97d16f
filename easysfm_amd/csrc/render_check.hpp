// Host-only part of esfm_mesh_render (include/esfm.h, "Mesh rendering"), free of HIP so that tests/cpp/render_check_main.cpp runs
// it under the sanitizers with g++ alone: the argument checks, which read the caller's arrays and return before any device call,
// and the byte layout of the scratch buffers.
#pragma once

#include "texture_check.hpp"      // texture_check_mesh, texture_check_cameras, TextureCam, kTextureMaxSide

namespace esfm {

constexpr int kRenderSmallBox = 64;             // bounding boxes of more pixels go to the wave-per-pair kernel

// Everything esfm_mesh_render rejects with ESFM_ERR_INVALID_ARG.  Reads, writes nothing.
inline int render_check_args(int V, int T, const float *vertices, const int32_t *triangles, const float *uv, int atlas_rows, int atlas_cols,
                             const uint8_t *atlas, int n_views, int rows, int cols, const float *K4, const float *poses,
                             const esfm_mesh_render_options *o, const uint8_t *rgb, const float *depth, const int32_t *triangle_id)
{
    ESFM_REQUIRE(o, "options are NULL");
    ESFM_REQUIRE(rgb || depth || triangle_id, "rgb, depth and triangle_id are all NULL");
    if (int rc = texture_check_mesh(V, T, vertices, triangles)) return rc;
    if (int rc = texture_check_cameras(n_views, rows, cols, K4, poses)) return rc;
    ESFM_REQUIRE((uv != nullptr) == (atlas != nullptr), "uv and atlas must both be given or both be NULL");
    if (atlas) {
        ESFM_REQUIRE(atlas_rows >= 2 && atlas_rows <= kTextureMaxSide && atlas_cols >= 2 && atlas_cols <= kTextureMaxSide, "the atlas must be 2..16384 texels per side");
        for (size_t i = 0; i < 6 * (size_t)T; ++i) ESFM_REQUIRE(std::isfinite(uv[i]), "a texture coordinate is not finite");
    }
    return ESFM_OK;
}

// Byte offsets of the arrays inside the context's scratch buffers; every array starts on a multiple of 256 bytes.
struct RenderLayout {
    // stage_a: the mesh and the cameras
    size_t vertices, tri, rgb, uv, cams, a_bytes;
    // stage_b: projected vertices (16 bytes per view and vertex), the key buffers (8 bytes per view and pixel), the list of large-box
    // pairs (4 bytes per view and triangle) and its counter
    size_t proj, keys, list, count, b_bytes;
    // stage_c: the atlas; stage_d: the outputs that were asked for
    size_t atlas, c_bytes, out_rgb, out_depth, out_id, d_bytes;
};

inline RenderLayout render_layout(size_t V, size_t T, size_t n_views, size_t pixels, bool rgb, size_t atlas_bytes, bool out_rgb, bool out_depth, bool out_id)
{
    RenderLayout l;
    ScratchCarver a, b, c, d;
    l.vertices = a.take(sizeof(float) * 3 * V);
    l.tri = a.take(sizeof(int32_t) * 3 * T);
    l.rgb = a.take(rgb ? 3 * V : 0);
    l.uv = a.take(atlas_bytes ? sizeof(float) * 6 * T : 0);
    l.cams = a.take(sizeof(TextureCam) * n_views);
    l.a_bytes = a.at;
    l.proj = b.take(16 * n_views * V);
    l.keys = b.take(sizeof(uint64_t) * n_views * pixels);
    l.list = b.take(sizeof(uint32_t) * n_views * T);
    l.count = b.take(sizeof(uint32_t));
    l.b_bytes = b.at;
    l.atlas = c.take(atlas_bytes);
    l.c_bytes = c.at;
    l.out_rgb = d.take(out_rgb ? 3 * n_views * pixels : 0);
    l.out_depth = d.take(out_depth ? sizeof(float) * n_views * pixels : 0);
    l.out_id = d.take(out_id ? sizeof(int32_t) * n_views * pixels : 0);
    l.d_bytes = d.at;
    return l;
}

}  // namespace esfm
