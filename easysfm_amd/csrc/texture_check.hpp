// Host-only part of esfm_mesh_texture_views / esfm_mesh_texture_bake (include/esfm.h, "Mesh texturing"), free of HIP so that
// tests/cpp/texture_check_main.cpp runs it under the sanitizers with g++ alone: the argument checks, which read the caller's arrays
// and return before any device call, the atlas layout with its uv corners, and the byte layout of the scratch buffers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "error.hpp"
#include "scratch_layout.hpp"

namespace esfm {

constexpr int kTextureMaxViews = 64;
constexpr int kTextureMaxSide = 16384;          // image and atlas, texels per side
constexpr int kTextureMaxTriangles = 1 << 25;   // what an atlas of 16384^2 texels holds at 4 texels per square
constexpr int kTextureSmallBox = 64;            // bounding boxes of more pixels go to the wave-per-pair kernel

struct TextureCam { float K[4], P[12]; };       // one view as the kernels read it

inline int texture_check_mesh(int V, int T, const float *vertices, const int32_t *triangles)
{
    ESFM_REQUIRE(V >= 0 && V <= (1 << 30), "n_vertices must be 0..2^30");
    ESFM_REQUIRE(T >= 0 && T <= kTextureMaxTriangles, "n_triangles must be 0..2^25");
    ESFM_REQUIRE(V == 0 || vertices, "NULL argument");
    ESFM_REQUIRE(T == 0 || triangles, "NULL argument");
    for (size_t i = 0; i < 3 * (size_t)V; ++i) ESFM_REQUIRE(std::isfinite(vertices[i]), "a vertex is not finite");
    for (size_t i = 0; i < 3 * (size_t)T; ++i) ESFM_REQUIRE(triangles[i] >= 0 && triangles[i] < V, "a triangle index is outside 0..n_vertices-1");
    return ESFM_OK;
}

inline int texture_check_cameras(int n_views, int rows, int cols, const float *K4, const float *poses)
{
    ESFM_REQUIRE(n_views >= 1 && n_views <= kTextureMaxViews, "n_views must be 1..64");
    ESFM_REQUIRE(rows >= 2 && rows <= kTextureMaxSide && cols >= 2 && cols <= kTextureMaxSide, "rows and cols must be 2..16384");
    ESFM_REQUIRE(K4 && poses, "NULL argument");
    for (int i = 0; i < 4 * n_views; ++i) ESFM_REQUIRE(std::isfinite(K4[i]), "K4 must be finite");
    for (int i = 0; i < 12 * n_views; ++i) ESFM_REQUIRE(std::isfinite(poses[i]), "poses must be finite");
    for (int v = 0; v < n_views; ++v) ESFM_REQUIRE(K4[4 * v] != 0.f && K4[4 * v + 2] != 0.f, "a focal length is 0");
    return ESFM_OK;
}

// Everything esfm_mesh_texture_views rejects with ESFM_ERR_INVALID_ARG.  Reads, writes nothing.
inline int texture_check_views_args(int V, int T, const float *vertices, const int32_t *triangles, int n_views, int rows, int cols, const float *K4,
                                    const float *poses, const esfm_mesh_texture_options *o, const int32_t *label, const float *score)
{
    ESFM_REQUIRE(o, "options are NULL");
    ESFM_REQUIRE(o->min_cos >= 0.f && o->min_cos < 1.f, "min_cos must be in [0, 1)");                    // (a NaN fails both)
    ESFM_REQUIRE(o->occlusion_tol >= 0.f && o->occlusion_tol < 1.f, "occlusion_tol must be in [0, 1)");
    if (int rc = texture_check_mesh(V, T, vertices, triangles)) return rc;
    if (int rc = texture_check_cameras(n_views, rows, cols, K4, poses)) return rc;
    ESFM_REQUIRE(T == 0 || (label && score), "NULL argument");
    return ESFM_OK;
}

// Atlas height in texels for T triangles; -1 if the layout is not allowed (the message is set).
inline int texture_atlas_rows(int T, int texels, int atlas_width)
{
    if (texels < 4 || texels > 64) { set_error("%s: texels must be 4..64", __func__); return -1; }
    if (atlas_width < 1) { set_error("%s: atlas_width must be >= 1", __func__); return -1; }
    if ((int64_t)atlas_width * texels > kTextureMaxSide) { set_error("%s: the atlas is wider than 16384 texels", __func__); return -1; }
    const int64_t squares = ((int64_t)T + 1) / 2, h = (squares + atlas_width - 1) / atlas_width * texels;
    if (h > kTextureMaxSide) { set_error("%s: the atlas is higher than 16384 texels", __func__); return -1; }
    return (int)h;
}

// Everything esfm_mesh_texture_bake rejects, the capacity aside.  *H receives the needed atlas height.
inline int texture_check_bake_args(int V, int T, const float *vertices, const int32_t *triangles, const int32_t *label, int n_views, int rows, int cols,
                                   int channels, const uint8_t *images, const float *K4, const float *poses, int texels, int atlas_width,
                                   int max_atlas_rows, const uint8_t *atlas, const float *uv, const int32_t *atlas_rows, int *H)
{
    ESFM_REQUIRE(atlas_rows, "NULL argument");
    ESFM_REQUIRE(channels == 1 || channels == 3, "channels must be 1 or 3");
    ESFM_REQUIRE(max_atlas_rows >= 0, "max_atlas_rows must be >= 0");
    if (int rc = texture_check_mesh(V, T, vertices, triangles)) return rc;
    if (int rc = texture_check_cameras(n_views, rows, cols, K4, poses)) return rc;
    ESFM_REQUIRE(images, "NULL argument");
    ESFM_REQUIRE(T == 0 || (label && uv), "NULL argument");
    for (int t = 0; t < T; ++t) ESFM_REQUIRE(label[t] >= -1 && label[t] < n_views, "a label is outside -1..n_views-1");
    const int h = texture_atlas_rows(T, texels, atlas_width);
    if (h < 0) return ESFM_ERR_INVALID_ARG;
    ESFM_REQUIRE(h == 0 || max_atlas_rows == 0 || atlas, "NULL argument");
    *H = h;
    return ESFM_OK;
}

// uv [T, 3, 2] (include/esfm.h: chart corners over the atlas size, origin at the outer corner of the first texel, v down the rows)
inline void texture_uv(int T, int S, int atlas_width, int H, float *uv)
{
    const float W = (float)(atlas_width * S), fs = (float)S;
    const float even[3][2] = {{0.5f, 0.5f}, {fs - 1.5f, 0.5f}, {0.5f, fs - 1.5f}}, odd[3][2] = {{fs - 0.5f, fs - 0.5f}, {2.5f, fs - 0.5f}, {fs - 0.5f, 2.5f}};
    for (int t = 0; t < T; ++t) {
        const int q = t / 2;
        const float X0 = (float)(q % atlas_width * S), Y0 = (float)(q / atlas_width * S);
        const float(*c)[2] = t % 2 ? odd : even;
        for (int k = 0; k < 3; ++k) {
            uv[6 * (size_t)t + 2 * k] = (X0 + c[k][0]) / W;
            uv[6 * (size_t)t + 2 * k + 1] = (Y0 + c[k][1]) / (float)H;
        }
    }
}

// Byte offsets of the arrays inside the context's scratch buffers; every array starts on a multiple of 256 bytes.
struct TextureLayout {
    // stage_a: the mesh, the cameras and the per-triangle results
    size_t vertices, tri, rgb, cams, label, score, a_bytes;
    // stage_b: the views call's own arrays: projected vertices (16 bytes per view and vertex), the depth buffers (4 bytes per view
    // and pixel), the list of large-box pairs (4 bytes per view and triangle) and its counter
    size_t proj, buffers, list, count, b_bytes;
    // stage_c: the bake's images; stage_d: its atlas
    size_t images, c_bytes, atlas, d_bytes;
};

// views: pixels = rows * cols, the bake's fields empty; bake: image_bytes and atlas_bytes, the views' fields empty
inline TextureLayout texture_layout(size_t V, size_t T, size_t n_views, bool rgb, size_t pixels, size_t image_bytes, size_t atlas_bytes)
{
    TextureLayout l;
    ScratchCarver a, b, c, d;
    l.vertices = a.take(sizeof(float) * 3 * V);
    l.tri = a.take(sizeof(int32_t) * 3 * T);
    l.rgb = a.take(rgb ? 3 * V : 0);
    l.cams = a.take(sizeof(TextureCam) * n_views);
    l.label = a.take(sizeof(int32_t) * T);
    l.score = a.take(sizeof(float) * T);
    l.a_bytes = a.at;
    l.proj = b.take(pixels ? 16 * n_views * V : 0);
    l.buffers = b.take(sizeof(uint32_t) * n_views * pixels);
    l.list = b.take(pixels ? sizeof(uint32_t) * n_views * T : 0);
    l.count = b.take(pixels ? sizeof(uint32_t) : 0);
    l.b_bytes = b.at;
    l.images = c.take(image_bytes);
    l.c_bytes = c.at;
    l.atlas = d.take(atlas_bytes);
    l.d_bytes = d.at;
    return l;
}

}  // namespace esfm
