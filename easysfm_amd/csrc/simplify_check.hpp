// Host-only part of esfm_mesh_simplify (include/esfm.h, "Mesh simplification"), free of HIP so that tests/cpp/simplify_check_main.cpp
// runs it under the sanitizers with g++ alone: the argument checks, which read the caller's arrays and return before any device
// call, and the byte layout of the four scratch buffers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "error.hpp"

namespace esfm {

#if defined(__HIPCC__)
#define ESFM_SIMPLIFY_HD __host__ __device__
#else
#define ESFM_SIMPLIFY_HD
#endif

constexpr int32_t kSimplifyMaxIndex = (1 << 21) - 1;   // cell index per axis, and the largest cell number a grouping key holds
constexpr int32_t kSimplifyMaxCells = 1 << 21;

// (p - origin) / cell in f32, floored: the kernel's own expression (simplify_kernels.hip), so host and device agree on every vertex
ESFM_SIMPLIFY_HD inline float simplify_cell_coordinate(float p, float origin, float cell) { return floorf((p - origin) / cell); }

// Everything esfm_mesh_simplify rejects with ESFM_ERR_INVALID_ARG.  Reads, writes nothing.
inline int simplify_check_args(int V, int T, const float *vertices, const uint8_t *vertex_rgb, const int32_t *triangles, const float *origin,
                               float cell, const esfm_mesh_simplify_options *o, const float *out_vertices, const uint8_t *out_rgb,
                               const int32_t *out_triangles, const int32_t *n_out_vertices, const int32_t *n_out_triangles)
{
    ESFM_REQUIRE(o, "options are NULL");
    ESFM_REQUIRE(std::isfinite(o->regularisation) && o->regularisation > 0.f && o->regularisation <= 1.f, "regularisation must be finite and in (0, 1]");
    ESFM_REQUIRE(o->use_quadric == 0 || o->use_quadric == 1, "use_quadric must be 0 or 1");
    ESFM_REQUIRE(n_out_vertices && n_out_triangles && origin, "NULL argument");
    ESFM_REQUIRE(V <= 0 || (vertices && out_vertices), "NULL argument");
    ESFM_REQUIRE(T <= 0 || out_triangles, "NULL argument");
    ESFM_REQUIRE(!out_rgb || vertex_rgb, "an output array is requested without its input");
    ESFM_REQUIRE(V >= 0 && V <= (1 << 30), "n_vertices must be 0..2^30");
    ESFM_REQUIRE(T >= 0 && T <= (1 << 28), "n_triangles must be 0..2^28");
    ESFM_REQUIRE(T == 0 || triangles, "NULL argument");
    for (size_t i = 0; i < 3 * (size_t)T; ++i) ESFM_REQUIRE(triangles[i] >= 0 && triangles[i] < V, "a triangle index is outside 0..n_vertices-1");
    ESFM_REQUIRE(std::isfinite(cell) && cell > 0.f, "cell must be finite and > 0");
    ESFM_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "origin must be finite");
    for (size_t i = 0; i < 3 * (size_t)V; ++i) {
        const float q = simplify_cell_coordinate(vertices[i], origin[i % 3], cell);
        ESFM_REQUIRE(q >= 0.f && q <= (float)kSimplifyMaxIndex, "a vertex lies outside the grid's 2^21 cells per axis");   // (NaN fails both)
    }
    return ESFM_OK;
}

// Byte offsets of the arrays inside the context's four scratch buffers; every array starts on a multiple of 256 bytes.
struct SimplifyLayout {
    // stage_a: what lives through the whole call
    size_t vertices, rgb, tri, cell_of, cell_start, cell_key, new_of_cell, used, keep, cell_blocks, used_blocks, tri_blocks, rep, rep_rgb, a_bytes;
    // stage_b: two key arrays and two value arrays of the largest list, then the sorts' scratch
    size_t key_in, key_out, val_in, val_out, sort, b_bytes;
    // stage_c: the normals' incidence starts and face vectors
    size_t inc_start, face, c_bytes;
    // stage_d: the outputs
    size_t out_vertices, out_normals, out_rgb, out_tri, vertex_map, triangle_map, d_bytes;
};

inline size_t simplify_align(size_t b) { return (b + 255) / 256 * 256; }

inline SimplifyLayout simplify_layout(size_t V, size_t T, bool rgb, bool normals, bool vertex_map, bool triangle_map, size_t sort_bytes)
{
    SimplifyLayout l;
    const size_t vb = (V + 255) / 256, tb = (T + 255) / 256, keys = 3 * T > V ? 3 * T : V, vals = T > V ? T : V;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += simplify_align(bytes); return here; };
    l.vertices = take(sizeof(float) * 3 * V);
    l.rgb = take(rgb ? 3 * V : 0);
    l.tri = take(sizeof(int32_t) * 3 * T);
    l.cell_of = take(sizeof(int32_t) * V);
    l.cell_start = take(sizeof(int32_t) * (V + 1));
    l.cell_key = take(sizeof(uint64_t) * V);
    l.new_of_cell = take(sizeof(int32_t) * V);
    l.used = take(V);
    l.keep = take(T);
    l.cell_blocks = take(sizeof(int32_t) * (vb + 1));
    l.used_blocks = take(sizeof(int32_t) * (vb + 1));
    l.tri_blocks = take(sizeof(int32_t) * (tb + 1));
    l.rep = take(sizeof(float) * 3 * V);
    l.rep_rgb = take(rgb ? 3 * V : 0);
    l.a_bytes = at;
    at = 0;
    l.key_in = take(sizeof(uint64_t) * keys);
    l.key_out = take(sizeof(uint64_t) * keys);
    l.val_in = take(sizeof(int32_t) * vals);
    l.val_out = take(sizeof(int32_t) * vals);
    l.sort = take(sort_bytes);
    l.b_bytes = at;
    at = 0;
    l.inc_start = take(normals ? sizeof(int32_t) * (V + 1) : 0);
    l.face = take(normals ? sizeof(float) * 3 * T : 0);
    l.c_bytes = at;
    at = 0;
    l.out_vertices = take(sizeof(float) * 3 * V);
    l.out_normals = take(normals ? sizeof(float) * 3 * V : 0);
    l.out_rgb = take(rgb ? 3 * V : 0);
    l.out_tri = take(sizeof(int32_t) * 3 * T);
    l.vertex_map = take(vertex_map ? sizeof(int32_t) * V : 0);
    l.triangle_map = take(triangle_map ? sizeof(int32_t) * T : 0);
    l.d_bytes = at;
    return l;
}

}  // namespace esfm
