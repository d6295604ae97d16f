// Host-only part of esfm_mesh_simplify (include/esfm.h, "Mesh simplification"), free of HIP so that tests/cpp/simplify_check_main.cpp
// runs it under the sanitizers with g++ alone: the argument checks, which read the caller's arrays and return before any device
// call, and the byte layout of the four scratch buffers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "mesh_check.hpp"
#include "scratch_layout.hpp"

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
    if (int rc = check_mesh(V, T, triangles)) return rc;
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

inline SimplifyLayout simplify_layout(size_t V, size_t T, bool rgb, bool normals, bool vertex_map, bool triangle_map, size_t sort_bytes)
{
    SimplifyLayout l;
    const size_t vb = (V + 255) / 256, tb = (T + 255) / 256, keys = 3 * T > V ? 3 * T : V, vals = T > V ? T : V;
    ScratchCarver a, b, c, d;
    l.vertices = a.take(sizeof(float) * 3 * V);
    l.rgb = a.take(rgb ? 3 * V : 0);
    l.tri = a.take(sizeof(int32_t) * 3 * T);
    l.cell_of = a.take(sizeof(int32_t) * V);
    l.cell_start = a.take(sizeof(int32_t) * (V + 1));
    l.cell_key = a.take(sizeof(uint64_t) * V);
    l.new_of_cell = a.take(sizeof(int32_t) * V);
    l.used = a.take(V);
    l.keep = a.take(T);
    l.cell_blocks = a.take(sizeof(int32_t) * (vb + 1));
    l.used_blocks = a.take(sizeof(int32_t) * (vb + 1));
    l.tri_blocks = a.take(sizeof(int32_t) * (tb + 1));
    l.rep = a.take(sizeof(float) * 3 * V);
    l.rep_rgb = a.take(rgb ? 3 * V : 0);
    l.a_bytes = a.at;
    l.key_in = b.take(sizeof(uint64_t) * keys);
    l.key_out = b.take(sizeof(uint64_t) * keys);
    l.val_in = b.take(sizeof(int32_t) * vals);
    l.val_out = b.take(sizeof(int32_t) * vals);
    l.sort = b.take(sort_bytes);
    l.b_bytes = b.at;
    l.inc_start = c.take(normals ? sizeof(int32_t) * (V + 1) : 0);
    l.face = c.take(normals ? sizeof(float) * 3 * T : 0);
    l.c_bytes = c.at;
    l.out_vertices = d.take(sizeof(float) * 3 * V);
    l.out_normals = d.take(normals ? sizeof(float) * 3 * V : 0);
    l.out_rgb = d.take(rgb ? 3 * V : 0);
    l.out_tri = d.take(sizeof(int32_t) * 3 * T);
    l.vertex_map = d.take(vertex_map ? sizeof(int32_t) * V : 0);
    l.triangle_map = d.take(triangle_map ? sizeof(int32_t) * T : 0);
    l.d_bytes = d.at;
    return l;
}

}  // namespace esfm
