// Launch interface between mesh_api.cpp and mesh_kernels.hip / mesh_sort.hip (esfm_mesh_components, esfm_mesh_clean).
#pragma once

#include "common.hpp"
#include "scratch_layout.hpp"   // bit_width

namespace esfm {

struct MeshLabelArgs {         // components of the input mesh
    const int32_t *tri;        // T x 3, every index in 0 .. V - 1 (checked on the host)
    int32_t *parent;           // V: the union-find forest
    int32_t *label;            // V: smallest vertex index of the component
    int32_t *tri_count;        // V: triangles of the component at its label vertex, 0 elsewhere (zero before the count)
    int32_t *stats;            // [0] largest count, [1] components (zero before the launches)
    int32_t V, T;
};

struct MeshCompactArgs {       // filter and ordered compaction
    const int32_t *tri;
    const int32_t *label, *tri_count, *stats;
    const float *vertices;
    const uint8_t *rgb;        // may be NULL
    int32_t V, T, min_triangles, min_permille;
    int32_t *vertex_blocks;    // per 256-vertex block: kept vertices, then their exclusive offset; the total behind them
    int32_t *triangle_blocks;  // the same per 256 triangles
    int32_t *remap;            // V: new index of a kept vertex
    float *out_vertices;
    uint8_t *out_rgb;          // may be NULL
    int32_t *out_tri, *vertex_map, *triangle_map;
};

struct MeshGraphArgs {         // adjacency, smoothing and normals of the output mesh
    const int32_t *tri;        // T x 3 (the compacted triangles)
    int32_t V, T;
    uint64_t *keys;            // 6 T directed keys, or 3 T incidence keys, before the sort
    const uint64_t *sorted;    // ... and after it
    int32_t *head_blocks;      // per 256 sorted keys: run heads, then their exclusive offset; the total behind them
    int32_t *head_rank;        // 6 T + 1: run heads before each sorted key
    int32_t *col;              // the distinct (a, b) keys' b in key order: the CSR columns
    int32_t *row_start;        // V + 1
    uint8_t *pinned;           // V (zero before the launch)
    int32_t *inc_start;        // V + 1: first incidence key of each vertex
    float *face;               // T x 3 face vectors
};

int launch_mesh_labels(hipStream_t st, const MeshLabelArgs &a);          // init, hook, flatten, counts, largest
int launch_mesh_compact(hipStream_t st, const MeshCompactArgs &a);       // keep counts, scans, ordered writes
// The key width of both sorts below: the high word is a vertex index, or V itself for a key that names no row.  The callers size
// the sorts' scratch with it (mesh_sort_scratch_bytes), for V or for a bound of it.
inline int mesh_key_bits(int64_t V) { return 32 + bit_width((uint64_t)V); }

// the adjacency of a mesh with T >= 1: the 6 T directed keys (a == b: behind every other key), their sort, then columns, row starts
// and pinned bytes
int mesh_build_adjacency(hipStream_t st, const MeshGraphArgs &g, void *sort_tmp, size_t sort_bytes);
int launch_mesh_smooth(hipStream_t st, const MeshGraphArgs &a, const float *p, float *q, float w, int pin_boundary);
// the vertex normals of a mesh with T >= 1: the 3 T (vertex, 3 t + corner) keys, their sort, the face vectors summed in incidence order
int mesh_build_normals(hipStream_t st, const MeshGraphArgs &g, void *sort_tmp, size_t sort_bytes, const float *p, float *normals);

// mesh_sort.hip: hipCUB's device radix sort of 64-bit keys, bits 0 .. end_bit - 1
int mesh_sort_scratch_bytes(int64_t n, int end_bit, size_t *bytes, hipStream_t st);
int mesh_sort_keys(void *tmp, size_t tmp_bytes, const uint64_t *keys_in, uint64_t *keys_out, int64_t n, int end_bit, hipStream_t st);

}  // namespace esfm
