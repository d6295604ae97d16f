// Launch interface between simplify_api.cpp and simplify_kernels.hip (esfm_mesh_simplify).  The sorts are voxel_sort.hip's
// (64-bit key, index) pairs and mesh_sort.hip's keys; the normals are mesh_kernels.hip's.
#pragma once

#include "common.hpp"
#include "simplify_check.hpp"

namespace esfm {

struct SimplifyArgs {
    const float *vertices;       // V x 3
    const uint8_t *rgb;          // V x 3, may be NULL
    const int32_t *tri;          // T x 3, every index in 0 .. V - 1 (checked on the host)
    int32_t V, T;
    float origin[3], cell, regularisation;
    int32_t use_quadric;
    uint64_t *key_in;            // the list being sorted: V cell keys, then 3 T corner keys, then T grouping keys
    const uint64_t *key_out;     // ... and after its sort
    int32_t *val_in;             // the index that travels with a cell key (vertex) or a grouping key (triangle)
    const int32_t *val_out;
    int32_t *cell_blocks;        // per 256 sorted vertices: run heads, then their exclusive offset; the total C behind them
    int32_t *cell_of;            // V: cell number of each vertex
    int32_t *cell_start;         // C + 1: first position of each cell in the sorted vertex list
    uint64_t *cell_key;          // C: the cell's key (aliases nothing that is sorted later)
    float *rep;                  // C x 3: representatives
    uint8_t *rep_rgb;            // C x 3, NULL without rgb
    uint8_t *keep;               // T (zero before the vote)
    uint8_t *used;               // V (zero before the vote): cells a kept triangle names
    int32_t *used_blocks;        // per 256 cells: used ones, then their exclusive offset; the total behind them
    int32_t *tri_blocks;         // the same per 256 triangles
    int32_t *new_of_cell;        // V: output vertex of a used cell
    float *out_vertices;
    uint8_t *out_rgb;            // may be NULL
    int32_t *out_tri, *vertex_map, *triangle_map;   // the maps may be NULL
};

int launch_simplify_cell_keys(hipStream_t st, const SimplifyArgs &a);     // V (key, vertex) pairs into key_in / val_in
int launch_simplify_cells(hipStream_t st, const SimplifyArgs &a);         // from the sorted pairs: cell numbers, cell_of, cell_start, cell_key
int launch_simplify_corner_keys(hipStream_t st, const SimplifyArgs &a);   // 3 T (cell, 3 t + corner) keys into key_in
int launch_simplify_place(hipStream_t st, const SimplifyArgs &a);          // per cell, from val_out (sorted vertices) and key_out (sorted corners)
int launch_simplify_group_keys(hipStream_t st, const SimplifyArgs &a);    // T (grouping key, triangle) pairs into key_in / val_in
int launch_simplify_vote(hipStream_t st, const SimplifyArgs &a);          // from the sorted pairs: keep and used
int launch_simplify_compact(hipStream_t st, const SimplifyArgs &a);       // keep counts, scans, ordered writes, vertex_map

}  // namespace esfm
