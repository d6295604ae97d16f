// Launch interface between level_api.cpp and level_kernels.hip (esfm_mesh_texture_level).
#pragma once

#include "common.hpp"
#include "level_check.hpp"

namespace esfm {

constexpr int kLevelRz = 0, kLevelAlpha = 3, kLevelBeta = 6, kLevelRr = 9, kLevelBb = 12;   // the scalars' places, 3 channels each

struct LevelArgs {
    const float *vertices;        // V x 3, finite (checked on the host)
    const int32_t *tri;           // T x 3, every index in 0 .. V - 1 (checked on the host)
    const int32_t *label;         // T, every value in -1 .. n - 1 (checked on the host)
    const TextureCam *cams;
    const uint8_t *images;        // n x rows x cols x channels
    int32_t V, T, rows, cols, channels;
    int32_t N;                    // nodes: known once the node table stands
    int64_t stride;               // elements between the channels of a vector
    int64_t partials;             // ... and between the channels of a set of block partials
    double lambda, mu;
    uint64_t *corner_keys;        // 3 T: vertex * 64 + label, or V * 64 where the triangle does not take part
    const uint64_t *sorted;       // ... sorted
    int32_t *head_blocks;         // per 256 sorted keys: run heads, then their exclusive offset; the total behind them
    uint64_t *node_keys;          // N distinct keys in ascending order
    int32_t *corner_node;         // 3 T: the corner's node; 0 where the triangle does not take part (its three edges then vanish)
    int32_t *seam_first, *seam_last;   // N: the run of nodes of the node's vertex
    const int32_t *col, *row_start;    // the smoothness neighbours as a CSR over the nodes
    int32_t *counters;            // [0] seam vertices (zero before the launches)
    float *f;                     // 3 x stride samples
    double *d, *g, *r, *p, *q;    // stride; 3 x stride each
    double *part_a, *part_b;      // 3 x partials block sums each, reduced in place by the scalar kernel
    double *scalars;              // rz[3], alpha[3], beta[3], rr[3], bb[3]
    float *offsets, *samples;     // T x 3 x 3 each
};

int launch_level_corner_keys(hipStream_t st, const LevelArgs &a);    // corner_keys
int launch_level_node_keys(hipStream_t st, const LevelArgs &a);      // from the sorted corner keys: node_keys, the count behind head_blocks
int launch_level_nodes(hipStream_t st, const LevelArgs &a);          // f, seam runs, the seam-vertex count, corner_node (needs N)
int launch_level_start(hipStream_t st, const LevelArgs &a);          // d, g = 0, r = rhs, p = r / d; rz and bb in the scalars
int launch_level_step(hipStream_t st, const LevelArgs &a);           // q = A p, alpha, g and r, rr and rz', beta: rr is ready to be read
int launch_level_direction(hipStream_t st, const LevelArgs &a);      // p = r / d + beta p
int launch_level_outputs(hipStream_t st, const LevelArgs &a);        // offsets, samples

}  // namespace esfm
