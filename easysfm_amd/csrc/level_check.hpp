// Host-only part of esfm_mesh_texture_level / esfm_mesh_texture_bake_ex (include/esfm.h, "Mesh texturing", seam levelling), free of
// HIP so that tests/cpp/level_check_main.cpp runs it under the sanitizers with g++ alone: the argument checks, which read the
// caller's arrays and return before any device call, the host's copy of tree_sum, and the byte layout of the scratch buffers.
#pragma once

#include <vector>

#include "texture_check.hpp"

namespace esfm {

constexpr int kLevelMaxIterations = 10000;

// Everything esfm_mesh_texture_level rejects with ESFM_ERR_INVALID_ARG.  Reads, writes nothing.
inline int level_check_args(int V, int T, const float *vertices, const int32_t *triangles, const int32_t *label, int n_views, int rows, int cols,
                            int channels, const uint8_t *images, const float *K4, const float *poses, const esfm_mesh_texture_level_options *o,
                            const float *offsets, const esfm_mesh_texture_level_stats *stats)
{
    ESFM_REQUIRE(o, "options are NULL");
    ESFM_REQUIRE(std::isfinite(o->lambda) && o->lambda > 0.0, "lambda must be finite and > 0");
    ESFM_REQUIRE(std::isfinite(o->mu) && o->mu > 0.0, "mu must be finite and > 0");
    ESFM_REQUIRE(o->tolerance >= 0.0 && o->tolerance < 1.0, "tolerance must be in [0, 1)");               // (a NaN fails both)
    ESFM_REQUIRE(o->max_iterations >= 0 && o->max_iterations <= kLevelMaxIterations, "max_iterations must be 0..10000");
    ESFM_REQUIRE(stats, "NULL argument");
    ESFM_REQUIRE(channels == 1 || channels == 3, "channels must be 1 or 3");
    if (int rc = texture_check_mesh(V, T, vertices, triangles)) return rc;
    if (int rc = texture_check_cameras(n_views, rows, cols, K4, poses)) return rc;
    ESFM_REQUIRE(images, "NULL argument");
    ESFM_REQUIRE(T == 0 || (label && offsets), "NULL argument");
    for (int t = 0; t < T; ++t) ESFM_REQUIRE(label[t] >= -1 && label[t] < n_views, "a label is outside -1..n_views-1");
    return ESFM_OK;
}

// What esfm_mesh_texture_bake_ex rejects beyond esfm_mesh_texture_bake's own list.
inline int level_check_offsets(int T, const float *offsets)
{
    if (!offsets) return ESFM_OK;
    for (size_t i = 0; i < 9 * (size_t)(T > 0 ? T : 0); ++i) ESFM_REQUIRE(std::isfinite(offsets[i]), "an offset is not finite");
    return ESFM_OK;
}

// The header's tree_sum, as the kernels add: blocks of 256 padded with +0.0, halved from 128 down to 1, the block results again.
inline double level_tree_sum(const double *x, size_t n)
{
    if (n == 0) return 0.0;
    std::vector<double> level(x, x + n);
    for (;;) {
        const size_t blocks = (level.size() + 255) / 256;
        level.resize(blocks * 256, 0.0);
        for (size_t b = 0; b < blocks; ++b) {
            double *s = level.data() + 256 * b;
            for (size_t h = 128; h >= 1; h >>= 1)
                for (size_t i = 0; i < h; ++i) s[i] += s[i + h];
            level[b] = s[0];
        }
        level.resize(blocks);
        if (blocks == 1) return level[0];
    }
}

// The stopping rule of one iteration: rr <= tolerance^2 bb in every channel.
inline bool level_converged(const double rr[3], const double bb[3], double tolerance)
{
    const double t2 = tolerance * tolerance;
    return rr[0] <= t2 * bb[0] && rr[1] <= t2 * bb[1] && rr[2] <= t2 * bb[2];
}

// Byte offsets of the arrays inside the context's scratch buffers; every array starts on a multiple of 256 bytes.  The number of
// nodes is known only on the device, so everything per node is laid out for its bound, the 3 T corners.
struct LevelLayout {
    size_t corners, stride, partials;   // 3 T; a vector's channel stride in elements (3 T rounded up to 256); block partials per channel
    // stage_a: the mesh, the labels, the cameras
    size_t vertices, tri, label, cams, a_bytes;
    // stage_b: 6 T directed keys and their sorted copy (the 3 T corner keys are sorted through the same pair), the run heads before
    // each sorted key, the head counts per 256 keys with their total, the sort's own scratch
    size_t keys, sorted, head_rank, head_blocks, sort, b_bytes;
    // stage_c: the images
    size_t images, c_bytes;
    // stage_d: corner keys, node keys, corner -> node, each node's seam run, the smoothness CSR, the samples (f32, 3 channels), the
    // diagonal, g, r, p, q (f64, 3 channels each), two sets of block partials, the scalars, the counters, and both outputs
    size_t corner_keys, node_keys, corner_node, seam_first, seam_last, col, row_start, pinned, f, d, g, r, p, q, part_a, part_b, scalars,
        counters, offsets, samples, d_bytes;
};

constexpr size_t kLevelScalars = 15;    // rz, alpha, beta, rr, bb: 3 doubles each

inline LevelLayout level_layout(size_t V, size_t T, size_t n_views, size_t image_bytes, size_t sort_bytes)
{
    LevelLayout l;
    l.corners = 3 * T;
    l.stride = (l.corners + 255) / 256 * 256;
    l.partials = (l.stride / 256 + 255) / 256 * 256;
    ScratchCarver a, b, c, d;
    l.vertices = a.take(sizeof(float) * 3 * V);
    l.tri = a.take(sizeof(int32_t) * 3 * T);
    l.label = a.take(sizeof(int32_t) * T);
    l.cams = a.take(sizeof(TextureCam) * n_views);
    l.a_bytes = a.at;
    l.keys = b.take(sizeof(uint64_t) * 6 * T);
    l.sorted = b.take(sizeof(uint64_t) * 6 * T);
    l.head_rank = b.take(sizeof(int32_t) * (6 * T + 1));
    l.head_blocks = b.take(sizeof(int32_t) * ((6 * T + 255) / 256 + 1));
    l.sort = b.take(sort_bytes);
    l.b_bytes = b.at;
    l.images = c.take(image_bytes);
    l.c_bytes = c.at;
    l.corner_keys = d.take(sizeof(uint64_t) * l.corners);
    l.node_keys = d.take(sizeof(uint64_t) * l.corners);
    l.corner_node = d.take(sizeof(int32_t) * l.corners);
    l.seam_first = d.take(sizeof(int32_t) * l.corners);
    l.seam_last = d.take(sizeof(int32_t) * l.corners);
    l.col = d.take(sizeof(int32_t) * 6 * T);
    l.row_start = d.take(sizeof(int32_t) * (l.corners + 1));
    l.pinned = d.take(l.corners);
    l.f = d.take(sizeof(float) * 3 * l.stride);
    l.d = d.take(sizeof(double) * l.stride);
    l.g = d.take(sizeof(double) * 3 * l.stride);
    l.r = d.take(sizeof(double) * 3 * l.stride);
    l.p = d.take(sizeof(double) * 3 * l.stride);
    l.q = d.take(sizeof(double) * 3 * l.stride);
    l.part_a = d.take(sizeof(double) * 3 * l.partials);
    l.part_b = d.take(sizeof(double) * 3 * l.partials);
    l.scalars = d.take(sizeof(double) * kLevelScalars);
    l.counters = d.take(sizeof(int32_t) * 4);
    l.offsets = d.take(sizeof(float) * 9 * T);
    l.samples = d.take(sizeof(float) * 9 * T);
    l.d_bytes = d.at;
    return l;
}

}  // namespace esfm
