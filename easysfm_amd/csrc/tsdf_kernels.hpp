// Launch interface between tsdf_api.cpp and tsdf_kernels.hip (include/esfm.h, "Surface reconstruction").
#pragma once

#include "common.hpp"

namespace esfm {

constexpr int kTsdfMaxViews = 64;      // views of one integration: their cameras fit one 4.25 KiB LDS table

struct TsdfCam {            // an integrated view (one with a positive depth somewhere)
    float K[4];             // fx, cx, fy, cy
    float P[12];            // [R | t] row-major
    int32_t view;           // its index into depth / images
};

struct TsdfVolume {         // device arrays of one grid, n = nx ny nz voxels each
    float origin[3], h;
    int32_t nx, ny, nz, n;
    float *tsdf;
    int32_t *weight;
    uint8_t *rgb;           // 3 per voxel, NULL = no colours
};

struct TsdfIntegrateArgs {
    TsdfVolume vol;
    const TsdfCam *cams;    // n_cams <= kTsdfMaxViews, in view order
    const float *depth;     // n_views x rows x cols
    const uint8_t *images;  // n_views x rows x cols x channels, NULL = no colours
    int32_t n_cams, rows, cols, channels;
    float trunc;
};

struct TsdfExtractArgs {
    TsdfVolume vol;
    int32_t min_weight, n_blocks;      // 256-voxel blocks of the linear index
    uint8_t *state;         // per voxel: bit 0 valid, bit 1 inside
    uint8_t *edge_mask;     // per voxel: its used edges, bit e
    uint8_t *tri_count;     // per voxel: triangles of its cell
    int32_t *vertex_base;   // per voxel: id of its first vertex
    int32_t *block_vertices, *block_triangles;   // per block counts, then their exclusive offsets; [n_blocks] = the total
    float *vertices, *normals;                   // output (normals, vertex_rgb may be NULL)
    uint8_t *vertex_rgb;
    int32_t *triangles;
};

int launch_tsdf_integrate(hipStream_t st, const TsdfIntegrateArgs &a);
int launch_tsdf_classify(hipStream_t st, const TsdfExtractArgs &a);    // state, masks and counts, both scans
int launch_tsdf_mesh(hipStream_t st, const TsdfExtractArgs &a);        // vertices, then triangles

}  // namespace esfm
