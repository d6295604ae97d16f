// C-ABI entry points of surface reconstruction (include/esfm.h, "Surface reconstruction"): esfm_tsdf_integrate,
// esfm_tsdf_extract and esfm_mvs_mesh, which chains the two with the volume staying on the device.  Host side: argument checks,
// the list of views that hold a depth, buffer layout, uploads, launches, the one read-back of the two counts that are compared
// with the capacities, and the copy of the mesh.  The voxel work runs in tsdf_kernels.hip; tests/tsdf_ref.py restates the rules.
#include <cmath>
#include <vector>

#include "scratch_layout.hpp"
#include "tsdf_kernels.hpp"

namespace {

int check_grid(const esfm_tsdf_grid *g, const esfm_tsdf_options *o)
{
    ESFM_REQUIRE(g && o, "grid or options are NULL");
    ESFM_REQUIRE(std::isfinite(g->origin[0]) && std::isfinite(g->origin[1]) && std::isfinite(g->origin[2]), "grid origin must be finite");
    ESFM_REQUIRE(g->voxel_size > 0.f && std::isfinite(g->voxel_size), "voxel_size must be finite and > 0");
    for (int c = 0; c < 3; ++c) ESFM_REQUIRE(g->dims[c] >= 2 && g->dims[c] <= 1024, "grid dims must each be 2..1024");
    ESFM_REQUIRE((int64_t)g->dims[0] * g->dims[1] * g->dims[2] <= ((int64_t)1 << 27), "the grid has more than 2^27 voxels");
    ESFM_REQUIRE(o->trunc == 0.f || (std::isfinite(o->trunc) && o->trunc >= g->voxel_size), "trunc must be 0 or finite and >= voxel_size");
    ESFM_REQUIRE(o->min_weight >= 1, "min_weight must be >= 1");
    return ESFM_OK;
}

int check_views(int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4, const float *poses, const float *depth)
{
    ESFM_REQUIRE(n_views >= 1 && n_views <= esfm::kTsdfMaxViews, "n_views must be 1..64");
    ESFM_REQUIRE(K4 && poses && depth, "NULL argument");
    ESFM_REQUIRE(rows >= 1 && cols >= 1 && rows <= 16384 && cols <= 16384, "image sides must be 1..16384");
    ESFM_REQUIRE((int64_t)n_views * rows * cols <= ((int64_t)1 << 31) - 256, "more than 2^31 pixels in one call");
    ESFM_REQUIRE(!images || channels == 1 || channels == 3, "images must be rows x cols x {1, 3}");
    for (int v = 0; v < n_views; ++v) {
        const float *k = K4 + 4 * (size_t)v;
        ESFM_REQUIRE(k[0] != 0.f && k[2] != 0.f && std::isfinite(k[0]) && std::isfinite(k[1]) && std::isfinite(k[2]) && std::isfinite(k[3]),
                     "K4 must be finite with non-zero focal lengths");
    }
    return ESFM_OK;
}

int check_mesh_outputs(bool have_rgb, int max_vertices, int max_triangles, const float *vertices, const uint8_t *vertex_rgb,
                       const int32_t *triangles, const int32_t *n_vertices, const int32_t *n_triangles)
{
    ESFM_REQUIRE(max_vertices >= 0 && max_triangles >= 0, "capacities must be >= 0");
    ESFM_REQUIRE(n_vertices && n_triangles && (max_vertices == 0 || vertices) && (max_triangles == 0 || triangles), "NULL argument");
    ESFM_REQUIRE(!vertex_rgb || have_rgb, "an output array is requested without its input");
    return ESFM_OK;
}

int check_ctx(esfm_ctx *ctx)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    return esfm::set_device(ctx);
}

// the volume's device arrays in stage_b: tsdf | weight | rgb
int place_volume(esfm_ctx *ctx, const esfm_tsdf_grid *g, bool with_rgb, esfm::TsdfVolume *vol)
{
    const size_t N = (size_t)g->dims[0] * g->dims[1] * g->dims[2];
    esfm::ScratchCarver at;
    const size_t tsdf = at.take(sizeof(float) * N), weight = at.take(sizeof(int32_t) * N), rgb = at.take(with_rgb ? 3 * N : 0);
    if (int rc = ctx->stage_b.reserve(at.at)) return rc;
    uint8_t *p = ctx->stage_b.as<uint8_t>();
    for (int c = 0; c < 3; ++c) vol->origin[c] = g->origin[c];
    vol->h = g->voxel_size;
    vol->nx = g->dims[0]; vol->ny = g->dims[1]; vol->nz = g->dims[2]; vol->n = (int32_t)N;
    vol->tsdf = reinterpret_cast<float *>(p + tsdf);
    vol->weight = reinterpret_cast<int32_t *>(p + weight);
    vol->rgb = with_rgb ? p + rgb : nullptr;
    return ESFM_OK;
}

// uploads the views (stage_a: depth | images | cameras) and integrates them into the placed volume
int integrate(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4, const float *poses,
              const float *depth, const esfm_tsdf_options *opt, const esfm::TsdfVolume &vol)
{
    hipStream_t st = ctx->stream;
    const size_t plane = (size_t)rows * cols, n_px = plane * n_views;
    std::vector<esfm::TsdfCam> cams;
    for (int v = 0; v < n_views; ++v) {
        const float *d = depth + plane * v;
        bool any = false;
        for (size_t i = 0; i < plane && !any; ++i) any = d[i] > 0.f;
        if (!any) continue;                                    // (no pixel of it can pass the rule's d > 0)
        esfm::TsdfCam c;
        memcpy(c.K, K4 + 4 * (size_t)v, sizeof(c.K));
        memcpy(c.P, poses + 12 * (size_t)v, sizeof(c.P));
        c.view = v;
        cams.push_back(c);
    }
    esfm::ScratchCarver at;
    const size_t dep = at.take(sizeof(float) * n_px), img = at.take(images ? n_px * channels : 0), cam = at.take(sizeof(esfm::TsdfCam) * esfm::kTsdfMaxViews);
    if (int rc = ctx->stage_a.reserve(at.at)) return rc;
    uint8_t *p = ctx->stage_a.as<uint8_t>();
    esfm::TsdfIntegrateArgs a;
    a.vol = vol;
    a.depth = reinterpret_cast<const float *>(p + dep);
    a.images = images ? p + img : nullptr;
    a.cams = reinterpret_cast<const esfm::TsdfCam *>(p + cam);
    a.n_cams = (int32_t)cams.size(); a.rows = rows; a.cols = cols; a.channels = images ? channels : 1;
    a.trunc = opt->trunc == 0.f ? 4.0f * vol.h : opt->trunc;
    if (!cams.empty()) {
        ESFM_HIP_TRY(esfm::copy_h2d(p + dep, depth, sizeof(float) * n_px, st));
        if (images) ESFM_HIP_TRY(esfm::copy_h2d(p + img, images, n_px * channels, st));
        ESFM_HIP_TRY(esfm::copy_h2d(p + cam, cams.data(), sizeof(esfm::TsdfCam) * cams.size(), st));
    }
    return esfm::launch_tsdf_integrate(st, a);
}

// the mesh of the placed volume; stage_c: per-voxel state | edge masks | triangle counts | vertex bases | block counts,
// stage_d: the mesh
int extract(esfm_ctx *ctx, const esfm::TsdfVolume &vol, const esfm_tsdf_options *opt, int max_vertices, int max_triangles, float *vertices,
            float *normals, uint8_t *vertex_rgb, int32_t *triangles, int32_t *n_vertices, int32_t *n_triangles)
{
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)vol.n, n_blocks = (N + 255) / 256;
    esfm::ScratchCarver work;
    const size_t state = work.take(N), edge_mask = work.take(N), tri_count = work.take(N), vertex_base = work.take(sizeof(int32_t) * N),
                 block_vertices = work.take(sizeof(int32_t) * (n_blocks + 1)), block_triangles = work.take(sizeof(int32_t) * (n_blocks + 1));
    if (int rc = ctx->stage_c.reserve(work.at)) return rc;
    uint8_t *p = ctx->stage_c.as<uint8_t>();
    esfm::TsdfExtractArgs a;
    memset(&a, 0, sizeof(a));
    a.vol = vol;
    a.min_weight = opt->min_weight; a.n_blocks = (int32_t)n_blocks;
    a.state = p + state; a.edge_mask = p + edge_mask; a.tri_count = p + tri_count;
    a.vertex_base = reinterpret_cast<int32_t *>(p + vertex_base);
    a.block_vertices = reinterpret_cast<int32_t *>(p + block_vertices);
    a.block_triangles = reinterpret_cast<int32_t *>(p + block_triangles);
    if (int rc = esfm::launch_tsdf_classify(st, a)) return rc;
    int32_t nv = 0, nt = 0;
    ESFM_HIP_TRY(esfm::copy_d2h(&nv, a.block_vertices + n_blocks, sizeof(int32_t), st));
    ESFM_HIP_TRY(esfm::copy_d2h(&nt, a.block_triangles + n_blocks, sizeof(int32_t), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    if (nv < 0 || nt < 0) { esfm::set_error("tsdf extract: %d vertices and %d triangles counted", nv, nt); return ESFM_ERR_NUMERIC; }
    *n_vertices = nv; *n_triangles = nt;
    if (nv > max_vertices || nt > max_triangles) {
        esfm::set_error("the mesh has %d vertices and %d triangles, the capacities are %d and %d", nv, nt, max_vertices, max_triangles);
        return ESFM_ERR_INVALID_ARG;
    }
    if (nv == 0) return ESFM_OK;                               // (no vertex: no triangle either)
    const size_t V = (size_t)nv, T = (size_t)nt;
    esfm::ScratchCarver out;
    const size_t o_vtx = out.take(sizeof(float) * 3 * V), o_nrm = out.take(normals ? sizeof(float) * 3 * V : 0), o_rgb = out.take(vertex_rgb ? 3 * V : 0),
                 o_tri = out.take(sizeof(int32_t) * 3 * T);
    if (int rc = ctx->stage_d.reserve(out.at)) return rc;
    uint8_t *o = ctx->stage_d.as<uint8_t>();
    a.vertices = reinterpret_cast<float *>(o + o_vtx);
    a.normals = normals ? reinterpret_cast<float *>(o + o_nrm) : nullptr;
    a.vertex_rgb = vertex_rgb ? o + o_rgb : nullptr;
    a.triangles = reinterpret_cast<int32_t *>(o + o_tri);
    if (int rc = esfm::launch_tsdf_mesh(st, a)) return rc;
    ESFM_HIP_TRY(esfm::copy_d2h(vertices, a.vertices, sizeof(float) * 3 * V, st));
    if (normals) ESFM_HIP_TRY(esfm::copy_d2h(normals, a.normals, sizeof(float) * 3 * V, st));
    if (vertex_rgb) ESFM_HIP_TRY(esfm::copy_d2h(vertex_rgb, a.vertex_rgb, 3 * V, st));
    if (T) ESFM_HIP_TRY(esfm::copy_d2h(triangles, a.triangles, sizeof(int32_t) * 3 * T, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

}  // namespace

extern "C" {

void esfm_tsdf_options_default(esfm_tsdf_options *opt)
{
    if (!opt) return;
    opt->trunc = 0.f;
    opt->min_weight = 2;
}

int esfm_tsdf_integrate(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4, const float *poses,
                        const float *depth, const esfm_tsdf_grid *grid, const esfm_tsdf_options *opt, float *tsdf, int32_t *weight,
                        uint8_t *rgb)
{
    if (int rc = check_grid(grid, opt)) return rc;
    if (int rc = check_views(n_views, rows, cols, channels, images, K4, poses, depth)) return rc;
    ESFM_REQUIRE(tsdf && weight, "NULL argument");
    ESFM_REQUIRE(!rgb || images, "an output array is requested without its input");
    if (int rc = check_ctx(ctx)) return rc;
    esfm::TsdfVolume vol;
    if (int rc = place_volume(ctx, grid, rgb != nullptr, &vol)) return rc;
    if (int rc = integrate(ctx, n_views, rows, cols, channels, rgb ? images : nullptr, K4, poses, depth, opt, vol)) return rc;
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)vol.n;
    ESFM_HIP_TRY(esfm::copy_d2h(tsdf, vol.tsdf, sizeof(float) * N, st));
    ESFM_HIP_TRY(esfm::copy_d2h(weight, vol.weight, sizeof(int32_t) * N, st));
    if (rgb) ESFM_HIP_TRY(esfm::copy_d2h(rgb, vol.rgb, 3 * N, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

int esfm_tsdf_extract(esfm_ctx *ctx, const esfm_tsdf_grid *grid, const float *tsdf, const int32_t *weight, const uint8_t *rgb,
                      const esfm_tsdf_options *opt, int max_vertices, int max_triangles, float *vertices, float *normals, uint8_t *vertex_rgb,
                      int32_t *triangles, int32_t *n_vertices, int32_t *n_triangles)
{
    if (int rc = check_grid(grid, opt)) return rc;
    ESFM_REQUIRE(tsdf && weight, "NULL argument");
    if (int rc = check_mesh_outputs(rgb != nullptr, max_vertices, max_triangles, vertices, vertex_rgb, triangles, n_vertices, n_triangles)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    esfm::TsdfVolume vol;
    const bool with_rgb = rgb && vertex_rgb;
    if (int rc = place_volume(ctx, grid, with_rgb, &vol)) return rc;
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)vol.n;
    ESFM_HIP_TRY(esfm::copy_h2d(vol.tsdf, tsdf, sizeof(float) * N, st));
    ESFM_HIP_TRY(esfm::copy_h2d(vol.weight, weight, sizeof(int32_t) * N, st));
    if (with_rgb) ESFM_HIP_TRY(esfm::copy_h2d(vol.rgb, rgb, 3 * N, st));
    return extract(ctx, vol, opt, max_vertices, max_triangles, vertices, normals, vertex_rgb, triangles, n_vertices, n_triangles);
}

int esfm_mvs_mesh(esfm_ctx *ctx, int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4, const float *poses,
                  const float *depth, const esfm_tsdf_grid *grid, const esfm_tsdf_options *opt, int max_vertices, int max_triangles,
                  float *vertices, float *normals, uint8_t *vertex_rgb, int32_t *triangles, int32_t *n_vertices, int32_t *n_triangles)
{
    if (int rc = check_grid(grid, opt)) return rc;
    if (int rc = check_views(n_views, rows, cols, channels, images, K4, poses, depth)) return rc;
    if (int rc = check_mesh_outputs(images != nullptr, max_vertices, max_triangles, vertices, vertex_rgb, triangles, n_vertices, n_triangles)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    esfm::TsdfVolume vol;
    const bool with_rgb = images && vertex_rgb;
    if (int rc = place_volume(ctx, grid, with_rgb, &vol)) return rc;
    if (int rc = integrate(ctx, n_views, rows, cols, channels, with_rgb ? images : nullptr, K4, poses, depth, opt, vol)) return rc;
    return extract(ctx, vol, opt, max_vertices, max_triangles, vertices, normals, vertex_rgb, triangles, n_vertices, n_triangles);
}

}  // extern "C"
