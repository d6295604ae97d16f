// C-ABI entry point of the seam levelling (include/esfm.h, "Mesh texturing"): esfm_mesh_texture_level.  Host side: the argument
// checks and the scratch layout (level_check.hpp), uploads, the launches of the node table, of the smoothness adjacency (the
// clean-up's kernels over the corner -> node table) and of the conjugate gradients, whose stopping rule the host applies to the
// three r r values it reads back after every iteration, and the copies back.  The work runs in level_kernels.hip;
// tests/level_ref.py restates the rule.  esfm_mesh_texture_bake_ex is in texture_api.cpp.
#include "level_kernels.hpp"
#include "mesh_kernels.hpp"

extern "C" {

void esfm_mesh_texture_level_options_default(esfm_mesh_texture_level_options *opt)
{
    if (!opt) return;
    opt->lambda = 0.1;
    opt->mu = 0.001;
    opt->tolerance = 1e-4;
    opt->max_iterations = 200;
}

int esfm_mesh_texture_level(esfm_ctx *ctx, int n_vertices, int n_triangles, const float *vertices, const int32_t *triangles, const int32_t *label,
                            int n_views, int rows, int cols, int channels, const uint8_t *images, const float *K4, const float *poses,
                            const esfm_mesh_texture_level_options *opt, float *offsets, float *samples, esfm_mesh_texture_level_stats *stats)
{
    if (int rc = esfm::level_check_args(n_vertices, n_triangles, vertices, triangles, label, n_views, rows, cols, channels, images, K4, poses, opt, offsets,
                                        stats)) return rc;
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(ctx)) return rc;
    const esfm_mesh_texture_level_stats nothing = {0, 0, 0, 1};
    if (n_triangles == 0) { *stats = nothing; return ESFM_OK; }
    hipStream_t st = ctx->stream;
    const size_t V = (size_t)n_vertices, T = (size_t)n_triangles, n = (size_t)n_views, image_bytes = n * rows * cols * channels;
    const int64_t n_corners = 3 * (int64_t)T, n_edges = 6 * (int64_t)T;

    // all scratch before the first launch: the number of nodes is not known yet, so the layout takes its bound, the corners
    const int corner_bits = 6 + esfm::bit_width((uint64_t)V), edge_bits_max = esfm::mesh_key_bits(n_corners);
    size_t sort_corners = 0, sort_edges = 0;
    if (int rc = esfm::mesh_sort_scratch_bytes(n_corners, corner_bits, &sort_corners, st)) return rc;
    if (int rc = esfm::mesh_sort_scratch_bytes(n_edges, edge_bits_max, &sort_edges, st)) return rc;
    const size_t sort_b = sort_corners > sort_edges ? sort_corners : sort_edges;
    const esfm::LevelLayout l = esfm::level_layout(V, T, n, image_bytes, sort_b);
    if (int rc = ctx->stage_a.reserve(l.a_bytes)) return rc;
    if (int rc = ctx->stage_b.reserve(l.b_bytes)) return rc;
    if (int rc = ctx->stage_c.reserve(l.c_bytes)) return rc;
    if (int rc = ctx->stage_d.reserve(l.d_bytes)) return rc;
    const size_t cams_b = esfm::align256(sizeof(esfm::TextureCam) * n);
    if (int rc = ctx->pin(cams_b + 256)) return rc;
    uint8_t *p_a = ctx->stage_a.as<uint8_t>(), *p_b = ctx->stage_b.as<uint8_t>(), *p_c = ctx->stage_c.as<uint8_t>(), *p_d = ctx->stage_d.as<uint8_t>();
    esfm::TextureCam *cams = static_cast<esfm::TextureCam *>(ctx->pinned);
    double *mail = reinterpret_cast<double *>(static_cast<uint8_t *>(ctx->pinned) + cams_b);     // the read-backs land here
    for (int v = 0; v < n_views; ++v) {
        memcpy(cams[v].K, K4 + 4 * v, sizeof(float) * 4);
        memcpy(cams[v].P, poses + 12 * v, sizeof(float) * 12);
    }
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.vertices, vertices, sizeof(float) * 3 * V, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.tri, triangles, sizeof(int32_t) * 3 * T, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_a + l.label, label, sizeof(int32_t) * T, st));
    ESFM_HIP_TRY(hipMemcpyAsync(p_a + l.cams, cams, sizeof(esfm::TextureCam) * n, hipMemcpyHostToDevice, st));
    ESFM_HIP_TRY(esfm::copy_h2d(p_c + l.images, images, image_bytes, st));
    ESFM_HIP_TRY(hipMemsetAsync(p_d + l.counters, 0, sizeof(int32_t) * 4, st));

    esfm::LevelArgs a;
    memset(&a, 0, sizeof(a));
    a.vertices = reinterpret_cast<const float *>(p_a + l.vertices);
    a.tri = reinterpret_cast<const int32_t *>(p_a + l.tri);
    a.label = reinterpret_cast<const int32_t *>(p_a + l.label);
    a.cams = reinterpret_cast<const esfm::TextureCam *>(p_a + l.cams);
    a.images = p_c + l.images;
    a.V = n_vertices; a.T = n_triangles; a.rows = rows; a.cols = cols; a.channels = channels;
    a.stride = (int64_t)l.stride; a.partials = (int64_t)l.partials;
    a.lambda = opt->lambda; a.mu = opt->mu;
    a.corner_keys = reinterpret_cast<uint64_t *>(p_d + l.corner_keys);
    a.sorted = reinterpret_cast<const uint64_t *>(p_b + l.sorted);
    a.head_blocks = reinterpret_cast<int32_t *>(p_b + l.head_blocks);
    a.node_keys = reinterpret_cast<uint64_t *>(p_d + l.node_keys);
    a.corner_node = reinterpret_cast<int32_t *>(p_d + l.corner_node);
    a.seam_first = reinterpret_cast<int32_t *>(p_d + l.seam_first);
    a.seam_last = reinterpret_cast<int32_t *>(p_d + l.seam_last);
    a.col = reinterpret_cast<const int32_t *>(p_d + l.col);
    a.row_start = reinterpret_cast<const int32_t *>(p_d + l.row_start);
    a.counters = reinterpret_cast<int32_t *>(p_d + l.counters);
    a.f = reinterpret_cast<float *>(p_d + l.f);
    a.d = reinterpret_cast<double *>(p_d + l.d);
    a.g = reinterpret_cast<double *>(p_d + l.g);
    a.r = reinterpret_cast<double *>(p_d + l.r);
    a.p = reinterpret_cast<double *>(p_d + l.p);
    a.q = reinterpret_cast<double *>(p_d + l.q);
    a.part_a = reinterpret_cast<double *>(p_d + l.part_a);
    a.part_b = reinterpret_cast<double *>(p_d + l.part_b);
    a.scalars = reinterpret_cast<double *>(p_d + l.scalars);
    a.offsets = reinterpret_cast<float *>(p_d + l.offsets);
    a.samples = reinterpret_cast<float *>(p_d + l.samples);

    // the node table; the one number the host needs from it is the node count
    if (int rc = esfm::launch_level_corner_keys(st, a)) return rc;
    if (int rc = esfm::mesh_sort_keys(p_b + l.sort, sort_b, a.corner_keys, const_cast<uint64_t *>(a.sorted), n_corners, corner_bits, st)) return rc;
    if (int rc = esfm::launch_level_node_keys(st, a)) return rc;
    int32_t *mail_i = reinterpret_cast<int32_t *>(mail);
    ESFM_HIP_TRY(hipMemcpyAsync(mail_i, a.head_blocks + (n_corners + 255) / 256, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    const int32_t N = mail_i[0];
    if (N < 0 || N > n_corners) { esfm::set_error("mesh texture level: %d nodes from %lld corners", N, (long long)n_corners); return ESFM_ERR_NUMERIC; }
    if (N == 0) {
        memset(offsets, 0, sizeof(float) * 9 * T);
        if (samples) memset(samples, 0, sizeof(float) * 9 * T);
        *stats = nothing;
        return ESFM_OK;
    }
    a.N = N;
    if (int rc = esfm::launch_level_nodes(st, a)) return rc;

    // the smoothness neighbours: the corner -> node table read as the triangles of a mesh over the nodes
    esfm::MeshGraphArgs g;
    memset(&g, 0, sizeof(g));
    g.tri = a.corner_node; g.V = N; g.T = n_triangles;
    g.keys = reinterpret_cast<uint64_t *>(p_b + l.keys);
    g.sorted = a.sorted;
    g.head_rank = reinterpret_cast<int32_t *>(p_b + l.head_rank);
    g.head_blocks = a.head_blocks;
    g.col = const_cast<int32_t *>(a.col);
    g.row_start = const_cast<int32_t *>(a.row_start);
    g.pinned = p_d + l.pinned;
    if (int rc = esfm::mesh_build_adjacency(st, g, p_b + l.sort, sort_b)) return rc;

    // conjugate gradients: rz and bb, then per iteration five launches and 24 bytes back
    if (int rc = esfm::launch_level_start(st, a)) return rc;
    ESFM_HIP_TRY(hipMemcpyAsync(mail, a.scalars + esfm::kLevelBb, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
    ESFM_HIP_TRY(hipMemcpyAsync(mail + 3, a.counters, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    const double bb[3] = {mail[0], mail[1], mail[2]};
    esfm_mesh_texture_level_stats s = {N, reinterpret_cast<int32_t *>(mail + 3)[0], 0, 0};
    if (bb[0] == 0.0 && bb[1] == 0.0 && bb[2] == 0.0) s.converged = 1;
    for (int k = 1; !s.converged && k <= opt->max_iterations; ++k) {
        if (int rc = esfm::launch_level_step(st, a)) return rc;
        ESFM_HIP_TRY(hipMemcpyAsync(mail, a.scalars + esfm::kLevelRr, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
        if (int rc = esfm::launch_level_direction(st, a)) return rc;      // (behind the copy: it runs while the host looks at r r)
        ESFM_HIP_TRY(hipStreamSynchronize(st));
        const double rr[3] = {mail[0], mail[1], mail[2]};
        s.iterations = k;
        s.converged = esfm::level_converged(rr, bb, opt->tolerance) ? 1 : 0;
    }
    if (int rc = esfm::launch_level_outputs(st, a)) return rc;
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    ESFM_HIP_TRY(esfm::copy_d2h(offsets, a.offsets, sizeof(float) * 9 * T, st));
    if (samples) ESFM_HIP_TRY(esfm::copy_d2h(samples, a.samples, sizeof(float) * 9 * T, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    *stats = s;
    return ESFM_OK;
}

}  // extern "C"
