// C-ABI entry point of the voxel-grid merge (include/esfm.h, "Dense-cloud merge", esfm_cloud_voxel_merge).  Host side: argument
// checks, the fold of the bounds partials and the 2^21 cell limit, buffer layout, uploads, launches and the read-back.  The point
// work runs in voxel_kernels.hip, the sort in voxel_sort.hip; tests/merge_ref.py restates the rule.
#include <cmath>
#include <vector>

#include "scratch_layout.hpp"
#include "voxel_kernels.hpp"

extern "C" int esfm_cloud_voxel_merge(esfm_ctx *ctx, int n, const float *xyz, const uint8_t *rgb, const float *normals, const int32_t *tags,
                                      float voxel_size, int min_points, int min_tags, float *out_xyz, uint8_t *out_rgb, float *out_normals,
                                      int32_t *out_count, uint64_t *out_tagmask, int32_t *n_out)
{
    ESFM_REQUIRE(n >= 0 && n <= (1 << 28), "n must be 0..2^28");
    ESFM_REQUIRE(n_out && (n == 0 || (xyz && out_xyz)), "NULL argument");
    ESFM_REQUIRE(voxel_size > 0.f && std::isfinite(voxel_size), "voxel_size must be finite and > 0");
    ESFM_REQUIRE(min_points >= 1 && min_tags >= 0, "min_points must be >= 1 and min_tags >= 0");
    ESFM_REQUIRE(min_tags == 0 || tags, "min_tags > 0 needs tags");
    ESFM_REQUIRE((!out_rgb || rgb) && (!out_normals || normals) && (!out_tagmask || tags), "an output array is requested without its input");
    if (tags)
        for (int i = 0; i < n; ++i) ESFM_REQUIRE(tags[i] >= 0 && tags[i] <= 63, "a tag is outside 0..63");
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(ctx)) return rc;
    if (n == 0) { *n_out = 0; return ESFM_OK; }
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)n, n_blocks = (N + 255) / 256;

    // stage_a: the input arrays
    esfm::ScratchCarver in;
    const size_t i_xyz = in.take(sizeof(float) * 3 * N), i_rgb = in.take(rgb ? 3 * N : 0), i_nrm = in.take(normals ? sizeof(float) * 3 * N : 0),
                 i_tag = in.take(tags ? sizeof(int32_t) * N : 0);
    if (int rc = ctx->stage_a.reserve(in.at)) return rc;
    uint8_t *p_in = ctx->stage_a.as<uint8_t>();
    esfm::VoxelArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz = reinterpret_cast<const float *>(p_in + i_xyz);
    ESFM_HIP_TRY(esfm::copy_h2d(p_in + i_xyz, xyz, sizeof(float) * 3 * N, st));
    if (rgb) { a.rgb = p_in + i_rgb; ESFM_HIP_TRY(esfm::copy_h2d(p_in + i_rgb, rgb, 3 * N, st)); }
    if (normals) {
        a.normals = reinterpret_cast<const float *>(p_in + i_nrm);
        ESFM_HIP_TRY(esfm::copy_h2d(p_in + i_nrm, normals, sizeof(float) * 3 * N, st));
    }
    if (tags) {
        a.tags = reinterpret_cast<const int32_t *>(p_in + i_tag);
        ESFM_HIP_TRY(esfm::copy_h2d(p_in + i_tag, tags, sizeof(int32_t) * N, st));
    }
    a.n = n; a.h = voxel_size; a.min_points = min_points; a.min_tags = min_tags;

    // stage_b: key and index pairs before and after the sort | head counts + n_voxels | keep counts + n_out | bounds partials | sort scratch
    size_t sort_b = 0;
    if (int rc = esfm::voxel_sort_scratch_bytes(n, &sort_b, st)) return rc;
    esfm::ScratchCarver work;
    const size_t w_keys_in = work.take(sizeof(uint64_t) * N), w_keys_out = work.take(sizeof(uint64_t) * N), w_idx_in = work.take(sizeof(int32_t) * N),
                 w_idx_out = work.take(sizeof(int32_t) * N), w_heads = work.take(sizeof(int32_t) * (n_blocks + 1)),
                 w_keeps = work.take(sizeof(int32_t) * (n_blocks + 1)), w_part = work.take(sizeof(esfm::VoxelBounds) * esfm::kVoxelBoundsBlocks),
                 w_sort = work.take(sort_b);
    if (int rc = ctx->stage_b.reserve(work.at)) return rc;
    uint8_t *p_b = ctx->stage_b.as<uint8_t>();
    uint64_t *keys_in = reinterpret_cast<uint64_t *>(p_b + w_keys_in), *keys_out = reinterpret_cast<uint64_t *>(p_b + w_keys_out);
    int32_t *idx_in = reinterpret_cast<int32_t *>(p_b + w_idx_in), *idx_out = reinterpret_cast<int32_t *>(p_b + w_idx_out);
    a.head_count = reinterpret_cast<int32_t *>(p_b + w_heads);
    a.keep_count = reinterpret_cast<int32_t *>(p_b + w_keeps);
    esfm::VoxelBounds *d_part = reinterpret_cast<esfm::VoxelBounds *>(p_b + w_part);
    void *d_sort = p_b + w_sort;

    // bounds: origin, number of valid points, the 2^21 limit with the coordinate maximum (floorf is monotone)
    int n_part = 0;
    if (int rc = esfm::launch_voxel_bounds(st, a.xyz, n, d_part, &n_part)) return rc;
    std::vector<esfm::VoxelBounds> part((size_t)n_part);
    ESFM_HIP_TRY(esfm::copy_d2h(part.data(), d_part, sizeof(esfm::VoxelBounds) * part.size(), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    float hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int64_t n_valid = 0;
    for (int c = 0; c < 3; ++c) a.o[c] = INFINITY;
    for (const esfm::VoxelBounds &b : part) {
        n_valid += b.n_valid;
        for (int c = 0; c < 3; ++c) { a.o[c] = std::fmin(a.o[c], b.lo[c]); hi[c] = std::fmax(hi[c], b.hi[c]); }
    }
    if (n_valid == 0) { *n_out = 0; return ESFM_OK; }
    for (int c = 0; c < 3; ++c) {
        const float top = std::floor((hi[c] - a.o[c]) / voxel_size);
        ESFM_REQUIRE(top < 2097152.f, "a cell index reaches 2^21: voxel_size is too small for the cloud's extent");
    }
    a.n_valid = (int32_t)n_valid;
    const size_t v_blocks = ((size_t)n_valid + 255) / 256;

    if (int rc = esfm::launch_voxel_keys(st, a, keys_in, idx_in)) return rc;
    if (int rc = esfm::voxel_sort_pairs(d_sort, sort_b, keys_in, keys_out, idx_in, idx_out, n, st)) return rc;
    a.keys = keys_out; a.order = idx_out;
    if (int rc = esfm::launch_voxel_heads(st, a)) return rc;
    int32_t n_vox = 0;
    ESFM_HIP_TRY(esfm::copy_d2h(&n_vox, a.head_count + v_blocks, sizeof(int32_t), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    if (n_vox < 1 || n_vox > n_valid) { esfm::set_error("voxel merge: %d voxels from %lld points", n_vox, (long long)n_valid); return ESFM_ERR_NUMERIC; }
    a.n_vox = n_vox;
    const size_t V = (size_t)n_vox, o_blocks = (V + 255) / 256;

    // stage_c: voxel keys | accumulators; stage_d: the compacted output
    esfm::ScratchCarver vox, out;
    const size_t acc_b = sizeof(int64_t) * esfm::kVoxelAccWords * V, v_key = vox.take(sizeof(uint64_t) * V), v_acc = vox.take(acc_b);
    if (int rc = ctx->stage_c.reserve(vox.at)) return rc;
    a.vox_key = reinterpret_cast<uint64_t *>(ctx->stage_c.as<uint8_t>() + v_key);
    a.acc = reinterpret_cast<int64_t *>(ctx->stage_c.as<uint8_t>() + v_acc);
    ESFM_HIP_TRY(hipMemsetAsync(a.acc, 0, acc_b, st));
    const size_t o_xyz = out.take(sizeof(float) * 3 * V), o_rgb = out.take(out_rgb ? 3 * V : 0), o_nrm = out.take(out_normals ? sizeof(float) * 3 * V : 0),
                 o_cnt = out.take(out_count ? sizeof(int32_t) * V : 0), o_msk = out.take(out_tagmask ? sizeof(uint64_t) * V : 0);
    if (int rc = ctx->stage_d.reserve(out.at)) return rc;
    uint8_t *p_o = ctx->stage_d.as<uint8_t>();
    a.out_xyz = reinterpret_cast<float *>(p_o + o_xyz);
    if (out_rgb) a.out_rgb = p_o + o_rgb;
    if (out_normals) a.out_normals = reinterpret_cast<float *>(p_o + o_nrm);
    if (out_count) a.out_count = reinterpret_cast<int32_t *>(p_o + o_cnt);
    if (out_tagmask) a.out_tagmask = reinterpret_cast<uint64_t *>(p_o + o_msk);
    if (int rc = esfm::launch_voxel_accumulate(st, a)) return rc;
    if (int rc = esfm::launch_voxel_finalise(st, a)) return rc;
    int32_t kept = 0;
    ESFM_HIP_TRY(esfm::copy_d2h(&kept, a.keep_count + o_blocks, sizeof(int32_t), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    if (kept < 0 || kept > n_vox) { esfm::set_error("voxel merge: %d of %d voxels kept", kept, n_vox); return ESFM_ERR_NUMERIC; }
    const size_t M = (size_t)kept;
    ESFM_HIP_TRY(esfm::copy_d2h(out_xyz, a.out_xyz, sizeof(float) * 3 * M, st));
    if (out_rgb) ESFM_HIP_TRY(esfm::copy_d2h(out_rgb, a.out_rgb, 3 * M, st));
    if (out_normals) ESFM_HIP_TRY(esfm::copy_d2h(out_normals, a.out_normals, sizeof(float) * 3 * M, st));
    if (out_count) ESFM_HIP_TRY(esfm::copy_d2h(out_count, a.out_count, sizeof(int32_t) * M, st));
    if (out_tagmask) ESFM_HIP_TRY(esfm::copy_d2h(out_tagmask, a.out_tagmask, sizeof(uint64_t) * M, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    *n_out = kept;
    return ESFM_OK;
}
