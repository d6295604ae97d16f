// C-ABI entry point for SIFT detection + description (include/esfm.h): the replacement for
// cv::xfeatures2d::SIFT_create(nfeatures)->detectAndCompute, the Python prototype's SIFT branch (feature type 'I' here).
// Host side: the pyramid plan (octave sizes and buffer offsets), the Gaussian taps (host exp(), as getGaussianKernel), the
// launches, and the ordering of the detected keypoints -- scan order by key, duplicates removed, the nfeatures cut.  All pixel
// work runs in sift_kernels.hip; tests/sift_ref/sift_ref.c restates the whole computation on the CPU.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sift_kernels.hpp"
#include "surf_kernels.hpp"

using esfm::SiftKp;
using esfm::SiftPyr;
using esfm::SiftTaps;

namespace {

// GaussianBlur's kernel for CV_32F: ksize = cvRound(8 sigma + 1) | 1, getGaussianKernel (double exp, normalised in double)
int gaussian_taps(double sigma, SiftTaps &T)
{
    const int n = ((int)std::lrint(sigma * 8 + 1)) | 1;
    if (n > esfm::kSiftMaxTaps) return -1;
    double tmp[esfm::kSiftMaxTaps], sum = 0;
    const double scale2x = -0.5 / (sigma * sigma);
    for (int i = 0; i < n; ++i) { const double x = i - (n - 1) * 0.5; tmp[i] = std::exp(scale2x * x * x); sum += tmp[i]; }
    sum = 1. / sum;
    T.n = n;
    for (int i = 0; i < n; ++i) T.w[i] = (float)(tmp[i] * sum);
    return n;
}

// the base blur (createInitialImage, float arithmetic) and the five layer-to-layer blurs (buildGaussianPyramid, double)
void blur_sigmas(double sig[esfm::kSiftGauss])
{
    const float s = 1.6f, init = 0.5f;
    float d = s * s - init * init * 4;
    if (d < 0.01f) d = 0.01f;
    sig[0] = std::sqrt(d);
    const double k = std::pow(2., 1. / esfm::kSiftLayers);
    for (int i = 1; i < esfm::kSiftGauss; ++i) {
        const double prev = std::pow(k, (double)(i - 1)) * 1.6, total = prev * k;
        sig[i] = std::sqrt(total * total - prev * prev);
    }
}

}  // namespace

extern "C" {

int esfm_sift_detect_and_compute(esfm_ctx *ctx, const uint8_t *image, int rows, int cols, int channels, int nfeatures, int max_keypoints,
                                 float *keypoints, float *descriptors, int32_t *n_keypoints)
{
    if (!ctx) { esfm::set_error("ctx is NULL"); return ESFM_ERR_INVALID_ARG; }
    ESFM_REQUIRE(image && n_keypoints, "NULL argument");
    ESFM_REQUIRE(rows > 0 && cols > 0 && (channels == 1 || channels == 3), "image must be rows x cols x {1, 3}");
    ESFM_REQUIRE(rows <= 16384 && cols <= 16384, "image sides are limited to 16384");
    ESFM_REQUIRE(nfeatures >= 0, "nfeatures must be >= 0");
    ESFM_REQUIRE(max_keypoints >= 0 && (max_keypoints == 0 || (keypoints && descriptors)), "output buffers");
    *n_keypoints = 0;
    if (int rc = esfm::set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;

    // ---- plan: octave sizes (nOctaves = cvRound(log2(min side of the x2 base) - 2) - firstOctave) and buffer offsets
    SiftPyr P;
    memset(&P, 0, sizeof(P));
    P.n_oct = std::min((int)std::lrint(std::log((double)std::min(2 * rows, 2 * cols)) / std::log(2.) - 2) + 1, esfm::kSiftMaxOctaves);
    if (P.n_oct <= 0) return ESFM_OK;
    int64_t total = 0, interior = 0;
    for (int o = 0, r = 2 * rows, c = 2 * cols; o < P.n_oct; ++o, r /= 2, c /= 2) {
        P.oct[o].rows = r; P.oct[o].cols = c;
        P.oct[o].g_off = total; total += (int64_t)esfm::kSiftGauss * r * c;
        P.oct[o].dog_off = total; total += (int64_t)esfm::kSiftDog * r * c;
        interior += (int64_t)std::max(r - 2 * esfm::kSiftBorder, 0) * std::max(c - 2 * esfm::kSiftBorder, 0);
    }
    double sig[esfm::kSiftGauss];
    blur_sigmas(sig);
    SiftTaps taps[esfm::kSiftGauss];
    for (int i = 0; i < esfm::kSiftGauss; ++i) ESFM_REQUIRE(gaussian_taps(sig[i], taps[i]) > 0, "Gaussian kernel wider than the kernels are built for");
    // a candidate is a strict-or-equal extremum of its 26 neighbours: a generous share of the interior samples, and at most a few
    // orientation peaks per candidate; a list that would not fit is reported, never truncated
    const int cand_cap = (int)std::min<int64_t>(interior * esfm::kSiftLayers / 16 + 4096, 1 << 22);
    const int kp_cap = 2 * cand_cap;

    // ---- device buffers: gray | BGR staging; pyramid; row-pass scratch; counters | candidates | keypoints; descriptors
    const size_t n_px = (size_t)rows * cols;
    esfm::DevBuf &b_img = ctx->stage_a, &b_pyr = ctx->stage_b, &b_tmp = ctx->stage_c, &b_kp = ctx->stage_d, &b_desc = ctx->stage_e;
    if (int rc = b_img.reserve(n_px * (channels == 3 ? 4 : 1) + 16)) return rc;
    if (int rc = b_pyr.reserve(sizeof(float) * (size_t)total)) return rc;
    if (int rc = b_tmp.reserve(sizeof(float) * 4 * n_px)) return rc;
    if (int rc = b_kp.reserve(64 + sizeof(SiftKp) * ((size_t)cand_cap + kp_cap))) return rc;
    uint8_t *d_gray = b_img.as<uint8_t>();
    uint8_t *d_bgr = d_gray + ((n_px + 15) / 16) * 16;
    float *d_pyr = b_pyr.as<float>(), *d_tmp = b_tmp.as<float>();
    int32_t *d_cnt = b_kp.as<int32_t>();
    SiftKp *d_cand = reinterpret_cast<SiftKp *>(b_kp.as<uint8_t>() + 64), *d_kps = d_cand + cand_cap;

    if (channels == 3) {
        ESFM_HIP_TRY(esfm::copy_h2d(d_bgr, image, n_px * 3, st));
        if (int rc = esfm::launch_surf_gray(st, d_bgr, (int)n_px, d_gray)) return rc;   // cvtColor's 14-bit weights, shared with SURF
    } else {
        ESFM_HIP_TRY(esfm::copy_h2d(d_gray, image, n_px, st));
    }
    ESFM_HIP_TRY(hipMemsetAsync(d_cnt, 0, 64, st));
    {
        esfm::KernelTimer tm(ctx, ESFM_K_SIFT_PYR);
        for (int o = 0; o < P.n_oct; ++o) {
            const int r = P.oct[o].rows, c = P.oct[o].cols;
            const size_t plane = (size_t)r * c;
            float *g = d_pyr + P.oct[o].g_off, *dog = d_pyr + P.oct[o].dog_off;
            if (o == 0) {
                // the upsampled image waits in DoG layer 0, which the first layer-to-layer blur overwrites
                if (int rc = esfm::launch_sift_upsample(st, d_gray, rows, cols, dog)) return rc;
                if (int rc = esfm::launch_sift_blur(st, dog, d_tmp, g, nullptr, nullptr, r, c, taps[0])) return rc;
            } else {
                const float *src = d_pyr + P.oct[o - 1].g_off + (size_t)esfm::kSiftLayers * P.oct[o - 1].rows * P.oct[o - 1].cols;
                if (int rc = esfm::launch_sift_downsample(st, src, P.oct[o - 1].cols, g, r, c)) return rc;
            }
            for (int i = 1; i < esfm::kSiftGauss; ++i)
                if (int rc = esfm::launch_sift_blur(st, g + plane * (i - 1), d_tmp, g + plane * i, g + plane * (i - 1), dog + plane * (i - 1), r, c, taps[i])) return rc;
            if (int rc = esfm::launch_sift_extrema(st, P, d_pyr, o, d_cand, d_cnt, cand_cap)) return rc;
        }
    }
    {
        esfm::KernelTimer tm(ctx, ESFM_K_SIFT_DESC);
        if (int rc = esfm::launch_sift_orient(st, P, d_pyr, d_cand, d_cnt, cand_cap, d_kps, kp_cap)) return rc;
    }
    int32_t cnt[2] = {0, 0};
    ESFM_HIP_TRY(esfm::copy_d2h(cnt, d_cnt, sizeof(cnt), st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    if (cnt[0] > cand_cap) { esfm::set_error("SIFT candidate buffer overflow (%d > %d)", cnt[0], cand_cap); return ESFM_ERR_NUMERIC; }
    if (cnt[1] > kp_cap) { esfm::set_error("SIFT keypoint buffer overflow (%d > %d)", cnt[1], kp_cap); return ESFM_ERR_NUMERIC; }
    const int n_all = cnt[1];
    if (n_all == 0 || max_keypoints == 0) return ESFM_OK;
    std::vector<SiftKp> kps((size_t)n_all);
    ESFM_HIP_TRY(esfm::copy_d2h(kps.data(), d_kps, sizeof(SiftKp) * (size_t)n_all, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));

    // ---- scan order, removeDuplicated (the first in scan order survives), the nfeatures cut (ties with the n-th response stay)
    std::sort(kps.begin(), kps.end(), [](const SiftKp &a, const SiftKp &b) { return a.key < b.key; });
    {
        std::vector<int32_t> idx((size_t)n_all);
        for (int k = 0; k < n_all; ++k) idx[(size_t)k] = k;
        std::sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) {
            const SiftKp &p = kps[(size_t)a], &q = kps[(size_t)b];
            if (p.x != q.x) return p.x < q.x;
            if (p.y != q.y) return p.y < q.y;
            if (p.size != q.size) return p.size < q.size;
            if (p.angle != q.angle) return p.angle < q.angle;
            return a < b;
        });
        std::vector<char> keep((size_t)n_all, 1);
        for (int k = 1; k < n_all; ++k) {
            const SiftKp &p = kps[(size_t)idx[(size_t)k - 1]], &q = kps[(size_t)idx[(size_t)k]];
            if (p.x == q.x && p.y == q.y && p.size == q.size && p.angle == q.angle) keep[(size_t)idx[(size_t)k]] = 0;
        }
        size_t m = 0;
        for (int k = 0; k < n_all; ++k) if (keep[(size_t)k]) kps[m++] = kps[(size_t)k];
        kps.resize(m);
    }
    if (nfeatures > 0 && (size_t)nfeatures < kps.size()) {
        std::vector<float> resp(kps.size());
        for (size_t k = 0; k < kps.size(); ++k) resp[k] = kps[k].response;
        std::nth_element(resp.begin(), resp.begin() + (nfeatures - 1), resp.end(), std::greater<float>());
        const float thr = resp[(size_t)nfeatures - 1];
        size_t m = 0;
        for (size_t k = 0; k < kps.size(); ++k) if (kps[k].response >= thr) kps[m++] = kps[k];
        kps.resize(m);
    }
    if (kps.size() > (size_t)max_keypoints) kps.resize((size_t)max_keypoints);
    const int n_kp = (int)kps.size();

    // ---- descriptors of the final list
    if (int rc = b_desc.reserve(sizeof(float) * 128 * (size_t)n_kp)) return rc;
    float *d_desc = b_desc.as<float>();
    ESFM_HIP_TRY(esfm::copy_h2d(d_kps, kps.data(), sizeof(SiftKp) * (size_t)n_kp, st));
    {
        esfm::KernelTimer tm(ctx, ESFM_K_SIFT_DESC);
        if (int rc = esfm::launch_sift_describe(st, P, d_pyr, d_kps, n_kp, d_desc)) return rc;
    }
    ESFM_HIP_TRY(esfm::copy_d2h(descriptors, d_desc, sizeof(float) * 128 * (size_t)n_kp, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    // the firstOctave = -1 adjustment: coordinates and size halved, the octave byte one lower
    for (int k = 0; k < n_kp; ++k) {
        const SiftKp &p = kps[(size_t)k];
        float *ko = keypoints + 7 * (size_t)k;
        ko[0] = p.x * 0.5f; ko[1] = p.y * 0.5f; ko[2] = p.size * 0.5f; ko[3] = p.angle; ko[4] = p.response;
        ko[5] = (float)((p.octave & ~255) | ((p.octave - 1) & 255)); ko[6] = -1.f;
    }
    *n_keypoints = n_kp;
    return ESFM_OK;
}

}  // extern "C"
