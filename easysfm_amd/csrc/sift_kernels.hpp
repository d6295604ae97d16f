// Launch interface between sift_api.cpp and sift_kernels.hip.
#pragma once

#include "common.hpp"

namespace esfm {

constexpr int kSiftLayers = 3, kSiftGauss = kSiftLayers + 3, kSiftDog = kSiftLayers + 2;
constexpr int kSiftBorder = 5, kSiftMaxOctaves = 16, kSiftMaxTaps = 64, kSiftOriBins = 36;
constexpr int kSiftDescThreads = 384;   // one thread per bin of the 6 x 6 x 10 descriptor histogram (360 used)

struct SiftOctave {
    int32_t rows, cols;
    int64_t g_off, dog_off;   // first float of Gaussian layer 0 / DoG layer 0 in the pyramid buffer (layers follow at rows * cols)
};

struct SiftPyr {
    int32_t n_oct, pad;
    SiftOctave oct[kSiftMaxOctaves];
};

struct SiftTaps { int32_t n; float w[kSiftMaxTaps]; };   // getGaussianKernel(n, sigma, CV_32F)

// a refined candidate (angle unset) or an oriented keypoint; coordinates before the firstOctave halving
struct SiftKp {
    float x, y, size, angle, response;
    int32_t octave;            // OpenCV's packed octave: o + (layer << 8) + (lrint((xi + 0.5) * 255) << 16)
    int32_t o, layer;          // octave index in the pyramid, refined layer
    float xo, yo, scl;         // octave-relative position (c + xc, r + xr) and scale 1.6 * 2^((layer + xi) / 3)
    int32_t r, c, pad;         // refined integer position
    int64_t key;               // scan order: candidates (((o * 4 + detection layer) * 65536 + row) * 65536 + col), keypoints key * 64 + peak bin
};
static_assert(sizeof(SiftKp) == 64, "SiftKp is 64 bytes");

int launch_sift_upsample(hipStream_t st, const uint8_t *gray, int rows, int cols, float *out);
int launch_sift_blur(hipStream_t st, const float *src, float *tmp, float *dst, const float *prev, float *dog, int rows, int cols, const SiftTaps &taps);
int launch_sift_downsample(hipStream_t st, const float *src, int src_cols, float *dst, int rows, int cols);
int launch_sift_extrema(hipStream_t st, const SiftPyr &pyr, const float *pyr_buf, int o, SiftKp *cand, int32_t *counters, int cand_cap);
int launch_sift_orient(hipStream_t st, const SiftPyr &pyr, const float *pyr_buf, const SiftKp *cand, int32_t *counters, int cand_cap, SiftKp *kps,
                       int kp_cap);
int launch_sift_describe(hipStream_t st, const SiftPyr &pyr, const float *pyr_buf, const SiftKp *kps, int n_kp, float *desc);

}  // namespace esfm
