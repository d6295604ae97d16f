// Host-side pieces of OpenCV's RANSAC point-set registrator shared by the essential-matrix and the PnP entry points
// [upstream opencv/modules/calib3d/src/ptsetreg.cpp, modules/core/include/opencv2/core/operations.hpp]: the cv::RNG
// recurrence, getSubset's sampling rule and RANSACUpdateNumIters.  Pure host arithmetic.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

namespace esfm {
namespace ransac {

constexpr int kModelPoints = 5;       // both the 5-point essential kernel and solvePnPRansac's EPnP kernel draw 5
constexpr int kMaxIters = 1000;       // RANSACPointSetRegistrator default (findEssentialMat does not override it)

struct CvRng {                        // cv::RNG((uint64)-1)
    uint64_t state = 0xFFFFFFFFFFFFFFFFull;
    unsigned next() { state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32); return (unsigned)state; }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

// RANSACPointSetRegistrator::getSubset for a model without checkSubset: distinct indices, a repeat is redrawn
inline void draw_subset(CvRng &rng, int count, int32_t idx[kModelPoints])
{
    for (int i = 0; i < kModelPoints;) {
        int v;
        for (;;) {
            v = idx[i] = rng.uniform(0, count);
            int j = 0;
            for (; j < i; ++j) if (v == idx[j]) break;
            if (j == i) break;
        }
        ++i;
    }
}

// ---- the 4-point form of the homography model (esfm.h "Homography RANSAC") ----------------------------------------------------------
constexpr int kHomogPoints = 4;
constexpr int kHomogMaxIters = 2000;  // cv::findHomography's maxIters default
constexpr int kSubsetAttempts = 1000; // getSubset's maxAttempts

// twice the signed area of the triangle (a, b, c), in double on the float coordinates
inline double tri_cross(const float *p, int a, int b, int c)
{
    const double dx1 = (double)p[2 * b] - (double)p[2 * a], dy1 = (double)p[2 * b + 1] - (double)p[2 * a + 1];
    const double dx2 = (double)p[2 * c] - (double)p[2 * a], dy2 = (double)p[2 * c + 1] - (double)p[2 * a + 1];
    return dx1 * dy2 - dy1 * dx2;
}
inline bool tri_collinear(const float *p, int a, int b, int c)
{
    const double dx1 = (double)p[2 * b] - (double)p[2 * a], dy1 = (double)p[2 * b + 1] - (double)p[2 * a + 1];
    const double dx2 = (double)p[2 * c] - (double)p[2 * a], dy2 = (double)p[2 * c + 1] - (double)p[2 * a + 1];
    return std::fabs(dx1 * dy2 - dy1 * dx2) <= (double)FLT_EPSILON * (std::fabs(dx1) + std::fabs(dy1) + std::fabs(dx2) + std::fabs(dy2));
}

// HomographyEstimatorCallback::checkSubset on the four correspondences idx[0..3] of pts1 -> pts2 (float pairs): false when one of the
// four triples (0,1,2), (1,2,3), (0,2,3), (0,1,3) is collinear (or two of its points coincide) in either image, or when the triples do
// not keep one orientation -- the product of the two images' signed areas is negative for some but not for all four.
inline bool check_subset4(const float *pts1, const float *pts2, const int32_t idx[kHomogPoints])
{
    static const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    for (int k = 0; k < 4; ++k) if (tri_collinear(pts1, idx[tt[k][0]], idx[tt[k][1]], idx[tt[k][2]])) return false;
    for (int k = 0; k < 4; ++k) if (tri_collinear(pts2, idx[tt[k][0]], idx[tt[k][1]], idx[tt[k][2]])) return false;
    int negative = 0;
    for (int k = 0; k < 4; ++k)
        negative += tri_cross(pts1, idx[tt[k][0]], idx[tt[k][1]], idx[tt[k][2]]) * tri_cross(pts2, idx[tt[k][0]], idx[tt[k][1]], idx[tt[k][2]]) < 0.0 ? 1 : 0;
    return negative == 0 || negative == 4;
}

// getSubset for the model with checkSubset: four distinct indices (a repeat is redrawn), then the subset check; a rejected subset is
// redrawn whole, up to kSubsetAttempts attempts.  false: no subset passed (the stream has advanced by all attempts).  *redraws (or
// NULL) is increased by the number of rejected subsets.
inline bool draw_subset(CvRng &rng, int count, const float *pts1, const float *pts2, int32_t idx[kHomogPoints], int64_t *redraws = nullptr)
{
    for (int attempt = 0; attempt < kSubsetAttempts; ++attempt) {
        for (int i = 0; i < kHomogPoints;) {
            int v;
            for (;;) {
                v = idx[i] = rng.uniform(0, count);
                int j = 0;
                for (; j < i; ++j) if (v == idx[j]) break;
                if (j == i) break;
            }
            ++i;
        }
        if (check_subset4(pts1, pts2, idx)) return true;
        if (redraws) ++*redraws;
    }
    return false;
}

inline int update_num_iters(double p, double ep, int model_points, int max_iters)   // cv::RANSACUpdateNumIters
{
    p = std::max(p, 0.0); p = std::min(p, 1.0);
    ep = std::max(ep, 0.0); ep = std::min(ep, 1.0);
    double num = std::max(1.0 - p, DBL_MIN);
    double denom = 1.0 - std::pow(1.0 - ep, model_points);
    if (denom < DBL_MIN) return 0;
    num = std::log(num); denom = std::log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::lrint(num / denom);
}

}  // namespace ransac
}  // namespace esfm
