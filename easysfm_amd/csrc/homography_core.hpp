// The 4-point homography model of the planar / panoramic check (include/esfm.h "Homography RANSAC") as small routines that compile
// for the host and for gfx950, the way five_point_core.hpp serves the essential matrix.  ONE arithmetic for both sides:
// tests/homography_ref.py restates every expression below, in the same order, in plain Python floats, and the host build, the kernels
// and that restatement agree to the BIT.  What that asks of this file: only + - * / sqrt and comparisons (correctly rounded on both
// sides; the library is built -ffp-contract=off), and a fixed order of every sum.
//
// The rules, in the order they run.  H maps image 1 to image 2, row-major, H[8] = 1 on return.
//
//   normalisation (Hartley), per image, of n points (x_k, y_k):
//     mx = sx / n, my = sy / n                  sx, sy: the sums of the coordinates
//     md = sd / n                               sd: the sum of sqrt((x_k - mx) * (x_k - mx) + (y_k - my) * (y_k - my))
//     s  = kSqrt2 / md                          (md = 0 gives s = inf: the model comes out non-finite and is rejected below)
//     u_k = (x_k - mx) * s, v_k = (y_k - my) * s
//     The minimal solve adds its four terms from 0.0 in the order k = 0, 1, 2, 3; the re-fit receives sx, sy, sd already summed
//     (in the refit kernel's order: homography_kernels.hip).
//
//   DLT rows of a normalised correspondence (u, v) -> (p, q):
//     r0 = (-u, -v, -1,  0,  0,  0, p * u, p * v, p)
//     r1 = ( 0,  0,  0, -u, -v, -1, q * u, q * v, q)
//
//   minimal solve (homography_from_4): the 8 x 9 system of the four correspondences, rows 2 k and 2 k + 1 from correspondence k.
//     Its null vector is the last column of the orthogonal factor of a Householder QR of its transpose -- five_point_core.hpp's
//     null_space with eight reflectors instead of five.  Reflector j (j = 0 .. 7) works on components j .. 8 of system row j:
//       s = sum_{r = j .. 8} a(j, r)^2 (ascending r, from 0.0); nrm = sqrt(s); x0 = a(j, j); v0 = x0 - (x0 >= 0 ? -nrm : nrm);
//       a(j, j) = v0; vtv = v0 * v0 + sum_{r = j + 1 .. 8} a(j, r)^2 (ascending); beta_j = vtv > 0 ? 2 / vtv : 0;
//       for c = j + 1 .. 7: d = sum_{r = j .. 8} a(j, r) * a(c, r) (ascending, from 0.0); f = beta_j * d; a(c, r) -= f * a(j, r).
//     h = e_8; for j = 7 .. 0: d = sum_{r = j .. 8} a(j, r) * h_r (ascending, from 0.0); f = beta_j * d; h_r -= f * a(j, r).
//
//   re-fit solve (homography_from_normal): G = A'A (9 x 9, symmetric, given by its 45 upper entries in row order (0,0), (0,1) ..
//     (0,8), (1,1) ..) of any number of normalised correspondences.  G is diagonalised by epnp_core.hpp's jacobi_sym<9> (cyclic
//     Jacobi, at most 30 sweeps, stop at off^2 <= (10 DBL_EPSILON)^2 diag^2, jacobi_cs's rotation); h is the column of V at the smallest
//     diagonal entry, the first one on ties.
//
//   de-normalisation (both solves), Hn = h as 3 x 3, (mx1, my1, s1) of image 1, (mx2, my2, s2) of image 2:
//     for each row r:  m0 = Hn[r][0] * s1;  m1 = Hn[r][1] * s1;  m2 = (Hn[r][2] - m0 * mx1) - m1 * my1
//     H[0][c] = M[0][c] / s2 + mx2 * M[2][c];  H[1][c] = M[1][c] / s2 + my2 * M[2][c];  H[2][c] = M[2][c]
//     big = max |H[i]| (i ascending).  "No model" when an entry is non-finite or |H[8]| <= DBL_EPSILON * big; else every entry is
//     DIVIDED by H[8] (i ascending; H[8] last, so it becomes exactly 1).
//
//   forward transfer error (transfer_inlier), in FLOAT like cv::HomographyEstimatorCallback::computeError: Hf = (float)H,
//     ww = 1.f / (Hf[6] * x + Hf[7] * y + 1.f);  dx = (Hf[0] * x + Hf[1] * y + Hf[2]) * ww - X;  dy likewise with Hf[3..5] and Y;
//     err = dx * dx + dy * dy;  inlier iff err <= (float)(threshold * threshold).  Sums left to right.
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include "epnp_core.hpp"

// (forced inline: the routines take register arrays by pointer, and a call would put them in scratch memory)
#define ESFM_HG_HD __host__ __device__ __forceinline__

namespace esfm {
namespace homog {

constexpr double kSqrt2 = 1.4142135623730951;             // the double nearest sqrt(2)

struct Norm { double mx, my, s; };

ESFM_HG_HD Norm norm_from_sums(double sx, double sy, double n) { Norm t; t.mx = sx / n; t.my = sy / n; t.s = 0.0; return t; }
ESFM_HG_HD void norm_set_scale(Norm &t, double sd, double n) { const double md = sd / n; t.s = kSqrt2 / md; }
ESFM_HG_HD double centred_distance(const Norm &t, double x, double y)
{
    const double dx = x - t.mx, dy = y - t.my;
    return sqrt(dx * dx + dy * dy);
}

// the two DLT rows of one correspondence in pixels (x, y) -> (X, Y) under the two normalisations
ESFM_HG_HD void dlt_rows(const Norm &t1, const Norm &t2, double x, double y, double X, double Y, double *r0, double *r1)
{
    const double u = (x - t1.mx) * t1.s, v = (y - t1.my) * t1.s, p = (X - t2.mx) * t2.s, q = (Y - t2.my) * t2.s;
    r0[0] = -u; r0[1] = -v; r0[2] = -1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = p * u; r0[7] = p * v; r0[8] = p;
    r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = -u; r1[4] = -v; r1[5] = -1.0; r1[6] = q * u; r1[7] = q * v; r1[8] = q;
}

ESFM_HG_HD bool denormalise(const double *h, const Norm &t1, const Norm &t2, double *H)
{
    double M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double m0 = h[3 * r] * t1.s, m1 = h[3 * r + 1] * t1.s;
        M[3 * r] = m0; M[3 * r + 1] = m1; M[3 * r + 2] = (h[3 * r + 2] - m0 * t1.mx) - m1 * t1.my;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        H[c] = M[c] / t2.s + t2.mx * M[6 + c];
        H[3 + c] = M[3 + c] / t2.s + t2.my * M[6 + c];
        H[6 + c] = M[6 + c];
    }
    double big = 0.0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double a = fabs(H[i]);
        finite = finite && (a <= DBL_MAX);                 // (false for NaN and inf)
        big = a > big ? a : big;
    }
    if (!finite || fabs(H[8]) <= DBL_EPSILON * big) return false;
    const double h8 = H[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = H[i] / h8;
    return true;
}

// Minimal solve: four correspondences in pixels, p1[2 k], p1[2 k + 1] -> p2[2 k], p2[2 k + 1].  false = no model (H then holds zeros).
// Every loop is unrolled, so every array index is a compile-time number and the 8 x 9 system lives in registers.
ESFM_HG_HD bool homography_from_4(const double *p1, const double *p2, double *H)
{
    Norm t1, t2;
    {
        double sx = 0.0, sy = 0.0, sX = 0.0, sY = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { sx += p1[2 * k]; sy += p1[2 * k + 1]; sX += p2[2 * k]; sY += p2[2 * k + 1]; }
        t1 = norm_from_sums(sx, sy, 4.0); t2 = norm_from_sums(sX, sY, 4.0);
        double d1 = 0.0, d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { d1 += centred_distance(t1, p1[2 * k], p1[2 * k + 1]); d2 += centred_distance(t2, p2[2 * k], p2[2 * k + 1]); }
        norm_set_scale(t1, d1, 4.0); norm_set_scale(t2, d2, 4.0);
    }
    double a[8][9], beta[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) dlt_rows(t1, t2, p1[2 * k], p1[2 * k + 1], p2[2 * k], p2[2 * k + 1], a[2 * k], a[2 * k + 1]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double s = 0.0;
#pragma unroll
        for (int r = j; r < 9; ++r) s += a[j][r] * a[j][r];
        const double nrm = sqrt(s), x0 = a[j][j];
        const double v0 = x0 - (x0 >= 0.0 ? -nrm : nrm);
        a[j][j] = v0;
        double vtv = v0 * v0;
#pragma unroll
        for (int r = j + 1; r < 9; ++r) vtv += a[j][r] * a[j][r];
        beta[j] = vtv > 0.0 ? 2.0 / vtv : 0.0;
#pragma unroll
        for (int c = j + 1; c < 8; ++c) {
            double d = 0.0;
#pragma unroll
            for (int r = j; r < 9; ++r) d += a[j][r] * a[c][r];
            const double f = beta[j] * d;
#pragma unroll
            for (int r = j; r < 9; ++r) a[c][r] -= f * a[j][r];
        }
    }
    double h[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) h[r] = r == 8 ? 1.0 : 0.0;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
        double d = 0.0;
#pragma unroll
        for (int r = j; r < 9; ++r) d += a[j][r] * h[r];
        const double f = beta[j] * d;
#pragma unroll
        for (int r = j; r < 9; ++r) h[r] -= f * a[j][r];
    }
    if (denormalise(h, t1, t2, H)) return true;
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    return false;
}

// a correspondence's contribution to the 45 upper entries of A'A: g[e] += r0[i] * r0[j] + r1[i] * r1[j], e in row order
ESFM_HG_HD void normal_accumulate(const double *r0, const double *r1, double *g)
{
    int e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j, ++e) g[e] += r0[i] * r0[j] + r1[i] * r1[j];
}

// Re-fit solve: g = the 45 upper entries of A'A.  A, V: 81 doubles of work space each (LDS on the device).  false = no model (H zeros).
ESFM_HG_HD bool homography_from_normal(const double *g, const Norm &t1, const Norm &t2, double *A, double *V, double *H)
{
    int e = 0;
    for (int i = 0; i < 9; ++i) for (int j = i; j < 9; ++j, ++e) { A[9 * i + j] = g[e]; A[9 * j + i] = g[e]; }
    epnp::jacobi_sym<9>(A, V);
    int best = 0;
    for (int k = 1; k < 9; ++k) if (A[10 * k] < A[10 * best]) best = k;
    double h[9];
    for (int r = 0; r < 9; ++r) h[r] = V[9 * r + best];
    if (denormalise(h, t1, t2, H)) return true;
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    return false;
}

ESFM_HG_HD bool transfer_inlier(const float *Hf, float x, float y, float X, float Y, float thresh_sq)
{
    const float ww = 1.f / (Hf[6] * x + Hf[7] * y + 1.f);
    const float dx = (Hf[0] * x + Hf[1] * y + Hf[2]) * ww - X;
    const float dy = (Hf[3] * x + Hf[4] * y + Hf[5]) * ww - Y;
    const float err = dx * dx + dy * dy;
    return err <= thresh_sq;
}

// ---- the refit's sums in the refit kernel's order, on the host: 256 virtual lanes, lane l adds the points l, l + 256, .. whose mask is
// set, ascending; the 256 partials are folded by a halving tree (stride 128, 64 .. 1: partial[l] += partial[l + stride] for l < stride)
constexpr int kRefitLanes = 256;

inline double tree_fold(double *part)
{
    for (int stride = kRefitLanes / 2; stride > 0; stride >>= 1) for (int l = 0; l < stride; ++l) part[l] += part[l + stride];
    return part[0];
}

// pts: n float pairs per image; mask: n bytes or NULL (all points).  false = fewer than 4 inliers or no model.
inline bool homography_refit_host(const float *pts1, const float *pts2, int n, const unsigned char *mask, double *H)
{
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += (!mask || mask[i]) ? 1 : 0;
    if (cnt < 4) return false;
    static thread_local double part[45][kRefitLanes];
    auto clear = [&](int k) { for (int a = 0; a < k; ++a) for (int l = 0; l < kRefitLanes; ++l) part[a][l] = 0.0; };
    clear(4);
    for (int l = 0; l < kRefitLanes; ++l)
        for (int i = l; i < n; i += kRefitLanes) {
            if (mask && !mask[i]) continue;
            part[0][l] += (double)pts1[2 * i]; part[1][l] += (double)pts1[2 * i + 1]; part[2][l] += (double)pts2[2 * i]; part[3][l] += (double)pts2[2 * i + 1];
        }
    const double nn = (double)cnt;
    const double sx = tree_fold(part[0]), sy = tree_fold(part[1]), sX = tree_fold(part[2]), sY = tree_fold(part[3]);
    Norm t1 = norm_from_sums(sx, sy, nn), t2 = norm_from_sums(sX, sY, nn);
    clear(2);
    for (int l = 0; l < kRefitLanes; ++l)
        for (int i = l; i < n; i += kRefitLanes) {
            if (mask && !mask[i]) continue;
            part[0][l] += centred_distance(t1, (double)pts1[2 * i], (double)pts1[2 * i + 1]);
            part[1][l] += centred_distance(t2, (double)pts2[2 * i], (double)pts2[2 * i + 1]);
        }
    const double d1 = tree_fold(part[0]), d2 = tree_fold(part[1]);
    norm_set_scale(t1, d1, nn); norm_set_scale(t2, d2, nn);
    clear(45);
    for (int l = 0; l < kRefitLanes; ++l) {
        double g[45];
        for (int a = 0; a < 45; ++a) g[a] = 0.0;
        for (int i = l; i < n; i += kRefitLanes) {
            if (mask && !mask[i]) continue;
            double r0[9], r1[9];
            dlt_rows(t1, t2, (double)pts1[2 * i], (double)pts1[2 * i + 1], (double)pts2[2 * i], (double)pts2[2 * i + 1], r0, r1);
            normal_accumulate(r0, r1, g);
        }
        for (int a = 0; a < 45; ++a) part[a][l] = g[a];
    }
    double g[45], A[81], V[81];
    for (int a = 0; a < 45; ++a) g[a] = tree_fold(part[a]);
    return homography_from_normal(g, t1, t2, A, V, H);
}

}  // namespace homog
}  // namespace esfm
