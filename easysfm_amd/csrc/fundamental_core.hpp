// The 7-point fundamental matrix of the uncalibrated start (include/esfm.h "Fundamental-matrix RANSAC") and the focal-length cost
// over fundamental matrices, as small routines that compile for the host and for gfx950, the way homography_core.hpp serves the
// homography.  ONE arithmetic for both sides: tests/fundamental_ref.py restates the rule list of esfm.h in plain Python floats, and
// the host build, the kernels and that restatement agree to the BIT.  What that asks of this file: only + - * / sqrt and comparisons
// (correctly rounded on both sides; the library is built -ffp-contract=off), and a fixed order of every sum.
//
// The rules, in the order they run.  F is row-major and x2' F x1 = 0 for a correspondence x1 = (x, y, 1) -> x2 = (X, Y, 1).
//
//   normalisation (Hartley), per image: homography_core.hpp's (centroid to the origin, mean distance kSqrt2), the minimal solve adds
//     its seven terms from 0.0 in the order k = 0 .. 6.
//
//   row of a normalised correspondence (u, v) -> (p, q):  r = (p u, p v, p, q u, q v, q, u, v, 1)
//
//   minimal solve (fundamental_from_7): the 7 x 9 system, row k from correspondence k.  Its null space is spanned by the last two
//     columns of the orthogonal factor of a Householder QR of its transpose: homography_core.hpp's reflectors, seven of them
//     (j = 0 .. 6, components j .. 8), applied in the order j = 6 .. 0 to e_7 (giving f1) and to e_8 (giving f2).
//     With a = f2 and b = f1 - f2 as 3 x 3 matrices of rows a0 a1 a2, b0 b1 b2, det(x f1 + (1 - x) f2) = det(a + x b) =
//     c0 + c1 x + c2 x^2 + c3 x^3 by ONE expansion:
//       w0 = a1 x a2;  w1 = a1 x b2 + b1 x a2;  w2 = b1 x b2      (cross(s, t) = (s1 t2 - s2 t1, s2 t0 - s0 t2, s0 t1 - s1 t0))
//       c0 = a0 . w0;  c1 = a0 . w1 + b0 . w0;  c2 = a0 . w2 + b0 . w1;  c3 = b0 . w2      (dot: ((s0 t0 + s1 t1) + s2 t2))
//     Real roots (cubic_roots), ascending, by a BRACKETED NEWTON with a fixed sweep cap (not five_point_core.hpp's iteration):
//       big = max |c_i|; no root when big is 0 or not finite.
//       vanishing leading coefficient: |c3| <= kLeadEps * big.  The cubic is then read as the quadratic c2 x^2 + c1 x + c0 (and by
//         the same test on c2 as the linear c1 x + c0, on c1: no root); the root that went to infinity -- the model f1 - f2 -- is
//         dropped.  Quadratic: disc = c1 c1 - 4 c2 c0; none when !(disc >= 0); q = -0.5 (c1 + sign(c1) sqrt(disc)) (sign(0) = +);
//         disc == 0: the one root q / c2; else q / c2 and c0 / q, the smaller first.
//       else monic x^3 + A x^2 + B x + D (A = c2 / c3, B = c1 / c3, D = c0 / c3), p(x) = ((x + A) x + B) x + D, every root inside
//         (-R, R) with R = 1 + max(|A|, |B|, |D|) (Cauchy).  disc = A A - 3 B.  !(disc > 0): p is monotone, one root in [-R, R].
//         Else the stationary points x1 = (-A - sqrt(disc)) / 3 < x2 = (-A + sqrt(disc)) / 3 with p1 = p(x1), p2 = p(x2) cut the line
//         in three: a root in [-R, x1] iff p1 >= 0, in [x1, x2] iff p1 > 0 and p2 < 0, in [x2, R] iff p2 <= 0.
//       root in a bracket [lo, hi] on which p rises (falls: the middle one): x = 0.5 (lo + hi); at most kRootSweeps times:
//         f = p(x); stop when f == 0; the bracket end on f's side moves to x; xn = x - f / ((3 x + 2 A) x + B);
//         xn = 0.5 (lo + hi) unless lo < xn < hi; stop when xn == x; x = xn.
//     Model of root x: F_i = x f1_i + (1 - x) f2_i, then de-normalisation, norm and sign (finish_model).  A model with a
//     non-finite entry is no model; the others are stored in root order and counted.
//
//   de-normalisation, (mx1, my1, s1) of image 1, (mx2, my2, s2) of image 2:  F = T2' Fn T1
//     for each row r:  m0 = Fn[r][0] * s1;  m1 = Fn[r][1] * s1;  m2 = (Fn[r][2] - m0 * mx1) - m1 * my1
//     F[0][c] = M[0][c] * s2;  F[1][c] = M[1][c] * s2;  F[2][c] = (M[2][c] - F[0][c] * mx2) - F[1][c] * my2
//   norm and sign: ss = sum F_i^2 (i ascending, from 0.0); F_i = F_i / sqrt(ss); the entry of largest magnitude (the first on ties)
//     is made positive by negating every entry.  "No model" when an entry is then not finite.
//
//   score (epipolar_inlier), in FLOAT on Ff = (float)F, sums left to right:
//     a = Ff0 x + Ff1 y + Ff2, b = Ff3 x + Ff4 y + Ff5, c = Ff6 x + Ff7 y + Ff8, d2 = X a + Y b + c, e2 = d2 d2 / (a a + b b)
//     a' = Ff0 X + Ff3 Y + Ff6, b' = Ff1 X + Ff4 Y + Ff7, c' = Ff2 X + Ff5 Y + Ff8, d1 = x a' + y b' + c', e1 = d1 d1 / (a' a' + b' b')
//     err = max(e1, e2); inlier iff err <= (float)(threshold * threshold), a NaN in either being no inlier: e1 <= t && e2 <= t.
//
//   re-fit (normalised 8-point, fundamental_from_normal): G = sum r r' (45 upper entries in row order) over the inliers, summed like
//     the homography re-fit; the eigenvector at the smallest diagonal entry after jacobi_sym<9> (first on ties) is Fn.  Rank 2
//     (rank2): one-sided Jacobi on the columns of Fn (geometry_kernels.hip's loop for 3 x 3: pairs (0,1), (0,2), (1,2), skip when
//     |c| <= DBL_EPSILON sqrt(a b) or c == 0, at most 60 sweeps) leaves W = U S and the rotations V; the column of smallest squared
//     norm (first on ties) is dropped: Fn[r][c] = sum over the two other columns k ascending of W[r][k] V[c][k].  Then finish_model.
//
//   focal cost (focal_term), f64: K = [f 0 cx; 0 f cy; 0 0 1], G = K' F K:
//     M[r][0] = F[r][0] f;  M[r][1] = F[r][1] f;  M[r][2] = (F[r][0] cx + F[r][1] cy) + F[r][2]
//     G[0][c] = f M[0][c];  G[1][c] = f M[1][c];  G[2][c] = (cx M[0][c] + cy M[1][c]) + M[2][c]
//     the same one-sided Jacobi on G; n_k = squared norm of column k (rows ascending); hi = the largest (first on ties), mid = the
//     largest of the other two (first on ties); s1 = sqrt(hi), s2 = sqrt(mid); term = (s1 - s2) / (s1 + s2).
//     cost[k] = (sum_p w_p term_kp) / (sum_p w_p), both sums in pair order over 256 lanes and the halving tree (tree_fold).
#pragma once

#include "homography_core.hpp"

#define ESFM_FM_HD __host__ __device__ __forceinline__

namespace esfm {
namespace fundm {

using homog::Norm;
using homog::kRefitLanes;

constexpr double kLeadEps = 1e-12;       // the leading coefficient counts as vanished at this share of the largest one
constexpr int kRootSweeps = 80;
constexpr int kSvdSweeps = 60;

ESFM_FM_HD void fm_row(const Norm &t1, const Norm &t2, double x, double y, double X, double Y, double *r)
{
    const double u = (x - t1.mx) * t1.s, v = (y - t1.my) * t1.s, p = (X - t2.mx) * t2.s, q = (Y - t2.my) * t2.s;
    r[0] = p * u; r[1] = p * v; r[2] = p; r[3] = q * u; r[4] = q * v; r[5] = q; r[6] = u; r[7] = v; r[8] = 1.0;
}

// de-normalisation, unit Frobenius norm, canonical sign; false: a non-finite entry
ESFM_FM_HD bool finish_model(const double *fn, const Norm &t1, const Norm &t2, double *F)
{
    double M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double m0 = fn[3 * r] * t1.s, m1 = fn[3 * r + 1] * t1.s;
        M[3 * r] = m0; M[3 * r + 1] = m1; M[3 * r + 2] = (fn[3 * r + 2] - m0 * t1.mx) - m1 * t1.my;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        F[c] = M[c] * t2.s;
        F[3 + c] = M[3 + c] * t2.s;
        F[6 + c] = (M[6 + c] - F[c] * t2.mx) - F[3 + c] * t2.my;
    }
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) ss += F[i] * F[i];
    const double nrm = sqrt(ss);
    double big = 0.0, at = 0.0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        F[i] = F[i] / nrm;
        const double a = fabs(F[i]);
        finite = finite && (a <= DBL_MAX);
        if (a > big) { big = a; at = F[i]; }
    }
    if (!finite) return false;
    if (at < 0.0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = -F[i];
    }
    return true;
}

ESFM_FM_HD double dot3(const double *s, const double *t) { return (s[0] * t[0] + s[1] * t[1]) + s[2] * t[2]; }
ESFM_FM_HD void cross3(const double *s, const double *t, double *o)
{
    o[0] = s[1] * t[2] - s[2] * t[1]; o[1] = s[2] * t[0] - s[0] * t[2]; o[2] = s[0] * t[1] - s[1] * t[0];
}

// c[0..3] of det(a + x b)
ESFM_FM_HD void det_cubic(const double *a, const double *b, double *c)
{
    double w0[3], w1[3], w2[3], t[3];
    cross3(a + 3, a + 6, w0);
    cross3(a + 3, b + 6, w1); cross3(b + 3, a + 6, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) w1[i] = w1[i] + t[i];
    cross3(b + 3, b + 6, w2);
    c[0] = dot3(a, w0);
    c[1] = dot3(a, w1) + dot3(b, w0);
    c[2] = dot3(a, w2) + dot3(b, w1);
    c[3] = dot3(b, w2);
}

ESFM_FM_HD double bracket_root(double A, double B, double D, double lo, double hi, bool rising)
{
    double x = 0.5 * (lo + hi);
#pragma unroll 1
    for (int it = 0; it < kRootSweeps; ++it) {
        const double f = ((x + A) * x + B) * x + D;
        if (f == 0.0) break;
        if ((f < 0.0) == rising) lo = x; else hi = x;
        double xn = x - f / ((3.0 * x + 2.0 * A) * x + B);
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
        if (xn == x) break;
        x = xn;
    }
    return x;
}

// the real roots of c0 + c1 x + c2 x^2 + c3 x^3, ascending -> their number
ESFM_FM_HD int cubic_roots(const double *c, double *x)
{
    double big = 0.0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const double a = fabs(c[i]); finite = finite && (a <= DBL_MAX); big = a > big ? a : big; }
    if (!finite || big == 0.0) return 0;
    const double tiny = kLeadEps * big;
    if (fabs(c[3]) <= tiny) {
        if (fabs(c[2]) <= tiny) {
            if (fabs(c[1]) <= tiny) return 0;
            x[0] = -c[0] / c[1];
            return 1;
        }
        const double disc = c[1] * c[1] - 4.0 * c[2] * c[0];
        if (!(disc >= 0.0)) return 0;
        const double sq = sqrt(disc);
        const double q = -0.5 * (c[1] + (c[1] >= 0.0 ? sq : -sq));
        if (disc == 0.0) { x[0] = q / c[2]; return 1; }
        const double r0 = q / c[2], r1 = c[0] / q;
        x[0] = r1 < r0 ? r1 : r0; x[1] = r1 < r0 ? r0 : r1;
        return 2;
    }
    const double A = c[2] / c[3], B = c[1] / c[3], D = c[0] / c[3];
    double m = fabs(A);
    m = fabs(B) > m ? fabs(B) : m; m = fabs(D) > m ? fabs(D) : m;
    const double R = 1.0 + m;
    const double disc = A * A - 3.0 * B;
    if (!(disc > 0.0)) { x[0] = bracket_root(A, B, D, -R, R, true); return 1; }
    const double sq = sqrt(disc);
    const double x1 = (-A - sq) / 3.0, x2 = (-A + sq) / 3.0;
    const double p1 = ((x1 + A) * x1 + B) * x1 + D, p2 = ((x2 + A) * x2 + B) * x2 + D;
    int n = 0;
    if (p1 >= 0.0) x[n++] = bracket_root(A, B, D, -R, x1, true);
    if (p1 > 0.0 && p2 < 0.0) x[n++] = bracket_root(A, B, D, x1, x2, false);
    if (p2 <= 0.0) x[n++] = bracket_root(A, B, D, x2, R, true);
    return n;
}

// Minimal solve: seven correspondences in pixels, p1[2 k], p1[2 k + 1] -> p2[2 k], p2[2 k + 1].  F: 27 doubles, the models in root
// order, zeros behind them.  Returns their number (0 .. 3).  Every loop over the system is unrolled: it lives in registers.
ESFM_FM_HD int fundamental_from_7(const double *p1, const double *p2, double *F)
{
    Norm t1, t2;
    {
        double sx = 0.0, sy = 0.0, sX = 0.0, sY = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) { sx += p1[2 * k]; sy += p1[2 * k + 1]; sX += p2[2 * k]; sY += p2[2 * k + 1]; }
        t1 = homog::norm_from_sums(sx, sy, 7.0); t2 = homog::norm_from_sums(sX, sY, 7.0);
        double d1 = 0.0, d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) { d1 += homog::centred_distance(t1, p1[2 * k], p1[2 * k + 1]); d2 += homog::centred_distance(t2, p2[2 * k], p2[2 * k + 1]); }
        homog::norm_set_scale(t1, d1, 7.0); homog::norm_set_scale(t2, d2, 7.0);
    }
    double a[7][9], beta[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) fm_row(t1, t2, p1[2 * k], p1[2 * k + 1], p2[2 * k], p2[2 * k + 1], a[k]);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
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
        for (int c = j + 1; c < 7; ++c) {
            double d = 0.0;
#pragma unroll
            for (int r = j; r < 9; ++r) d += a[j][r] * a[c][r];
            const double f = beta[j] * d;
#pragma unroll
            for (int r = j; r < 9; ++r) a[c][r] -= f * a[j][r];
        }
    }
    double f1[9], f2[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) { f1[r] = r == 7 ? 1.0 : 0.0; f2[r] = r == 8 ? 1.0 : 0.0; }
#pragma unroll
    for (int j = 6; j >= 0; --j) {
        double d = 0.0, e = 0.0;
#pragma unroll
        for (int r = j; r < 9; ++r) { d += a[j][r] * f1[r]; e += a[j][r] * f2[r]; }
        const double fd = beta[j] * d, fe = beta[j] * e;
#pragma unroll
        for (int r = j; r < 9; ++r) { f1[r] -= fd * a[j][r]; f2[r] -= fe * a[j][r]; }
    }
    double b[9], c[4], x[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) b[i] = f1[i] - f2[i];
    det_cubic(f2, b, c);
    const int n_roots = cubic_roots(c, x);
    int n = 0;
#pragma unroll
    for (int i = 0; i < 27; ++i) F[i] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k < n_roots) {
            double fn[9], Fm[9];
            const double xr = x[k], om = 1.0 - xr;
#pragma unroll
            for (int i = 0; i < 9; ++i) fn[i] = xr * f1[i] + om * f2[i];
            if (finish_model(fn, t1, t2, Fm)) {
                // (n is 0 .. k: written with compile-time indices so that F stays in registers)
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    if (m == n) {
#pragma unroll
                        for (int i = 0; i < 9; ++i) F[9 * m + i] = Fm[i];
                    }
                ++n;
            }
        }
    }
    return n;
}

// One-sided (Hestenes) Jacobi on the columns of the row-major 3 x 3 W, rotations accumulated in V (geometry_kernels.hip's loop).
ESFM_FM_HD void jacobi_cols3(double *W, double *V)
{
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kSvdSweeps; ++sweep) {
        bool changed = false;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) { a += W[3 * r + p] * W[3 * r + p]; b += W[3 * r + q] * W[3 * r + q]; c += W[3 * r + p] * W[3 * r + q]; }
                if (fabs(c) <= DBL_EPSILON * sqrt(a * b) || c == 0.0) continue;
                changed = true;
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double u = W[3 * r + p], v = W[3 * r + q];
                    W[3 * r + p] = cs * u - sn * v; W[3 * r + q] = sn * u + cs * v;
                    const double vu = V[3 * r + p], vv = V[3 * r + q];
                    V[3 * r + p] = cs * vu - sn * vv; V[3 * r + q] = sn * vu + cs * vv;
                }
            }
        if (!changed) break;
    }
}

ESFM_FM_HD void col_norms3(const double *W, double *n)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double sq = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) sq += W[3 * r + k] * W[3 * r + k];
        n[k] = sq;
    }
}

// the nearest rank-2 matrix in place: the smallest singular value zeroed
ESFM_FM_HD void rank2(double *Fn)
{
    double W[9], V[9], n[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) W[i] = Fn[i];
    jacobi_cols3(W, V);
    col_norms3(W, n);
    int drop = 0;
    if (n[1] < n[drop]) drop = 1;
    if (n[2] < n[drop]) drop = 2;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) if (k != drop) s += W[3 * r + k] * V[3 * c + k];
            Fn[3 * r + c] = s;
        }
}

// a correspondence's contribution to the 45 upper entries of the normal matrix: g[e] += r[i] * r[j], e in row order
ESFM_FM_HD void normal_accumulate(const double *r, double *g)
{
    int e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j, ++e) g[e] += r[i] * r[j];
}

// Re-fit solve: g = the 45 upper entries of the normal matrix.  A, V: 81 doubles of work space each (LDS on the device).
ESFM_FM_HD bool fundamental_from_normal(const double *g, const Norm &t1, const Norm &t2, double *A, double *V, double *F)
{
    int e = 0;
    for (int i = 0; i < 9; ++i) for (int j = i; j < 9; ++j, ++e) { A[9 * i + j] = g[e]; A[9 * j + i] = g[e]; }
    epnp::jacobi_sym<9>(A, V);
    int best = 0;
    for (int k = 1; k < 9; ++k) if (A[10 * k] < A[10 * best]) best = k;
    double fn[9];
    for (int r = 0; r < 9; ++r) fn[r] = V[9 * r + best];
    rank2(fn);
    if (finish_model(fn, t1, t2, F)) return true;
    for (int i = 0; i < 9; ++i) F[i] = 0.0;
    return false;
}

ESFM_FM_HD bool epipolar_inlier(const float *Ff, float x, float y, float X, float Y, float thresh_sq)
{
    const float a = Ff[0] * x + Ff[1] * y + Ff[2], b = Ff[3] * x + Ff[4] * y + Ff[5], c = Ff[6] * x + Ff[7] * y + Ff[8];
    const float d2 = X * a + Y * b + c;
    const float e2 = d2 * d2 / (a * a + b * b);
    const float a1 = Ff[0] * X + Ff[3] * Y + Ff[6], b1 = Ff[1] * X + Ff[4] * Y + Ff[7], c1 = Ff[2] * X + Ff[5] * Y + Ff[8];
    const float d1 = x * a1 + y * b1 + c1;
    const float e1 = d1 * d1 / (a1 * a1 + b1 * b1);
    return e1 <= thresh_sq && e2 <= thresh_sq;
}

// (s1 - s2) / (s1 + s2) of the two largest singular values of K' F K
ESFM_FM_HD double focal_term(const double *F, double f, double cx, double cy)
{
    double M[9], G[9], V[9], n[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        M[3 * r] = F[3 * r] * f; M[3 * r + 1] = F[3 * r + 1] * f; M[3 * r + 2] = (F[3 * r] * cx + F[3 * r + 1] * cy) + F[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { G[c] = f * M[c]; G[3 + c] = f * M[3 + c]; G[6 + c] = (cx * M[c] + cy * M[3 + c]) + M[6 + c]; }
    jacobi_cols3(G, V);
    col_norms3(G, n);
    int top = 0;
    if (n[1] > n[top]) top = 1;
    if (n[2] > n[top]) top = 2;
    double mid = -1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) if (k != top && n[k] > mid) mid = n[k];
    const double s1 = sqrt(n[top]), s2 = sqrt(mid);
    return (s1 - s2) / (s1 + s2);
}

// ---- host: the sums in the kernels' order (homography_core.hpp's 256 virtual lanes and halving tree) ----------------------------
// pts: n float pairs per image; mask: n bytes or NULL (all points).  false = fewer than 8 inliers or no model.
inline bool fundamental_refit_host(const float *pts1, const float *pts2, int n, const unsigned char *mask, double *F)
{
    for (int i = 0; i < 9; ++i) F[i] = 0.0;
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += (!mask || mask[i]) ? 1 : 0;
    if (cnt < 8) return false;
    static thread_local double part[45][kRefitLanes];
    auto clear = [&](int k) { for (int a = 0; a < k; ++a) for (int l = 0; l < kRefitLanes; ++l) part[a][l] = 0.0; };
    clear(4);
    for (int l = 0; l < kRefitLanes; ++l)
        for (int i = l; i < n; i += kRefitLanes) {
            if (mask && !mask[i]) continue;
            part[0][l] += (double)pts1[2 * i]; part[1][l] += (double)pts1[2 * i + 1]; part[2][l] += (double)pts2[2 * i]; part[3][l] += (double)pts2[2 * i + 1];
        }
    const double nn = (double)cnt;
    const double sx = homog::tree_fold(part[0]), sy = homog::tree_fold(part[1]), sX = homog::tree_fold(part[2]), sY = homog::tree_fold(part[3]);
    Norm t1 = homog::norm_from_sums(sx, sy, nn), t2 = homog::norm_from_sums(sX, sY, nn);
    clear(2);
    for (int l = 0; l < kRefitLanes; ++l)
        for (int i = l; i < n; i += kRefitLanes) {
            if (mask && !mask[i]) continue;
            part[0][l] += homog::centred_distance(t1, (double)pts1[2 * i], (double)pts1[2 * i + 1]);
            part[1][l] += homog::centred_distance(t2, (double)pts2[2 * i], (double)pts2[2 * i + 1]);
        }
    const double d1 = homog::tree_fold(part[0]), d2 = homog::tree_fold(part[1]);
    homog::norm_set_scale(t1, d1, nn); homog::norm_set_scale(t2, d2, nn);
    clear(45);
    for (int l = 0; l < kRefitLanes; ++l) {
        double g[45];
        for (int a = 0; a < 45; ++a) g[a] = 0.0;
        for (int i = l; i < n; i += kRefitLanes) {
            if (mask && !mask[i]) continue;
            double r[9];
            fm_row(t1, t2, (double)pts1[2 * i], (double)pts1[2 * i + 1], (double)pts2[2 * i], (double)pts2[2 * i + 1], r);
            normal_accumulate(r, g);
        }
        for (int a = 0; a < 45; ++a) part[a][l] = g[a];
    }
    double g[45], A[81], V[81];
    for (int a = 0; a < 45; ++a) g[a] = homog::tree_fold(part[a]);
    return fundamental_from_normal(g, t1, t2, A, V, F);
}

// cost[k] of n_cand candidates over n_pairs matrices (9 doubles each) with weights
inline void focal_cost_host(int n_pairs, const double *F, const double *weight, double cx, double cy, int n_cand, const double *cand, double *cost)
{
    double num[kRefitLanes], den[kRefitLanes];
    for (int l = 0; l < kRefitLanes; ++l) { den[l] = 0.0; for (int p = l; p < n_pairs; p += kRefitLanes) den[l] += weight[p]; }
    const double wsum = homog::tree_fold(den);
    for (int k = 0; k < n_cand; ++k) {
        for (int l = 0; l < kRefitLanes; ++l) {
            num[l] = 0.0;
            for (int p = l; p < n_pairs; p += kRefitLanes) num[l] += weight[p] * focal_term(F + 9 * (size_t)p, cand[k], cx, cy);
        }
        cost[k] = homog::tree_fold(num) / wsum;
    }
}

}  // namespace fundm
}  // namespace esfm
