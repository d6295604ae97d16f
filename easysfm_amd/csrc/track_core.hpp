// Robust multi-view track triangulation and the reprojection filter (include/esfm.h "Track triangulation") as small routines that
// compile for the host and for gfx950, the way homography_core.hpp and five_point_core.hpp serve their models.  ONE arithmetic:
// tests/track_ref.py restates every expression below, in the same order, in plain Python floats, and the host build, the kernels and
// that restatement agree to the BIT.  What that asks of this file: f64 throughout, only + - * / sqrt and comparisons (correctly
// rounded on both sides; the library is built -ffp-contract=off), and a fixed order of every sum.  include/esfm.h holds the rule
// list; the comments here only say where each rule lives.
//
// A track's observations are staged as 64-byte records (Obs).  ESFM_TRACK_STAGE_CAP = kStageCap = 256 of them (16 KB) fit the LDS
// staging of a wave; a longer track keeps the same records in global memory.  The routines take a plain pointer and serve both.
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#define ESFM_TK_HD __host__ __device__ __forceinline__

namespace esfm {
namespace track {

constexpr int kStageCap = 256;          // observations of one track held in LDS (ESFM_TRACK_STAGE_CAP)
constexpr int kMaxObs = 65535;          // the longest track (ESFM_TRACK_MAX_OBS)
constexpr double kDetEps = 1e-12;       // a ray pair is parallel unless det > kDetEps * (aa * bb)

struct Options { double thr2, cos_min_angle; int32_t min_views, max_hypotheses, refine_iterations; };

// One staged observation.  C, d: camera centre and ray direction in the world.  Once the track's point is final, d holds the unit
// vector from the point to the centre and C[0] the squared pixel error (finish_obs).  flags: bit 0 inlier of the hypothesis, later of
// the final point.
struct Obs { double C[3], d[3]; float u, v; int32_t cam, flags; };
static_assert(sizeof(Obs) == 64, "an observation record is 64 bytes");

enum Status { kKept = 0, kTooFew = 1, kNoHypothesis = 2, kFewInliers = 3, kSmallAngle = 4, kNonFinite = 5 };

ESFM_TK_HD bool finite_d(double x) { return fabs(x) <= DBL_MAX; }                       // (false for NaN and inf)
ESFM_TK_HD double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// centre and direction of an observation; false when uv, K4 or Rt holds a non-finite value
ESFM_TK_HD bool make_obs(const double *Rt, const float *K, float u, float v, int32_t cam, Obs &o)
{
    bool ok = finite_d((double)u) && finite_d((double)v);
#pragma unroll
    for (int i = 0; i < 4; ++i) ok = ok && finite_d((double)K[i]);
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && finite_d(Rt[i]);
    const double fx = (double)K[0], cx = (double)K[1], fy = (double)K[2], cy = (double)K[3];
    const double x = ((double)u - cx) / fx, y = ((double)v - cy) / fy;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o.C[j] = -((Rt[j] * Rt[3] + Rt[4 + j] * Rt[7]) + Rt[8 + j] * Rt[11]);
        o.d[j] = (Rt[j] * x + Rt[4 + j] * y) + Rt[8 + j];
    }
    o.u = u; o.v = v; o.cam = cam; o.flags = 0;
    return ok;
}

struct Proj { double xn, yn, iz, ru, rv, err2; bool inlier; };

ESFM_TK_HD Proj project(const double *Rt, const float *K, float u, float v, const double *X, double thr2)
{
    const double p0 = ((Rt[0] * X[0] + Rt[1] * X[1]) + Rt[2] * X[2]) + Rt[3];
    const double p1 = ((Rt[4] * X[0] + Rt[5] * X[1]) + Rt[6] * X[2]) + Rt[7];
    const double p2 = ((Rt[8] * X[0] + Rt[9] * X[1]) + Rt[10] * X[2]) + Rt[11];
    Proj p;
    p.iz = 1.0 / p2; p.xn = p0 * p.iz; p.yn = p1 * p.iz;
    p.ru = ((double)K[0] * p.xn + (double)K[1]) - (double)u;
    p.rv = ((double)K[2] * p.yn + (double)K[3]) - (double)v;
    p.err2 = p.ru * p.ru + p.rv * p.rv;
    p.inlier = p2 > 0.0 && p.err2 <= thr2;
    return p;
}

ESFM_TK_HD Proj project_obs(const Obs &o, const double *Rt_all, const float *K_all, const double *X, double thr2)
{
    return project(Rt_all + 12 * (size_t)o.cam, K_all + 4 * (size_t)o.cam, o.u, o.v, X, thr2);
}

// ---- hypotheses ------------------------------------------------------------------------------------------------------------
ESFM_TK_HD int64_t pair_count(int n) { return (int64_t)n * (n - 1) / 2; }
ESFM_TK_HD int hypothesis_count(int n, int max_hypotheses) { const int64_t P = pair_count(n); return P <= max_hypotheses ? (int)P : max_hypotheses; }
ESFM_TK_HD int64_t hypothesis_pair(int h, int n, int max_hypotheses)
{
    const int64_t P = pair_count(n);
    return P <= max_hypotheses ? (int64_t)h : (int64_t)h * P / max_hypotheses;
}
// pairs before the first pair whose lower member is a
ESFM_TK_HD int64_t pair_offset(int64_t a, int64_t n) { return a * (2 * n - a - 1) / 2; }
// pair number q of the lexicographic list (0, 1), (0, 2) .. (n - 2, n - 1); the square root only guesses, the integers decide
ESFM_TK_HD void pair_from_number(int64_t q, int n, int &a, int &b)
{
    const double m = (double)(2 * (int64_t)n - 1);
    double disc = m * m - 8.0 * (double)q;
    disc = disc > 0.0 ? disc : 0.0;
    int64_t ai = (int64_t)((m - sqrt(disc)) * 0.5);
    ai = ai < 0 ? 0 : ai;
    ai = ai > n - 2 ? n - 2 : ai;
    while (pair_offset(ai, n) > q) --ai;
    while (ai < n - 2 && pair_offset(ai + 1, n) <= q) ++ai;
    a = (int)ai;
    b = (int)(q - pair_offset(ai, n)) + (int)ai + 1;
}

// the midpoint of two rays; false = void
ESFM_TK_HD bool hypothesis_point(const Obs &A, const Obs &B, double *X)
{
    double w[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = A.C[j] - B.C[j];
    const double aa = dot3(A.d, A.d), bb = dot3(B.d, B.d), ab = dot3(A.d, B.d), dw = dot3(A.d, w), ew = dot3(B.d, w);
    const double det = aa * bb - ab * ab;
    if (!(det > kDetEps * (aa * bb))) return false;
    const double s = (ab * ew - bb * dw) / det, t = (aa * ew - ab * dw) / det;
    if (!(s > 0.0) || !(t > 0.0)) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j) X[j] = 0.5 * ((A.C[j] + s * A.d[j]) + (B.C[j] + t * B.d[j]));
    return true;
}

// (inliers, cost, hypothesis index) as one key; a void hypothesis is {-1, 0, INT32_MAX}
struct Rank { int32_t inliers; double cost; int32_t h; };
ESFM_TK_HD Rank void_rank() { Rank r; r.inliers = -1; r.cost = 0.0; r.h = INT32_MAX; return r; }
ESFM_TK_HD bool better(const Rank &a, const Rank &b)
{
    if (a.inliers != b.inliers) return a.inliers > b.inliers;
    if (a.cost != b.cost) return a.cost < b.cost;
    return a.h < b.h;
}

ESFM_TK_HD Rank score(const Obs *rec, int n, const double *Rt_all, const float *K_all, const double *X, double thr2, int h)
{
    Rank r; r.inliers = 0; r.cost = 0.0; r.h = h;
    for (int k = 0; k < n; ++k) {
        const Proj p = project_obs(rec[k], Rt_all, K_all, X, thr2);
        r.inliers += p.inlier ? 1 : 0;
        r.cost += p.inlier ? p.err2 : thr2;
    }
    return r;
}

ESFM_TK_HD Rank hypothesis_rank(const Obs *rec, int n, const double *Rt_all, const float *K_all, const Options &o, int h, double *X)
{
    int a, b;
    pair_from_number(hypothesis_pair(h, n, o.max_hypotheses), n, a, b);
    if (!hypothesis_point(rec[a], rec[b], X)) return void_rank();
    return score(rec, n, Rt_all, K_all, X, o.thr2, h);
}

// ---- refit -----------------------------------------------------------------------------------------------------------------
// One Gauss-Newton step on the observations whose flags bit 0 is set; false ends the refit (X unchanged).
ESFM_TK_HD bool gn_step(const Obs *rec, int n, const double *Rt_all, const float *K_all, double thr2, double *X)
{
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int k = 0; k < n; ++k) {
        if (!(rec[k].flags & 1)) continue;
        const double *Rt = Rt_all + 12 * (size_t)rec[k].cam;
        const float *K = K_all + 4 * (size_t)rec[k].cam;
        const Proj p = project(Rt, K, rec[k].u, rec[k].v, X, thr2);
        const double a = (double)K[0] * p.iz, b = (double)K[2] * p.iz;
        const double u0 = a * (Rt[0] - p.xn * Rt[8]), u1 = a * (Rt[1] - p.xn * Rt[9]), u2 = a * (Rt[2] - p.xn * Rt[10]);
        const double v0 = b * (Rt[4] - p.yn * Rt[8]), v1 = b * (Rt[5] - p.yn * Rt[9]), v2 = b * (Rt[6] - p.yn * Rt[10]);
        A00 += u0 * u0 + v0 * v0; A01 += u0 * u1 + v0 * v1; A02 += u0 * u2 + v0 * v2;
        A11 += u1 * u1 + v1 * v1; A12 += u1 * u2 + v1 * v2; A22 += u2 * u2 + v2 * v2;
        g0 += u0 * p.ru + v0 * p.rv; g1 += u1 * p.ru + v1 * p.rv; g2 += u2 * p.ru + v2 * p.rv;
    }
    const double d0 = A00;
    if (!(d0 > 0.0)) return false;
    const double l10 = A01 / d0, l20 = A02 / d0;
    const double d1 = A11 - l10 * A01;
    if (!(d1 > 0.0)) return false;
    const double m = A12 - l20 * A01;
    const double l21 = m / d1;
    const double d2 = (A22 - l20 * A02) - l21 * m;
    if (!(d2 > 0.0)) return false;
    const double y0 = -g0, y1 = -g1 - l10 * y0, y2 = (-g2 - l20 * y0) - l21 * y1;
    const double z0 = y0 / d0, z1 = y1 / d1, z2 = y2 / d2;
    const double e2 = z2, e1 = z1 - l21 * e2, e0 = (z0 - l10 * e1) - l20 * e2;
    const double n0 = X[0] + e0, n1 = X[1] + e1, n2 = X[2] + e2;
    if (!(finite_d(n0) && finite_d(n1) && finite_d(n2))) return false;
    X[0] = n0; X[1] = n1; X[2] = n2;
    return true;
}

ESFM_TK_HD void refit(const Obs *rec, int n, const double *Rt_all, const float *K_all, const Options &o, double *X)
{
    for (int it = 0; it < o.refine_iterations; ++it) if (!gn_step(rec, n, Rt_all, K_all, o.thr2, X)) break;
}

// ---- the final point -------------------------------------------------------------------------------------------------------
// the record's last form: inlier flag, squared error in C[0], the unit vector from the point to the centre in d
ESFM_TK_HD void finish_obs(Obs &o, const double *Rt_all, const float *K_all, const double *X, double thr2)
{
    const Proj p = project_obs(o, Rt_all, K_all, X, thr2);
    double w[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = o.C[j] - X[j];
    const double len = sqrt(dot3(w, w));
#pragma unroll
    for (int j = 0; j < 3; ++j) o.d[j] = w[j] / len;
    o.C[0] = p.err2;
    o.flags = p.inlier ? 1 : 0;
}
// what obs_err2 reports: the squared error as a float, +inf where it is not a number (a point on the camera's focal plane)
ESFM_TK_HD float err2_out(double err2) { return err2 == err2 ? (float)err2 : (float)INFINITY; }

// the cosines of inlier i against the inliers behind it (records in their last form)
ESFM_TK_HD double min_cos_row(const Obs *rec, int n, int i, double m)
{
    if (!(rec[i].flags & 1)) return m;
    for (int j = i + 1; j < n; ++j) {
        if (!(rec[j].flags & 1)) continue;
        const double c = dot3(rec[i].d, rec[j].d);
        m = c < m ? c : m;
    }
    return m;
}

ESFM_TK_HD double inlier_mse(const Obs *rec, int n, int n_inliers)
{
    double s = 0.0;
    for (int k = 0; k < n; ++k) if (rec[k].flags & 1) s += rec[k].C[0];
    return n_inliers > 0 ? s / (double)n_inliers : 0.0;
}

// min_cos arrives as the minimum over the rows starting from 1.0; + 0.0 turns a -0.0 into +0.0 so that the minimum's bits do not
// depend on which of two equal zeros came first
ESFM_TK_HD int verdict(int n_inliers, double &min_cos, const Options &o)
{
    min_cos = min_cos + 0.0;
    if (n_inliers < o.min_views) return kFewInliers;
    if (min_cos > o.cos_min_angle) return kSmallAngle;
    return kKept;
}

// ---- the whole track on one host thread: the order the kernel's lanes share out ---------------------------------------------
struct Result { double X[3]; int32_t status, n_inliers; double min_cos, mse; };

// rec: n >= 2 records from make_obs, all finite.  Xgiven: the point to judge (evaluate) or NULL (triangulate).
inline void solve_host(Obs *rec, int n, const double *Rt_all, const float *K_all, const Options &o, const double *Xgiven, Result &r)
{
    r.n_inliers = 0; r.min_cos = 1.0; r.mse = 0.0; r.X[0] = r.X[1] = r.X[2] = 0.0;
    double X[3];
    if (Xgiven) {
        for (int j = 0; j < 3; ++j) X[j] = Xgiven[j];
    } else {
        Rank best = void_rank();
        const int H = hypothesis_count(n, o.max_hypotheses);
        for (int h = 0; h < H; ++h) {
            double Xh[3];
            const Rank rk = hypothesis_rank(rec, n, Rt_all, K_all, o, h, Xh);
            if (better(rk, best)) best = rk;
        }
        if (best.inliers < 0) { r.status = kNoHypothesis; return; }
        int a, b;
        pair_from_number(hypothesis_pair(best.h, n, o.max_hypotheses), n, a, b);
        double Xh[3];
        hypothesis_point(rec[a], rec[b], Xh);
        for (int k = 0; k < n; ++k) rec[k].flags = project_obs(rec[k], Rt_all, K_all, Xh, o.thr2).inlier ? 1 : 0;
        for (int j = 0; j < 3; ++j) X[j] = Xh[j];
        refit(rec, n, Rt_all, K_all, o, X);
        int n_ref = 0;
        for (int k = 0; k < n; ++k) n_ref += project_obs(rec[k], Rt_all, K_all, X, o.thr2).inlier ? 1 : 0;
        if (n_ref < best.inliers) for (int j = 0; j < 3; ++j) X[j] = Xh[j];
    }
    for (int k = 0; k < n; ++k) { finish_obs(rec[k], Rt_all, K_all, X, o.thr2); r.n_inliers += rec[k].flags & 1; }
    double m = 1.0;
    for (int i = 0; i < n; ++i) m = min_cos_row(rec, n, i, m);
    r.mse = inlier_mse(rec, n, r.n_inliers);
    r.min_cos = m;
    r.status = verdict(r.n_inliers, r.min_cos, o);
    for (int j = 0; j < 3; ++j) r.X[j] = X[j];
}

}  // namespace track
}  // namespace esfm
