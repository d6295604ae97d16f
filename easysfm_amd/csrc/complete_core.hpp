// Track completion (include/esfm.h "Track completion") as small routines that compile for the host and for gfx950: ONE arithmetic
// for the kernels (complete_kernels.hip), the host build (esfm_track_complete_host) and the restatement in tests/complete_ref.py.
// The projection is track_core.hpp's, called, not copied; the pixel of the projection is formed once per (point, camera) and the
// residual of a keypoint against it is track::project's own `(fx xn + cx) - u`, the same operations in the same association.
// The search grid below is an acceleration only: the predicate decides, and every grid routine is monotone in its arguments, so a
// keypoint the predicate admits lies in the cells the window names (see window_cells).
#pragma once

#include "track_core.hpp"

namespace esfm {
namespace complete {

constexpr int kMaxRefs = 8;              // reference rows of a point: its first max_refs observations (ESFM_TRACK_COMPLETE_MAX_REFS)
constexpr int kMaxCellsAxis = 1024;      // grid cells per axis and camera: a cell number fits 20 bits of the sort key
constexpr int kCellBits = 20, kRowBits = 21;

struct Options { double thr2, pad, max_distance, ratio; int32_t max_refs, whole; };
// thr2 = search_radius_px squared; pad = 2 search_radius_px, the half width of the window the grid walks; whole = 1 when thr2
// overflows to +inf: every keypoint is then in the window and the grid is one cell per camera

// The pixel of point X in a camera, and whether the point is in front of it.  pu, pv are exactly the minuends of track::project's ru, rv.
struct Pixel { double pu, pv; bool front; };
ESFM_TK_HD Pixel project_pixel(const double *Rt, const float *K, const double *X)
{
    const track::Proj p = track::project(Rt, K, 0.0f, 0.0f, X, 0.0);
    const double p2 = ((Rt[8] * X[0] + Rt[9] * X[1]) + Rt[10] * X[2]) + Rt[11];
    Pixel q;
    q.pu = (double)K[0] * p.xn + (double)K[1];
    q.pv = (double)K[2] * p.yn + (double)K[3];
    q.front = p2 > 0.0;
    return q;
}
// err2 of keypoint (u, v) against the pixel, as track::project forms it; admissible iff front and err2 <= thr2 (false for NaN)
ESFM_TK_HD bool admissible(const Pixel &q, float u, float v, double thr2)
{
    const double ru = q.pu - (double)u, rv = q.pv - (double)v;
    const double err2 = ru * ru + rv * rv;
    return q.front && err2 <= thr2;
}

// ---- distances ---------------------------------------------------------------------------------------------------------------
// The matcher's canonical squared L2 distance (match_device.hpp l2sqr_canonical, oracle order): 8 partial sums over blocks of 8,
// (acc[c] + acc[c + 4]) summed left to right, then the scalar tail; separate multiply and add.  The kernels call the matcher's own
// routine; this is its host form (the library is built -ffp-contract=off).
inline float l2sqr_host(const float *a, const float *b, int n)
{
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int j = 0;
    for (; j <= n - 8; j += 8)
        for (int c = 0; c < 8; ++c) { const float t = a[j + c] - b[j + c]; acc[c] = acc[c] + t * t; }
    const float s0 = acc[0] + acc[4], s1 = acc[1] + acc[5], s2 = acc[2] + acc[6], s3 = acc[3] + acc[7];
    float d = s0 + s1;
    d = d + s2;
    d = d + s3;
    for (; j < n; ++j) { const float t = a[j] - b[j]; d = d + t * t; }
    return d;
}
inline float hamming_host(const uint8_t *a, const uint8_t *b, int nbytes)
{
    int c = 0;
    for (int j = 0; j < nbytes; ++j) c += __builtin_popcount((unsigned)(a[j] ^ b[j]));
    return (float)c;
}

// ---- score, two-best fold, acceptance, conflict key ---------------------------------------------------------------------------
// the minimum over the reference rows; a NaN distance is never the minimum (the start value NaN means "no distance yet")
ESFM_TK_HD float min_score(float best, float d) { return (d == d && !(best <= d)) ? d : best; }

// A score takes part iff it is below FLT_MAX (the matcher's rule: FLT_MAX, +inf and NaN are never neighbours).
ESFM_TK_HD bool is_candidate(float d) { return d < FLT_MAX; }

struct Best2 { float d0, d1; int32_t k0, k1; };                       // an empty slot: FLT_MAX, -1
ESFM_TK_HD Best2 empty_best() { Best2 b; b.d0 = b.d1 = FLT_MAX; b.k0 = b.k1 = -1; return b; }
ESFM_TK_HD bool before(float d, int32_t k, float bd, int32_t bk) { return k >= 0 && (bk < 0 || d < bd || (d == bd && k < bk)); }
// ascending (d, k): a total order over distinct rows, so any order of insertion gives the same two
ESFM_TK_HD void insert(Best2 &b, float d, int32_t k)
{
    if (!before(d, k, b.d1, b.k1)) return;
    if (before(d, k, b.d0, b.k0)) { b.d1 = b.d0; b.k1 = b.k0; b.d0 = d; b.k0 = k; }
    else { b.d1 = d; b.k1 = k; }
}
ESFM_TK_HD void merge(Best2 &b, const Best2 &o) { insert(b, o.d0, o.k0); insert(b, o.d1, o.k1); }

ESFM_TK_HD bool proposes(const Best2 &b, const Options &o)
{
    if (b.k0 < 0 || !((double)b.d0 <= o.max_distance)) return false;
    return b.k1 < 0 || (double)b.d0 < o.ratio * (double)b.d1;
}

// the claim on a keypoint: ascending (d0, point index) as one unsigned integer (d0 >= 0: its bit pattern ascends with its value)
constexpr uint64_t kNoClaim = ~0ull;
ESFM_TK_HD uint32_t float_bits(float f) { union { float f; uint32_t u; } c; c.f = f + 0.0f; return c.u; }   // (+ 0.0f: -0 becomes +0)
ESFM_TK_HD float bits_float(uint32_t u) { union { float f; uint32_t u; } c; c.u = u; return c.f; }
ESFM_TK_HD uint64_t claim_key(float d0, int32_t p) { return (uint64_t)float_bits(d0) << 32 | (uint64_t)(uint32_t)p; }

// ---- the grid ----------------------------------------------------------------------------------------------------------------
// Per camera: the box of the keypoints that take part (free, and finite unless `whole`), square cells of side s >= pad, at most
// kMaxCellsAxis per axis.  n = 0: the camera has no such keypoint and no job.
struct CamGrid { double x0, y0, x1, y1, s; int32_t nx, ny, n, pad_; };

ESFM_TK_HD bool finite_f(float x) { return fabsf(x) <= FLT_MAX; }
ESFM_TK_HD bool takes_part(uint8_t free_flag, float u, float v, const Options &o) { return free_flag != 0 && (o.whole || (finite_f(u) && finite_f(v))); }

// floor((x - x0) / s) clamped to 0 .. n - 1; every step is monotone non-decreasing in x (NaN gives 0)
ESFM_TK_HD int32_t cell_of(double x, double x0, double s, int32_t n)
{
    const double c = floor((x - x0) / s);
    return c >= (double)(n - 1) ? n - 1 : (c > 0.0 ? (int32_t)c : 0);
}
ESFM_TK_HD CamGrid make_grid(float x0, float y0, float x1, float y1, int32_t n, const Options &o)
{
    CamGrid g;
    g.x0 = (double)x0; g.y0 = (double)y0; g.x1 = (double)x1; g.y1 = (double)y1; g.n = n; g.pad_ = 0;
    g.s = 1.0; g.nx = g.ny = 1;
    if (n <= 0 || o.whole) return g;
    const double ex = g.x1 - g.x0, ey = g.y1 - g.y0, e = ex > ey ? ex : ey;
    const double smin = e / (double)kMaxCellsAxis;
    g.s = o.pad > smin ? o.pad : smin;
    g.nx = cell_of(g.x1, g.x0, g.s, kMaxCellsAxis) + 1;
    g.ny = cell_of(g.y1, g.y0, g.s, kMaxCellsAxis) + 1;
    return g;
}
ESFM_TK_HD int32_t keypoint_cell(const CamGrid &g, float u, float v, const Options &o)
{
    if (o.whole) return 0;
    return cell_of((double)v, g.y0, g.s, g.ny) * g.nx + cell_of((double)u, g.x0, g.s, g.nx);
}
// The cells a job walks: columns cx0 .. cx1 of rows cy0 .. cy1.  An admissible keypoint has |pu - u| <= r (1 + 2^-51) < pad = 2 r, so
// pu - pad <= u <= pu + pad in exact arithmetic; u is a float, hence exact as a double, and rounding is monotone, so
// fl(pu - pad) <= u <= fl(pu + pad) and cell_of keeps the order: the keypoint's cell is inside.
struct Window { int32_t cx0, cx1, cy0, cy1; };
ESFM_TK_HD Window window_cells(const CamGrid &g, const Pixel &q, const Options &o)
{
    Window w;
    if (o.whole) { w.cx0 = w.cx1 = w.cy0 = w.cy1 = 0; return w; }
    w.cx0 = cell_of(q.pu - o.pad, g.x0, g.s, g.nx); w.cx1 = cell_of(q.pu + o.pad, g.x0, g.s, g.nx);
    w.cy0 = cell_of(q.pv - o.pad, g.y0, g.s, g.ny); w.cy1 = cell_of(q.pv + o.pad, g.y0, g.s, g.ny);
    return w;
}
// whether (point, camera) can have an admissible keypoint at all: in front, and the window meets the box (false for NaN)
ESFM_TK_HD bool job_possible(const CamGrid &g, const Pixel &q, const Options &o)
{
    if (g.n <= 0 || !q.front) return false;
    if (o.whole) return true;
    return q.pu + o.pad >= g.x0 && q.pu - o.pad <= g.x1 && q.pv + o.pad >= g.y0 && q.pv - o.pad <= g.y1;
}

// sort key of a keypoint that takes part: camera | cell | row local to the camera
ESFM_TK_HD uint64_t grid_key(int32_t cam, int32_t cell, int32_t local_row)
{
    return (uint64_t)(uint32_t)cam << (kCellBits + kRowBits) | (uint64_t)(uint32_t)cell << kRowBits | (uint64_t)(uint32_t)local_row;
}

}  // namespace complete
}  // namespace esfm
