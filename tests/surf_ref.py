"""Independent numpy statement of the SURF detector + 64-float descriptor, written from the rule list in the header of
oracle/surf_ref.c and from Bay et al. 2008 (sections 3 and 4): exact integers for gray / integral image / box sums, float64
elsewhere, whole-array formulations.  It imports neither `oracle` nor `easysfm_amd` and uses no ctypes.

It does not reproduce a detector's output; `verify` checks the claims in one.  The reference enumerates its own maxima and sorts
every candidate into kept / rejected / undecided, where undecided means that a float32 evaluation of the stated expressions could
fall on either side of one of its decisions (the bounds are derived at `_layer` and `_refine`).  Reported keypoints and decided
reference keypoints must correspond one to one; orientation and descriptor are recomputed from the REPORTED x, y, size (and
angle), so a disagreement in one stage does not leak into the next.

Descriptor check.  Two uchar roundings (window, 21 x 21 patch) stand between the image and the descriptor, and a patch value may
sit on an exact tie (area averages of integers often end in .5).  Measured on the sampled keypoints of the four CPU cases, a
plain L2 comparison of the float64 descriptor with the one whose sample / shrink / gradient arithmetic runs in float32 shows up to
7.0e-3 (one patch value rounded the other way); 4 x that is 2.8e-2, while a descriptor recomputed with its window shifted by one
pixel lies as close as 1.3e-2 and one with its angle off by 2 degrees as close as 5.7e-3.  A tolerance must stay below half of
that, so the reference was tightened instead of the tolerance widened, in two ways:
  * the window's row starts are taken in float, as the rule states them (see `window`: their rounding drifts linearly, it is not noise);
  * `descriptor_distance` lets every patch value that lies within its derived slack of a tie round either way and reports the
    distance that is left, which is float arithmetic alone.
Measured that way (tests/test_surf_ref_cpu.py::test_descriptor_tolerance_measured asserts all of it):
  DESC_F32_DISTANCE  largest distance of the float32 run from the float64 run ......... 1.54e-7 measured, recorded as 1.6e-7
  DESC_TOL           4 x that (covers summation orders the float32 run does not try) .. 6.4e-7
  DESC_TAMPER_MIN    smallest distance of a tampered descriptor, same keypoints ....... 5.67e-3 measured (angle off 2 degrees; one-pixel
                     shift: 1.27e-2), recorded as 5.6e-3;  DESC_TOL < DESC_TAMPER_MIN / 2 holds by four orders of magnitude.

The orientation disc: the paper samples "a circular neighbourhood of radius 6s around the interest point" at step s, and OpenCV
keeps the grid points with i^2 + j^2 <= 36.  That set has 113 points (the 13 x 13 grid's 169 minus 14 per corner), not 109.
"""
import functools
import math

import numpy as np

N_OCTAVES, N_LAYERS, ORI_RADIUS, PATCH = 4, 3, 6, 20
U = 2.0 ** -24
DESC_F32_DISTANCE = 1.6e-7
DESC_TOL = 4 * DESC_F32_DISTANCE
DESC_TAMPER_MIN = 5.6e-3
ANGLE_UNDECIDED_DEG = 0.5        # an orientation whose own bound exceeds this counts as undecided


def bgr2gray(bgr):
    b = bgr.astype(np.int64)
    return ((b[..., 0] * 1868 + b[..., 1] * 9617 + b[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def as_gray(image):
    image = np.asarray(image)
    return bgr2gray(image) if image.ndim == 3 else image.astype(np.uint8)


def integral(gray):
    S = np.zeros((gray.shape[0] + 1, gray.shape[1] + 1), np.int64)
    S[1:, 1:] = gray.astype(np.int64).cumsum(0).cumsum(1)
    return S


def fast_atan2_deg(y, x):
    """cv::fastAtan2's 7th-order polynomial in float64, over arrays."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    p1, p3, p5, p7 = (k * 180 / math.pi for k in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
    ax, ay = np.abs(x), np.abs(y)
    eps = 2.220446049250313e-16
    c = np.where(ax >= ay, ay / (ax + eps), ax / (ay + eps))
    a = (((p7 * c * c + p5) * c * c + p3) * c * c + p1) * c
    a = np.where(ax >= ay, a, 90.0 - a)
    a = np.where(x < 0, 180.0 - a, a)
    return np.where(y < 0, 360.0 - a, a)


# ----------------------------------------------------------------------------------------------------------- Hessian layers
# The 9 x 9 template of the paper (figure 2 / OpenCV's tables), as (x0, y0, x1, y1, weight) with exclusive ends: Dxx has three
# 3-wide, 5-tall lobes side by side weighted 1 -2 1, Dyy is its transpose, Dxy four 3 x 3 lobes around the centre weighted 1 -1 -1 1.
DXX = [(0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1)]
DYY = [(y0, x0, y1, x1, w) for x0, y0, x1, y1, w in DXX]
DXY = [(1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1)]


def layer_table():
    """(octave, layer, filter size, sample step) of the 20 layers."""
    return [(o, k, (9 + 6 * k) << o, 1 << o) for o in range(N_OCTAVES) for k in range(N_LAYERS + 2)]


def _scaled(coord, size):
    return (2 * size * coord + 9) // 18          # cvRound(size / 9 * coord): size * coord / 9 is a multiple of 1/3, never a tie


def _filter(S, tmpl, size, st, ni, nj):
    """Response and magnitude sum of a box filter whose top-left corner visits (i st, j st): each box divided by its area."""
    val = np.zeros((ni, nj)); mag = np.zeros((ni, nj))
    at = lambda y, x: S[y:y + (ni - 1) * st + 1:st, x:x + (nj - 1) * st + 1:st]
    for x0, y0, x1, y1, w in tmpl:
        x0, y0, x1, y1 = (_scaled(c, size) for c in (x0, y0, x1, y1))
        b = (at(y1, x1) - at(y0, x1) - at(y1, x0) + at(y0, x0)) * (w / ((x1 - x0) * (y1 - y0)))
        val += b; mag += np.abs(b)
    return val, mag


# Forward error of the float32 determinant.  The box sums B_k are exact integers; a filter response is d = fl(sum_k w_k B_k) with
# w_k = fl(c_k / area) (one rounding), products and sum in double, one rounding to float: |delta d| <= 2u A, A = sum_k |w_k B_k| --
# relative to the magnitudes, since the lobes cancel.  Then det = fl(fl(dx dy) - fl(fl(0.81f dxy) dxy)):
#     |delta (dx dy)|      <= 2u (|dy| A_x + |dx| A_y) + u |dx dy|
#     |delta (.81 dxy^2)|  <= 0.81 (4u |dxy| A_xy + 3u dxy^2)            (the constant and two products)
#     the subtraction      <= u (|dx dy| + 0.81 dxy^2)
#     E_det = u (2 |dy| A_x + 2 |dx| A_y + 3.24 |dxy| A_xy + 2 |dx dy| + 3.24 dxy^2), times DET_SAFETY = 2 for the second-order terms
# and for a kernel that sums the lobes in float instead of double (one more rounding per lobe).
DET_SAFETY = 2.0


def _layer(S, size, st):
    rows, cols = S.shape[0] - 1, S.shape[1] - 1
    shape = (max(rows // st, 1), max(cols // st, 1))
    det, trace, err = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    if size > rows or size > cols:
        return det, trace, err, False
    ni, nj, m = 1 + (rows - size) // st, 1 + (cols - size) // st, (size // 2) // st
    dx, ax = _filter(S, DXX, size, st, ni, nj)
    dy, ay = _filter(S, DYY, size, st, ni, nj)
    dxy, axy = _filter(S, DXY, size, st, ni, nj)
    det[m:m + ni, m:m + nj] = dx * dy - 0.81 * dxy * dxy
    trace[m:m + ni, m:m + nj] = dx + dy
    err[m:m + ni, m:m + nj] = DET_SAFETY * U * (2 * np.abs(dy) * ax + 2 * np.abs(dx) * ay + 3.24 * np.abs(dxy) * axy + 2 * np.abs(dx * dy) + 3.24 * dxy * dxy)
    return det, trace, err, True


class Cand:
    __slots__ = ("octave", "layer", "i", "j", "x", "y", "size", "size_f", "response", "class_id", "kept", "why", "ex", "e_resp", "fits")

    @property
    def undecided(self):
        return bool(self.why)


def _refine(N, E):
    """N, E: [3 layers, 3 rows, 3 cols] determinants and their error bounds about a maximum.  Returns (x, bound on x): the offset
    (columns, rows, layers) of the quadratic's extremum, A x = b with b = -gradient, A = Hessian by central differences.
    Bound: the inputs carry E, every float32 difference adds u times the magnitudes involved (folded into dA, db below), and a
    3 x 3 LU solve in float32 has |delta x| <= 3 gamma_3 |A^-1| |L| |U| |x| <~ 16u |A^-1| |A| |x| for the mild pivot growth of a
    symmetric 3 x 3 system; in all |delta x| <= |A^-1| (db + dA |x|) + 16u |A^-1| |A| |x|."""
    c = N[1, 1, 1]
    b = -0.5 * np.array([N[1, 1, 2] - N[1, 1, 0], N[1, 2, 1] - N[1, 0, 1], N[2, 1, 1] - N[0, 1, 1]])
    cross = lambda p, q, r, s: (p - q - r + s) / 4
    dxy = cross(N[1, 2, 2], N[1, 2, 0], N[1, 0, 2], N[1, 0, 0])
    dxs = cross(N[2, 1, 2], N[2, 1, 0], N[0, 1, 2], N[0, 1, 0])
    dys = cross(N[2, 2, 1], N[2, 0, 1], N[0, 2, 1], N[0, 0, 1])
    A = np.array([[N[1, 1, 0] - 2 * c + N[1, 1, 2], dxy, dxs], [dxy, N[1, 0, 1] - 2 * c + N[1, 2, 1], dys], [dxs, dys, N[0, 1, 1] - 2 * c + N[2, 1, 1]]])
    M = np.abs(N) * 3 * U + E                       # every input with the roundings of the differences it enters
    db = 0.5 * np.array([M[1, 1, 2] + M[1, 1, 0], M[1, 2, 1] + M[1, 0, 1], M[2, 1, 1] + M[0, 1, 1]])
    cm = lambda p, q, r, s: (p + q + r + s) / 4
    mxy, mxs, mys = cm(M[1, 2, 2], M[1, 2, 0], M[1, 0, 2], M[1, 0, 0]), cm(M[2, 1, 2], M[2, 1, 0], M[0, 1, 2], M[0, 1, 0]), cm(M[2, 2, 1], M[2, 0, 1], M[0, 2, 1], M[0, 0, 1])
    mc = M[1, 1, 1]
    dA = np.array([[M[1, 1, 0] + 2 * mc + M[1, 1, 2], mxy, mxs], [mxy, M[1, 0, 1] + 2 * mc + M[1, 2, 1], mys], [mxs, mys, M[0, 1, 1] + 2 * mc + M[2, 1, 1]]])
    if abs(np.linalg.det(A)) < 1e-30 or np.linalg.cond(A) > 1e6:
        return None, None
    Ai = np.abs(np.linalg.inv(A))
    x = np.linalg.solve(A, b)
    return x, Ai @ (db + dA @ np.abs(x)) + 16 * U * (Ai @ (np.abs(A) @ np.abs(x)))


# -------------------------------------------------------------------------------------------------------------- orientation
@functools.lru_cache(maxsize=None)
def disc_points():
    """(i, j, weight) of the 113 grid points with i^2 + j^2 <= 36; weights exp(-(i^2 + j^2) / (2 * 2.5^2)) (their common
    normalisation scales every response alike and changes no angle)."""
    g = np.arange(-ORI_RADIUS, ORI_RADIUS + 1)
    i, j = np.meshgrid(g, g, indexing="ij")
    keep = i * i + j * j <= ORI_RADIUS ** 2
    return i[keep], j[keep], np.exp(-(i[keep] ** 2 + j[keep] ** 2) / (2 * 2.5 ** 2))


def _box(S, y0, x0, y1, x1):
    return S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0]


class Orientation:
    __slots__ = ("angle", "bound", "undecided", "n_fit", "n_skipped", "why")


def orientation(S, x, y, size):
    """Dominant orientation at the reported (x, y, size).  s = 1.2 size / 9; Haar wavelets of side g = 2 cvRound(2 s) whose top-left
    corner is cvRound(p + (i, j) s - (g - 1) / 2); a point takes part iff its wavelet lies inside the image.  X = right half minus
    left half, Y = upper half minus lower half, each half divided by its area; angle of a sample = fastAtan2(Y, X); the window at
    0, 5, .. 355 degrees takes the samples whose ROUNDED angle lies less than 30 away (circularly); the window with the largest
    |sum|^2 wins (the first of equals) and the keypoint's angle is fastAtan2(-sum Y, sum X).

    Samples whose float32 evaluation could differ in kind -- a corner coordinate or an angle within rounding of a tie -- are
    'uncertain': their magnitude goes into the error radius of every window they may touch instead of being trusted."""
    rows, cols = S.shape[0] - 1, S.shape[1] - 1
    out = Orientation(); out.why = []
    s = size * 1.2 / 9.0
    g = 2 * int(np.rint(2 * s))
    pi, pj, w = disc_points()
    fx, fy = x + pi * s - (g - 1) / 2.0, y + pj * s - (g - 1) / 2.0
    cx, cy = np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64)
    # float32: fl(i s) errs by u 6s, the sum and the difference by u of their results: a tie within u (2 |f| + 12 s + g) is not decided
    tie = lambda f: np.abs(np.abs(f - np.floor(f)) - 0.5) <= U * (2 * np.abs(f) + 12 * s + g)
    fits = (cy >= 0) & (cy + g <= rows) & (cx >= 0) & (cx + g <= cols)
    pos_unsure = (tie(fx) | tie(fy))
    out.n_fit, out.n_skipped = int(fits.sum()), int((~fits).sum())
    if g > rows + 1 or g > cols + 1 or out.n_fit == 0:
        out.angle = None; out.bound = 0.0; out.undecided = bool((pos_unsure & ~fits).any())
        return out
    # an uncertain corner that decides whether the point takes part at all: keep it out, charge nothing (its value is unknown) -> undecided
    if (pos_unsure & ~fits).any():
        out.why.append("a sample that may or may not fit")
    cx, cy, w, pos_unsure = cx[fits], cy[fits], w[fits], pos_unsure[fits]
    h = g // 2
    left, right = _box(S, cy, cx, cy + g, cx + h), _box(S, cy, cx + h, cy + g, cx + g)
    up, down = _box(S, cy, cx, cy + h, cx + g), _box(S, cy + h, cx, cy + g, cx + g)
    area = float(h * g)
    X, Y = (right - left) / area * w, (up - down) / area * w
    # float32 error of a sample: the two halves carry the same weight +-fl(1 / area), so their exact integer difference is scaled,
    # not cancelled: fl(1 / area), the rounding to float, the float Gaussian weight (a product of two floats: 3), the product with it -- 6u |X|
    eX, eY = 6 * U * np.abs(X), 6 * U * np.abs(Y)
    mag = np.hypot(X, Y)
    ang = fast_atan2_deg(Y, X)
    # the float32 polynomial: a few roundings at 90 and one at up to 360 degrees (2^-24 * 360 = 2e-5 each): 1e-4 in all
    e_ang = np.where(mag > 0, np.degrees((eX + eY) / np.where(mag > 0, mag, 1.0)), 0.0) + 1e-4
    ang_unsure = (mag > 0) & (np.abs(np.abs(ang - np.floor(ang)) - 0.5) <= e_ang)
    unsure = pos_unsure | ang_unsure
    R = np.rint(ang)
    R_alt = np.where(R > ang, R - 1, R + 1)                       # the other side of the tie
    win = np.arange(0, 360, 5)[:, None]
    inside = lambda r: (np.abs(r[None, :] - win) < 30) | (np.abs(r[None, :] - win) > 330)
    member = inside(R)
    d = np.abs(R[None, :] - win)
    # windows an uncertain sample may enter, leave or change: a moved corner changes the sample itself (any window within 35 degrees),
    # an angle tie only the windows whose membership differs between the two roundings
    near = (pos_unsure[None, :] & ((d < 35) | (d > 325))) | (ang_unsure[None, :] & ~pos_unsure[None, :] & (member != inside(R_alt)))
    sx, sy = member @ X, member @ Y
    n = len(X)
    touched = (near & unsure[None, :]).any(axis=1)
    rad = member @ (eX + eY) + (n + 2) * U * (member @ (np.abs(X) + np.abs(Y))) + near @ np.where(unsure, mag * (1 + 1e-3) + eX + eY, 0.0)
    mod = sx * sx + sy * sy
    norm = np.sqrt(mod)
    lo, hi = np.maximum(norm - rad, 0.0), norm + rad
    best = int(np.argmax(mod))                                   # the first of equals
    # a window made of the very same samples has the very same sum, in any arithmetic: no rival
    rivals = ~(np.all(member == member[best], axis=1) & ~touched & ~touched[best])
    rivals[best] = False
    if norm[best] == 0:
        out.angle, out.bound, out.undecided = 0.0, 0.0, bool(rad[best] > 0)
        return out
    if rivals.any() and hi[rivals].max() >= lo[best]:
        out.why.append("two windows within the error bound of each other")
    out.angle = float(fast_atan2_deg(-sy[best], sx[best]))
    out.bound = math.degrees(math.asin(min(1.0, rad[best] / norm[best]))) + 2e-4
    if out.bound > ANGLE_UNDECIDED_DEG:
        out.why.append("an uncertain sample inside the winning window")
    out.undecided = bool(out.why)
    return out


# --------------------------------------------------------------------------------------------------------------- descriptor
def window_size(size):
    """(int)(21 s), s = 1.2 size / 9, i.e. floor(2.8 size) -- in integers, since size is a whole number and 2.8 size may be one too."""
    assert size == int(size)
    return (28 * int(size)) // 10


def _area_matrix(n_src, n_dst, dtype):
    """[n_dst, n_src] interval-overlap lengths of destination cell [d c, (d + 1) c) with source pixel [s, s + 1), over c = n_src / n_dst."""
    c = n_src / n_dst
    lo, hi = np.arange(n_dst)[:, None] * c, (np.arange(n_dst)[:, None] + 1) * c
    s = np.arange(n_src)[None, :]
    return (np.clip(np.minimum(hi, s + 1) - np.maximum(lo, s), 0, None) / c).astype(dtype)


def _desc_weights():
    g = np.exp(-(np.arange(PATCH) - (PATCH - 1) / 2.0) ** 2 / (2 * 3.3 ** 2))
    return np.outer(g, g)


def window(gray, x, y, size, angle_deg, dtype=np.float64):
    """The rotated window before its rounding to uchar: sample (row i, col j) lies at p + R (j - c, i - c), c = (win - 1) / 2, R the
    rotation that takes the window's column axis onto (cos a, sin a) in image coordinates (y down).  Bilinear where the four
    neighbours exist, else the nearest pixel clamped into the image.
    Returns (values before cvRound, amplitude by which a sample may differ after cvRound in float32, number of clamped samples).

    The rule states the row starts in float: cos, sin and the first row's start p - c (cos a - sin a, sin a + cos a) are floats and
    every further row start is the previous one plus the float step (-sin a, cos a).  That is part of the rule, not of its rounding
    noise: a float on the grid plus a fixed step rounds the same way every time, so the row starts DRIFT linearly, by up to half an
    ulp of the coordinate per row (1e-2 px over a 300-row window), and a tolerance wide enough to absorb the drift's uchar flips
    would also absorb a one-pixel shift of a large keypoint.  So the row starts are taken as stated, in float, in both runs;
    positions along a row, the bilinear form, the shrink and the gradients run in `dtype`.

    The amplitude: along a row a float32 evaluation places a sample within dp = 4u (max(|x|, |y|) + win) of that position.  The
    bilinear surface moves by at most (largest difference along x + along y of the four neighbours) per pixel, plus 4u * 255 for its
    own arithmetic; a value within that of a tie may round either way (amplitude 1).  A clamped sample within dp of a pixel boundary
    may take the neighbouring pixel."""
    f, f32 = dtype, np.float32
    rows, cols = gray.shape
    n = window_size(size)
    a = f32(angle_deg) * f32(math.pi / 180)
    ca, sa = f32(math.cos(float(a))), f32(math.sin(float(a)))
    off = -f32(n - 1) / f32(2)
    x0, y0 = f32(x) + off * ca - off * sa, f32(y) + off * sa + off * ca
    steps = lambda first, step: np.cumsum(np.concatenate([[first], np.full(n - 1, step, f32)]).astype(f32), dtype=f32)   # float additions, one after the other
    sx, sy = steps(x0, -sa), steps(y0, ca)
    j = np.arange(n, dtype=f)[None, :]
    px, py = sx[:, None].astype(f) + j * f(ca), sy[:, None].astype(f) + j * f(sa)
    ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    inside = (ix >= 0) & (ix < cols - 1) & (iy >= 0) & (iy < rows - 1)
    jx, jy = np.clip(ix, 0, max(cols - 2, 0)), np.clip(iy, 0, max(rows - 2, 0))
    kx, ky = np.minimum(jx + 1, cols - 1), np.minimum(jy + 1, rows - 1)
    fa, fb = (px - ix).astype(f), (py - iy).astype(f)
    G = gray.astype(f)
    one = f(1)
    p00, p01, p10, p11 = G[jy, jx], G[jy, kx], G[ky, jx], G[ky, kx]
    bil = p00 * (one - fa) * (one - fb) + p01 * fa * (one - fb) + p10 * (one - fa) * fb + p11 * fa * fb
    cl = lambda r, hi: np.clip(np.rint(r).astype(np.int64), 0, hi)
    near = G[cl(py, rows - 1), cl(px, cols - 1)]
    val = np.where(inside, bil, near)
    dp = 4 * U * (max(abs(x), abs(y)) + n)
    slope = np.maximum(np.abs(p01 - p00), np.abs(p11 - p10)) + np.maximum(np.abs(p10 - p00), np.abs(p11 - p01))
    amp = np.where(np.abs(np.abs(bil - np.floor(bil)) - 0.5) <= dp * slope + 4 * U * 255, 1.0, 0.0)
    other = lambda r: np.where(np.rint(r) > r, np.rint(r) - 1, np.rint(r) + 1)                     # the pixel across the nearest boundary
    amp_near = np.maximum(np.where(np.abs(np.abs(px - np.floor(px)) - 0.5) <= dp, np.abs(G[cl(py, rows - 1), cl(other(px), cols - 1)] - near), 0.0),
                          np.where(np.abs(np.abs(py - np.floor(py)) - 0.5) <= dp, np.abs(G[cl(other(py), rows - 1), cl(px, cols - 1)] - near), 0.0))
    # a sample within dp of the edge of the bilinear region may be taken by the other rule
    edge = (np.minimum(np.abs(px - 0), np.abs(px - (cols - 1))) <= dp) | (np.minimum(np.abs(py - 0), np.abs(py - (rows - 1))) <= dp)
    amp = np.where(inside, amp, amp_near) + np.where(edge, np.abs(np.rint(bil) - near) + 1.0, 0.0)
    return val, amp, int((~inside).sum())


def patch(gray, x, y, size, angle_deg, dtype=np.float64):
    """The 21 x 21 patch before its rounding to uchar, and the slack by which a float32 evaluation may move it: the area average of
    the rounded window (a matrix of interval-overlap lengths on each side), slack = the same average of the window's amplitudes
    + 2 (c + 3) u 255 for float sums of c + 2 terms along each axis, c = win / 21."""
    val, amp, _ = window(gray, x, y, size, angle_deg, dtype)
    A = _area_matrix(val.shape[0], PATCH + 1, dtype)
    A64 = A.astype(np.float64)
    return (A @ np.rint(val).astype(dtype)) @ A.T, (A64 @ amp) @ A64.T + 2 * (val.shape[0] / (PATCH + 1) + 3) * U * 255


def vector(P, dtype=np.float64):
    """64 floats from a 21 x 21 uchar patch: 2 x 2 differences, sigma-3.3 weights, 4 x 4 cells of 5 x 5 samples holding
    (sum dx, sum dy, sum |dx|, sum |dy|), unit length.  The float32 form adds the 25 samples of a cell one after the other."""
    f = dtype
    P = np.clip(P, 0, 255).astype(f)
    wt = _desc_weights().astype(f)
    dx = (P[:-1, 1:] - P[:-1, :-1] + P[1:, 1:] - P[1:, :-1]) * wt
    dy = (P[1:, :-1] - P[:-1, :-1] + P[1:, 1:] - P[:-1, 1:]) * wt
    cells = lambda t: np.cumsum(t.reshape(4, 5, 4, 5).transpose(0, 2, 1, 3).reshape(4, 4, 25), axis=2, dtype=f)[:, :, -1]
    v = np.stack([cells(dx), cells(dy), cells(np.abs(dx)), cells(np.abs(dy))], axis=-1).reshape(64)
    return (v / f(np.sqrt(np.sum((v * v).astype(np.float64))) + 2.220446049250313e-16)).astype(np.float64)


def describe(gray, x, y, size, angle_deg, dtype=np.float64):
    """The 64-float descriptor at the given x, y, size, angle, every rounding taken at its nominal value."""
    pre, _ = patch(gray, x, y, size, angle_deg, dtype)
    return vector(np.rint(pre), dtype)


def descriptor_distance(gray, x, y, size, angle_deg, reported):
    """L2 distance of `reported` from the float64 descriptor, where every patch value that lies within its slack of a rounding tie
    may take either neighbour: the roundings are chosen one by one, in sweeps until none helps, to bring the descriptor closest.  What is left
    is float arithmetic alone.  Returns (distance, number of patch values that could round either way)."""
    pre, slack = patch(gray, x, y, size, angle_deg)
    P = np.rint(pre)
    frac = pre - np.floor(pre)
    free = np.argwhere(np.abs(frac - 0.5) <= np.minimum(slack, 0.5))
    rep = np.asarray(reported, np.float64)
    best = float(np.linalg.norm(vector(P) - rep))
    for _ in range(8):
        before = best
        for i, j in free:
            alt = P.copy()
            alt[i, j] = np.floor(pre[i, j]) + np.ceil(pre[i, j]) - P[i, j] if np.floor(pre[i, j]) != np.ceil(pre[i, j]) else P[i, j]
            d = float(np.linalg.norm(vector(alt) - rep))
            if d < best:
                best, P = d, alt
        if best == before:
            break
    return best, len(free)


# ------------------------------------------------------------------------------------------------------------------- stages
class Stages:
    """Gray image, integral image, the 20 determinant / trace layers with their error bounds, and every candidate maximum."""

    def __init__(self, image, threshold):
        self.gray = as_gray(image)
        self.S = integral(self.gray)
        self.threshold = float(np.float32(threshold))
        self.table = layer_table()
        self.layers = [_layer(self.S, size, st) for _, _, size, st in self.table]
        self.cands = []
        for L, (o, k, size, st) in enumerate(self.table):
            if 1 <= k <= N_LAYERS:
                self._maxima(L, o, k, size, st)

    def _maxima(self, L, o, k, size, st):
        det, trace, err, valid = self.layers[L]
        rows, cols = det.shape
        m = (self.table[L + 1][2] // 2) // st + 1
        if not valid or rows - m <= m or cols - m <= m:
            return
        stack = np.stack([self.layers[L + t][0] for t in (-1, 0, 1)]), np.stack([self.layers[L + t][2] for t in (-1, 0, 1)])
        c, ce = det[m:rows - m, m:cols - m], err[m:rows - m, m:cols - m]
        loose = c + ce > self.threshold
        gap = np.full(c.shape, np.inf)                       # smallest (margin over a neighbour) minus (the pair's error bounds)
        for t in range(3):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (t, dy, dx) == (1, 0, 0):
                        continue
                    nb = stack[0][t][m + dy:rows - m + dy, m + dx:cols - m + dx]
                    ne = stack[1][t][m + dy:rows - m + dy, m + dx:cols - m + dx]
                    loose &= c + ce + ne > nb
                    gap = np.minimum(gap, c - nb - ce - ne)
        for i, j in np.argwhere(loose) + m:
            cd = Cand(); cd.why = []
            cd.octave, cd.layer, cd.i, cd.j = o, k, int(i), int(j)
            cd.response, cd.e_resp = float(det[i, j]), float(err[i, j])
            if cd.response - self.threshold <= cd.e_resp:
                cd.why.append("threshold margin")
            if gap[i - m, j - m] <= 0:
                cd.why.append("margin over a neighbour")
            is_max = cd.response > self.threshold and all(cd.response > stack[0][t][i + dy, j + dx] for t in range(3) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (t, dy, dx) != (1, 0, 0))
            N, E = stack[0][:, i - 1:i + 2, j - 1:j + 2], stack[1][:, i - 1:i + 2, j - 1:j + 2]
            x, ex = _refine(N, E)
            tr = float(trace[i, j])
            cd.class_id = (tr > 0) - (tr < 0)
            if x is None:
                cd.kept, cd.ex = False, np.zeros(3); cd.x = cd.y = cd.size = cd.size_f = 0.0
                cd.why.append("singular refinement")
                self.cands.append(cd); continue
            cd.ex = ex
            if np.any(np.abs(np.abs(x) - 1.0) <= ex):
                cd.why.append("|x_i| against 1")
            cd.kept = bool(is_max and np.any(x != 0) and np.all(np.abs(x) <= 1))
            corner = st * (np.array([j, i]) - (size // 2) // st)             # the filter's top-left corner in the image
            cd.x, cd.y = (corner + (size - 1) * 0.5 + x[:2] * st).tolist()
            ds = size - self.table[L - 1][2]
            cd.size_f = size + x[2] * ds
            cd.size = float(np.rint(cd.size_f))
            if abs(abs(cd.size_f - math.floor(cd.size_f)) - 0.5) <= ex[2] * ds + 4 * U * size:
                cd.why.append("cvRound of the size")
            self.cands.append(cd)

    def kept(self):
        return [c for c in self.cands if c.kept]

    def sort_key(self, c):
        return (-c.response, -c.size, -c.octave, -c.y, c.x)


# ------------------------------------------------------------------------------------------------------------------- verify
class Report:
    def __init__(self):
        self.errors, self.undecided = [], []
        self.n_reference = self.n_reported = self.n_described = self.n_clamped = self.n_partial_disc = self.n_free_roundings = 0
        self.max_desc_distance = 0.0

    @property
    def ok(self):
        return not self.errors

    def undecided_share(self):
        return len(self.undecided) / max(self.n_reference, 1)

    def __repr__(self):
        return (f"<surf report: {self.n_reported} reported, {self.n_reference} reference, {len(self.undecided)} undecided, {self.n_described} described "
                f"(max distance {self.max_desc_distance:.3g}, {self.n_free_roundings} free roundings), {self.n_clamped} with clamped samples, {self.n_partial_disc} with a partial disc, "
                f"{len(self.errors)} errors: {self.errors[:4]}>")


def sample_indices(keypoints, limit=150, seed=0):
    """At most `limit` keypoints for the descriptor check: the ten largest sizes and a seeded draw of the rest."""
    n = len(keypoints)
    if n <= limit:
        return np.arange(n)
    big = np.argsort(-np.asarray(keypoints)[:, 2], kind="stable")[:10]
    rest = np.setdiff1d(np.arange(n), big)
    return np.sort(np.concatenate([big, np.random.default_rng(seed).choice(rest, limit - 10, replace=False)]))


def verify(image, params, keypoints, descriptors, stages=None):
    """params: {'hessian_threshold': t, optional 'describe': indices or None for the seeded sample}.  keypoints [n, 7] float32
    (x, y, size, angle, response, octave, class_id), descriptors [n, 64] float32."""
    st = stages or Stages(image, params["hessian_threshold"])
    rep = Report()
    err = rep.errors.append
    kp = np.asarray(keypoints, np.float64)
    rep.n_reported = len(kp)
    if len(kp) != len(descriptors):
        err("keypoint and descriptor counts differ")
        return rep
    rows, cols = st.gray.shape
    # the reference's own keypoints: kept by its float64 decisions and with an orientation that can be sampled
    ori_ref = {}
    for c in st.cands:
        if c.kept or c.undecided:
            o = orientation(st.S, float(np.float32(c.x)), float(np.float32(c.y)), c.size) if c.size > 0 else None
            c.fits = o is not None and o.angle is not None
            if o is not None and o.angle is None and o.undecided and "orientation that may or may not be sampled" not in c.why:
                c.why.append("orientation that may or may not be sampled")
        else:
            c.fits = False
    ref = [c for c in st.cands if c.kept and c.fits]
    rep.n_reference = len(ref)
    rep.undecided += [("candidate", c.octave, c.layer, c.i, c.j, tuple(c.why)) for c in st.cands if c.undecided]
    # one to one: every reported keypoint takes the nearest candidate of its octave
    by_oct = {}
    for c in st.cands:
        by_oct.setdefault(c.octave, []).append(c)
    taken = {}
    for k, (x, y, size, angle, resp, octave, cid) in enumerate(kp):
        pool = by_oct.get(int(octave), []) if octave == int(octave) else []
        step = 1 << int(octave) if pool else 1
        best = min(pool, key=lambda c: (c.x - x) ** 2 + (c.y - y) ** 2 + (0 if abs(c.size_f - size) <= 0.5 + c.ex[2] * 64 else 1e6), default=None)
        tol = lambda c, t: c.ex[t] * step + 8 * U * (abs(x) + abs(y) + step)
        if best is None or abs(best.x - x) > tol(best, 0) or abs(best.y - y) > tol(best, 1):
            err(f"kp {k}: ({x:.4f}, {y:.4f}) octave {octave} matches no maximum of the reference"
                + (f" (nearest ({best.x:.4f}, {best.y:.4f}), bounds {tol(best, 0):.2g}, {tol(best, 1):.2g})" if best else ""))
            continue
        c = best
        if id(c) in taken:
            err(f"kp {k}: the maximum at ({c.x:.3f}, {c.y:.3f}) is reported twice (also kp {taken[id(c)]})"); continue
        taken[id(c)] = k
        if not c.kept and not c.undecided:
            err(f"kp {k}: ({x:.3f}, {y:.3f}) is a candidate the reference rejects")
        if size != c.size and "cvRound of the size" not in c.why:
            err(f"kp {k}: size {size} vs {c.size} ({c.size_f:.5f})")
        if abs(resp - c.response) > c.e_resp + 2 * U * abs(c.response):
            err(f"kp {k}: response {resp!r} vs {c.response!r} (bound {c.e_resp:.3g})")
        if cid != c.class_id:
            err(f"kp {k}: class_id {cid} vs sign of the trace {c.class_id}")
    for c in ref:
        if id(c) not in taken and not c.undecided:
            err(f"missing keypoint ({c.x:.3f}, {c.y:.3f}) size {c.size} octave {c.octave}")
    # order: (response, size, octave, y) descending, then x ascending
    key = [(-float(r[4]), -float(r[2]), -float(r[5]), -float(r[1]), float(r[0])) for r in np.asarray(keypoints, np.float32)]
    for k in range(len(key) - 1):
        if key[k] >= key[k + 1]:
            err(f"order: kp {k} {key[k]} before kp {k + 1} {key[k + 1]}")
    # orientation and descriptor from the reported fields
    which = params.get("describe")
    which = sample_indices(keypoints) if which is None else np.asarray(which, np.int64)
    tolerance = params.get("desc_tol", DESC_TOL)
    for k, (x, y, size, angle, resp, octave, cid) in enumerate(kp):
        if size != int(size) or size <= 0:
            err(f"kp {k}: size {size}"); continue
        o = orientation(st.S, x, y, size)
        if o.angle is None:
            err(f"kp {k}: reported although no orientation sample fits"); continue
        rep.n_partial_disc += o.n_skipped > 0
        if o.undecided:
            rep.undecided.append(("orientation", k, tuple(o.why)))
        elif abs((angle - o.angle + 180.0) % 360.0 - 180.0) > o.bound:
            err(f"kp {k}: angle {angle} vs {o.angle} (bound {o.bound:.3g})")
    for k in which:
        x, y, size, angle = kp[k, :4]
        if size != int(size) or size <= 0:
            continue
        rep.n_clamped += window(st.gray, x, y, size, angle)[2] > 0
        dist, n_free = descriptor_distance(st.gray, x, y, size, angle, descriptors[k])
        rep.n_free_roundings += n_free
        rep.n_described += 1
        rep.max_desc_distance = max(rep.max_desc_distance, dist)
        if not dist <= tolerance:
            err(f"kp {k}: descriptor at L2 distance {dist:.3g} (tolerance {tolerance:.3g})")
    return rep
