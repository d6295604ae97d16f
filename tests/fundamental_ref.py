"""References for the fundamental-matrix model and the focal-length cost (esfm.h "Fundamental-matrix RANSAC"; a helper, not a test
module).  Two routes that share no code:

Route (a), the RESTATEMENT: the rule list of esfm.h, operation by operation in the order easysfm_amd/csrc/fundamental_core.hpp's
comment states, on plain Python floats (IEEE doubles; math.sqrt is correctly rounded).  The host build, the kernels and this route
agree to the bit.  The float scoring runs on numpy float32 arrays: every numpy elementwise operation is one correctly rounded float
operation (nothing is fused).

Route (b), an INDEPENDENT route for the minimal solve: numpy reductions for the normalisation, numpy.linalg.svd for the null space,
the cubic's coefficients by interpolating numpy.linalg.det at four points, numpy.roots.  It agrees with (a) only as far as the
problem's conditioning allows."""
import math

import numpy as np

from homography_ref import (CvRng, DBL_EPSILON, DBL_MAX, LANES, SQRT2, _as_lists, _dist, _div, _tree, jacobi_sym, update_num_iters,
                            with_silent_numpy)

LEAD_EPS = 1e-12
ROOT_SWEEPS = 80
SVD_SWEEPS = 60
MAX_ITERS = 1000


# ---- route (a) -------------------------------------------------------------------------------------------------------------
def _row(t1, t2, x, y, X, Y):
    u = (x - t1[0]) * t1[2]; v = (y - t1[1]) * t1[2]; p = (X - t2[0]) * t2[2]; q = (Y - t2[1]) * t2[2]
    return [p * u, p * v, p, q * u, q * v, q, u, v, 1.0]


def _finish(fn, t1, t2):
    """de-normalisation, unit Frobenius norm, canonical sign -> list of 9 or None"""
    mx1, my1, s1 = t1
    mx2, my2, s2 = t2
    M = [0.0] * 9
    for r in range(3):
        m0 = fn[3 * r] * s1
        m1 = fn[3 * r + 1] * s1
        M[3 * r] = m0; M[3 * r + 1] = m1; M[3 * r + 2] = (fn[3 * r + 2] - m0 * mx1) - m1 * my1
    F = [0.0] * 9
    for c in range(3):
        F[c] = M[c] * s2
        F[3 + c] = M[3 + c] * s2
        F[6 + c] = (M[6 + c] - F[c] * mx2) - F[3 + c] * my2
    ss = 0.0
    for i in range(9):
        ss += F[i] * F[i]
    nrm = math.sqrt(ss) if ss >= 0.0 else float("nan")
    big = 0.0; at = 0.0; finite = True
    for i in range(9):
        F[i] = _div(F[i], nrm)
        a = abs(F[i])
        finite = finite and (a <= DBL_MAX)
        if a > big:
            big = a; at = F[i]
    if not finite:
        return None
    if at < 0.0:
        F = [-v for v in F]
    return F


def _dot(s, t):
    return (s[0] * t[0] + s[1] * t[1]) + s[2] * t[2]


def _cross(s, t):
    return [s[1] * t[2] - s[2] * t[1], s[2] * t[0] - s[0] * t[2], s[0] * t[1] - s[1] * t[0]]


def det_cubic(a, b):
    """c0 .. c3 of det(a + x b), a and b lists of 9"""
    a0, a1, a2 = a[0:3], a[3:6], a[6:9]
    b0, b1, b2 = b[0:3], b[3:6], b[6:9]
    w0 = _cross(a1, a2)
    w1 = _cross(a1, b2); t = _cross(b1, a2)
    w1 = [w1[i] + t[i] for i in range(3)]
    w2 = _cross(b1, b2)
    return [_dot(a0, w0), _dot(a0, w1) + _dot(b0, w0), _dot(a0, w2) + _dot(b0, w1), _dot(b0, w2)]


def _bracket_root(A, B, D, lo, hi, rising):
    x = 0.5 * (lo + hi)
    for _ in range(ROOT_SWEEPS):
        f = ((x + A) * x + B) * x + D
        if f == 0.0:
            break
        if (f < 0.0) == rising:
            lo = x
        else:
            hi = x
        xn = x - _div(f, (3.0 * x + 2.0 * A) * x + B)
        if not (xn > lo and xn < hi):
            xn = 0.5 * (lo + hi)
        if xn == x:
            break
        x = xn
    return x


@with_silent_numpy
def cubic_roots(c):
    """the real roots of c0 + c1 x + c2 x^2 + c3 x^3 by the written rule, ascending"""
    big = 0.0; finite = True
    for i in range(4):
        a = abs(c[i])
        finite = finite and (a <= DBL_MAX)
        big = a if a > big else big
    if not finite or big == 0.0:
        return []
    tiny = LEAD_EPS * big
    if abs(c[3]) <= tiny:
        if abs(c[2]) <= tiny:
            if abs(c[1]) <= tiny:
                return []
            return [_div(-c[0], c[1])]
        disc = c[1] * c[1] - 4.0 * c[2] * c[0]
        if not disc >= 0.0:
            return []
        sq = math.sqrt(disc)
        q = -0.5 * (c[1] + (sq if c[1] >= 0.0 else -sq))
        if disc == 0.0:
            return [_div(q, c[2])]
        r0 = _div(q, c[2]); r1 = _div(c[0], q)
        return [r1, r0] if r1 < r0 else [r0, r1]
    A = _div(c[2], c[3]); B = _div(c[1], c[3]); D = _div(c[0], c[3])
    m = abs(A)
    m = abs(B) if abs(B) > m else m
    m = abs(D) if abs(D) > m else m
    R = 1.0 + m
    disc = A * A - 3.0 * B
    if not disc > 0.0:
        return [_bracket_root(A, B, D, -R, R, True)]
    sq = math.sqrt(disc)
    x1 = (-A - sq) / 3.0; x2 = (-A + sq) / 3.0
    p1 = ((x1 + A) * x1 + B) * x1 + D; p2 = ((x2 + A) * x2 + B) * x2 + D
    out = []
    if p1 >= 0.0:
        out.append(_bracket_root(A, B, D, -R, x1, True))
    if p1 > 0.0 and p2 < 0.0:
        out.append(_bracket_root(A, B, D, x1, x2, False))
    if p2 <= 0.0:
        out.append(_bracket_root(A, B, D, x2, R, True))
    return out


@with_silent_numpy
def minimal_solve(p1, p2, detail=False):
    """fundamental_from_7: p1, p2 [7][2] pixels -> list of models (each a list of 9 floats), in root order.
    detail=True: (models, dict with the normalised null vectors f1, f2, the normalisations, the cubic and its roots)"""
    p1 = [[float(v) for v in r] for r in p1]; p2 = [[float(v) for v in r] for r in p2]
    sx = sy = sX = sY = 0.0
    for k in range(7):
        sx += p1[k][0]; sy += p1[k][1]; sX += p2[k][0]; sY += p2[k][1]
    mx1, my1, mx2, my2 = sx / 7.0, sy / 7.0, sX / 7.0, sY / 7.0
    d1 = d2 = 0.0
    for k in range(7):
        d1 += _dist(mx1, my1, p1[k][0], p1[k][1]); d2 += _dist(mx2, my2, p2[k][0], p2[k][1])
    t1 = (mx1, my1, _div(SQRT2, d1 / 7.0)); t2 = (mx2, my2, _div(SQRT2, d2 / 7.0))
    a = [_row(t1, t2, p1[k][0], p1[k][1], p2[k][0], p2[k][1]) for k in range(7)]
    beta = [0.0] * 7
    for j in range(7):
        aj = a[j]
        s = 0.0
        for r in range(j, 9):
            s += aj[r] * aj[r]
        nrm = math.sqrt(s) if s >= 0.0 else float("nan")
        x0 = aj[j]
        v0 = x0 - (-nrm if x0 >= 0.0 else nrm)
        aj[j] = v0
        vtv = v0 * v0
        for r in range(j + 1, 9):
            vtv += aj[r] * aj[r]
        bj = _div(2.0, vtv) if vtv > 0.0 else 0.0
        beta[j] = bj
        for c in range(j + 1, 7):
            ac = a[c]
            d = 0.0
            for r in range(j, 9):
                d += aj[r] * ac[r]
            f = bj * d
            for r in range(j, 9):
                ac[r] -= f * aj[r]
    f1 = [0.0] * 9; f1[7] = 1.0
    f2 = [0.0] * 9; f2[8] = 1.0
    for j in range(6, -1, -1):
        aj = a[j]
        d = e = 0.0
        for r in range(j, 9):
            d += aj[r] * f1[r]; e += aj[r] * f2[r]
        fd = beta[j] * d; fe = beta[j] * e
        for r in range(j, 9):
            f1[r] -= fd * aj[r]; f2[r] -= fe * aj[r]
    b = [f1[i] - f2[i] for i in range(9)]
    c = det_cubic(f2, b)
    roots = cubic_roots(c)
    models, normalised = [], []
    for x in roots:
        om = 1.0 - x
        fn = [x * f1[i] + om * f2[i] for i in range(9)]
        F = _finish(fn, t1, t2)
        if F is not None:
            models.append(F); normalised.append(fn)
    if detail:
        return models, dict(f1=f1, f2=f2, t1=t1, t2=t2, cubic=c, roots=roots, normalised=normalised)
    return models


def jacobi_cols3(W):
    """one-sided Jacobi on the columns of the row-major 3 x 3 W (in place) -> V"""
    V = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for _ in range(SVD_SWEEPS):
        changed = False
        for p in range(2):
            for q in range(p + 1, 3):
                a = b = c = 0.0
                for r in range(3):
                    a += W[3 * r + p] * W[3 * r + p]; b += W[3 * r + q] * W[3 * r + q]; c += W[3 * r + p] * W[3 * r + q]
                ab = a * b
                if abs(c) <= DBL_EPSILON * (math.sqrt(ab) if ab >= 0.0 else float("nan")) or c == 0.0:
                    continue
                changed = True
                zeta = _div(b - a, 2.0 * c)
                t = _div(1.0 if zeta >= 0.0 else -1.0, abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / math.sqrt(1.0 + t * t); sn = cs * t
                for r in range(3):
                    u, v = W[3 * r + p], W[3 * r + q]
                    W[3 * r + p] = cs * u - sn * v; W[3 * r + q] = sn * u + cs * v
                    vu, vv = V[3 * r + p], V[3 * r + q]
                    V[3 * r + p] = cs * vu - sn * vv; V[3 * r + q] = sn * vu + cs * vv
        if not changed:
            break
    return V


def _col_norms(W):
    n = []
    for k in range(3):
        sq = 0.0
        for r in range(3):
            sq += W[3 * r + k] * W[3 * r + k]
        n.append(sq)
    return n


def rank2(fn):
    W = list(fn)
    V = jacobi_cols3(W)
    n = _col_norms(W)
    drop = 0
    if n[1] < n[drop]:
        drop = 1
    if n[2] < n[drop]:
        drop = 2
    out = [0.0] * 9
    for r in range(3):
        for c in range(3):
            s = 0.0
            for k in range(3):
                if k != drop:
                    s += W[3 * r + k] * V[3 * c + k]
            out[3 * r + c] = s
    return out


@with_silent_numpy
def refit(pts1, pts2, mask=None):
    """fundamental_refit_host / fundamental_refit_kernel -> (F list of 9, True) or ([0.0] * 9, False)"""
    a = _as_lists(pts1); b = _as_lists(pts2)
    n = len(a)
    keep = [True] * n if mask is None else [bool(v) for v in mask]
    cnt = sum(keep)
    if cnt < 8:
        return [0.0] * 9, False
    lanes = [[i for i in range(l, n, LANES) if keep[i]] for l in range(LANES)]
    parts = [[0.0] * LANES for _ in range(4)]
    for l in range(LANES):
        for i in lanes[l]:
            parts[0][l] += a[i][0]; parts[1][l] += a[i][1]; parts[2][l] += b[i][0]; parts[3][l] += b[i][1]
    nn = float(cnt)
    mx1, my1, mx2, my2 = _tree(parts[0]) / nn, _tree(parts[1]) / nn, _tree(parts[2]) / nn, _tree(parts[3]) / nn
    parts = [[0.0] * LANES for _ in range(2)]
    for l in range(LANES):
        for i in lanes[l]:
            parts[0][l] += _dist(mx1, my1, a[i][0], a[i][1]); parts[1][l] += _dist(mx2, my2, b[i][0], b[i][1])
    t1 = (mx1, my1, _div(SQRT2, _tree(parts[0]) / nn)); t2 = (mx2, my2, _div(SQRT2, _tree(parts[1]) / nn))
    parts = [[0.0] * LANES for _ in range(45)]
    for l in range(LANES):
        g = [0.0] * 45
        for i in lanes[l]:
            r = _row(t1, t2, a[i][0], a[i][1], b[i][0], b[i][1])
            e = 0
            for p in range(9):
                for q in range(p, 9):
                    g[e] += r[p] * r[q]
                    e += 1
        for e in range(45):
            parts[e][l] = g[e]
    g = [_tree(parts[e]) for e in range(45)]
    A = [0.0] * 81
    e = 0
    for p in range(9):
        for q in range(p, 9):
            A[9 * p + q] = g[e]; A[9 * q + p] = g[e]
            e += 1
    V = jacobi_sym(A, 9)
    best = 0
    for k in range(1, 9):
        if A[10 * k] < A[10 * best]:
            best = k
    F = _finish(rank2([V[9 * r + best] for r in range(9)]), t1, t2)
    return (F, True) if F is not None else ([0.0] * 9, False)


def epipolar_errors(F, pts1, pts2):
    """(e1, e2) on float32 arrays: one correctly rounded float operation per numpy call, sums left to right"""
    Ff = np.asarray(F, np.float64).reshape(9).astype(np.float32)
    a_ = np.asarray(pts1, np.float32).reshape(-1, 2); b_ = np.asarray(pts2, np.float32).reshape(-1, 2)
    x, y, X, Y = a_[:, 0], a_[:, 1], b_[:, 0], b_[:, 1]
    with np.errstate(all="ignore"):
        a = Ff[0] * x + Ff[1] * y + Ff[2]; b = Ff[3] * x + Ff[4] * y + Ff[5]; c = Ff[6] * x + Ff[7] * y + Ff[8]
        d2 = X * a + Y * b + c
        e2 = d2 * d2 / (a * a + b * b)
        a1 = Ff[0] * X + Ff[3] * Y + Ff[6]; b1 = Ff[1] * X + Ff[4] * Y + Ff[7]; c1 = Ff[2] * X + Ff[5] * Y + Ff[8]
        d1 = x * a1 + y * b1 + c1
        e1 = d1 * d1 / (a1 * a1 + b1 * b1)
    assert e1.dtype == np.float32 and e2.dtype == np.float32
    return e1, e2


def inlier_mask(F, pts1, pts2, threshold):
    e1, e2 = epipolar_errors(F, pts1, pts2)
    t = np.float32(float(threshold) * float(threshold))
    with np.errstate(all="ignore"):
        return (e1 <= t) & (e2 <= t)


def draw7(rng, count):
    idx = []
    while len(idx) < 7:
        v = rng.uniform(0, count)
        if v not in idx:
            idx.append(v)
    return idx


def sample_stream(count, n_samples):
    rng = CvRng()
    return np.array([draw7(rng, count) for _ in range(n_samples)], np.int32).reshape(-1, 7)


def find_fundamental(pts1, pts2, threshold, confidence=0.99):
    """The whole rule of esfm_find_fundamental -> (F [3,3] or None, mask [n] bool, iterations, n_inliers under the returned F).
    Raises ValueError for n < 7 (the library's ESFM_ERR_UNSUPPORTED)."""
    a32 = np.asarray(pts1, np.float32).reshape(-1, 2); b32 = np.asarray(pts2, np.float32).reshape(-1, 2)
    n = len(a32)
    if n < 7:
        raise ValueError("n < 7")
    p1, p2 = _as_lists(a32), _as_lists(b32)
    if n == 7:
        best, best_c = None, -1
        for F in minimal_solve(p1, p2):
            c = int(np.count_nonzero(inlier_mask(F, a32, b32, threshold)))
            if c > best_c:
                best, best_c = F, c
        if best is None:
            return None, np.zeros(n, bool), 0, 0
        return np.array(best).reshape(3, 3), np.ones(n, bool), 0, int(np.count_nonzero(inlier_mask(best, a32, b32, threshold)))
    rng = CvRng()
    niters, max_good, it, best = MAX_ITERS, 0, 0, None
    while it < niters:
        idx = draw7(rng, n)
        for F in minimal_solve([p1[i] for i in idx], [p2[i] for i in idx]):
            good = int(np.count_nonzero(inlier_mask(F, a32, b32, threshold)))
            if good > max(max_good, 6):
                best, max_good = F, good
                niters = update_num_iters(confidence, (n - good) / n, 7, niters)
        it += 1
    if best is None:
        return None, np.zeros(n, bool), it, 0
    mask = inlier_mask(best, a32, b32, threshold)
    Fr, ok = refit(a32, b32, mask)
    out = Fr if ok else best
    return np.array(out).reshape(3, 3), mask, it, int(np.count_nonzero(inlier_mask(out, a32, b32, threshold)))


@with_silent_numpy
def focal_term(F, f, cx, cy):
    F = [float(v) for v in np.asarray(F, np.float64).reshape(9)]
    M = [0.0] * 9
    for r in range(3):
        M[3 * r] = F[3 * r] * f; M[3 * r + 1] = F[3 * r + 1] * f; M[3 * r + 2] = (F[3 * r] * cx + F[3 * r + 1] * cy) + F[3 * r + 2]
    G = [0.0] * 9
    for c in range(3):
        G[c] = f * M[c]; G[3 + c] = f * M[3 + c]; G[6 + c] = (cx * M[c] + cy * M[3 + c]) + M[6 + c]
    jacobi_cols3(G)
    n = _col_norms(G)
    top = 0
    if n[1] > n[top]:
        top = 1
    if n[2] > n[top]:
        top = 2
    mid = -1.0
    for k in range(3):
        if k != top and n[k] > mid:
            mid = n[k]
    s1 = math.sqrt(n[top]) if n[top] >= 0.0 else float("nan")
    s2 = math.sqrt(mid) if mid >= 0.0 else float("nan")
    return _div(s1 - s2, s1 + s2)


def focal_cost(Fs, weights, cx, cy, candidates):
    Fs = np.asarray(Fs, np.float64).reshape(-1, 9)
    w = [float(v) for v in np.asarray(weights, np.float64).reshape(-1)]
    n = len(Fs)
    den = [0.0] * LANES
    for l in range(LANES):
        for p in range(l, n, LANES):
            den[l] += w[p]
    wsum = _tree(den)
    out = []
    for f in candidates:
        f = float(f)
        num = [0.0] * LANES
        for l in range(LANES):
            for p in range(l, n, LANES):
                num[l] += w[p] * focal_term(Fs[p], f, float(cx), float(cy))
        out.append(_div(_tree(num), wsum))
    return np.array(out, np.float64)


# ---- route (b) -------------------------------------------------------------------------------------------------------------
def _hartley_b(p):
    p = np.asarray(p, np.float64)
    c = p.mean(axis=0)
    s = np.sqrt(2.0) / np.linalg.norm(p - c, axis=1).mean()
    return (p - c) * s, np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def svd_route(p1, p2):
    """The 7-point solve through numpy -> dict: roots (complex, all three), real (the real ones, ascending, imaginary part exactly 0
    as numpy.roots reports a real pair), models (normalised frame, unit norm, one per real root), A (the normalised 7 x 9 system),
    sv (its singular values); None when the system is not finite."""
    with np.errstate(all="ignore"):
        u, _ = _hartley_b(p1)
        v, _ = _hartley_b(p2)
    A = np.stack([v[:, 0] * u[:, 0], v[:, 0] * u[:, 1], v[:, 0], v[:, 1] * u[:, 0], v[:, 1] * u[:, 1], v[:, 1], u[:, 0], u[:, 1], np.ones(7)], 1)
    if not np.all(np.isfinite(A)):
        return None
    _, sv, Vt = np.linalg.svd(A, full_matrices=True)
    F1, F2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    xs = np.array([-1.0, 0.0, 1.0, 2.0])
    dets = np.array([np.linalg.det(x * F1 + (1.0 - x) * F2) for x in xs])
    coef = np.linalg.solve(np.vander(xs, 4), dets)            # highest power first
    roots = np.roots(coef)
    real = np.sort(roots[np.abs(roots.imag) == 0.0].real)
    models = []
    for x in real:
        Fn = x * F1 + (1.0 - x) * F2
        models.append(Fn / np.linalg.norm(Fn))
    return dict(roots=roots, real=real, models=models, A=A, sv=sv, coef=coef)


def residuals_normalised(Fn, A):
    """(max |x2' F x1| over the seven rows of the normalised system, |det F|) of a normalised-frame model scaled to unit norm"""
    Fn = np.asarray(Fn, np.float64).reshape(3, 3)
    Fn = Fn / np.linalg.norm(Fn)
    return float(np.max(np.abs(A @ Fn.reshape(9)))), float(abs(np.linalg.det(Fn)))
