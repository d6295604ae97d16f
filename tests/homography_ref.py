"""References for the homography model (esfm.h "Homography RANSAC"; a helper, not a test module).  Two routes that share no code:

Route (a), the RESTATEMENT: easysfm_amd/csrc/homography_core.hpp and ransac_host.hpp's 4-point sampler, operation by operation in
the order the header comment states, on plain Python floats (IEEE doubles; math.sqrt is correctly rounded).  The host build, the
kernels and this route agree to the bit.  The float scoring runs on numpy float32: every numpy elementwise operation is one correctly
rounded float operation (nothing is fused), so the array form `transfer_errors` equals the scalar form `transfer_error_scalar`
entry by entry -- tests/test_homography_cpu.py checks that -- and the RANSAC loop uses the array form for speed.

Route (b), an INDEPENDENT route: the same Hartley normalisation written with numpy reductions, numpy.linalg.svd of the 2n x 9 system,
last right singular vector.  It agrees with (a) only as far as the problem's conditioning allows."""
import math

import numpy as np

SQRT2 = 1.4142135623730951
DBL_EPSILON = 2.220446049250313e-16
DBL_MAX = 1.7976931348623157e308
FLT_EPSILON = 1.1920928955078125e-07
JACOBI_SWEEPS = 30
JACOBI_OFF = 4.9303806576313238e-30
MAX_ITERS = 2000
SUBSET_ATTEMPTS = 1000
LANES = 256


# ---- route (a) -------------------------------------------------------------------------------------------------------------
def _div(a, b):
    """IEEE division of doubles (Python raises on a zero divisor)"""
    return float(np.float64(a) / np.float64(b))


def _denormalise(h, t1, t2):
    mx1, my1, s1 = t1
    mx2, my2, s2 = t2
    M = [0.0] * 9
    for r in range(3):
        m0 = h[3 * r] * s1
        m1 = h[3 * r + 1] * s1
        M[3 * r] = m0; M[3 * r + 1] = m1; M[3 * r + 2] = (h[3 * r + 2] - m0 * mx1) - m1 * my1
    H = [0.0] * 9
    for c in range(3):
        H[c] = _div(M[c], s2) + mx2 * M[6 + c]
        H[3 + c] = _div(M[3 + c], s2) + my2 * M[6 + c]
        H[6 + c] = M[6 + c]
    big = 0.0
    finite = True
    for i in range(9):
        a = abs(H[i])
        finite = finite and (a <= DBL_MAX)
        big = a if a > big else big
    if not finite or abs(H[8]) <= DBL_EPSILON * big:
        return None
    h8 = H[8]
    return [_div(v, h8) for v in H]


def _dlt_rows(t1, t2, x, y, X, Y):
    u = (x - t1[0]) * t1[2]; v = (y - t1[1]) * t1[2]; p = (X - t2[0]) * t2[2]; q = (Y - t2[1]) * t2[2]
    return ([-u, -v, -1.0, 0.0, 0.0, 0.0, p * u, p * v, p], [0.0, 0.0, 0.0, -u, -v, -1.0, q * u, q * v, q])


def _dist(mx, my, x, y):
    dx = x - mx; dy = y - my
    return math.sqrt(dx * dx + dy * dy)


def with_silent_numpy(fn):
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    return wrapped


@with_silent_numpy
def minimal_solve(p1, p2):
    """homography_from_4: p1, p2 [4][2] pixels (floats) -> (H as a list of 9 floats, True) or ([0.0] * 9, False)"""
    p1 = [[float(v) for v in r] for r in p1]; p2 = [[float(v) for v in r] for r in p2]
    sx = sy = sX = sY = 0.0
    for k in range(4):
        sx += p1[k][0]; sy += p1[k][1]; sX += p2[k][0]; sY += p2[k][1]
    mx1, my1, mx2, my2 = sx / 4.0, sy / 4.0, sX / 4.0, sY / 4.0
    d1 = d2 = 0.0
    for k in range(4):
        d1 += _dist(mx1, my1, p1[k][0], p1[k][1]); d2 += _dist(mx2, my2, p2[k][0], p2[k][1])
    t1 = (mx1, my1, _div(SQRT2, d1 / 4.0)); t2 = (mx2, my2, _div(SQRT2, d2 / 4.0))
    a = []
    for k in range(4):
        r0, r1 = _dlt_rows(t1, t2, p1[k][0], p1[k][1], p2[k][0], p2[k][1])
        a.append(r0); a.append(r1)
    beta = [0.0] * 8
    for j in range(8):
        aj = a[j]
        s = 0.0
        for r in range(j, 9):
            s += aj[r] * aj[r]
        nrm = math.sqrt(s)
        x0 = aj[j]
        v0 = x0 - (-nrm if x0 >= 0.0 else nrm)
        aj[j] = v0
        vtv = v0 * v0
        for r in range(j + 1, 9):
            vtv += aj[r] * aj[r]
        bj = _div(2.0, vtv) if vtv > 0.0 else 0.0
        beta[j] = bj
        for c in range(j + 1, 8):
            ac = a[c]
            d = 0.0
            for r in range(j, 9):
                d += aj[r] * ac[r]
            f = bj * d
            for r in range(j, 9):
                ac[r] -= f * aj[r]
    h = [0.0] * 8 + [1.0]
    for j in range(7, -1, -1):
        aj = a[j]
        d = 0.0
        for r in range(j, 9):
            d += aj[r] * h[r]
        f = beta[j] * d
        for r in range(j, 9):
            h[r] -= f * aj[r]
    H = _denormalise(h, t1, t2)
    return (H, True) if H is not None else ([0.0] * 9, False)


def _jacobi_cs(th):
    ath = abs(th)
    if 134217728.0 <= ath <= 2.0 ** 500:
        return 1.0, (1.0 if th >= 0.0 else -1.0) / (ath + ath)
    t = (1.0 if th >= 0.0 else -1.0) / (ath + math.sqrt(1.0 + th * th))
    c = 1.0 / math.sqrt(1.0 + t * t)
    return c, t * c


def jacobi_sym(A, N):
    """epnp_core.hpp's jacobi_sym<N> on the flat list A (in place) -> V (flat list)"""
    V = [1.0 if i == j else 0.0 for i in range(N) for j in range(N)]
    for _ in range(JACOBI_SWEEPS):
        off = diag = 0.0
        for i in range(N):
            diag += A[i * N + i] * A[i * N + i]
            for j in range(i + 1, N):
                off += A[i * N + j] * A[i * N + j]
        if off <= JACOBI_OFF * diag or off == 0.0:
            break
        for p in range(N - 1):
            for q in range(p + 1, N):
                apq = A[p * N + q]
                if apq == 0.0:
                    continue
                th = (A[q * N + q] - A[p * N + p]) / (2.0 * apq)
                c, s = _jacobi_cs(th)
                for r in range(N):
                    x, y = A[r * N + p], A[r * N + q]
                    A[r * N + p] = c * x - s * y; A[r * N + q] = s * x + c * y
                for r in range(N):
                    x, y = A[p * N + r], A[q * N + r]
                    A[p * N + r] = c * x - s * y; A[q * N + r] = s * x + c * y
                for r in range(N):
                    x, y = V[r * N + p], V[r * N + q]
                    V[r * N + p] = c * x - s * y; V[r * N + q] = s * x + c * y
    return V


def _tree(part):
    part = list(part)
    stride = LANES // 2
    while stride > 0:
        for l in range(stride):
            part[l] += part[l + stride]
        stride >>= 1
    return part[0]


@with_silent_numpy
def refit(pts1, pts2, mask=None):
    """homography_refit_host / homography_refit_kernel: 256 lanes, lane l the points l, l + 256, .. whose mask is set, ascending;
    halving tree; Jacobi eigenvector -> (H list of 9, True) or ([0.0] * 9, False)"""
    a = [[float(v) for v in r] for r in np.asarray(pts1, np.float32).reshape(-1, 2)]
    b = [[float(v) for v in r] for r in np.asarray(pts2, np.float32).reshape(-1, 2)]
    n = len(a)
    keep = [True] * n if mask is None else [bool(v) for v in mask]
    cnt = sum(keep)
    if cnt < 4:
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
            r0, r1 = _dlt_rows(t1, t2, a[i][0], a[i][1], b[i][0], b[i][1])
            e = 0
            for p in range(9):
                for q in range(p, 9):
                    g[e] += r0[p] * r0[q] + r1[p] * r1[q]
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
    H = _denormalise([V[9 * r + best] for r in range(9)], t1, t2)
    return (H, True) if H is not None else ([0.0] * 9, False)


def transfer_error_scalar(H, x, y, X, Y):
    """the float forward transfer error of ONE correspondence through np.float32 scalars"""
    f = np.float32
    Hf = [f(v) for v in H]
    x, y, X, Y = f(x), f(y), f(X), f(Y)
    with np.errstate(all="ignore"):
        ww = f(1.0) / (Hf[6] * x + Hf[7] * y + f(1.0))
        dx = (Hf[0] * x + Hf[1] * y + Hf[2]) * ww - X
        dy = (Hf[3] * x + Hf[4] * y + Hf[5]) * ww - Y
        return dx * dx + dy * dy


def transfer_errors(H, pts1, pts2):
    """the same on float32 arrays: one correctly rounded float operation per numpy call, in the scalar form's order"""
    Hf = np.asarray(H, np.float64).reshape(9).astype(np.float32)
    a = np.asarray(pts1, np.float32).reshape(-1, 2); b = np.asarray(pts2, np.float32).reshape(-1, 2)
    x, y, X, Y = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    with np.errstate(all="ignore"):
        ww = np.float32(1.0) / (Hf[6] * x + Hf[7] * y + np.float32(1.0))
        dx = (Hf[0] * x + Hf[1] * y + Hf[2]) * ww - X
        dy = (Hf[3] * x + Hf[4] * y + Hf[5]) * ww - Y
        err = dx * dx + dy * dy
    assert err.dtype == np.float32
    return err


def inlier_mask(H, pts1, pts2, threshold):
    with np.errstate(all="ignore"):
        return transfer_errors(H, pts1, pts2) <= np.float32(float(threshold) * float(threshold))


class CvRng:
    """cv::RNG((uint64)-1)"""

    def __init__(self):
        self.state = 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        return a if a == b else self.next() % (b - a) + a


_TRIPLES = ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3))


def _cross(p, a, b, c):
    dx1 = p[b][0] - p[a][0]; dy1 = p[b][1] - p[a][1]; dx2 = p[c][0] - p[a][0]; dy2 = p[c][1] - p[a][1]
    return dx1 * dy2 - dy1 * dx2, abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)


def check_subset(p1, p2, idx):
    """ransac_host.hpp check_subset4 on lists of (x, y) Python floats (the float32 coordinates, widened)"""
    for p in (p1, p2):
        for t in _TRIPLES:
            c, s = _cross(p, idx[t[0]], idx[t[1]], idx[t[2]])
            if abs(c) <= FLT_EPSILON * s:
                return False
    negative = 0
    for t in _TRIPLES:
        if _cross(p1, idx[t[0]], idx[t[1]], idx[t[2]])[0] * _cross(p2, idx[t[0]], idx[t[1]], idx[t[2]])[0] < 0.0:
            negative += 1
    return negative in (0, 4)


def _as_lists(pts):
    return [[float(v) for v in r] for r in np.asarray(pts, np.float32).reshape(-1, 2)]


def draw_subset(rng, count, p1, p2, stats=None):
    """-> four indices, or None after SUBSET_ATTEMPTS rejected subsets; stats["redraws"] counts the rejected ones"""
    for _ in range(SUBSET_ATTEMPTS):
        idx = []
        while len(idx) < 4:
            v = rng.uniform(0, count)
            if v not in idx:
                idx.append(v)
        if check_subset(p1, p2, idx):
            return idx
        if stats is not None:
            stats["redraws"] = stats.get("redraws", 0) + 1
    return None


def sample_stream(pts1, pts2, n_samples):
    p1, p2 = _as_lists(pts1), _as_lists(pts2)
    rng = CvRng()
    stats = {"redraws": 0}
    out = []
    for _ in range(n_samples):
        idx = draw_subset(rng, len(p1), p1, p2, stats)
        assert idx is not None
        out.append(idx)
    return np.array(out, np.int32).reshape(-1, 4), stats["redraws"]


def update_num_iters(p, ep, model_points, max_iters):
    p = min(max(p, 0.0), 1.0); ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, 2.2250738585072014e-308)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < 2.2250738585072014e-308:
        return 0
    num = math.log(num); denom = math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


def find_homography(pts1, pts2, threshold, confidence=0.995):
    """The whole rule of esfm_find_homography -> (H [3,3] or None, mask [n] bool, iterations, H of the RANSAC winner before the re-fit).
    Raises ValueError for n < 4 (the library's ESFM_ERR_UNSUPPORTED)."""
    a32 = np.asarray(pts1, np.float32).reshape(-1, 2); b32 = np.asarray(pts2, np.float32).reshape(-1, 2)
    n = len(a32)
    if n < 4:
        raise ValueError("n < 4")
    p1, p2 = _as_lists(a32), _as_lists(b32)
    if n == 4:
        H, ok = minimal_solve(p1, p2)
        if not ok:
            return None, np.zeros(n, bool), 0, None
        return np.array(H).reshape(3, 3), np.ones(n, bool), 0, np.array(H).reshape(3, 3)
    rng = CvRng()
    niters, max_good, it, best = MAX_ITERS, 0, 0, None
    while it < niters:
        idx = draw_subset(rng, n, p1, p2)
        if idx is None:
            break
        H, ok = minimal_solve([p1[i] for i in idx], [p2[i] for i in idx])
        if ok:
            good = int(np.count_nonzero(inlier_mask(H, a32, b32, threshold)))
            if good > max(max_good, 3):
                best, max_good = H, good
                niters = update_num_iters(confidence, (n - good) / n, 4, niters)
        it += 1
    if best is None:
        return None, np.zeros(n, bool), it, None
    mask = inlier_mask(best, a32, b32, threshold)
    Hr, ok = refit(a32, b32, mask)
    return np.array(Hr if ok else best).reshape(3, 3), mask, it, np.array(best).reshape(3, 3)


# ---- route (b) -------------------------------------------------------------------------------------------------------------
def _hartley_b(p):
    p = np.asarray(p, np.float64)
    c = p.mean(axis=0)
    s = np.sqrt(2.0) / np.linalg.norm(p - c, axis=1).mean()
    T = np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])
    return (p - c) * s, T


def svd_system(p1, p2):
    """the normalised 2n x 9 DLT matrix and the two normalising transforms"""
    u, T1 = _hartley_b(p1)
    v, T2 = _hartley_b(p2)
    n = len(u)
    A = np.zeros((2 * n, 9))
    A[0::2, 0:2] = -u; A[0::2, 2] = -1.0; A[0::2, 6:8] = v[:, :1] * u; A[0::2, 8] = v[:, 0]
    A[1::2, 3:5] = -u; A[1::2, 5] = -1.0; A[1::2, 6:8] = v[:, 1:] * u; A[1::2, 8] = v[:, 1]
    return A, T1, T2


def svd_solve(p1, p2):
    """-> (H [3,3] with H[2,2] = 1, sigma_8 / sigma_1 of the normalised system); (None, 0.0) when the system is not finite"""
    with np.errstate(all="ignore"):
        A, T1, T2 = svd_system(p1, p2)
    if not np.all(np.isfinite(A)):
        return None, 0.0
    _, sv, Vt = np.linalg.svd(A, full_matrices=True)
    H = np.linalg.inv(T2) @ Vt[-1].reshape(3, 3) @ T1
    return H / H[2, 2], (sv[7] / sv[0] if len(sv) > 7 else 0.0)


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------------------------
def _project(K, R, t, X):
    Xc = X @ R.T + t
    return np.stack([Xc[:, 0] / Xc[:, 2] * K[0, 0] + K[0, 2], Xc[:, 1] / Xc[:, 2] * K[1, 1] + K[1, 2]], 1)


def _rot_y(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def scene_pairs(noise=0.2, seed=11):
    """Correspondence sets from synth.sfm_scene()'s cameras and K (float32 pixels, `noise` px of Gaussian noise per coordinate):
    "general" -- (camera 3, camera 2) and (camera 5, camera 1) on the scene as it is; "planar" -- the same camera pairs with the
    points moved onto the plane z = 0.3 x + 0.1 y; "rotation" -- camera 0 against itself rotated 0.1 rad about its vertical axis.
    -> dict name -> list of (pts1, pts2, exact1, exact2, H_true or None)"""
    from easysfm_amd import synth
    _, K, poses, pts = synth.sfm_scene()
    K = K.astype(np.float64)
    rng = np.random.default_rng(seed)
    flat = pts.copy(); flat[:, 2] = 0.3 * flat[:, 0] + 0.1 * flat[:, 1]

    def pair(X, T1, T2, H_true):
        a = _project(K, T1[:3, :3], T1[:3, 3], X); b = _project(K, T2[:3, :3], T2[:3, 3], X)
        ok = (X @ T1[:3, :3].T + T1[:3, 3])[:, 2] > 1
        ok &= (X @ T2[:3, :3].T + T2[:3, 3])[:, 2] > 1
        for uv in (a, b):
            ok &= (uv[:, 0] > 5) & (uv[:, 0] < 763) & (uv[:, 1] > 5) & (uv[:, 1] < 507)
        a, b = a[ok], b[ok]
        return ((a + noise * rng.standard_normal(a.shape)).astype(np.float32), (b + noise * rng.standard_normal(b.shape)).astype(np.float32), a, b, H_true)

    def plane_h(T1, T2):
        # X on the plane n.X = 0 with n = (0.3, 0.1, -1): in camera 1, X1 = R1 X + t1, so n'R1'(X1 - t1) = 0, i.e. m.X1 = d
        n = np.array([0.3, 0.1, -1.0])
        R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
        m = R1 @ n; d = m @ t1
        R = R2 @ R1.T; t = t2 - R @ t1
        H = K @ (R + np.outer(t, m) / d) @ np.linalg.inv(K)
        return H / H[2, 2]

    out = {"general": [], "planar": [], "rotation": []}
    for i, j in ((3, 2), (5, 1)):
        out["general"].append(pair(pts, poses[i], poses[j], None))
        out["planar"].append(pair(flat, poses[i], poses[j], plane_h(poses[i], poses[j])))
    T2 = poses[0].copy(); Rr = _rot_y(0.1); T2[:3, :3] = Rr @ poses[0][:3, :3]; T2[:3, 3] = Rr @ poses[0][:3, 3]
    Hr = K @ Rr @ np.linalg.inv(K)
    out["rotation"].append(pair(pts, poses[0], T2, Hr / Hr[2, 2]))
    return out, K


def correspondence_sets(n=200, seed=5):
    """three sets of n correspondences: a plane, a rotation, general relief with 30 % random outliers"""
    pairs, _ = scene_pairs(noise=0.3, seed=seed)
    rng = np.random.default_rng(seed + 1)
    sets = {}
    for name, src in (("plane", pairs["planar"][0]), ("rotation", pairs["rotation"][0]), ("general", pairs["general"][0])):
        a, b = src[0][:n].copy(), src[1][:n].copy()
        assert len(a) == n
        if name == "general":
            bad = rng.permutation(n)[:int(0.3 * n)]
            b[bad] = np.stack([rng.uniform(5, 763, len(bad)), rng.uniform(5, 507, len(bad))], 1).astype(np.float32)
        sets[name] = (a, b)
    return sets


def degenerate_samples():
    """hand-made samples [k, 4, 2] x 2: four identical points; three collinear points (handed in directly, past the subset check);
    a correspondence mapped to infinity; coordinates of 1e6"""
    sq = np.array([[0.0, 0.0], [100.0, 0.0], [100.0, 100.0], [0.0, 100.0]])
    same = np.tile([[37.5, 91.25]], (4, 1))
    line = np.array([[10.0, 10.0], [20.0, 20.0], [30.0, 30.0], [15.0, 80.0]])
    far = sq.copy(); far[2] = [np.inf, 50.0]
    big = sq * 1e4 + 1e6
    q1 = np.stack([same, line, sq, sq, big, sq])
    q2 = np.stack([same, line + [3.0, -2.0], line, far, big * 1.001 + 7.0, same])
    return q1, q2


def solver_samples(total=4096):
    """`total` samples drawn by the sampler from the three correspondence sets, then the degenerate ones -> q1, q2 [n, 4, 2] float64"""
    q1, q2 = [], []
    sets = correspondence_sets()
    per = [total // 3 + (1 if k < total % 3 else 0) for k in range(3)]
    for (name, (a, b)), cnt in zip(sets.items(), per):
        idx, _ = sample_stream(a, b, cnt)
        q1.append(a[idx].astype(np.float64)); q2.append(b[idx].astype(np.float64))
    d1, d2 = degenerate_samples()
    return np.concatenate(q1 + [d1]), np.concatenate(q2 + [d2])


def ransac_case(n, outlier_frac=0.2, seed=0, noise=0.3):
    """n correspondences under one homography with `noise` px noise; a fraction replaced by random points -> float32 pts1, pts2"""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    Ht = np.array([[1.08, 0.04, 25.0], [-0.03, 0.96, -14.0], [9e-5, -4e-5, 1.0]])
    a = np.stack([rng.uniform(5, 763, n), rng.uniform(5, 507, n)], 1)
    h = np.c_[a, np.ones(n)] @ Ht.T
    b = h[:, :2] / h[:, 2:] + noise * rng.standard_normal((n, 2))
    bad = rng.permutation(n)[:int(round(outlier_frac * n))]
    b[bad] = np.stack([rng.uniform(5, 763, len(bad)), rng.uniform(5, 507, len(bad))], 1)
    return a.astype(np.float32), b.astype(np.float32)
