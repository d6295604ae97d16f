"""Track triangulation restated in plain Python floats (include/esfm.h "Track triangulation"; easysfm_amd/csrc/track_core.hpp is
the product's statement of the same rules).  Every expression is written in the header's order, so the host build, the kernels and
this file agree to the bit.  Scalar loops, no np.linalg.  Also: the plain all-observation refit the robustness test compares
against, and the case builders on top of synth.ba_scene."""
import math

import numpy as np

from easysfm_amd import synth

KEPT, TOO_FEW, NO_HYPOTHESIS, FEW_INLIERS, SMALL_ANGLE, NON_FINITE = range(6)
STAGE_CAP = 256          # ESFM_TRACK_STAGE_CAP
DET_EPS = 1e-12
INF = float("inf")
NAN = float("nan")


class Options:
    def __init__(self, max_reproj_error_px=4.0, min_angle_deg=1.5, min_views=2, max_hypotheses=64, refine_iterations=5):
        self.thr2 = float(max_reproj_error_px) * float(max_reproj_error_px)
        self.cos_min_angle = math.cos(float(min_angle_deg) * (3.14159265358979323846 / 180.0))
        self.min_views, self.max_hypotheses, self.refine_iterations = int(min_views), int(max_hypotheses), int(refine_iterations)
        self.kw = dict(max_reproj_error_px=max_reproj_error_px, min_angle_deg=min_angle_deg, min_views=min_views,
                       max_hypotheses=max_hypotheses, refine_iterations=refine_iterations)


def div(a, b):
    """IEEE division (Python raises on a zero divisor)"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def finite(x):
    return abs(x) <= 1.7976931348623157e308


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def make_obs(Rt, K, u, v):
    """(C, d) of one observation"""
    fx, cx, fy, cy = K
    x = div(u - cx, fx); y = div(v - cy, fy)
    C = [-((Rt[j] * Rt[3] + Rt[4 + j] * Rt[7]) + Rt[8 + j] * Rt[11]) for j in range(3)]
    d = [(Rt[j] * x + Rt[4 + j] * y) + Rt[8 + j] for j in range(3)]
    return C, d


def project(Rt, K, u, v, X, thr2):
    """(xn, yn, iz, ru, rv, err2, inlier)"""
    p0 = ((Rt[0] * X[0] + Rt[1] * X[1]) + Rt[2] * X[2]) + Rt[3]
    p1 = ((Rt[4] * X[0] + Rt[5] * X[1]) + Rt[6] * X[2]) + Rt[7]
    p2 = ((Rt[8] * X[0] + Rt[9] * X[1]) + Rt[10] * X[2]) + Rt[11]
    iz = div(1.0, p2); xn = p0 * iz; yn = p1 * iz
    ru = (K[0] * xn + K[1]) - u
    rv = (K[2] * yn + K[3]) - v
    err2 = ru * ru + rv * rv
    return xn, yn, iz, ru, rv, err2, (p2 > 0.0 and err2 <= thr2)


def pair_from_number(q, n):
    a = 0
    while (a + 1) * (2 * n - (a + 1) - 1) // 2 <= q:
        a += 1
    return a, q - a * (2 * n - a - 1) // 2 + a + 1


def hypothesis_pairs(n, max_hypotheses):
    """the pair of every hypothesis, in hypothesis order"""
    P = n * (n - 1) // 2
    if P <= max_hypotheses:
        return [(a, b) for a in range(n) for b in range(a + 1, n)]
    return [pair_from_number(h * P // max_hypotheses, n) for h in range(max_hypotheses)]


def hypothesis_point(Ca, da, Cb, db):
    w = [Ca[j] - Cb[j] for j in range(3)]
    aa = dot3(da, da); bb = dot3(db, db); ab = dot3(da, db); dw = dot3(da, w); ew = dot3(db, w)
    det = aa * bb - ab * ab
    if not det > DET_EPS * (aa * bb):
        return None
    s = (ab * ew - bb * dw) / det; t = (aa * ew - ab * dw) / det
    if not s > 0.0 or not t > 0.0:
        return None
    return [0.5 * ((Ca[j] + s * da[j]) + (Cb[j] + t * db[j])) for j in range(3)]


def score(obs, X, thr2):
    """(inliers, cost, flags) over the observations (Rt, K, u, v, C, d) in order"""
    inl = 0; cost = 0.0; flags = []
    for Rt, K, u, v, _, _ in obs:
        p = project(Rt, K, u, v, X, thr2)
        flags.append(p[6])
        if p[6]:
            inl += 1; cost += p[5]
        else:
            cost += thr2
    return inl, cost, flags


def gn_step(obs, flags, X, thr2):
    """one Gauss-Newton step on the flagged observations: the new X, or None when the refit ends"""
    A00 = A01 = A02 = A11 = A12 = A22 = g0 = g1 = g2 = 0.0
    for (Rt, K, u, v, _, _), f in zip(obs, flags):
        if not f:
            continue
        xn, yn, iz, ru, rv, _, _ = project(Rt, K, u, v, X, thr2)
        a = K[0] * iz; b = K[2] * iz
        u0 = a * (Rt[0] - xn * Rt[8]); u1 = a * (Rt[1] - xn * Rt[9]); u2 = a * (Rt[2] - xn * Rt[10])
        v0 = b * (Rt[4] - yn * Rt[8]); v1 = b * (Rt[5] - yn * Rt[9]); v2 = b * (Rt[6] - yn * Rt[10])
        A00 += u0 * u0 + v0 * v0; A01 += u0 * u1 + v0 * v1; A02 += u0 * u2 + v0 * v2
        A11 += u1 * u1 + v1 * v1; A12 += u1 * u2 + v1 * v2; A22 += u2 * u2 + v2 * v2
        g0 += u0 * ru + v0 * rv; g1 += u1 * ru + v1 * rv; g2 += u2 * ru + v2 * rv
    d0 = A00
    if not d0 > 0.0:
        return None
    l10 = A01 / d0; l20 = A02 / d0
    d1 = A11 - l10 * A01
    if not d1 > 0.0:
        return None
    m = A12 - l20 * A01
    l21 = m / d1
    d2 = (A22 - l20 * A02) - l21 * m
    if not d2 > 0.0:
        return None
    y0 = -g0; y1 = -g1 - l10 * y0; y2 = (-g2 - l20 * y0) - l21 * y1
    z0 = y0 / d0; z1 = y1 / d1; z2 = y2 / d2
    e2 = z2; e1 = z1 - l21 * e2; e0 = (z0 - l10 * e1) - l20 * e2
    n = [X[0] + e0, X[1] + e1, X[2] + e2]
    if not (finite(n[0]) and finite(n[1]) and finite(n[2])):
        return None
    return n


def refit(obs, flags, X, o):
    for _ in range(o.refine_iterations):
        n = gn_step(obs, flags, X, o.thr2)
        if n is None:
            break
        X = n
    return X


def judge(obs, X, o):
    """inlier flags, squared errors, (status, n_inliers, min_cos, mse) of the final point X"""
    flags, err2, e = [], [], []
    for Rt, K, u, v, C, _ in obs:
        p = project(Rt, K, u, v, X, o.thr2)
        w = [C[j] - X[j] for j in range(3)]
        ln = math.sqrt(dot3(w, w))
        e.append([div(w[j], ln) for j in range(3)])
        flags.append(p[6]); err2.append(p[5])
    n_inl = sum(flags)
    m = 1.0
    for i in range(len(obs)):
        if not flags[i]:
            continue
        for j in range(i + 1, len(obs)):
            if flags[j]:
                c = dot3(e[i], e[j])
                if c < m:
                    m = c
    s = 0.0
    for k in range(len(obs)):
        if flags[k]:
            s += err2[k]
    mse = s / float(n_inl) if n_inl > 0 else 0.0
    m = m + 0.0
    status = FEW_INLIERS if n_inl < o.min_views else SMALL_ANGLE if m > o.cos_min_angle else KEPT
    return flags, err2, (status, n_inl, m, mse)


def solve_track(obs, o, Xgiven=None):
    """obs: the track's (Rt, K, u, v) in input order, python floats.  Returns (X or None, flags, err2, (status, n_inliers, min_cos,
    mse)); X is None unless the status is KEPT (evaluate: always None)."""
    n = len(obs)
    blank = (None, [False] * n, [INF] * n)
    if n < 2:
        return blank + ((TOO_FEW, 0, 1.0, 0.0),)
    ok = all(finite(x) for Rt, K, u, v in obs for x in (u, v, *K, *Rt))
    if Xgiven is not None:
        ok = ok and all(finite(x) for x in Xgiven)
    if not ok:
        return blank + ((NON_FINITE, 0, 1.0, 0.0),)
    obs = [(Rt, K, u, v) + make_obs(Rt, K, u, v) for Rt, K, u, v in obs]
    if Xgiven is not None:
        flags, err2, stats = judge(obs, list(Xgiven), o)
        return None, flags, err2, stats
    best = None                                              # (inliers, cost, h): more, then lower, then lower
    for h, (a, b) in enumerate(hypothesis_pairs(n, o.max_hypotheses)):
        X = hypothesis_point(obs[a][4], obs[a][5], obs[b][4], obs[b][5])
        if X is None:
            continue
        inl, cost, flags = score(obs, X, o.thr2)
        if best is None or inl > best[0] or (inl == best[0] and cost < best[1]):
            best = (inl, cost, h, X, flags)
    if best is None:
        return blank + ((NO_HYPOTHESIS, 0, 1.0, 0.0),)
    Xh = best[3]
    X = refit(obs, best[4], Xh, o)
    if score(obs, X, o.thr2)[0] < best[0]:
        X = Xh
    flags, err2, stats = judge(obs, X, o)
    return (X if stats[0] == KEPT else None), flags, err2, stats


def err2_out(e):
    return np.float32(e) if e == e else np.float32(INF)


class Result:
    pass


def run(cam_idx, pt_idx, uv, K4, Rt, n_pt, o, xyz_in=None, evaluate=False):
    """esfm_track_triangulate / esfm_track_evaluate over arrays: the outputs as numpy arrays (xyz None for evaluate)"""
    Rt_l = [[float(x) for x in r] for r in np.asarray(Rt, np.float64).reshape(-1, 12)]
    K_l = [[float(x) for x in r] for r in np.asarray(K4, np.float32).reshape(-1, 4)]
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    tracks = [[] for _ in range(n_pt)]
    for i, p in enumerate(np.asarray(pt_idx)):
        tracks[int(p)].append(i)
    r = Result()
    r.xyz = None if evaluate else np.zeros((n_pt, 3), np.float64)
    r.obs_inlier = np.zeros(len(uv), bool); r.obs_err2 = np.zeros(len(uv), np.float32)
    r.status = np.zeros(n_pt, np.int32); r.n_inliers = np.zeros(n_pt, np.int32)
    r.min_cos = np.zeros(n_pt, np.float64); r.mse = np.zeros(n_pt, np.float64)
    with np.errstate(all="ignore"):
        for p, idx in enumerate(tracks):
            obs = [(Rt_l[int(cam_idx[i])], K_l[int(cam_idx[i])], float(uv[i, 0]), float(uv[i, 1])) for i in idx]
            Xg = [float(x) for x in xyz_in[p]] if evaluate else None
            X, flags, err2, stats = solve_track(obs, o, Xg)
            for k, i in enumerate(idx):
                r.obs_inlier[i] = flags[k]; r.obs_err2[i] = err2_out(err2[k])
            r.status[p], r.n_inliers[p], r.min_cos[p], r.mse[p] = stats
            if not evaluate:
                r.xyz[p] = X if X is not None else (xyz_in[p] if xyz_in is not None else 0.0)
    return r


def all_observation_refit(cam_idx, pt_idx, uv, K4, Rt, n_pt, o):
    """The baseline of the robustness test: the same Gauss-Newton refit from the first valid hypothesis, on EVERY observation, no
    scoring.  Returns xyz [n_pt, 3] (NaN rows where a track has no valid hypothesis)."""
    Rt_l = [[float(x) for x in r] for r in np.asarray(Rt, np.float64).reshape(-1, 12)]
    K_l = [[float(x) for x in r] for r in np.asarray(K4, np.float32).reshape(-1, 4)]
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    tracks = [[] for _ in range(n_pt)]
    for i, p in enumerate(np.asarray(pt_idx)):
        tracks[int(p)].append(i)
    out = np.full((n_pt, 3), np.nan)
    for p, idx in enumerate(tracks):
        obs = [(Rt_l[int(cam_idx[i])], K_l[int(cam_idx[i])], float(uv[i, 0]), float(uv[i, 1])) for i in idx]
        obs = [t + make_obs(*t) for t in obs]
        for a, b in hypothesis_pairs(len(obs), o.max_hypotheses) if len(obs) >= 2 else []:
            X = hypothesis_point(obs[a][4], obs[a][5], obs[b][4], obs[b][5])
            if X is not None:
                out[p] = refit(obs, [True] * len(obs), X, o)
                break
    return out


# ---- case builders --------------------------------------------------------------------------------------------------------
def gt_cameras(sc):
    """[n_cam, 3, 4] world -> camera from the scene's ground-truth cameras"""
    Rt = np.zeros((sc.n_cam, 3, 4))
    for c in range(sc.n_cam):
        Rt[c, :, :3] = synth.aa_to_R(sc.cams_gt[c, :3]); Rt[c, :, 3] = sc.cams_gt[c, 3:]
    return Rt


def scene(n_cam, n_pt, obs_per_pt, seed=4000, uv_noise=0.5, outlier_frac=0.1, camera_major=True):
    """(scene, Rt, injected): injected marks the observations whose uv differs from the same seed's outlier-free scene (the generator
    draws the pixel noise before it chooses the outliers, so the two scenes agree elsewhere)"""
    sc = synth.ba_scene(n_cam, n_pt, obs_per_pt, seed=seed, uv_noise=uv_noise, outlier_frac=outlier_frac, camera_major=camera_major)
    clean = synth.ba_scene(n_cam, n_pt, obs_per_pt, seed=seed, uv_noise=uv_noise, outlier_frac=0.0, camera_major=camera_major)
    return sc, gt_cameras(sc), np.any(sc.uv != clean.uv, axis=1), clean


def ring_case(lengths, n_cam=160, seed=7, noise=0.4, outliers=True, empty=()):
    """One track per entry of `lengths` (0 = a point nobody observes), observations interleaved across the tracks so that no track
    is contiguous in the input; every fifth observation of a track of five or more is displaced by tens of pixels.  Cameras on a
    ring of `n_cam`; a track longer than the ring revisits cameras with fresh noise."""
    rng = np.random.default_rng(seed)
    sc = synth.ba_scene(n_cam, len(lengths), 1, seed=seed, uv_noise=0.0, outlier_frac=0.0)
    Rt = gt_cameras(sc)
    K = np.array(synth.FOUNTAIN_K4, np.float64)
    rows = []
    for p, n in enumerate(lengths):
        start = int(rng.integers(0, n_cam))
        for k in range(n):
            c = (start + 3 * k) % n_cam
            Xc = Rt[c, :, :3] @ sc.pts_gt[p] + Rt[c, :, 3]
            uv = np.array([K[0] * Xc[0] / Xc[2] + K[1], K[2] * Xc[1] / Xc[2] + K[3]]) + noise * rng.standard_normal(2)
            if outliers and n >= 5 and k % 5 == 4:
                uv += rng.uniform(20, 50, 2) * rng.choice([-1.0, 1.0], 2)
            rows.append((k, p, c, uv[0], uv[1]))
    rows.sort(key=lambda r: (r[0], r[1]))                    # round-robin over the tracks: each keeps its internal order
    cam_idx = np.array([r[2] for r in rows], np.int32); pt_idx = np.array([r[1] for r in rows], np.int32)
    uv = np.array([[r[3], r[4]] for r in rows], np.float32).reshape(-1, 2)
    return cam_idx, pt_idx, uv, np.tile(np.array(synth.FOUNTAIN_K4, np.float32), (n_cam, 1)), Rt, len(lengths), sc.pts_gt


EDGE_LENGTHS = [0, 1, 2, 3, 11, 12, 0, 63, 64, 65, 129, STAGE_CAP + 44, 0]   # first and last point unobserved; one track above the cap


# ---- shared by the CPU and the GPU tests ------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(got, ref, what=""):
    """every output of a call, f64 as bit patterns"""
    assert np.array_equal(got.status, ref.status), (what, got.status, ref.status)
    assert np.array_equal(got.n_inliers, ref.n_inliers), what
    assert np.array_equal(got.obs_inlier, ref.obs_inlier), what
    assert np.array_equal(np.asarray(got.obs_err2).view(np.uint32), np.asarray(ref.obs_err2).view(np.uint32)), what
    assert np.array_equal(bits(got.min_cos), bits(ref.min_cos)), what
    assert np.array_equal(bits(got.mse), bits(ref.mse)), what
    if ref.xyz is not None:
        assert np.array_equal(bits(got.xyz), bits(ref.xyz)), what


def behind_point(cams, Rt):
    """1.5 x the sum of two camera centres a quarter of the ring apart: behind both cameras, which look at the origin"""
    return 1.5 * sum(-Rt[c, :, :3].T @ Rt[c, :, 3] for c in cams)


def degenerate_case():
    """point 0: two observations from one camera; 1: a point behind both of its cameras; 2: four unrelated pixels; 3: a duplicated
    observation (two hypotheses tie in count and cost); 4: a NaN pixel; 5: a good track seen by a camera with an infinite focal
    length; 6: a good track"""
    base = ring_case([6] * 7, n_cam=12, seed=21, outliers=False)
    cam_idx, pt_idx, uv, K4, Rt, n_pt, gt = [np.array(a) if isinstance(a, np.ndarray) else a for a in base]
    K4 = np.concatenate([K4, K4[:1]]); K4[12, 0] = np.inf
    Rt = np.concatenate([Rt, Rt[:1]])
    rows = {p: np.nonzero(pt_idx == p)[0] for p in range(7)}
    keep = np.ones(len(pt_idx), bool)
    keep[rows[0][2:]] = False; cam_idx[rows[0][1]] = cam_idx[rows[0][0]]
    keep[rows[1][2:]] = False
    K = np.array(K4[0], np.float64)
    behind = behind_point(cam_idx[rows[1][:2]], Rt)
    for i in rows[1][:2]:                                           # project a point BEHIND both cameras: the rays meet at negative depth
        c = cam_idx[i]
        Xc = Rt[c, :, :3] @ behind + Rt[c, :, 3]
        assert Xc[2] < 0
        uv[i] = [K[0] * Xc[0] / Xc[2] + K[1], K[2] * Xc[1] / Xc[2] + K[3]]
    keep[rows[2][4:]] = False
    uv[rows[2][:4]] = np.random.default_rng(1).uniform(100, 1900, (4, 2))
    keep[rows[3][3:]] = False; cam_idx[rows[3][2]] = cam_idx[rows[3][1]]; uv[rows[3][2]] = uv[rows[3][1]]
    uv[rows[4][3], 1] = np.nan
    cam_idx[rows[5][2]] = 12
    return cam_idx[keep], pt_idx[keep], uv[keep], K4, Rt, n_pt, gt
