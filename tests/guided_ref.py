"""numpy restatement of epipolar-guided matching (include/esfm.h "Epipolar-guided matching") and the repeated-structure scene its
tests share.  Every expression is written as the header defines it: numpy evaluates a vectorised expression left to right, one
rounded operation per operator, without fused multiply-add, so the results are the definition's, bit for bit."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
L2, HAMMING = 0, 1


# ----------------------------------------------------------------------------- 1. admissibility
def _predicate(kq, kt, E, K4, max_epipolar_px, outer):
    kq = np.asarray(kq, np.float32).reshape(-1, 2); kt = np.asarray(kt, np.float32).reshape(-1, 2)
    E = np.asarray(E, np.float64).reshape(9)
    fx, cx, fy, cy = (np.float64(v) for v in np.asarray(K4, np.float32).reshape(4))
    qs, ts = ((slice(None), None), (None, slice(None))) if outer else ((slice(None),), (slice(None),))
    with np.errstate(all="ignore"):
        thr = np.float64(max_epipolar_px) / ((fx + fy) / 2.0)
        tsq = np.float32(thr * thr)
        x1 = ((kq[:, 0].astype(np.float64) - cx) / fx)[qs]; y1 = ((kq[:, 1].astype(np.float64) - cy) / fy)[qs]
        x2 = ((kt[:, 0].astype(np.float64) - cx) / fx)[ts]; y2 = ((kt[:, 1].astype(np.float64) - cy) / fy)[ts]
        Ex0 = E[0] * x1 + E[1] * y1 + E[2]; Ex1 = E[3] * x1 + E[4] * y1 + E[5]; Ex2 = E[6] * x1 + E[7] * y1 + E[8]
        Et0 = E[0] * x2 + E[3] * y2 + E[6]; Et1 = E[1] * x2 + E[4] * y2 + E[7]
        v = x2 * Ex0 + y2 * Ex1 + Ex2
        err = (v * v / (Ex0 * Ex0 + Ex1 * Ex1 + Et0 * Et0 + Et1 * Et1)).astype(np.float32)
        return err <= tsq


def admissible(kp_q, kp_t, E, K4, max_epipolar_px):
    """adm [nq, nt] bool: the essential-matrix RANSAC's inlier test on every (query row, train row)."""
    return _predicate(kp_q, kp_t, E, K4, max_epipolar_px, True)


def admissible_rows(kp_q, kp_t, E, K4, max_epipolar_px):
    """The predicate on matched rows: adm [n] for (kp_q[i], kp_t[i])."""
    return _predicate(kp_q, kp_t, E, K4, max_epipolar_px, False)


# ----------------------------------------------------------------------------- distances of listed (query row, train row)
def l2_rows(a, b):
    """sqrtf(esfm_ref_l2sqr(a[i], b[i])) for every i: 8 partial sums over blocks of 8, (acc[c] + acc[c + 4]) summed left to right,
    then the scalar tail -- float32 throughout."""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    n, dim = a.shape
    with np.errstate(all="ignore"):
        t = a - b
        sq = t * t
        acc = np.zeros((n, 8), np.float32)
        j = 0
        while j <= dim - 8:
            acc = acc + sq[:, j:j + 8]
            j += 8
        s = acc[:, :4] + acc[:, 4:]
        d = s[:, 0] + s[:, 1]
        d = d + s[:, 2]
        d = d + s[:, 3]
        while j < dim:
            d = d + sq[:, j]
            j += 1
        return np.sqrt(d).astype(np.float32)


def hamming_rows(a, b):
    a = np.asarray(a, np.uint8); b = np.asarray(b, np.uint8)
    return np.unpackbits(a ^ b, axis=1).sum(axis=1).astype(np.float32)


# ----------------------------------------------------------------------------- 2. guided 2-NN
def _best2(adm, own, other, metric):
    """For every row r of `adm`: the two best columns c with adm[r, c] under ascending (distance(own[r], other[c]), c)."""
    n = adm.shape[0]
    idx = np.full((n, 2), -1, np.int32); dist = np.full((n, 2), FLT_MAX, np.float32)
    r, c = np.nonzero(adm)
    if len(r):
        d = l2_rows(own[r], other[c]) if metric == L2 else hamming_rows(own[r], other[c])
        keep = d < FLT_MAX                       # FLT_MAX, +inf and NaN are never neighbours
        r, c, d = r[keep], c[keep], d[keep]
        order = np.lexsort((c, d, r))
        r, c, d = r[order], c[order], d[order]
        first = np.nonzero(np.concatenate([[True], r[1:] != r[:-1]]))[0] if len(r) else np.zeros(0, np.int64)
        idx[r[first], 0] = c[first]; dist[r[first], 0] = d[first]
        second = first + 1
        ok = (second < len(r))
        second = second[ok]
        ok2 = r[second] == r[second - 1]
        second = second[ok2]
        idx[r[second], 1] = c[second]; dist[r[second], 1] = d[second]
    return idx, dist


def knn2_guided(metric, dq, kq, dt, kt, E, K4, max_epipolar_px):
    """(idx [nq, 2], dist [nq, 2], n_adm [nq]) forward, (ridx [nt, 2], rdist [nt, 2]) reverse -- from ONE admissibility matrix."""
    dq = np.asarray(dq); dt = np.asarray(dt)
    adm = admissible(kq, kt, E, K4, max_epipolar_px)
    idx, dist = _best2(adm, dq, dt, metric)
    ridx, rdist = _best2(adm.T, dt, dq, metric)
    return idx, dist, adm.sum(axis=1).astype(np.int32), ridx, rdist


# ----------------------------------------------------------------------------- 3. filters
def ratio_ok(idx, dist, ratio):
    return (idx[:, 0] >= 0) & (idx[:, 1] >= 0) & (dist[:, 0].astype(np.float64) < np.float64(ratio) * dist[:, 1].astype(np.float64))


def filter_lists(idx, dist, ridx, rdist, ratio, cross):
    """ratio: None (use_ratio = 0) or the number; cross: bool.  Returns (queryIdx, trainIdx, distance), query-ascending."""
    nq, nt = len(idx), len(ridx)
    f = idx[:, 0]
    ok = f >= 0
    if ratio is not None:
        ok &= ratio_ok(idx, dist, ratio)
    if cross:
        fc = np.where(ok, f, 0)
        if nt:
            ok &= ridx[fc, 0] == np.arange(nq)
            if ratio is not None:
                ok &= ratio_ok(ridx, rdist, ratio)[fc]
        else:
            ok &= False
    q = np.nonzero(ok)[0]
    return q.astype(np.int32), f[q].astype(np.int32), dist[q, 0].astype(np.float32)


def match_guided(metric, dq, kq, dt, kt, E, K4, max_epipolar_px, ratio, cross):
    idx, dist, _, ridx, rdist = knn2_guided(metric, dq, kq, dt, kt, E, K4, max_epipolar_px)
    return filter_lists(idx, dist, ridx, rdist, ratio, cross)


def union(plain, guided):
    """Property (b)'s union of the plain RANSAC inliers and the guided list, (queryIdx, trainIdx, distance) each: the plain
    entries, and the guided entries of the queries the plain list does not hold, in ascending query order."""
    pq, pt, pd = (np.asarray(v) for v in plain)
    gq, gt, gd = (np.asarray(v) for v in guided)
    new = ~np.isin(gq, pq)
    q = np.concatenate([pq, gq[new]]).astype(np.int32); t = np.concatenate([pt, gt[new]]).astype(np.int32)
    d = np.concatenate([pd, gd[new]]).astype(np.float32)
    order = np.argsort(q, kind="stable")
    return q[order], t[order], d[order]


# ----------------------------------------------------------------------------- plain filters on oracle tables (CPU)
def plain_lists(oracle, dq, dt, ratio, cross):
    """The plain matcher's lists from the oracle's 2-NN tables: "ratio" (ratio, not cross), "cross" (None, cross), "ratio+cross"."""
    idx, dist = oracle.knn2_l2(dq, dt)
    ridx, rdist = oracle.knn2_l2(dt, dq)
    return filter_lists(idx, dist, ridx, rdist, ratio, cross)


# ----------------------------------------------------------------------------- the scene
SCENE_SEED = 123


def scene(seed=SCENE_SEED):
    """easysfm_amd.synth.sfm_scene(8, 900, 7000, 0.3, 150, 0.03) with the real points' descriptors re-drawn so that most of the
    structure repeats: points 0..224 keep a base vector of their own, points 225..899 share one base per group of four
    (base = 225 + (id - 225) // 4); a descriptor is its base plus N(0, 0.03^2) noise, renormalised, float32.  Clutter keeps its
    random descriptors.  Returns (frames, K [3,3], poses, points) as sfm_scene does."""
    from easysfm_amd import synth
    frames, K, poses, pts = synth.sfm_scene(8, 900, 7000, 0.3, 150, 0.03)
    rng = np.random.default_rng(np.random.PCG64(seed))
    base = rng.standard_normal((900, 64)); base /= np.linalg.norm(base, axis=1, keepdims=True)
    for f in frames:
        pid = f["point_id"]
        real = np.nonzero(pid >= 0)[0]
        ids = pid[real].astype(np.int64)
        bid = np.where(ids < 225, ids, 225 + (ids - 225) // 4)
        d = base[bid] + 0.03 * rng.standard_normal((len(real), 64))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        desc = f["descriptors"].copy()
        desc[real] = d.astype(np.float32)
        f["descriptors"] = np.ascontiguousarray(desc, np.float32)
    return frames, K, poses, pts


def k4_of(K):
    return np.array([K[0, 0], K[0, 2], K[1, 1], K[1, 2]], np.float32)


FILTERS = {"ratio": (0.5, False), "cross": (None, True), "ratio+cross": (0.5, True)}      # SURF-like rows: the reference's ratio 0.5
