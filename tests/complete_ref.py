"""Track completion restated in numpy by brute force (include/esfm.h "Track completion"; easysfm_amd/csrc/complete_core.hpp is the
product's statement of the same rules): no grid, every keypoint row of every camera is asked the predicate.  The projection is
track_ref.project's, the distances are guided_ref.l2_rows / hamming_rows; numpy evaluates a vectorised expression one rounded
operation per operator, without fused multiply-add, so the results are the definition's, bit for bit."""
import numpy as np

import guided_ref
import track_ref

FLT_MAX = np.finfo(np.float32).max
NO_CLAIM = np.uint64(0xFFFFFFFFFFFFFFFF)


class Result:
    pass


def pixel(Rt, K, X):
    """(pu, pv, front): the minuends of track_ref.project's ru, rv (u = v = 0 leaves them as they are) and p_2 > 0"""
    _, _, _, ru, rv, _, _ = track_ref.project(Rt, K, 0.0, 0.0, X, track_ref.INF)
    p2 = ((Rt[8] * X[0] + Rt[9] * X[1]) + Rt[10] * X[2]) + Rt[11]
    return ru, rv, p2 > 0.0


def run(desc, kp, kp_free, off, K4, Rt, xyz, cam_idx, pt_idx, obs_kp, search_radius_px=4.0, max_distance=np.inf, ratio=0.8, max_refs=8):
    """esfm_track_complete over arrays: kp_point, kp_dist, stats"""
    desc = np.asarray(desc)
    hamming = desc.dtype == np.uint8
    kp = np.asarray(kp, np.float32).reshape(-1, 2).astype(np.float64)
    free = np.asarray(kp_free).astype(np.uint8).reshape(-1) != 0
    off = np.asarray(off, np.int64)
    Rt_l = [[float(x) for x in r] for r in np.asarray(Rt, np.float64).reshape(-1, 12)]
    K_l = [[float(x) for x in r] for r in np.asarray(K4, np.float32).reshape(-1, 4)]
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    n_cam, n_pt, rows = len(K_l), len(xyz), len(kp)
    thr2 = np.float64(search_radius_px) * np.float64(search_radius_px)
    # tracks in input order: the reference rows, and which cameras a point has
    n_obs_of = np.zeros(n_pt, np.int64)
    ref_row = np.zeros((n_pt, max_refs), np.int64)
    in_track = np.zeros((n_pt, max(n_cam, 1)), bool)
    for c, p, k in zip(np.asarray(cam_idx), np.asarray(pt_idx), np.asarray(obs_kp)):
        if n_obs_of[p] < max_refs:
            ref_row[p, n_obs_of[p]] = off[c] + k
        n_obs_of[p] += 1
        in_track[p, c] = True
    n_ref = np.minimum(n_obs_of, max_refs)
    claim = np.full(rows, NO_CLAIM, np.uint64)
    stats = np.zeros(4, np.int64)
    dist = guided_ref.hamming_rows if hamming else guided_ref.l2_rows
    with np.errstate(all="ignore"):
        for c in range(n_cam):
            r0, r1 = int(off[c]), int(off[c + 1])
            job = (n_obs_of > 0) & ~in_track[:, c]
            if r1 == r0 or not job.any():
                continue
            pu = np.full(n_pt, np.nan); pv = np.full(n_pt, np.nan)
            for p in np.nonzero(job)[0]:
                pu[p], pv[p], front = pixel(Rt_l[c], K_l[c], [float(x) for x in xyz[p]])
                job[p] = front
            ru = pu[:, None] - kp[None, r0:r1, 0]; rv = pv[:, None] - kp[None, r0:r1, 1]
            err2 = ru * ru + rv * rv
            adm = job[:, None] & free[None, r0:r1] & (err2 <= thr2)
            stats[0] += int(np.count_nonzero(adm.any(axis=1)))
            p, k = np.nonzero(adm)
            if len(p) == 0:
                continue
            d = np.full(len(p), np.nan, np.float32)
            for t in range(max_refs):
                sel = n_ref[p] > t
                dt = np.full(len(p), np.nan, np.float32)
                if sel.any():
                    dt[sel] = dist(desc[ref_row[p[sel], t]], desc[r0 + k[sel]])
                take = sel & (dt == dt) & ~(d <= dt)                    # a NaN distance is never the minimum
                d = np.where(take, dt, d)
            cand = d < FLT_MAX
            p, k, d = p[cand], k[cand], d[cand]
            if len(p) == 0:
                continue
            order = np.lexsort((k, d, p))
            p, k, d = p[order], k[order], d[order]
            first = np.nonzero(np.concatenate([[True], p[1:] != p[:-1]]))[0]
            nxt = np.minimum(first + 1, len(p) - 1)
            has2 = (first + 1 < len(p)) & (p[nxt] == p[first])
            d0 = d[first].astype(np.float64); d1 = d[nxt].astype(np.float64)
            prop = (d0 <= np.float64(max_distance)) & (~has2 | (d0 < np.float64(ratio) * d1))
            stats[1] += int(np.count_nonzero(prop))
            key = ((d[first][prop] + np.float32(0.0)).view(np.uint32).astype(np.uint64) << np.uint64(32)) | p[first][prop].astype(np.uint64)
            np.minimum.at(claim, r0 + k[first][prop], key)
    r = Result()
    won = claim != NO_CLAIM
    r.kp_point = np.where(won, (claim & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    r.kp_dist = np.where(won, (claim >> np.uint64(32)).astype(np.uint32).view(np.float32), FLT_MAX).astype(np.float32)
    stats[3] = int(np.count_nonzero(won)); stats[2] = stats[1] - stats[3]
    r.stats = stats
    return r


def run_case(case):
    return run(*case["args"], **case["opts"])


def assert_same(got, ref, what=""):
    """kp_point, kp_dist (as bit patterns) and stats of a call"""
    assert np.array_equal(got.kp_point, ref.kp_point), (what, np.nonzero(got.kp_point != ref.kp_point)[0][:10], got.kp_point[:20], ref.kp_point[:20])
    assert np.array_equal(np.asarray(got.kp_dist, np.float32).view(np.uint32), np.asarray(ref.kp_dist, np.float32).view(np.uint32)), what
    assert np.array_equal(np.asarray(got.stats, np.int64), np.asarray(ref.stats, np.int64)), (what, got.stats, ref.stats)


def apply(case, res):
    """The inputs of a second call once the assignments of `res` are applied: the won keypoints are no longer free and are
    observations of their points."""
    desc, kp, kp_free, off, K4, Rt, xyz, cam_idx, pt_idx, obs_kp = case["args"]
    off = np.asarray(off, np.int64)
    rows = np.nonzero(res.kp_point >= 0)[0]
    cams = np.searchsorted(off, rows, side="right") - 1
    free = np.asarray(kp_free).astype(np.uint8).copy(); free[rows] = 0
    args = (desc, kp, free, case["args"][3], K4, Rt, xyz, np.concatenate([cam_idx, cams]).astype(np.int32),
            np.concatenate([pt_idx, res.kp_point[rows]]).astype(np.int32), np.concatenate([obs_kp, rows - off[cams]]).astype(np.int32))
    return dict(name=case["name"] + "+applied", args=args, opts=case["opts"])
