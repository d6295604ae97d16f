"""Generators the fundamental-matrix and auto-focal tests share (a helper, not a test module): the two synthetic scenes, the
correspondence sets drawn from them, the 4096 solver samples and the RANSAC cases."""
import numpy as np

from easysfm_amd import synth

import fundamental_ref as R

WIDTH, HEIGHT = 768, 512
FREEHAND_F = 620.0


def arc_scene(**kw):
    """synth.sfm_scene as it is: eight cameras on an arc, equidistant from the point they all fixate -- the critical configuration
    for equal focal lengths"""
    return synth.sfm_scene(**kw)


def freehand_scene(seed: int = 0, n_cam: int = 8, n_pt: int = 900, pix_noise: float = 0.3, n_clutter: int = 150, desc_noise: float = 0.03,
                   focal: float = FREEHAND_F, pp_offset=(0.0, 0.0)):
    """The scene of synth.sfm_scene (same point box, 768 x 512 images, descriptors and clutter drawn the same way) photographed free
    hand: focal length `focal`, principal point the image centre (+ pp_offset), camera c at angle (c - 3.5) * 0.16 on a radius drawn
    from 9 +- 2.5, height +- 1.5, aiming at a point uniform in +- 1.5 per axis, rolled by +- 0.15 rad about the viewing direction.
    Returns (frames, K, poses, pts) like sfm_scene."""
    rng = np.random.default_rng(np.random.PCG64(9100 + seed))
    K = np.array([[focal, 0, WIDTH / 2 + pp_offset[0]], [0, focal, HEIGHT / 2 + pp_offset[1]], [0, 0, 1]], np.float32)
    pts = np.stack([rng.uniform(-3, 3, n_pt), rng.uniform(-2, 2, n_pt), rng.uniform(-1.5, 1.5, n_pt)], 1)
    base = rng.standard_normal((n_pt, 64)); base /= np.linalg.norm(base, axis=1, keepdims=True)
    poses, frames = [], []
    for c in range(n_cam):
        ang = (c - (n_cam - 1) / 2) * 0.16
        rad = 9.0 + rng.uniform(-2.5, 2.5)
        C = np.array([rad * np.sin(ang), rng.uniform(-1.5, 1.5), -rad * np.cos(ang)])
        aim = rng.uniform(-1.5, 1.5, 3)
        roll = rng.uniform(-0.15, 0.15)
        z = (aim - C) / np.linalg.norm(aim - C)
        x = np.cross(np.array([0.0, 1.0, 0.0]), z); x /= np.linalg.norm(x)
        y = np.cross(z, x)
        x, y = np.cos(roll) * x + np.sin(roll) * y, -np.sin(roll) * x + np.cos(roll) * y
        Rm = np.stack([x, y, z], 0)
        T = np.eye(4); T[:3, :3] = Rm; T[:3, 3] = -Rm @ C
        poses.append(T)
        Xc = pts @ Rm.T + T[:3, 3]
        uv = np.stack([Xc[:, 0] / Xc[:, 2] * K[0, 0] + K[0, 2], Xc[:, 1] / Xc[:, 2] * K[1, 1] + K[1, 2]], 1)
        vis = (Xc[:, 2] > 1) & (uv[:, 0] > 5) & (uv[:, 0] < WIDTH - 5) & (uv[:, 1] > 5) & (uv[:, 1] < HEIGHT - 5)
        ids = np.nonzero(vis)[0]
        ids = ids[rng.random(len(ids)) < 0.9]
        kp = uv[ids] + pix_noise * rng.standard_normal((len(ids), 2))
        d = base[ids] + desc_noise * rng.standard_normal((len(ids), 64))
        ck = np.stack([rng.uniform(5, WIDTH - 5, n_clutter), rng.uniform(5, HEIGHT - 5, n_clutter)], 1)
        cd = rng.standard_normal((n_clutter, 64))
        kp = np.concatenate([kp, ck]); d = np.concatenate([d, cd]); pid = np.concatenate([ids, -np.ones(n_clutter, np.int64)])
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        order = rng.permutation(len(kp))
        frames.append(dict(keypoints=kp[order].astype(np.float32), descriptors=np.ascontiguousarray(d[order], np.float32), point_id=pid[order]))
    return frames, K, np.stack(poses), pts


def true_correspondences(frames, i, j):
    """the keypoints of frames i and j that show the same scene point -> float32 pts_i, pts_j (in point-id order)"""
    a, b = frames[i], frames[j]
    ia = {int(p): k for k, p in enumerate(a["point_id"]) if p >= 0}
    ib = {int(p): k for k, p in enumerate(b["point_id"]) if p >= 0}
    common = sorted(set(ia) & set(ib))
    return a["keypoints"][[ia[p] for p in common]], b["keypoints"][[ib[p] for p in common]]


def scene_fundamentals(frames, min_points: int = 30):
    """The 8-point F (the restatement's re-fit on all points) of the true correspondences of every pair (i, j < i) with at least
    min_points of them -> (F [p, 9], weights [p] = the number of correspondences)"""
    Fs, w = [], []
    for i in range(len(frames)):
        for j in range(i):
            a, b = true_correspondences(frames, i, j)
            if len(a) < min_points:
                continue
            F, ok = R.refit(a, b)
            if ok:
                Fs.append(F); w.append(float(len(a)))
    return np.array(Fs, np.float64).reshape(-1, 9), np.array(w, np.float64)


def correspondence_sets(seed: int = 0):
    """name -> (pts1, pts2) float32: 'general' (frames 3, 2 of the free-hand scene), 'wide' (frames 6, 1), 'plane' (the points moved onto
    the plane z = 0.3 x + 0.1 y, frames 3, 2; 0.3 px noise)"""
    frames, K, poses, pts = freehand_scene(seed)
    out = {"general": true_correspondences(frames, 3, 2), "wide": true_correspondences(frames, 6, 1)}
    rng = np.random.default_rng(77 + seed)
    flat = pts.copy(); flat[:, 2] = 0.3 * flat[:, 0] + 0.1 * flat[:, 1]
    Kd = K.astype(np.float64)
    uv = []
    for T in (poses[3], poses[2]):
        Xc = flat @ T[:3, :3].T + T[:3, 3]
        uv.append(np.stack([Xc[:, 0] / Xc[:, 2] * Kd[0, 0] + Kd[0, 2], Xc[:, 1] / Xc[:, 2] * Kd[1, 1] + Kd[1, 2]], 1))
    ok = np.ones(len(flat), bool)
    for p in uv:
        ok &= (p[:, 0] > 5) & (p[:, 0] < WIDTH - 5) & (p[:, 1] > 5) & (p[:, 1] < HEIGHT - 5)
    out["plane"] = tuple((p[ok] + 0.3 * rng.standard_normal(p[ok].shape)).astype(np.float32) for p in uv)
    return out


def degenerate_samples():
    """hand-made samples [k, 7, 2] x 2: seven identical points; a point repeated three times; seven exactly collinear points in image 1;
    collinear in both; a non-finite coordinate; coordinates of 1e6; an exact affine map (rank-deficient system)"""
    rng = np.random.default_rng(5)
    gen1 = rng.uniform(50, 700, (7, 2)); gen2 = gen1 + rng.uniform(-30, 30, (7, 2))
    same = np.tile([[37.5, 91.25]], (7, 1))
    rep1 = gen1.copy(); rep1[1] = rep1[0]; rep1[2] = rep1[0]
    rep2 = gen2.copy(); rep2[1] = rep2[0]; rep2[2] = rep2[0]
    line = np.stack([np.arange(7) * 40.0 + 10.0, np.arange(7) * 20.0 + 30.0], 1)
    far = gen2.copy(); far[3] = [np.inf, 50.0]
    big1 = gen1 * 1e3 + 1e6; big2 = gen2 * 1e3 + 1e6
    aff = gen1 @ np.array([[1.1, 0.2], [-0.1, 0.9]]) + [12.0, -7.0]
    q1 = np.stack([same, rep1, line, line, gen1, big1, gen1, gen1])
    q2 = np.stack([same, rep2, gen2, line * 1.5 + 3.0, far, big2, aff, same])
    return q1, q2


def solver_samples(total: int = 4096, seed: int = 0):
    """`total` samples: sevens the sampler draws from 'general' and 'wide' (half each of the bulk), 64 from 'plane', 64 noisy collinear
    sevens (points of 'general' pulled onto a line in image 1, 0.3 px off it), 16 with a repeated point, then the hand-made degenerate
    ones -> q1, q2 [total, 7, 2] float64"""
    sets = correspondence_sets(seed)
    d1, d2 = degenerate_samples()
    n_plane, n_line, n_rep = 64, 64, 16
    bulk = total - n_plane - n_line - n_rep - len(d1)
    q1, q2 = [], []
    for name, cnt in (("general", bulk // 2), ("wide", bulk - bulk // 2), ("plane", n_plane)):
        a, b = sets[name]
        idx = R.sample_stream(len(a), cnt)
        q1.append(a[idx].astype(np.float64)); q2.append(b[idx].astype(np.float64))
    a, b = sets["general"]
    rng = np.random.default_rng(31 + seed)
    idx = R.sample_stream(len(a), n_line + n_rep)
    l1 = a[idx[:n_line]].astype(np.float64); l2 = b[idx[:n_line]].astype(np.float64)
    l1[:, :, 1] = 0.4 * l1[:, :, 0] + 60.0 + 0.3 * rng.standard_normal(l1.shape[:2])
    q1.append(l1); q2.append(l2)
    r1 = a[idx[n_line:]].astype(np.float64); r2 = b[idx[n_line:]].astype(np.float64)
    r1[:, 5] = r1[:, 2]; r2[:, 5] = r2[:, 2]
    q1.append(r1); q2.append(r2)
    q1 = np.concatenate(q1 + [d1]); q2 = np.concatenate(q2 + [d2])
    assert len(q1) == total
    return q1, q2


def ransac_case(n, outlier_frac=0.2, seed=0):
    """n correspondences of the free-hand scene's frames 3 and 2 (0.3 px noise), a fraction replaced by random points -> float32 pts1, pts2"""
    a, b = correspondence_sets(0)["general"]
    assert n <= len(a), (n, len(a))
    rng = np.random.default_rng(2000 + 7 * n + seed)
    pick = rng.permutation(len(a))[:n]
    a, b = a[pick].copy(), b[pick].copy()
    bad = rng.permutation(n)[:int(round(outlier_frac * n))]
    b[bad] = np.stack([rng.uniform(5, WIDTH - 5, len(bad)), rng.uniform(5, HEIGHT - 5, len(bad))], 1).astype(np.float32)
    return a, b


def no_model_case(n=40, seed=3):
    """random points in both images, for a threshold of 0: a model's own seven points sit at rounding distance from their lines, not
    at distance 0, so no model reaches 7 inliers (the test states whatever outcome the restatement gives)"""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(5, WIDTH - 5, n), rng.uniform(5, HEIGHT - 5, n)], 1).astype(np.float32)
    b = np.stack([rng.uniform(5, WIDTH - 5, n), rng.uniform(5, HEIGHT - 5, n)], 1).astype(np.float32)
    return a, b
