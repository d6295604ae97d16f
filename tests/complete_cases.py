"""Seeded case builders of track completion, shared by the CPU and the GPU tests (esfm.h "Track completion").  A case is a dict:
name, args = (desc, kp, kp_free, set_row_offset, K4, Rt, xyz, cam_idx, pt_idx, obs_kp) and opts = the four options."""
import numpy as np

UNIT_K = (1.0, 0.0, 1.0, 0.0)
EYE = np.hstack([np.eye(3), np.zeros((3, 1))])
OPTS = dict(search_radius_px=4.0, max_distance=np.inf, ratio=0.8, max_refs=8)


def opts(**kw):
    o = dict(OPTS); o.update(kw)
    return o


def manual(name, cams, points, obs, o=None, dtype=np.float32):
    """cams: [(K4, Rt[3, 4], [(u, v, free, descriptor row), ...]), ...]; points: [xyz, ...]; obs: [(cam, point, keypoint), ...]"""
    width = max([len(k[3]) for c in cams for k in c[2]] + [1])
    desc = np.array([k[3] for c in cams for k in c[2]], dtype).reshape(-1, width)
    kp = np.array([[k[0], k[1]] for c in cams for k in c[2]], np.float32).reshape(-1, 2)
    free = np.array([k[2] for c in cams for k in c[2]], np.uint8)
    off = np.concatenate([[0], np.cumsum([len(c[2]) for c in cams])]).astype(np.int32)
    K4 = np.array([c[0] for c in cams], np.float32).reshape(-1, 4)
    Rt = np.array([c[1] for c in cams], np.float64).reshape(-1, 3, 4)
    ob = np.array(obs, np.int32).reshape(-1, 3)
    args = (desc, kp, free, off, K4, Rt, np.array(points, np.float64).reshape(-1, 3), ob[:, 0].copy(), ob[:, 1].copy(), ob[:, 2].copy())
    return dict(name=name, args=args, opts=o or opts())


def vec(*head, dim=8):
    """a descriptor row: `head`, then zeros"""
    return list(head) + [0.0] * (dim - len(head))


def home(rows):
    """camera 0: identity, unit K; it holds the (non-free) keypoints that give the points their first observation"""
    return (UNIT_K, EYE, [(0.0, 0.0, 0, r) for r in rows])


# ---- the radius edge, in exact arithmetic --------------------------------------------------------------------------------------
def radius_edge(radius):
    """point (3, 4, 1) under K4 = (1, 0, 1, 0) and the identity projects to (3, 4); a free keypoint at (0, 0): err2 == 25"""
    cams = [home([vec(1.0)]), (UNIT_K, EYE, [(0.0, 0.0, 1, vec(1.0))])]
    return manual(f"radius-edge-{radius!r}", cams, [(3.0, 4.0, 1.0)], [(0, 0, 0)], opts(search_radius_px=radius))


# ---- cell borders ----------------------------------------------------------------------------------------------------------------
def cell_borders(radius=4.0):
    """Free keypoints on the box's edge (0, 0) .. (32, 32); radius 4 makes cells of 8.  Points project onto (16, 16), a corner where
    four cells meet, with one free keypoint in each of them; onto (-3, 10) and (33, 5), outside the box but within the radius of
    an edge keypoint; next to a box corner; and far outside."""
    pts = [(16.0, 16.0, 1.0), (-3.0, 10.0, 1.0), (33.0, 5.0, 1.0), (31.0, 31.5, 1.0), (80.0, 80.0, 1.0), (7.99, 8.01, 1.0), (24.0, 0.0, 1.0)]
    d = [vec(float(i + 1), 0.25 * i) for i in range(len(pts))]
    kps = [(15.0, 15.0, 1, vec(1.0, 0.1)), (17.0, 15.0, 1, vec(1.0, 0.2)), (15.0, 17.0, 1, vec(1.0, 0.3)), (17.0, 17.0, 1, vec(1.0, 0.05)),
           (0.0, 0.0, 1, vec(9.0)), (32.0, 32.0, 1, vec(4.0, 0.8)), (0.0, 10.0, 1, vec(2.0, 0.3)), (32.0, 5.0, 1, vec(3.0, 0.4)),
           (8.0, 8.0, 1, vec(6.0, 1.2)), (7.0, 9.0, 1, vec(6.0, 1.5)), (24.0, 3.9, 1, vec(7.0, 1.4)), (20.1, 0.0, 1, vec(7.0, 1.7)),
           (28.0, 0.0, 1, vec(7.0, 1.9)), (16.0, 12.0, 1, vec(1.5)), (16.0, 20.0, 0, vec(1.0))]
    cams = [home(d), (UNIT_K, EYE, kps)]
    return manual(f"cell-borders-{radius:g}", cams, pts, [(0, i, i) for i in range(len(pts))], opts(search_radius_px=radius, ratio=0.99))


# ---- jobs that must not exist, candidates that must be ignored ------------------------------------------------------------------
def no_jobs():
    """point 0 behind camera 1 (p_2 < 0), point 1 on its focal plane (p_2 == 0), point 2 already seen by camera 1 while a free
    keypoint with its descriptor sits at the projection, point 3 without observations; point 4 is an ordinary job"""
    pts = [(1.0, 1.0, -1.0), (1.0, 1.0, 0.0), (2.0, 2.0, 1.0), (5.0, 5.0, 1.0), (9.0, 9.0, 1.0)]
    d = [vec(float(i + 1)) for i in range(5)]
    kps = [(-1.0, -1.0, 1, d[0]), (1.0, 1.0, 1, d[1]), (2.0, 2.0, 1, d[2]), (2.5, 2.0, 0, d[2]), (5.0, 5.0, 1, d[3]), (9.0, 9.5, 1, d[4])]
    cams = [home(d), (UNIT_K, EYE, kps)]
    return manual("no-jobs", cams, pts, [(0, 0, 0), (0, 1, 1), (0, 2, 2), (1, 2, 3), (0, 4, 4)])


def non_free_ignored():
    """a non-free keypoint nearer and more similar than the free one"""
    cams = [home([vec(1.0)]), (UNIT_K, EYE, [(5.0, 5.0, 0, vec(1.0)), (6.0, 6.0, 1, vec(1.0, 0.5))])]
    return manual("non-free-ignored", cams, [(5.0, 5.0, 1.0)], [(0, 0, 0)])


# ---- ties and gates --------------------------------------------------------------------------------------------------------------
def tie(ratio):
    """two candidates of equal distance (5: a 3-4-5 difference): the lower row is k0"""
    cams = [home([vec(0.0, 0.0)]), (UNIT_K, EYE, [(9.0, 9.0, 1, vec(9.0)), (5.0, 6.0, 1, vec(3.0, 4.0)), (6.0, 5.0, 1, vec(4.0, 3.0))])]
    return manual(f"tie-ratio-{ratio:g}", cams, [(5.5, 5.5, 1.0)], [(0, 0, 0)], opts(ratio=ratio))


def gate(max_distance, hamming=False):
    """a lone candidate at distance exactly 5 (L2: a 3-4-5 difference; Hamming: five bits)"""
    if hamming:
        a = [0] * 16; b = [0] * 16; b[3] = 0b10110001; b[9] = 0b00000001
        cams = [home([a]), (UNIT_K, EYE, [(5.0, 5.0, 1, b)])]
        return manual(f"gate-hamming-{max_distance!r}", cams, [(5.0, 5.0, 1.0)], [(0, 0, 0)], opts(max_distance=max_distance), np.uint8)
    cams = [home([vec(0.0, 0.0)]), (UNIT_K, EYE, [(5.0, 5.0, 1, vec(3.0, 4.0))])]
    return manual(f"gate-l2-{max_distance!r}", cams, [(5.0, 5.0, 1.0)], [(0, 0, 0)], opts(max_distance=max_distance))


# ---- conflicts -------------------------------------------------------------------------------------------------------------------
def conflict(n, equal):
    """n points propose keypoint 0 of camera 1, with distinct distances (the LAST point is nearest) or with equal ones (the lowest
    index wins); every point has further admissible candidates (keypoints 1 .. n, farther in descriptor space), yet a loser gains
    nothing in this camera"""
    pts = [(10.0 + 0.5 * i, 10.0, 1.0) for i in range(n)]
    d = [vec(1.0, 0.0 if equal else 0.1 * (n - i), float(i)) for i in range(n)]
    kps = [(10.5, 10.0, 1, vec(1.0, 0.0, 0.0))] + [(10.0 + 0.5 * i, 11.0, 1, vec(1.0, 3.0, float(i))) for i in range(n)]
    for i in range(n):          # the shared keypoint must be equally near every point in the descriptor's third entry
        d[i][2] = 0.0
    cams = [home(d), (UNIT_K, EYE, kps)]
    return manual(f"conflict-{n}-{'equal' if equal else 'distinct'}", cams, pts, [(0, i, i) for i in range(n)], opts(ratio=0.9))


# ---- reference rows --------------------------------------------------------------------------------------------------------------
def references(n_obs, max_refs=8):
    """one point seen by n_obs cameras; only its LAST observation's descriptor is near the free keypoint of the last camera"""
    far, near = vec(0.0, 0.0), vec(3.0, 4.0)
    cams = [(UNIT_K, EYE, [(2.0, 2.0, 0, near if c == n_obs - 1 else far)]) for c in range(n_obs)]
    cams.append((UNIT_K, EYE, [(2.0, 2.5, 1, vec(3.0, 4.0, 1.0))]))
    return manual(f"references-{n_obs}-of-{max_refs}", cams, [(2.0, 2.0, 1.0)], [(c, 0, 0) for c in range(n_obs)], opts(max_distance=2.0, max_refs=max_refs))


# ---- a crowded window ------------------------------------------------------------------------------------------------------------
def crowded(n, seed=5):
    """n free keypoints inside one window of radius 4 about (50, 50), and a few outside"""
    rng = np.random.default_rng(seed + n)
    ang, rad = rng.uniform(0, 2 * np.pi, n), 3.9 * np.sqrt(rng.uniform(0, 1, n))
    inside = np.stack([50 + rad * np.cos(ang), 50 + rad * np.sin(ang)], 1)
    outside = rng.uniform(0, 100, (20, 2))
    d0 = rng.standard_normal(16)
    kps = [(float(u), float(v), 1, list(d0 + 0.3 * rng.standard_normal(16))) for u, v in np.concatenate([inside, outside])]
    cams = [home([list(d0)]), (UNIT_K, EYE, kps)]
    return manual(f"crowded-{n}", cams, [(50.0, 50.0, 1.0)], [(0, 0, 0)], opts(ratio=0.999))


# ---- the general scene -----------------------------------------------------------------------------------------------------------
K_SCENE = (500.0, 320.0, 500.0, 240.0)


def arc_cameras(n_cam, span=0.6):
    Rt = np.zeros((n_cam, 3, 4))
    for c, a in enumerate(np.linspace(-span / 2, span / 2, n_cam)):
        Rt[c] = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 6.0]])
    return Rt


def scene(name, n_cam=6, n_pt=400, n_clutter=400, width=64, hamming=False, seed=11, withhold=0.3, noise=0.3, o=None):
    """n_cam cameras on an arc, n_pt points at depth about 6 seen by all of them with pixel noise `noise`; per-point descriptors
    (L2: unit norm + N(0, 0.02^2) per view; Hamming: random bits, 3 % flipped per view); n_clutter free keypoints per camera with random
    positions and descriptors; a seeded share `withhold` of the true observations is left out of the input and marked free.
    Returns the case with truth = the point of every keypoint row (-1: clutter) and withheld = the rows left out."""
    rng = np.random.default_rng(seed)
    Rt = arc_cameras(n_cam)
    X = rng.uniform(-1.0, 1.0, (n_pt, 3)) * [2.0, 1.5, 1.0]
    if hamming:
        base = rng.integers(0, 256, (n_pt, width), dtype=np.uint8)
    else:
        base = rng.standard_normal((n_pt, width)); base /= np.linalg.norm(base, axis=1, keepdims=True)
    desc, kp, free, truth, off, cam_idx, pt_idx, obs_kp, withheld = [], [], [], [], [0], [], [], [], []
    for c in range(n_cam):
        Xc = X @ Rt[c, :, :3].T + Rt[c, :, 3]
        uv = Xc[:, :2] / Xc[:, 2:3] * [K_SCENE[0], K_SCENE[2]] + [K_SCENE[1], K_SCENE[3]] + noise * rng.standard_normal((n_pt, 2))
        if hamming:
            flip = (rng.uniform(0, 1, (n_pt, width, 8)) < 0.03).astype(np.uint8)
            d = base ^ np.packbits(flip, axis=2).reshape(n_pt, width)
            dc = rng.integers(0, 256, (n_clutter, width), dtype=np.uint8)
        else:
            d = (base + 0.02 * rng.standard_normal((n_pt, width))).astype(np.float32)
            dc = rng.standard_normal((n_clutter, width)); dc = (dc / np.linalg.norm(dc, axis=1, keepdims=True)).astype(np.float32)
        uvc = rng.uniform(0, 1, (n_clutter, 2)) * [640, 480]
        order = rng.permutation(n_pt + n_clutter)
        all_d = np.concatenate([d, dc])[order]; all_uv = np.concatenate([uv, uvc])[order]
        tr = np.concatenate([np.arange(n_pt), np.full(n_clutter, -1)])[order]
        hold = rng.uniform(0, 1, n_pt + n_clutter) < withhold
        seen = np.nonzero((tr >= 0) & ~hold)[0]
        desc.append(all_d); kp.append(all_uv); truth.append(tr); free.append(((tr < 0) | hold).astype(np.uint8))
        withheld.append(off[-1] + np.nonzero((tr >= 0) & hold)[0])
        cam_idx.append(np.full(len(seen), c)); pt_idx.append(tr[seen]); obs_kp.append(seen)
        off.append(off[-1] + n_pt + n_clutter)
    mix = rng.permutation(sum(len(a) for a in cam_idx))                    # the observations in no particular order
    args = (np.concatenate(desc), np.concatenate(kp).astype(np.float32), np.concatenate(free), np.array(off, np.int32),
            np.tile(np.array(K_SCENE, np.float32), (n_cam, 1)), Rt, X, np.concatenate(cam_idx).astype(np.int32)[mix],
            np.concatenate(pt_idx).astype(np.int32)[mix], np.concatenate(obs_kp).astype(np.int32)[mix])
    return dict(name=name, args=args, opts=o or opts(), truth=np.concatenate(truth), withheld=np.concatenate(withheld))


def purpose_scene():
    """the issue's construction: 6 cameras, 400 points, 400 distractors per camera, 30 % withheld; radius 4, max_distance 0.5, ratio 0.8"""
    return scene("purpose", seed=2024, o=opts(max_distance=0.5))


def widths():
    out = [scene(f"l2-dim-{w}", 3, 30, 30, w, False, seed=100 + w, o=opts(ratio=0.95)) for w in (1, 3, 64, 67, 128)]
    return out + [scene(f"hamming-{w}", 3, 30, 30, w, True, seed=200 + w) for w in (16, 32, 64)]


# ---- job counts ------------------------------------------------------------------------------------------------------------------
def job_count(n_pt, n_other, seed=31, in_all=False):
    """n_pt points seen by camera 0 only (in_all: by every camera, so that there is no job); n_other further cameras with three free
    keypoints each inside the points' square and a radius (3) that reaches every one of them from every point: n_pt x n_other jobs survive
    the compaction and each has an admissible keypoint, so stats[0] counts them"""
    rng = np.random.default_rng(seed)
    n_cam = 1 + n_other
    X = np.concatenate([rng.uniform(-1, 1, (n_pt, 2)), np.ones((n_pt, 1))], 1)
    base = rng.standard_normal((n_pt, 8)).astype(np.float32)
    desc = [base]; kp = [X[:, :2].astype(np.float32)]; free = [np.zeros(n_pt, np.uint8)]; off = [0, n_pt]
    cam_idx = [np.zeros(n_pt, np.int32)]; pt_idx = [np.arange(n_pt, dtype=np.int32)]; obs_kp = [np.arange(n_pt, dtype=np.int32)]
    for c in range(1, n_cam):
        take = rng.integers(0, n_pt, 3)
        extra = n_pt if in_all else 0
        d = base[take] + 0.05 * rng.standard_normal((3, 8)).astype(np.float32)
        desc.append(np.concatenate([d, base[:extra]])); kp.append(np.concatenate([X[take, :2] + 0.01, X[:extra, :2]]).astype(np.float32))
        free.append(np.concatenate([np.ones(3, np.uint8), np.zeros(extra, np.uint8)]))
        if in_all:
            cam_idx.append(np.full(n_pt, c, np.int32)); pt_idx.append(np.arange(n_pt, dtype=np.int32)); obs_kp.append(3 + np.arange(n_pt, dtype=np.int32))
        off.append(off[-1] + 3 + extra)
    args = (np.concatenate(desc), np.concatenate(kp), np.concatenate(free), np.array(off, np.int32), np.tile(np.array(UNIT_K, np.float32), (n_cam, 1)),
            np.tile(EYE, (n_cam, 1, 1)), X, np.concatenate(cam_idx), np.concatenate(pt_idx), np.concatenate(obs_kp))
    return dict(name=f"jobs-{0 if in_all else n_pt * n_other}", args=args, opts=opts(search_radius_px=3.0, ratio=0.9), n_jobs=0 if in_all else n_pt * n_other)


# ---- empty and degenerate inputs -------------------------------------------------------------------------------------------------
def small():
    return scene("small", 4, 40, 25, 16, False, seed=77)


def no_points():
    c = small()
    a = c["args"]
    e = np.zeros(0, np.int32)
    return dict(name="n_pt-0", args=a[:6] + (np.zeros((0, 3)), e, e, e), opts=c["opts"])


def empty_camera():
    """camera 1 of the small scene has no keypoint rows (its observations go with them)"""
    c = small()
    desc, kp, free, off, K4, Rt, X, cam, pt, ok = c["args"]
    keep_rows = np.ones(len(kp), bool); keep_rows[off[1]:off[2]] = False
    off2 = off.copy(); off2[2:] -= off[2] - off[1]
    keep_obs = cam != 1
    return dict(name="empty-camera", args=(desc[keep_rows], kp[keep_rows], free[keep_rows], off2, K4, Rt, X, cam[keep_obs], pt[keep_obs], ok[keep_obs]), opts=c["opts"])


def none_free():
    c = small()
    a = c["args"]
    return dict(name="none-free", args=a[:2] + (np.zeros_like(a[2]),) + a[3:], opts=c["opts"])


def with_nan(what):
    """the small scene with a NaN in a point, in a camera's Rt, in free keypoints or in descriptor rows (free rows and the reference
    rows of a few points)"""
    c = small()
    desc, kp, free, off, K4, Rt, X, cam, pt, ok = [np.array(a) for a in c["args"]]
    withheld = c["withheld"]
    if what == "point":
        X[3, 1] = np.nan; X[11, 2] = np.nan
    elif what == "Rt":
        Rt[2, 1, 3] = np.nan
    elif what == "keypoint":
        kp[withheld[::3], 0] = np.nan; kp[withheld[1::5], 1] = np.inf
    else:
        desc[withheld[::4], 5] = np.nan
        for p in (0, 7):                                                # every reference row of point 0, the first of point 7
            rows = (off[cam] + ok)[pt == p]
            desc[rows if p == 0 else rows[:1], 2] = np.nan
    return dict(name=f"nan-{what}", args=(desc, kp, free, off, K4, Rt, X, cam, pt, ok), opts=c["opts"], truth=c["truth"], withheld=withheld)


def exact_cases():
    """every case but the purpose scene and the largest job count"""
    five_below = float(np.nextafter(np.float64(5.0), 0.0))
    out = [radius_edge(5.0), radius_edge(five_below), cell_borders(4.0), cell_borders(1e4), cell_borders(0.3), no_jobs(), non_free_ignored()]
    out += [tie(r) for r in (0.5, 1.0, 1.5)]
    out += [gate(5.0), gate(five_below), gate(5.0, True), gate(five_below, True)]
    out += [conflict(n, eq) for n in (2, 3) for eq in (False, True)]
    out += [references(n) for n in (1, 2, 8, 9)] + [references(2, 1), references(9, 1)]
    out += [crowded(n) for n in (1, 63, 64, 65, 300)]
    out += widths()
    out += [job_count(3, 2, in_all=True), job_count(1, 1), job_count(128, 2), job_count(257, 1), job_count(130, 4)]
    out += [small(), no_points(), empty_camera(), none_free()] + [with_nan(w) for w in ("point", "Rt", "keypoint", "descriptor")]
    return out


def many_jobs():
    """more than 65 536 jobs after the compaction (2 200 points x 31 cameras): several block-scan tiles"""
    return job_count(2200, 31)
