"""A seeded ray-cast scene with exact depth for the dense-reconstruction tests: a textured plane slanted about 28 degrees from
fronto-parallel behind a textured sphere, seen by cameras on an arc of +-10 degrees around the scene centre.  The texture is
a sum of sinusoids in world coordinates (wavelengths 0.2 - 0.6 units, at least 6 px where projected head-on)."""
import numpy as np

ROWS, COLS = 180, 240
FX = FY = 200.0
CX, CY = (COLS - 1) / 2.0, (ROWS - 1) / 2.0
CENTRE = np.array([0.0, 0.0, 5.0])
PLANE_N = np.array([0.5, 0.2, -1.0]) / np.linalg.norm([0.5, 0.2, -1.0])
PLANE_P = np.array([0.0, 0.0, 6.0])
SPHERE_C = np.array([0.3, -0.2, 4.4])
SPHERE_R = 0.7


def texture(X, seed=7):
    rng = np.random.default_rng(seed)
    v = np.full(X.shape[:-1], 128.0)
    for _ in range(8):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        lam = rng.uniform(0.2, 0.6)
        v += rng.uniform(8, 14) * np.sin(2 * np.pi / lam * (X @ d) + rng.uniform(0, 2 * np.pi))
    return v


def camera(angle_deg):
    a = np.deg2rad(angle_deg)
    C = CENTRE + 5.0 * np.array([np.sin(a), 0.0, -np.cos(a)])
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return R, -R @ C


def render(R, t):
    """(grey u8 image, exact depth f64, object id: 0 plane, 1 sphere)."""
    ys, xs = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    dc = np.stack([(xs - CX) / FX, (ys - CY) / FY, np.ones_like(xs)], axis=-1)   # camera ray with z = 1: the hit's depth is s
    dw = dc @ R                                                                   # R^T dc
    C = -R.T @ t
    s_plane = ((PLANE_P - C) @ PLANE_N) / (dw @ PLANE_N)
    oc = C - SPHERE_C
    a = np.sum(dw * dw, -1)
    b = 2 * (dw @ oc)
    c = oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        s_sph = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    s_sph = np.where(s_sph > 0, s_sph, np.inf)
    obj = (s_sph < s_plane).astype(np.int32)
    depth = np.where(obj == 1, s_sph, s_plane)
    X = C + depth[..., None] * dw
    img = np.clip(np.rint(texture(X)), 0, 255).astype(np.uint8)
    return img, depth, obj


def make_scene(n_views=5):
    """Views on the arc from -10 to +10 degrees.  Returns dict with images [n, rows, cols] u8, depth [n, rows, cols] f64,
    obj, K4 [n, 4] f32, poses [n, 12] f32."""
    angles = np.linspace(-10.0, 10.0, n_views)
    imgs, depths, objs, poses = [], [], [], []
    for a in angles:
        R, t = camera(a)
        img, d, o = render(R, t)
        imgs.append(img); depths.append(d); objs.append(o)
        poses.append(np.concatenate([R, t[:, None]], axis=1).reshape(12))
    K4 = np.tile(np.array([FX, CX, FY, CY], np.float32), (n_views, 1))
    return dict(images=np.stack(imgs), depth=np.stack(depths), obj=np.stack(objs), K4=K4, poses=np.stack(poses).astype(np.float32))


def edge_distance_mask(obj, depth, margin):
    """True where no occlusion edge (an object change or a depth jump over 2 %) lies within `margin` px (Chebyshev)."""
    edge = np.zeros(obj.shape, bool)
    for dy, dx in ((0, 1), (1, 0)):
        a = (obj[:obj.shape[0] - dy, :obj.shape[1] - dx] != obj[dy:, dx:]) | \
            (np.abs(depth[:depth.shape[0] - dy, :depth.shape[1] - dx] - depth[dy:, dx:]) > 0.02 * depth[dy:, dx:])
        edge[:edge.shape[0] - dy, :edge.shape[1] - dx] |= a
        edge[dy:, dx:] |= a
    near = edge.copy()
    for _ in range(margin):
        grown = near.copy()
        grown[1:] |= near[:-1]; grown[:-1] |= near[1:]
        grown[:, 1:] |= near[:, :-1]; grown[:, :-1] |= near[:, 1:]
        grown[1:, 1:] |= near[:-1, :-1]; grown[:-1, :-1] |= near[1:, 1:]
        grown[1:, :-1] |= near[:-1, 1:]; grown[:-1, 1:] |= near[1:, :-1]
        near = grown
    return ~near


def visible_count(sc, v, sources):
    """Per pixel of view v: the number of sources that see its true surface point (inside the image, not occluded)."""
    R = sc["poses"][v].reshape(3, 4).astype(np.float64)
    ys, xs = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    d = sc["depth"][v]
    Xc = np.stack([(xs - CX) / FX * d, (ys - CY) / FY * d, d], -1)
    Xw = (Xc - R[:, 3]) @ R[:, :3]
    cnt = np.zeros(d.shape, np.int32)
    for s in sources:
        Ps = sc["poses"][s].reshape(3, 4).astype(np.float64)
        p = Xw @ Ps[:, :3].T + Ps[:, 3]
        u, w = FX * p[..., 0] / p[..., 2] + CX, FY * p[..., 1] / p[..., 2] + CY
        iu, iw = np.rint(u).astype(int), np.rint(w).astype(int)
        ins = (iu >= 0) & (iu < COLS) & (iw >= 0) & (iw < ROWS) & (p[..., 2] > 0)
        ds = sc["depth"][s][np.clip(iw, 0, ROWS - 1), np.clip(iu, 0, COLS - 1)]
        cnt += ins & (np.abs(ds - p[..., 2]) < 0.01 * p[..., 2])
    return cnt


def ray_depth(sc, v, X):
    """Depth in view v of the true surface along the ray through each world point X [m, 3], and the point's own depth."""
    P = sc["poses"][v].reshape(3, 4).astype(np.float64)
    R, t = P[:, :3], P[:, 3]
    p = np.asarray(X, np.float64) @ R.T + t
    dc = p / p[:, 2:3]                                   # ray with z = 1
    dw = dc @ R
    C = -R.T @ t
    s_plane = ((PLANE_P - C) @ PLANE_N) / (dw @ PLANE_N)
    oc = C - SPHERE_C
    a = np.sum(dw * dw, -1)
    b = 2 * (dw @ oc)
    c = oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        s_sph = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    s_sph = np.where(s_sph > 0, s_sph, np.inf)
    return np.minimum(s_sph, s_plane), p[:, 2]
