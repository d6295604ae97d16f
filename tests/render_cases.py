"""Meshes, cameras and the chain reference shared by the mesh-rendering tests (tests/test_mesh_render_cpu.py, _gpu.py)."""
import functools

import numpy as np

import mvs_scene as S
import render_ref as R
import texture_cases as TC
import texture_ref as X

F = np.float32
ROWS, COLS = 64, 96


def pixel_camera(rows, cols, focal=64.0):
    """front_camera with its principal point at the image centre: a world point (x, y, focal) lands on pixel (x + cx, y + cy)."""
    return TC.front_camera(rows, cols, focal)


def pixel_points(px, rows, cols, z=64.0, focal=64.0):
    """World points [m, 3] at depth z (scalar or [m]) that project exactly onto the pixel coordinates px [m, 2] under
    pixel_camera(rows, cols, focal), as long as the numbers are short enough for f32 (quarters of a pixel, z a power of two)."""
    p = np.asarray(px, np.float64).reshape(-1, 2)
    zz = np.broadcast_to(np.asarray(z, np.float64), (len(p),))
    x = (p[:, 0] - (cols - 1) / 2.0) * zz / focal
    y = (p[:, 1] - (rows - 1) / 2.0) * zz / focal
    return np.stack([x, y, zz], 1).astype(F)


def grid_mesh(n=12, seed=11):
    """A jittered n x n vertex grid near z = 4 that projects to about 33 x 22 pixels of the 64 x 96 image under
    front_camera(64, 96, 60): (vertices [n n, 3], triangles [2 (n - 1)^2, 3], interior [T] bool: the triangles of the quadrilaterals
    that do not touch the grid's border).  The jitter is a fifth of the spacing, so no quadrilateral folds over."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(-1.1, 1.1, n), np.linspace(-0.73, 0.73, n))
    v = np.stack([gx, gy, np.full_like(gx, 4.0)], -1)
    v[..., 0] += rng.uniform(-0.2, 0.2, gx.shape) * 2.2 / (n - 1)
    v[..., 1] += rng.uniform(-0.2, 0.2, gx.shape) * 1.46 / (n - 1)
    v[..., 2] += rng.uniform(-0.05, 0.05, gx.shape)
    t, interior = [], []
    for r in range(n - 1):
        for c in range(n - 1):
            a, b, d, e = r * n + c, r * n + c + 1, (r + 1) * n + c + 1, (r + 1) * n + c
            t += [[a, d, b], [a, e, d]] if (r + c) % 2 else [[a, e, b], [b, e, d]]        # both diagonals occur
            interior += [0 < r < n - 2 and 0 < c < n - 2] * 2
    return v.reshape(-1, 3).astype(F), np.array(t, np.int32), np.array(interior)


def grid_camera():
    return TC.front_camera(ROWS, COLS, 60.0)


LANE_LIMIT_LEGS = ((7, 8), (8, 8), (9, 8), (9, 9), (8, 8), (9, 8))


def lane_limit_scene():
    """Right triangles under pixel_camera(64, 96) whose corners lie a quarter of a pixel past a pixel centre, with legs of w and h
    pixels: the fixed-point box of each holds exactly w h pixel centres -- 56, 64, 72, 81, 64, 72 --, on both sides of the 64 up to
    which one lane walks a box alone; 72 and 81 give the large kernel's wave a partial second stride.  They overlap, each deeper
    than the one before.  Returns (vertices, triangles, the box sizes)."""
    v, t = [], []
    for k, (w, h) in enumerate(LANE_LIMIT_LEGS):
        x0, y0 = 8.25 + 7 * k, 10.25 + 4 * k
        v.append(pixel_points([(x0, y0), (x0 + w, y0), (x0, y0 + h)], ROWS, COLS, 64.0 * 2 ** k if k < 2 else 64.0 + 64.0 * k))
        t.append(np.array([[0, 2, 1]], np.int32) + 3 * k)
    return np.concatenate(v), np.concatenate(t), [w * h for w, h in LANE_LIMIT_LEGS]


def noise_atlas(H, W, seed=9):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


def noise_colours(V, seed=4):
    return np.random.default_rng(seed).integers(0, 256, (V, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def chain():
    """The chain mesh under the scene's five views, textured by the restatement (S = 4, a square atlas), and the restatement's
    renders in both modes: computed once per session and left unchanged."""
    v, rgb, t = TC.chain_mesh()
    scene = S.make_scene()
    label, score, _ = X.texture_views(v, t, S.ROWS, S.COLS, scene["K4"], scene["poses"])
    atlas, uv = X.texture_bake(v, rgb, t, label, scene["images"], scene["K4"], scene["poses"], X.auto_texels(label, score), 32)
    textured = R.mesh_render(v, t, scene["K4"], scene["poses"], S.ROWS, S.COLS, uv=uv, atlas=atlas)
    coloured = R.mesh_render(v, t, scene["K4"], scene["poses"], S.ROWS, S.COLS, vertex_rgb=rgb)
    for a in textured + coloured + (atlas, uv):
        a.setflags(write=False)
    return dict(v=v, rgb=rgb, t=t, scene=scene, atlas=atlas, uv=uv, textured=textured, coloured=coloured)


# The chain mesh re-rendered into the scene's five views of 180 x 240 by tests/render_ref.py (the head comment of
# tests/test_mesh_render_cpu.py says how the figures arose): per view, the mean absolute error against the photograph over the
# covered pixels and three channels, the share of covered pixels whose depth is within 2 % of the scene's exact depth, coverage.
MIN_DEPTH_SHARE = 0.95                                     # the condition the chain must meet


def chain_figures(rgb, depth, tid, scene):
    """Per view: (mean absolute error, share of covered pixels within 2 % of the exact depth, coverage)."""
    import easysfm_amd as E
    total, covered = E.mesh_render_error(rgb, tid, scene["images"])
    out = []
    for view in range(len(tid)):
        m = tid[view] >= 0
        exact = scene["depth"][view][m]
        share = float((np.abs(depth[view][m].astype(np.float64) - exact) <= 0.02 * exact).mean())
        out.append((float(total[view]) / (3.0 * float(covered[view])), share, float(m.mean())))
    return out
