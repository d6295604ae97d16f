"""Mesh rendering on the GPU against tests/render_ref.py: single triangles with vertices on pixel centres in both windings, ties and
interpenetration, every kind of skipped triangle, empty meshes, the jittered grid, boxes on both sides of the lane limit and a
triangle over the whole image, an odd image size, two views with different intrinsics, the three colour modes with the atlas's
border clamps, the background colour, the chain mesh, every combination of outputs and every rejection.  Pictures, depths and
identities are compared as bit patterns: there is no tolerance, and every case runs twice for identical bytes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import easysfm_amd as E
import mesh_clean_cases as K
import mvs_scene as S
import render_cases as RC
import render_ref as R
import texture_cases as TC

pytestmark = pytest.mark.gpu
F = np.float32
ROWS, COLS = RC.ROWS, RC.COLS


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _opt(background):
    o = E.default_mesh_render_options()
    o.background[:] = background
    return o


def _check(gpu_ctx, v, t, K4, P, rows, cols, rgb=None, uv=None, atlas=None, background=(0, 0, 0), ref=None):
    """The GPU's picture, depth and identities against the restatement's, twice for identical bytes."""
    got = E.mesh_render(v, t, K4, P, rows, cols, rgb, uv, atlas, _opt(background), gpu_ctx)
    ref = ref or R.mesh_render(v, t, K4, P, rows, cols, rgb, uv, atlas, background)
    for name, g, r in zip(("rgb", "depth", "triangle_id"), got, ref):
        assert _same(g, r), (name, np.count_nonzero(np.asarray(g) != np.asarray(r)))
    again = E.mesh_render(v, t, K4, P, rows, cols, rgb, uv, atlas, _opt(background), gpu_ctx)
    assert all(_same(a, b) for a, b in zip(again, got))
    return got


def _small(points_px, z=8.0):
    return RC.pixel_points(points_px, 8, 8, z, 8.0)


CAM8 = RC.pixel_camera(8, 8, 8.0)


# ---- 1: single triangles on 8 x 8 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pts", [[(2, 2), (6, 2), (2, 6)], [(2, 2), (6.25, 2.5), (2.5, 6.75)], [(4, 4), (-3, 9.5), (11, 1.25)]], ids=["centres", "one_centre", "clipped"])
def test_one_triangle_in_both_windings(gpu_ctx, pts):
    v = _small(pts)
    colours = RC.noise_colours(3)
    first = _check(gpu_ctx, v, np.array([[0, 1, 2]], np.int32), *CAM8, 8, 8, colours)
    second = _check(gpu_ctx, v, np.array([[0, 2, 1]], np.int32), *CAM8, 8, 8, colours)
    assert (first[2] >= 0).sum() >= 6 and _same(first[2], second[2])                   # the same pixels whichever way round


def test_coincident_triangles_go_to_the_lower_index(gpu_ctx):
    v = _small([(1, 1), (7, 1.5), (1.5, 7)] * 2)
    rgb, _, tid = _check(gpu_ctx, v, np.array([[0, 1, 2], [3, 4, 5]], np.int32), *CAM8, 8, 8, np.repeat(np.array([[200, 10, 10], [10, 200, 10]], np.uint8), 3, axis=0))
    assert set(np.unique(tid)) == {-1, 0} and np.all(rgb[tid == 0] == (200, 10, 10))
    tid = _check(gpu_ctx, v, np.array([[3, 5, 4], [0, 1, 2]], np.int32), *CAM8, 8, 8)[2]
    assert set(np.unique(tid)) == {-1, 0}


def test_interpenetrating_triangles(gpu_ctx):
    """Two triangles over the same pixels whose depths cross along a line: each wins on its side."""
    px = [(0.5, 0.5), (7.5, 0.75), (3.75, 7.5)]
    v = np.concatenate([RC.pixel_points(px, 8, 8, [4.0, 8.0, 6.0], 8.0), RC.pixel_points(px, 8, 8, [8.0, 4.0, 6.0], 8.0)])
    _, depth, tid = _check(gpu_ctx, v, np.array([[0, 1, 2], [3, 4, 5]], np.int32), *CAM8, 8, 8, RC.noise_colours(6))
    assert (tid == 0).sum() > 5 and (tid == 1).sum() > 5 and depth[tid >= 0].max() < 6.5


@pytest.mark.parametrize("kind", ["behind", "beyond", "flat", "repeated"])
def test_skipped_triangles(gpu_ctx, kind):
    """Triangle 1 is skipped whole: the picture is that of triangle 0 alone."""
    v = np.concatenate([_small([(1, 1), (6, 2), (2, 6)], 16.0), _small([(0, 0), (7, 0), (0, 7)])])
    t = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    if kind == "behind":
        v[5, 2] = -1.0                                                   # no clipping: one vertex behind the camera drops the triangle
    elif kind == "beyond":
        v[4, 0] = 2.0e6                                                  # u = 2e6 + 3.5 > 2^20
    elif kind == "flat":
        v[3:6] = _small([(0, 0), (3, 3), (7, 7)])                        # area2 == 0 in fixed point
    else:
        t[1] = (3, 4, 4)
    got = _check(gpu_ctx, v, t, *CAM8, 8, 8, RC.noise_colours(6))
    alone = _check(gpu_ctx, v, t[:1], *CAM8, 8, 8, RC.noise_colours(6))
    assert all(_same(a, b) for a, b in zip(got, alone)) and set(np.unique(got[2])) == {-1, 0}


def test_no_vertex_and_no_triangle(gpu_ctx):
    none_v, none_t = np.zeros((0, 3), F), np.zeros((0, 3), np.int32)
    for v in (none_v, _small([(1, 1), (6, 2), (2, 6)])):
        rgb, depth, tid = _check(gpu_ctx, v, none_t, *CAM8, 8, 8, background=(9, 8, 7))
        assert np.all(rgb == (9, 8, 7)) and not depth.any() and np.all(tid == -1)
    atlas = RC.noise_atlas(4, 4)
    rgb = _check(gpu_ctx, none_v, none_t, *CAM8, 8, 8, uv=np.zeros((0, 3, 2), F), atlas=atlas)[0]
    assert not rgb.any()


# ---- 2: both raster paths ---------------------------------------------------------------------------------------------------------
def test_the_grid_mesh(gpu_ctx):
    v, t, _ = RC.grid_mesh()
    K4, P = RC.grid_camera()
    tid = _check(gpu_ctx, v, t, K4, P, ROWS, COLS, RC.noise_colours(len(v)))[2][0]
    assert np.array_equal(tid >= 0, R.coverage_count(v, t, K4[0], P[0], ROWS, COLS) == 1) and len(np.unique(tid)) > 200


def test_boxes_at_the_lane_limit_and_over_the_whole_image(gpu_ctx):
    """Boxes of 56, 64, 72 and 81 pixels (the renderer's own, counted here from the restatement's screen triangles) on both sides of
    the 64 a lane walks alone; then one triangle over all 6 144 pixels in front of 300 small ones, and behind them."""
    v, t, sizes = RC.lane_limit_scene()
    K4, P = RC.pixel_camera(ROWS, COLS)
    tr = R.Tris(v, t, K4[0], P[0], ROWS, COLS)
    assert list((tr.bx1 - tr.bx0 + 1) * (tr.by1 - tr.by0 + 1)) == sizes == [56, 64, 72, 81, 64, 72] and len(tr.live) == 6
    tid = _check(gpu_ctx, v, t, K4, P, ROWS, COLS, RC.noise_colours(len(v)))[2]
    assert set(np.unique(tid)) == {-1, 0, 1, 2, 3, 4, 5}
    v, t = TC.big_triangle_scene(ROWS, COLS)
    K4, P = TC.front_camera(ROWS, COLS, 60.0)
    _, depth, tid = _check(gpu_ctx, v, t, K4, P, ROWS, COLS, RC.noise_colours(len(v)))
    assert np.all(tid == 0) and np.abs(depth - 2.0).max() < 1e-5
    v[:3, 2] = 9.0
    v[:3, :2] *= 4.5
    tid = _check(gpu_ctx, v, t[::-1], K4, P, ROWS, COLS, RC.noise_colours(len(v)))[2]
    assert np.all(tid >= 0) and (tid == len(t) - 1).mean() > 0.5 and len(np.unique(tid)) > 100


# ---- 3: image sizes and views -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three():
    v, _, rgb, t = K.three_spheres()[:4]
    return dict(v=v, rgb=rgb, t=t)


def test_an_odd_image_size(gpu_ctx, three):
    K4, P = TC.arc_views(1, 37, 53, (1.0, 0.9, 0.8), 4.0, 60.0)
    tid = _check(gpu_ctx, three["v"], three["t"], K4, P, 37, 53, three["rgb"])[2]
    assert 0.05 < (tid >= 0).mean() < 0.6 and len(np.unique(tid)) > 100


def test_two_views_with_different_intrinsics(gpu_ctx, three):
    K4, P = TC.arc_views(2, ROWS, COLS, (1.0, 0.9, 0.8), 4.0, 100.0)
    K4[1] = (60.0, 40.25, 75.0, 20.5)
    tid = _check(gpu_ctx, three["v"], three["t"], K4, P, ROWS, COLS, three["rgb"], background=(1, 2, 3))[2]
    assert (tid[0] >= 0).sum() > 1.3 * (tid[1] >= 0).sum() > 0


# ---- 4: colour modes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (16, 16)])
def test_textured_mode_and_the_atlas_border(gpu_ctx, H, W):
    """A quadrilateral over most of the image whose texture coordinates run from -0.25 to 1.25: the fetch clamps on all four sides,
    and inside it blends unrelated texels."""
    v = RC.pixel_points([(3, 2), (90.5, 4.25), (93, 60.5), (5.5, 58)], ROWS, COLS, [64.0, 128.0, 64.0, 32.0])
    t = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uv = np.array([[[-0.25, -0.25], [1.25, -0.25], [1.25, 1.25]], [[-0.25, -0.25], [1.25, 1.25], [-0.25, 1.25]]], F)
    K4, P = RC.pixel_camera(ROWS, COLS)
    atlas = RC.noise_atlas(H, W)
    rgb, _, tid = _check(gpu_ctx, v, t, K4, P, ROWS, COLS, uv=uv, atlas=atlas, background=(255, 0, 255))
    assert (tid >= 0).mean() > 0.7 and len(np.unique(rgb[tid >= 0].reshape(-1, 3), axis=0)) > (3 if H == 2 else 50)
    corners = {tuple(atlas[y, x]) for y in (0, H - 1) for x in (0, W - 1)}
    assert corners <= {tuple(c) for c in rgb[tid >= 0].reshape(-1, 3)}                  # each clamped corner region shows its texel
    # with vertex colours as well: the atlas wins
    assert _same(_check(gpu_ctx, v, t, K4, P, ROWS, COLS, RC.noise_colours(4), uv, atlas, (255, 0, 255))[0], rgb)


def test_vertex_colour_mode_grey_mode_and_background(gpu_ctx, three):
    K4, P = TC.arc_views(1, ROWS, COLS, (1.0, 0.9, 0.8), 4.0, 100.0)
    coloured = _check(gpu_ctx, three["v"], three["t"], K4, P, ROWS, COLS, three["rgb"])
    grey = _check(gpu_ctx, three["v"], three["t"], K4, P, ROWS, COLS, background=(10, 20, 30))
    m = grey[2] >= 0
    assert np.all(grey[0][m] == 128) and np.all(grey[0][~m] == (10, 20, 30)) and not coloured[0][~m].any()
    assert len(np.unique(coloured[0][m].reshape(-1, 3), axis=0)) > 50 and _same(coloured[1], grey[1]) and _same(coloured[2], grey[2])


# ---- 5: the chain mesh ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["textured", "coloured"])
def test_chain_mesh(gpu_ctx, mode):
    c = RC.chain()
    sc = c["scene"]
    kw = dict(uv=c["uv"], atlas=c["atlas"]) if mode == "textured" else dict(rgb=c["rgb"])
    got = _check(gpu_ctx, c["v"], c["t"], sc["K4"], sc["poses"], S.ROWS, S.COLS, ref=c[mode], **kw)
    for view, (err, share, coverage) in enumerate(RC.chain_figures(*got, sc)):
        print(f"view {view}, {mode}: error {err:.3f}, within 2 % depth {share:.4f}, coverage {coverage:.4f}")
        assert share >= RC.MIN_DEPTH_SHARE


# ---- 6: outputs and rejections ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [c for k in (1, 2) for c in itertools.combinations(("rgb", "depth", "triangle_id"), k)], ids="+".join)
def test_outputs_that_are_not_asked_for(gpu_ctx, names):
    v, t, _ = RC.grid_mesh()
    K4, P = RC.grid_camera()
    colours = RC.noise_colours(len(v))
    ref = dict(zip(("rgb", "depth", "triangle_id"), R.mesh_render(v, t, K4, P, ROWS, COLS, colours)))
    got = dict(zip(("rgb", "depth", "triangle_id"), E.mesh_render(v, t, K4, P, ROWS, COLS, colours, ctx=gpu_ctx, outputs=names)))
    for name in ("rgb", "depth", "triangle_id"):
        assert (got[name] is None) if name not in names else _same(got[name], ref[name]), name


def test_rejections_write_nothing(gpu_ctx):
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    v, t, _ = RC.grid_mesh()
    K4, P = RC.grid_camera()
    uv, atlas = np.full((len(t), 3, 2), 0.5, F), RC.noise_atlas(4, 6)
    rgb = np.full((1, ROWS, COLS, 3), 7, np.uint8); depth = np.full((1, ROWS, COLS), 7.0, F); tid = np.full((1, ROWS, COLS), 7, np.int32)
    o = E.default_mesh_render_options()

    def call(v=v, t=t, uv=uv, atlas=atlas, H=4, W=6, n=1, rows=ROWS, cols=COLS, K=K4, poses=P, o=o, outs=(rgb, depth, tid)):
        return L.esfm_mesh_render(gpu_ctx.handle, len(v), len(t), p(v), p(t), None, p(uv), H, W, p(atlas), n, rows, cols, p(K), p(poses), C.byref(o) if o else None,
                                  p(outs[0]), p(outs[1]), p(outs[2]))
    bad_v = v.copy(); bad_v[100, 1] = np.nan
    bad_t = t.copy(); bad_t[17, 1] = len(v)
    bad_uv = uv.copy(); bad_uv[2, 2, 1] = np.inf
    bad_K = K4.copy(); bad_K[0, 2] = 0
    bad_P = P.copy(); bad_P[0, 5] = np.inf
    for kw in (dict(v=bad_v), dict(t=bad_t), dict(n=0), dict(n=65), dict(rows=1), dict(cols=1), dict(rows=16385), dict(K=bad_K), dict(poses=bad_P), dict(uv=None),
               dict(atlas=None), dict(uv=bad_uv), dict(H=1), dict(W=1), dict(H=16385), dict(o=None), dict(outs=(None, None, None))):
        assert call(**kw) == -1, kw
    assert np.all(rgb == 7) and np.all(depth == 7.0) and np.all(tid == 7)
    assert call() == 0 and tid.max() > 200 and not np.all(rgb == 7)
    ref = R.mesh_render(v, t, K4, P, ROWS, COLS, None, uv, atlas)
    assert _same(rgb, ref[0]) and _same(depth, ref[1]) and _same(tid, ref[2])
