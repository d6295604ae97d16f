"""Mesh texturing on the GPU against tests/texture_ref.py: the three spheres under four views over image kinds, chart sizes,
colours and atlas widths, a triangle that covers the whole image in front of small ones, a triangle through the camera plane, a
mesh behind the camera, no triangle, 64 views, rejections, and the synthetic-scene chain.  Outputs are compared as bit patterns:
there is no tolerance, and every case runs twice for identical bytes."""
import ctypes as C

import numpy as np
import pytest

import easysfm_amd as E
import mesh_clean_cases as K
import mvs_ref as M
import mvs_scene as S
import texture_cases as TC
import texture_ref as X
import tsdf_ref as T

pytestmark = pytest.mark.gpu
F = np.float32
ROWS, COLS = 64, 96
far_grid, chain_mesh, check_chain = TC.far_grid, TC.chain_mesh, TC.check_chain


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _opt(**kw):
    o = E.default_mesh_texture_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _check_views(gpu_ctx, v, t, rows, cols, K4, P, o=None):
    """The GPU's labels, scores and buffers against the restatement's, twice for identical bytes; also without the buffers."""
    o = o or _opt()
    got = E.mesh_texture_views(v, t, rows, cols, K4, P, o, gpu_ctx, return_buffers=True)
    ref = X.texture_views(v, t, rows, cols, K4, P, X.options(o.min_cos, o.occlusion_tol))
    for name, g, r in zip(("label", "score", "buffers"), got, ref):
        assert _same(g, r), (name, np.count_nonzero(np.asarray(g) != np.asarray(r)))
    again = E.mesh_texture_views(v, t, rows, cols, K4, P, o, gpu_ctx, return_buffers=True)
    assert all(_same(a, b) for a, b in zip(again, got))
    assert all(_same(a, b) for a, b in zip(E.mesh_texture_views(v, t, rows, cols, K4, P, o, gpu_ctx), got[:2]))
    return got


def _check_bake(gpu_ctx, v, rgb, t, label, images, K4, P, S_, A):
    got = E.mesh_texture_bake(v, rgb, t, label, images, K4, P, S_, A, gpu_ctx)
    ref = X.texture_bake(v, rgb, t, label, images, K4, P, S_, A)
    for name, g, r in zip(("atlas", "uv"), got, ref):
        assert _same(g, r), (name, g.shape, r.shape, np.count_nonzero(np.asarray(g) != np.asarray(r)) if g.shape == r.shape else None)
    assert all(_same(a, b) for a, b in zip(E.mesh_texture_bake(v, rgb, t, label, images, K4, P, S_, A, gpu_ctx), got))
    return got


# ---- 1: three spheres -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three():
    v, _, rgb, t = K.three_spheres()[:4]
    K4, P = TC.arc_views(4, ROWS, COLS, (1.0, 0.9, 0.8), 4.0, 100.0)
    return dict(v=v, rgb=rgb, t=t, K4=K4, P=P)


@pytest.fixture(scope="module")
def three_views(gpu_ctx, three):
    return _check_views(gpu_ctx, three["v"], three["t"], ROWS, COLS, three["K4"], three["P"])


def test_three_spheres_views(three, three_views):
    label, score, buffers = three_views
    assert (len(three["v"]), len(three["t"])) == (2310, 4608)
    assert set(np.unique(label)) == {-1, 0, 1, 2, 3} and 0.3 < (label >= 0).mean() < 0.5      # about the half that faces the arc
    assert np.all((score > 0) == (label >= 0)) and 0.1 < (buffers > 0).mean() < 0.2


@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
@pytest.mark.parametrize("colours", [False, True], ids=["plain", "rgb"])
@pytest.mark.parametrize("S_,A", [(4, 37), (7, 61), (16, 50)])
@pytest.mark.parametrize("channels", [1, 3], ids=["grey", "bgr"])
def test_three_spheres_bake(gpu_ctx, three, three_views, channels, S_, A, colours, odd):
    """2 304 squares in rows of 37, 61 or 50 leave a last row of 10, 47 or 4; the odd case drops the last triangle."""
    T_ = len(three["t"]) - (1 if odd else 0)
    images = TC.noise_images(4, ROWS, COLS, channels)
    atlas, uv = _check_bake(gpu_ctx, three["v"], three["rgb"] if colours else None, three["t"][:T_], three_views[0][:T_], images, three["K4"], three["P"], S_, A)
    assert atlas.shape == (-(-2304 // A) * S_, A * S_, 3) and uv.shape == (T_, 3, 2)
    assert atlas.any() and 0 < uv.min() and uv.max() < 1


def test_options_move_the_labels(gpu_ctx, three, three_views):
    strict = _check_views(gpu_ctx, three["v"], three["t"], ROWS, COLS, three["K4"], three["P"], _opt(min_cos=0.7, occlusion_tol=0.0))
    assert (strict[0] >= 0).sum() < (three_views[0] >= 0).sum()
    loose = _check_views(gpu_ctx, three["v"], three["t"], ROWS, COLS, three["K4"], three["P"], _opt(min_cos=0.0, occlusion_tol=0.9))
    assert (loose[0] >= 0).sum() > (three_views[0] >= 0).sum()


# ---- 2: large boxes ---------------------------------------------------------------------------------------------------------------
def test_a_triangle_over_the_whole_image(gpu_ctx):
    """One triangle covers all 6 144 pixels (a box far above the 64 pixels a lane walks alone), 300 small ones lie behind it: every
    pixel holds the large triangle's 1 / 2 and nothing behind it is labelled.  Without it the small ones are."""
    v, t = TC.big_triangle_scene(ROWS, COLS)
    K4, P = TC.front_camera(ROWS, COLS, 60.0)
    label, score, buffers = _check_views(gpu_ctx, v, t, ROWS, COLS, K4, P)
    assert np.all(buffers.view(F) == F(0.5)) and np.all(label == -1)
    label, _, buffers = _check_views(gpu_ctx, v, t[1:], ROWS, COLS, K4, P)
    assert (label == 0).sum() > 100 and 0 < (buffers > 0).mean() < 0.5
    # a second view from behind the large triangle, close to the small ones: boxes of 1 to some hundred pixels next to each other
    K2, P2 = np.tile(K4, (2, 1)), np.tile(P, (2, 1))
    P2[1, 11] = -2.5
    label, _, _ = _check_views(gpu_ctx, v, t[::-1], ROWS, COLS, K2, P2)
    assert (label == 1).sum() > 20 and not (label == 0).any()
    _check_bake(gpu_ctx, v, None, t[::-1], label, TC.noise_images(2, ROWS, COLS, 3), K2, P2, 9, 5)


def test_boxes_at_the_lane_limit(gpu_ctx):
    v, t = TC.lane_limit_scene()
    K4, P = TC.front_camera(ROWS, COLS, 64.0)
    label, _, buffers = _check_views(gpu_ctx, v, t, ROWS, COLS, K4, P)
    assert np.all(label == 0) and 300 < (buffers > 0).sum() < 500


# ---- 3: edge cases ----------------------------------------------------------------------------------------------------------------
def test_a_triangle_through_the_camera_plane(gpu_ctx):
    """It is skipped: the buffer and the other labels are those of the mesh without it."""
    fv, ft = far_grid()
    v = np.concatenate([fv, np.array([[-1, -1, 2], [1, -1, 2], [0, 1, -1], [0, 1, 0]], F)])
    t = np.concatenate([ft, np.array([[0, 2, 1], [0, 3, 1]], np.int32) + len(fv)])
    K4, P = TC.front_camera(ROWS, COLS, 60.0)
    label, score, buffers = _check_views(gpu_ctx, v, t, ROWS, COLS, K4, P)
    plain = _check_views(gpu_ctx, fv, ft, ROWS, COLS, K4, P)
    assert np.all(label[32:] == -1) and np.all(label[:32] == 0) and _same(buffers, plain[2])
    _check_bake(gpu_ctx, v, None, t, label, TC.noise_images(1, ROWS, COLS, 1), K4, P, 6, 4)


@pytest.mark.parametrize("colours", [False, True], ids=["plain", "rgb"])
def test_a_mesh_behind_the_camera(gpu_ctx, three, colours):
    K4, P = TC.front_camera(ROWS, COLS, 60.0)
    v = three["v"] - F([0, 0, 5])
    label, score, buffers = _check_views(gpu_ctx, v, three["t"], ROWS, COLS, K4, P)
    assert np.all(label == -1) and not score.any() and not buffers.any()
    atlas, _ = _check_bake(gpu_ctx, v, three["rgb"] if colours else None, three["t"], label, TC.noise_images(1, ROWS, COLS, 3), K4, P, 5, 48)
    assert np.all(atlas == 128) if not colours else len(np.unique(atlas)) > 100


def test_no_triangle(gpu_ctx, three):
    none = np.zeros((0, 3), np.int32)
    label, score, buffers = _check_views(gpu_ctx, three["v"], none, ROWS, COLS, three["K4"], three["P"])
    assert len(label) == 0 and len(score) == 0 and buffers.shape == (4, ROWS, COLS) and not buffers.any()
    atlas, uv = _check_bake(gpu_ctx, three["v"], three["rgb"], none, label, TC.noise_images(4, ROWS, COLS, 1), three["K4"], three["P"], 8, 3)
    assert atlas.shape == (0, 24, 3) and uv.shape == (0, 3, 2)
    out = E.mesh_texture(np.zeros((0, 3), F), None, none, TC.noise_images(4, ROWS, COLS, 1), three["K4"], three["P"], ctx=gpu_ctx)
    assert out[0].shape == (0, 4, 3) and len(out[2]) == 0


def test_64_views_of_8_by_8(gpu_ctx, three):
    K4, P = TC.arc_views(64, 8, 8, (1.0, 0.9, 0.8), 4.0, 8.0, span_deg=300.0)
    label, _, buffers = _check_views(gpu_ctx, three["v"], three["t"], 8, 8, K4, P)
    assert len(np.unique(label)) > 32 and buffers.shape == (64, 8, 8)
    _check_bake(gpu_ctx, three["v"], three["rgb"], three["t"], label, TC.noise_images(64, 8, 8, 3), K4, P, 4, 48)


def test_mesh_texture_derives_the_chart_size(gpu_ctx):
    fv, ft = far_grid()
    K4, P = TC.front_camera(ROWS, COLS, 60.0)
    images = TC.noise_images(1, ROWS, COLS, 3)
    atlas, uv, label, score = E.mesh_texture(fv, None, ft, images, K4, P, ctx=gpu_ctx)
    assert np.all(label == 0) and np.all(score == F(84.375))
    assert atlas.shape == (4 * 13, 4 * 13, 3)                         # sqrt(2 * 84.375) = 12.99 -> 13 texels; 16 squares, 4 per row
    ref = X.texture_bake(fv, None, ft, label, images, K4, P, X.auto_texels(label, score), E.mesh.default_atlas_width(len(ft)))
    assert _same(atlas, ref[0]) and _same(uv, ref[1])
    assert E.mesh_texture(fv, None, ft, images, K4, P, texels=6, atlas_width=16, ctx=gpu_ctx)[0].shape == (6, 96, 3)


# ---- 4: rejections ----------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(gpu_ctx, three):
    v, rgb, t, K4, P = three["v"], three["rgb"], three["t"], three["K4"], three["P"]
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    label = np.full(len(t), 7, np.int32); score = np.full(len(t), 7.0, F); buffers = np.full((4, ROWS, COLS), 7, np.uint32)

    def views(vertices=v, tri=t, n=4, rows=ROWS, cols=COLS, K=K4, poses=P, o=None):
        return L.esfm_mesh_texture_views(gpu_ctx.handle, len(vertices), len(tri), p(vertices), p(tri), n, rows, cols, p(K), p(poses), C.byref(o or _opt()),
                                         p(label), p(score), p(buffers))
    bad_v = v.copy(); bad_v[100, 1] = np.nan
    bad_t = t.copy(); bad_t[17, 1] = len(v)
    bad_K = K4.copy(); bad_K[2, 0] = 0
    bad_P = P.copy(); bad_P[3, 5] = np.inf
    for kw in (dict(vertices=bad_v), dict(tri=bad_t), dict(n=0), dict(n=65), dict(rows=1), dict(cols=1), dict(K=bad_K), dict(poses=bad_P),
               dict(o=_opt(min_cos=1.0)), dict(o=_opt(min_cos=-0.5)), dict(o=_opt(occlusion_tol=1.0)), dict(o=_opt(occlusion_tol=float("nan")))):
        assert views(**kw) == -1, kw
    assert np.all(label == 7) and np.all(score == 7.0) and np.all(buffers == 7)
    assert views() == 0 and label.max() == 3 and not np.all(buffers == 7)

    images = TC.noise_images(4, ROWS, COLS, 3)
    lab = np.where(label == 7, -1, label).astype(np.int32)
    atlas = np.full((63 * 4, 37 * 4, 3), 7, np.uint8); uv = np.full((len(t), 3, 2), 7.0, F)
    need = C.c_int32(5)

    def bake(vertices=v, tri=t, lab=lab, n=4, ch=3, S_=4, A=37, cap=63 * 4, K=K4):
        return L.esfm_mesh_texture_bake(gpu_ctx.handle, len(vertices), len(tri), p(vertices), p(rgb), p(tri), p(lab), n, ROWS, COLS, ch, p(images), p(K), p(P),
                                        S_, A, cap, p(atlas), p(uv), C.byref(need))
    high = lab.copy(); high[5] = 4
    low = lab.copy(); low[9] = -2
    for kw in (dict(vertices=bad_v), dict(tri=bad_t), dict(n=0), dict(n=65), dict(S_=3), dict(S_=65), dict(A=0), dict(A=4097), dict(A=1, S_=8), dict(lab=high),
               dict(lab=low), dict(ch=2), dict(K=bad_K), dict(cap=-1)):
        assert bake(**kw) == -1 and need.value == 5, kw
    # an atlas buffer too small: the needed rows, nothing else
    assert bake(cap=63 * 4 - 1) == -1 and need.value == 63 * 4 and "needs 252 rows" in L.esfm_last_error().decode()
    assert np.all(atlas == 7) and np.all(uv == 7.0)
    with pytest.raises(E.EsfmError):
        E.mesh_texture_bake(v, rgb, t, high, images, K4, P, 4, 37, gpu_ctx)
    assert bake() == 0 and need.value == 63 * 4
    ref = X.texture_bake(v, rgb, t, lab, images, K4, P, 4, 37)
    assert _same(atlas, ref[0]) and _same(uv, ref[1])


# ---- 5: the chain on the synthetic scene ------------------------------------------------------------------------------------------
def test_chain_on_synthetic_scene(gpu_ctx):
    """The GPU's cleaned and simplified scene mesh (that of tests/test_mesh_simplify_gpu.py; the fixture of the CPU test holds the same
    bits), textured from the scene's five views: the restatement's result bit for bit, and the two scene figures."""
    scene = S.make_scene()
    nb, rng, _ = T.chain_plan(scene, M)
    o = E.default_mvs_options()
    o.num_planes = 48
    depth, _ = E.mvs_depth_maps(scene["images"], scene["K4"], scene["poses"], nb, rng, o, gpu_ctx)
    _, _, index = E.mvs_fuse(scene["images"], scene["K4"], scene["poses"], nb, depth, o, gpu_ctx, return_index=True)
    origin, h, dims = T.CHAIN_GRID
    v, _, rgb, t = E.mvs_mesh(scene["images"], scene["K4"], scene["poses"], E.masked_depth(depth, index), E.tsdf_grid(origin, h, dims), None, gpu_ctx)
    cv, _, crgb, ct = E.mesh_clean(v, rgb, t, None, gpu_ctx)
    sv, _, srgb, st = E.mesh_simplify(cv, crgb, ct, F(2 * 0.04), origin, None, gpu_ctx)
    assert all(_same(a, b) for a, b in zip((sv, srgb, st), chain_mesh()))
    label, score, _ = _check_views(gpu_ctx, sv, st, S.ROWS, S.COLS, scene["K4"], scene["poses"])
    atlas, uv, label2, score2 = E.mesh_texture(sv, srgb, st, scene["images"], scene["K4"], scene["poses"], ctx=gpu_ctx)
    assert _same(label, label2) and _same(score, score2) and atlas.shape == (128, 128, 3)
    _check_bake(gpu_ctx, sv, srgb, st, label, scene["images"], scene["K4"], scene["poses"], 4, 32)
    check_chain(sv, srgb, st, label, score, atlas, 4, 32, scene)
