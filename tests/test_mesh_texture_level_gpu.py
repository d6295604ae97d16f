"""Seam levelling on the GPU against tests/level_ref.py: two flat halves, a fan of labels, degenerate input, striped grids under
grey and BGR noise, the chain mesh under the scene's images and under five exposures, and a plane of 260 x 260 vertices (more than
65 536 nodes: three levels of tree_sum, scans over many blocks).  Offsets, samples, stats and the levelled atlas are compared as bit
patterns: there is no tolerance, and every case runs twice for identical bytes."""
import ctypes as C

import numpy as np
import pytest

import easysfm_amd as E
import level_cases as LC
import level_ref as L
import mvs_scene as S
import texture_cases as TC
import texture_ref as X

pytestmark = pytest.mark.gpu
F = np.float32


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _opt(**kw):
    o = E.default_mesh_texture_level_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _stats(st):
    return dict(nodes=st.nodes, seam_vertices=st.seam_vertices, iterations=st.iterations, converged=st.converged)


def _check_level(gpu_ctx, v, rgb, t, label, images, K4, P, S_=4, A=None, **kw):
    """The GPU's offsets, samples, stats and levelled atlas against the restatement's, twice for identical bytes.  Returns the GPU's
    (offsets, samples, stats dict, atlas)."""
    o = _opt(**kw)
    ro = L.options(o.lam, o.mu, o.tolerance, o.max_iterations)
    off, smp, st = E.mesh_texture_level(v, t, label, images, K4, P, o, gpu_ctx)
    roff, rsmp, rst = L.texture_level(v, t, label, images, K4, P, ro)
    print(f"level: {len(t)} triangles, gpu {_stats(st)}, restatement {rst}")
    assert _stats(st) == rst
    assert _same(smp, rsmp), np.count_nonzero(smp != rsmp)
    assert _same(off, roff), (np.count_nonzero(off.view(np.uint32) != roff.view(np.uint32)), float(np.abs(off - roff).max()))
    off2, smp2, st2 = E.mesh_texture_level(v, t, label, images, K4, P, o, gpu_ctx)
    assert _same(off, off2) and _same(smp, smp2) and _stats(st2) == rst
    A = A or E.mesh.default_atlas_width(len(t))
    atlas, uv = E.mesh_texture_bake(v, rgb, t, label, images, K4, P, S_, A, gpu_ctx, offsets=off)
    ratlas, ruv = L.texture_bake(v, rgb, t, label, images, K4, P, S_, A, offsets=roff)
    assert _same(atlas, ratlas), np.count_nonzero(atlas != ratlas)
    assert _same(uv, ruv)
    assert _same(E.mesh_texture_bake(v, rgb, t, label, images, K4, P, S_, A, gpu_ctx, offsets=off)[0], atlas)
    return off, smp, rst, atlas


# ---- small scenes -----------------------------------------------------------------------------------------------------------------
def test_two_flat_halves(gpu_ctx):
    v, t, label, images, K4, P = LC.two_halves()
    off, smp, st, atlas = _check_level(gpu_ctx, v, None, t, label, images, K4, P, S_=8, tolerance=1e-12)
    assert (st["nodes"], st["seam_vertices"], st["converged"]) == (30, 5, 1)
    nt = L.node_table(v, t, label, images, K4, P)
    assert LC.seam_step(nt, off, smp) < 0.5 and LC.seam_step(nt, np.zeros_like(off), smp) == 40.0
    assert 100 < atlas.mean() < 140 and len(np.unique(atlas)) > 2                   # no longer two flat colours


def test_fan_of_three_and_four_labels(gpu_ctx):
    v, t, label, images, K4, P = LC.fan()
    st = _check_level(gpu_ctx, v, None, t, label, images, K4, P, S_=7, A=3)[2]
    assert (st["nodes"], st["seam_vertices"], st["converged"]) == (28, 9, 1)


def test_degenerate_mix(gpu_ctx):
    v, t, label, images, K4, P = LC.degenerate_mix()
    off, smp, st, _ = _check_level(gpu_ctx, v, None, t, label, images, K4, P, S_=5, A=6)
    part = L.node_table(v, t, label, images, K4, P)["part"]
    assert not part.all() and not off[~part].any() and not smp[~part].any() and off[part].any() and st["converged"] == 1


@pytest.mark.parametrize("channels,n_views", [(1, 2), (3, 3)], ids=["grey", "bgr"])
def test_striped_grid_under_noise(gpu_ctx, channels, n_views):
    v, t, label, images, K4, P = LC.striped(n_views, channels)
    rgb = TC.noise_images(1, len(v), 1, 3, seed=4).reshape(-1, 3)
    off, smp, st, _ = _check_level(gpu_ctx, v, rgb, t, label, images, K4, P, S_=6, A=4)
    assert st["seam_vertices"] == 15 and st["converged"] == 1
    if channels == 1:
        assert np.array_equal(off[..., 0], off[..., 1]) and np.array_equal(off[..., 0], off[..., 2]) and np.array_equal(smp[..., 0], smp[..., 2])
    else:
        assert not np.array_equal(off[..., 0], off[..., 2])
    # a stop by the iteration count, and no stop at all
    st = _check_level(gpu_ctx, v, rgb, t, label, images, K4, P, S_=6, A=4, max_iterations=3)[2]
    assert (st["iterations"], st["converged"]) == (3, 0)
    st = _check_level(gpu_ctx, v, rgb, t, label, images, K4, P, S_=6, A=4, tolerance=0.0, max_iterations=40, lam=1.0, mu=0.01)[2]
    assert st["iterations"] == 40


def test_plane_of_260_by_260_vertices(gpu_ctx):
    """70 720 nodes: 277 block sums per dot product, so tree_sum has three levels; 402 486 corner keys and 804 972 edge keys go through
    the sort and the scans in many blocks.  Twelve iterations keep the restatement within seconds."""
    v, t, label, images, K4, P = LC.plane_grid()
    st = _check_level(gpu_ctx, v, None, t, label, images, K4, P, max_iterations=12)[2]
    assert st["nodes"] == 260 * 260 + 12 * 260 and st["nodes"] > 65536 and st["seam_vertices"] == 12 * 260 and (st["iterations"], st["converged"]) == (12, 0)


# ---- what changes nothing ---------------------------------------------------------------------------------------------------------
def test_no_offsets_and_no_iterations_are_the_plain_bake(gpu_ctx):
    v, t, label, images, K4, P = LC.striped(3, 3)
    plain = E.mesh_texture_bake(v, None, t, label, images, K4, P, 6, 4, gpu_ctx)
    lib = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    atlas = np.zeros_like(plain[0]); uv = np.zeros_like(plain[1]); need = C.c_int32(0)
    assert lib.esfm_mesh_texture_bake_ex(gpu_ctx.handle, len(v), len(t), p(v), None, p(t), p(label), 3, LC.ROWS, LC.COLS, 3, p(images), p(K4), p(P), 6, 4,
                                         atlas.shape[0], p(atlas), p(uv), C.byref(need), None) == 0
    assert _same(atlas, plain[0]) and _same(uv, plain[1]) and _same(plain[0], X.texture_bake(v, None, t, label, images, K4, P, 6, 4)[0])
    off, smp, st = E.mesh_texture_level(v, t, label, images, K4, P, _opt(max_iterations=0), gpu_ctx)
    assert (st.nodes, st.seam_vertices, st.iterations, st.converged) == (40, 15, 0, 0) and not off.any() and smp.any()
    assert _same(E.mesh_texture_bake(v, None, t, label, images, K4, P, 6, 4, gpu_ctx, offsets=off)[0], plain[0])
    # one label everywhere, nothing labelled, no triangle
    for lab in (np.zeros_like(label), np.full_like(label, -1)):
        off, smp, st = E.mesh_texture_level(v, t, lab, images, K4, P, None, gpu_ctx)
        roff, rsmp, rst = L.texture_level(v, t, lab, images, K4, P)
        assert _stats(st) == rst and st.iterations == 0 and st.converged == 1 and not off.any() and _same(smp, rsmp)
    off, smp, st = E.mesh_texture_level(v, t[:0], label[:0], images, K4, P, None, gpu_ctx)
    assert off.shape == (0, 3, 3) and (st.nodes, st.iterations, st.converged) == (0, 0, 1)
    out = E.mesh_texture(v, None, t, images, K4, P, texels=6, atlas_width=4, ctx=gpu_ctx, level=True)
    ref_off = L.texture_level(v, t, out[2], images, K4, P)[0]
    assert _same(out[0], L.texture_bake(v, None, t, out[2], images, K4, P, 6, 4, offsets=ref_off)[0])


def test_rejections_write_nothing(gpu_ctx):
    v, t, label, images, K4, P = LC.striped(2, 1)
    lib = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    offsets = np.full((len(t), 3, 3), 7.0, F); samples = np.full((len(t), 3, 3), 7.0, F)
    stats = E.MeshTextureLevelStats(7, 7, 7, 7)

    def level(vertices=v, tri=t, lab=label, n=2, ch=1, o=None):
        return lib.esfm_mesh_texture_level(gpu_ctx.handle, len(vertices), len(tri), p(vertices), p(tri), p(lab), n, LC.ROWS, LC.COLS, ch, p(images), p(K4), p(P),
                                           C.byref(o or _opt()), p(offsets), p(samples), C.byref(stats))
    bad_v = v.copy(); bad_v[10, 1] = np.nan
    bad_t = t.copy(); bad_t[17, 1] = len(v)
    for kw in (dict(vertices=bad_v), dict(tri=bad_t), dict(lab=label + 1), dict(lab=label - 2), dict(n=0), dict(n=65), dict(ch=2), dict(o=_opt(lam=0.0)),
               dict(o=_opt(lam=float("nan"))), dict(o=_opt(mu=0.0)), dict(o=_opt(mu=float("inf"))), dict(o=_opt(tolerance=1.0)), dict(o=_opt(tolerance=-0.1)),
               dict(o=_opt(max_iterations=-1)), dict(o=_opt(max_iterations=10001))):
        assert level(**kw) == -1, kw
    assert np.all(offsets == 7.0) and np.all(samples == 7.0) and (stats.nodes, stats.seam_vertices, stats.iterations, stats.converged) == (7, 7, 7, 7)
    assert level() == 0 and stats.nodes == 40 and stats.converged == 1 and not np.all(offsets == 7.0)
    atlas = np.full((32, 32, 3), 7, np.uint8); uv = np.full((len(t), 3, 2), 7.0, F); need = C.c_int32(5)
    bad = offsets.copy(); bad[3, 0, 1] = np.inf
    args = (gpu_ctx.handle, len(v), len(t), p(v), None, p(t), p(label), 2, LC.ROWS, LC.COLS, 1, p(images), p(K4), p(P), 8, 4, 32, p(atlas), p(uv), C.byref(need))
    assert lib.esfm_mesh_texture_bake_ex(*args, p(bad)) == -1 and need.value == 5 and np.all(atlas == 7) and np.all(uv == 7.0)
    with pytest.raises(E.EsfmError):
        E.mesh_texture_bake(v, None, t, label, images, K4, P, 8, 4, gpu_ctx, offsets=bad)
    assert lib.esfm_mesh_texture_bake_ex(*args, p(offsets)) == 0 and need.value == 32
    assert _same(atlas, L.texture_bake(v, None, t, label, images, K4, P, 8, 4, offsets=offsets)[0])


# ---- the chain mesh ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(gpu_ctx):
    v, rgb, t = TC.chain_mesh()
    scene = S.make_scene()
    label, score = E.mesh_texture_views(v, t, S.ROWS, S.COLS, scene["K4"], scene["poses"], None, gpu_ctx)
    return dict(v=v, rgb=rgb, t=t, scene=scene, label=label, score=score, K4=scene["K4"], P=scene["poses"])


def test_chain_mesh_scene_images(gpu_ctx, chain):
    c = chain
    images = c["scene"]["images"]
    off, smp, st, levelled = _check_level(gpu_ctx, c["v"], c["rgb"], c["t"], c["label"], images, c["K4"], c["P"], 4, 32)
    assert (st["nodes"], st["seam_vertices"], st["converged"]) == (1916, 493, 1) and st["iterations"] <= 200
    plain, _ = E.mesh_texture_bake(c["v"], c["rgb"], c["t"], c["label"], images, c["K4"], c["P"], 4, 32, gpu_ctx)
    LC.check_level_chain(c["v"], c["rgb"], c["t"], c["label"], c["score"], images, c["K4"], c["P"], plain, levelled, off, smp, c["scene"])
    assert _same(E.mesh_texture(c["v"], c["rgb"], c["t"], images, c["K4"], c["P"], ctx=gpu_ctx, level=True)[0], levelled)
    assert _same(E.mesh_texture(c["v"], c["rgb"], c["t"], images, c["K4"], c["P"], ctx=gpu_ctx)[0], plain)


def test_chain_mesh_exposure_images(gpu_ctx, chain):
    c = chain
    images = LC.exposure_images(c["scene"]["images"])
    off, smp, st, levelled = _check_level(gpu_ctx, c["v"], c["rgb"], c["t"], c["label"], images, c["K4"], c["P"], 4, 32)
    plain, _ = E.mesh_texture_bake(c["v"], c["rgb"], c["t"], c["label"], images, c["K4"], c["P"], 4, 32, gpu_ctx)
    LC.check_level_exposure(c["v"], c["rgb"], c["t"], c["label"], images, c["K4"], c["P"], plain, levelled, off, smp, st)
