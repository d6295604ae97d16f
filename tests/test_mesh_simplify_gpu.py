"""Mesh simplification on the GPU against tests/simplify_ref.py: the three spheres over cell sizes, colours, placements and maps,
the 40^3 sphere, a long strip with unequal and with one single cell run, degenerate meshes, rejections, and the synthetic-scene
chain.  Outputs are compared as bit patterns: there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import easysfm_amd as E
import mesh_clean_cases as K
import mvs_ref as M
import mvs_scene as S
import simplify_ref as Q
import tsdf_ref as T

pytestmark = pytest.mark.gpu
F = np.float32

# The cleaned chain mesh of tests/test_mesh_clean_gpu.py (12 978 vertices, 24 792 triangles; median relative depth error 0.001450,
# 0.9778 within 1 %), simplified by tests/simplify_ref.py at cell = 2 x 0.04 from the grid origin, computed on the CPU chain mesh
# (tests/mvs_ref.py depth maps, tests/merge_ref.py mask, tests/tsdf_ref.py, tests/mesh_clean_ref.py): 1 138 vertices and 2 000
# triangles stay; chain_quality of the simplified vertices (871 of them selected): median relative depth error 0.001414, 0.9736
# within 1 %.  The GPU gives identical bits, so the margins only leave room for a later change of defaults.
REF_CHAIN_KEPT = (1138, 2000)
REF_MEDIAN_REL_DEPTH_ERROR = 0.001414
REF_SHARE_WITHIN_1_PERCENT = 0.9736
MAX_MEDIAN_REL_DEPTH_ERROR = 1.5 * REF_MEDIAN_REL_DEPTH_ERROR
MIN_SHARE_WITHIN_1_PERCENT = REF_SHARE_WITHIN_1_PERCENT - 0.05

NAMES = ("vertices", "normals", "rgb", "triangles", "vertex_map", "triangle_map")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_mesh(got, ref):
    return all((g is None and r is None) or (g is not None and r is not None and _same(g, r)) for g, r in zip(got, ref))


def _opt(**kw):
    o = E.default_mesh_simplify_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _check(gpu_ctx, v, rgb, t, cell, origin, use_quadric=1, maps=True):
    """The GPU's mesh against the restatement's, twice for identical bytes; maps=False also runs the call without the maps."""
    o = _opt(use_quadric=use_quadric)
    got = E.mesh_simplify(v, rgb, t, cell, origin, o, gpu_ctx, return_maps=True)
    ref = Q.simplify(v, rgb, t, cell, origin, Q.options(o.regularisation, use_quadric))
    assert len(got[0]) == len(ref[0]) and len(got[3]) == len(ref[3]), (len(got[0]), len(ref[0]), len(got[3]), len(ref[3]))
    for name, g, r in zip(NAMES, got, ref):
        assert (g is None and r is None) or _same(g, r), (name, np.count_nonzero(_bits(g) != _bits(r)))
    assert _same_mesh(E.mesh_simplify(v, rgb, t, cell, origin, o, gpu_ctx, return_maps=True), got)      # twice: identical bytes
    if not maps:
        assert _same_mesh(E.mesh_simplify(v, rgb, t, cell, origin, o, gpu_ctx), got[:4])                # the maps are optional
    return got


@pytest.fixture(scope="module")
def three():
    return K.three_spheres()[:4]


@pytest.fixture(scope="module")
def sphere40():
    f, w, _, _ = T.sphere_volume((40, 40, 40), 0.1)
    v, _, _, t = T.extract(f, w, None, (0, 0, 0), 0.1)
    return v, t


# ---- 1: three spheres -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maps", [False, True], ids=["nomaps", "maps"])
@pytest.mark.parametrize("use_quadric", [0, 1], ids=["mean", "quadric"])
@pytest.mark.parametrize("colours", [False, True], ids=["plain", "rgb"])
@pytest.mark.parametrize("cells", [1.5, 3.0])
def test_three_spheres_bit_parity(gpu_ctx, three, cells, colours, use_quadric, maps):
    v, _, rgb, t = three
    assert (len(v), len(t)) == (2310, 4608)
    got = _check(gpu_ctx, v, rgb if colours else None, t, F(cells * K.THREE_H), (0, 0, 0), use_quadric, maps)
    assert 0 < len(got[3]) < len(t) and 0 < len(got[0]) < len(v) and (got[2] is not None) == colours
    assert got[3].min() == 0 and got[3].max() == len(got[0]) - 1 and np.all(np.diff(got[5]) > 0)
    assert np.array_equal(got[4] >= 0, np.isin(got[4], got[3]))     # a vertex has a new index iff its cell is in a kept triangle


# ---- 2: the 40^3 sphere ---------------------------------------------------------------------------------------------------------
def test_sphere_40_bit_parity(gpu_ctx, sphere40):
    v, t = sphere40
    assert (len(v), len(t)) == (11684, 23364)
    got = _check(gpu_ctx, v, None, t, F(0.2), (0, 0, 0))
    assert (len(got[0]), len(got[3])) == (872, 1740)
    assert T.mesh_topology(got[3])[:2] == (0, 0)


# ---- 3: a triangle strip on a line ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def strip():
    t = K.strip(70001, "random", seed=9)
    v = np.zeros((70001, 3), F)
    v[:, 0] = np.arange(70001)
    return v, t


def test_strip_unequal_runs(gpu_ctx, strip):
    """Vertex i at x = i, cell 7.3: 9 590 cells of 7 or 8 vertices over 274 workgroups, their triangles anywhere along the line."""
    v, t = strip
    got = _check(gpu_ctx, v, None, t, F(7.3), (-0.5, -0.5, -0.5))
    assert len(got[0]) > 9000 and len(got[3]) > 60000


def test_strip_one_cell(gpu_ctx, strip):
    v, t = strip
    got = _check(gpu_ctx, v, None, t, F(1e5), (-0.5, -0.5, -0.5))
    assert len(got[0]) == 0 and len(got[3]) == 0 and np.all(got[4] == -1)


# Cell 1 from the origin.  Vertices 1 and 6 share a cell, so do 2 and 8; 7 is in no surviving triangle; 9, 10, 11 are collinear.
# Triangles 0, 3, 6 lie on the same three cells with orientations even, odd, odd: 3 stays.  1, 7, 8 likewise (odd, even, even): 7
# stays.  2 and 9 are a flap, one of each: neither stays.  4 and 5 name a cell twice.  10 has no area and three cells: it stays.
SMALL_P = np.array([[0.1, 0.1, 0.1], [1.2, 0.1, 0.2], [0.2, 1.3, 0.1], [1.1, 1.2, 1.3], [2.5, 0.1, 0.1], [3.5, 0.1, 0.1], [1.3, 0.2, 0.1],
                    [5.5, 5.5, 5.5], [0.3, 1.1, 0.3], [0.5, 2.5, 0.5], [1.5, 2.5, 0.5], [2.5, 2.5, 0.5]], F)
SMALL_T = np.array([[0, 1, 2], [2, 1, 3], [1, 4, 5], [0, 2, 6], [3, 3, 4], [7, 7, 7], [8, 6, 0], [3, 1, 2], [2, 3, 1], [5, 4, 6], [9, 10, 11]],
                   np.int32)
SMALL_KEPT = [3, 7, 10]


# ---- 4: edge cases ----------------------------------------------------------------------------------------------------------------
def test_degenerate_meshes(gpu_ctx, three):
    v, _, rgb, t = three
    # one cell for everything; every vertex alone
    none = _check(gpu_ctx, v, rgb, t, F(100.0), (-1, -1, -1))
    assert [len(a) for a in none[:4]] == [0, 0, 0, 0] and np.all(none[4] == -1) and len(none[5]) == 0
    alone = _check(gpu_ctx, v, rgb, t, F(1e-4), (0, 0, 0))
    assert len(alone[3]) == len(t) and np.abs(alone[0][alone[4]].astype(np.float64) - v).max() <= 1e-5 * 1e-4
    # no triangle at all
    empty = E.mesh_simplify(v, None, np.zeros((0, 3), np.int32), 0.1, None, None, gpu_ctx, return_maps=True)
    assert [len(a) for a in (empty[0], empty[1], empty[3], empty[5])] == [0] * 4 and np.all(empty[4] == -1)
    for q in (0, 1):
        got = _check(gpu_ctx, SMALL_P, None, SMALL_T, F(1.0), (0, 0, 0), q)
        assert got[5].tolist() == SMALL_KEPT
    # origin=None: the per-axis minimum of the vertices
    assert _same_mesh(E.mesh_simplify(v, None, t, 0.15, None, None, gpu_ctx), E.mesh_simplify(v, None, t, 0.15, v.min(axis=0), None, gpu_ctx))


def test_rejections_write_nothing(gpu_ctx, three):
    v, _, rgb, t = three
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    out_v = np.full_like(v, 7.0); out_n = np.full_like(v, 7.0); out_c = np.full_like(rgb, 7); out_t = np.full_like(t, 7)
    vmap = np.full(len(v), 7, np.int32); tmap = np.full(len(t), 7, np.int32)
    nv, nt = C.c_int32(5), C.c_int32(5)

    def call(cell=0.15, origin=(0, 0, 0), o=None, in_rgb=rgb, vertices=v):
        org = np.asarray(origin, F)
        return L.esfm_mesh_simplify(gpu_ctx.handle, len(v), len(t), p(vertices), p(in_rgb), p(t), p(org), C.c_float(cell), C.byref(o or _opt()),
                                    p(out_v), p(out_n), p(out_c), p(out_t), p(vmap), p(tmap), C.byref(nv), C.byref(nt))
    moved = v.copy(); moved[100, 1] = np.nan
    for kw in (dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(origin=(0.5, 0, 0)),
               dict(origin=(0, float("inf"), 0)), dict(in_rgb=None), dict(o=_opt(regularisation=0.0)), dict(o=_opt(regularisation=1.5)),
               dict(o=_opt(use_quadric=2)), dict(vertices=moved), dict(cell=1e-7)):
        assert call(**kw) == -1, kw
        with pytest.raises(Q.Rejected):
            Q.simplify(kw.get("vertices", v), kw.get("in_rgb", rgb), t, kw.get("cell", 0.15), kw.get("origin", (0, 0, 0)),
                       Q.options(kw["o"].regularisation, kw["o"].use_quadric) if "o" in kw else None, want_rgb=True)
    assert (nv.value, nt.value) == (5, 5)
    assert np.all(out_v == 7.0) and np.all(out_n == 7.0) and np.all(out_c == 7) and np.all(out_t == 7) and np.all(vmap == 7) and np.all(tmap == 7)
    assert call() == 0 and nv.value > 0 and nt.value > 0


def test_more_cells_than_a_grouping_key_holds(gpu_ctx):
    """2^21 + 1 vertices on a 2049 x 1024 lattice with a cell of their own each: ESFM_ERR_UNSUPPORTED, nothing written; one vertex
    fewer is served."""
    n = 2 ** 21 + 1
    i = np.arange(n)
    v = np.stack([(i // 1024).astype(F) + F(0.5), (i % 1024).astype(F) + F(0.5), np.full(n, 0.5, F)], 1)
    t = np.array([[0, 1, 1024], [n - 1, 5, 7]], np.int32)
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    out_v = np.full_like(v, 7.0); out_t = np.full_like(t, 7); vmap = np.full(n, 7, np.int32)
    nv, nt = C.c_int32(5), C.c_int32(5)
    origin = np.zeros(3, F)

    def call(count):
        return L.esfm_mesh_simplify(gpu_ctx.handle, count, 1, p(v), None, p(t), p(origin), C.c_float(1.0), C.byref(_opt()), p(out_v), None, None,
                                    p(out_t), p(vmap), None, C.byref(nv), C.byref(nt))
    assert call(n) == -5 and "2^21" in L.esfm_last_error().decode()                      # ESFM_ERR_UNSUPPORTED
    assert (nv.value, nt.value) == (5, 5) and np.all(out_v == 7.0) and np.all(out_t == 7) and np.all(vmap == 7)
    with pytest.raises(Q.Unsupported):
        Q.simplify(v, None, t[:1], 1.0, origin)
    assert call(n - 1) == 0 and (nv.value, nt.value) == (3, 1)
    assert np.array_equal(out_t[0], [0, 1, 2]) and np.array_equal(np.nonzero(vmap[:n - 1] >= 0)[0], [0, 1, 1024])


# ---- 5: the chain on the synthetic scene ----------------------------------------------------------------------------------------
def test_chain_on_synthetic_scene(gpu_ctx):
    """The cleaned chain mesh of tests/test_mesh_clean_gpu.py, simplified at two voxels per cell from the grid origin: the
    restatement's result on the same mesh, bit for bit, and it still lies on the true surface."""
    scene = S.make_scene()
    nb, rng, _ = T.chain_plan(scene, M)
    o = E.default_mvs_options()
    o.num_planes = 48
    depth, _ = E.mvs_depth_maps(scene["images"], scene["K4"], scene["poses"], nb, rng, o, gpu_ctx)
    _, _, index = E.mvs_fuse(scene["images"], scene["K4"], scene["poses"], nb, depth, o, gpu_ctx, return_index=True)
    origin, h, dims = T.CHAIN_GRID
    v, _, rgb, t = E.mvs_mesh(scene["images"], scene["K4"], scene["poses"], E.masked_depth(depth, index), E.tsdf_grid(origin, h, dims), None, gpu_ctx)
    cv, _, crgb, ct = E.mesh_clean(v, rgb, t, None, gpu_ctx)
    got = _check(gpu_ctx, cv, crgb, ct, F(2 * 0.04), origin)
    n, median, share = T.chain_quality(scene, S, got[0])
    print(f"chain: {len(cv)} vertices, {len(ct)} triangles -> {len(got[0])} vertices, {len(got[3])} triangles; {n} vertices away from "
          f"edges: median relative depth error {median:.6f}, {share:.4f} within 1 %")
    assert (len(got[0]), len(got[3])) == REF_CHAIN_KEPT
    assert n > 500
    assert median <= MAX_MEDIAN_REL_DEPTH_ERROR and share >= MIN_SHARE_WITHIN_1_PERCENT
