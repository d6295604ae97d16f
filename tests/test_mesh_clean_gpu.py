"""Mesh clean-up on the GPU against tests/mesh_clean_ref.py: the labelling on meshes that make the union-find hook in every
direction, the whole clean-up over its options, and the synthetic-scene chain.  Outputs are compared as bit patterns: there is
no tolerance."""
import numpy as np
import pytest

import easysfm_amd as E
import mesh_clean_cases as K
import mesh_clean_ref as R
import mvs_ref as M
import mvs_scene as S
import tsdf_ref as T

pytestmark = pytest.mark.gpu
F = np.float32

# The chain of tests/test_tsdf_gpu.py test_chain_on_synthetic_scene (13 115 vertices, 24 926 triangles, 18 components), cleaned
# with the defaults by tests/mesh_clean_ref.py: 3 components, 12 978 vertices and 24 792 triangles stay; chain_quality of the
# cleaned vertices (10 296 of them selected): median relative depth error 0.001450, 0.9778 within 1 % (0.001487 and 0.9774 before
# the clean-up).  The GPU gives identical bits, so the margins only leave room for a later change of defaults.
REF_CHAIN_KEPT = (3, 12978, 24792)
REF_MEDIAN_REL_DEPTH_ERROR = 0.001450
REF_SHARE_WITHIN_1_PERCENT = 0.9778
MAX_MEDIAN_REL_DEPTH_ERROR = 1.5 * REF_MEDIAN_REL_DEPTH_ERROR
MIN_SHARE_WITHIN_1_PERCENT = REF_SHARE_WITHIN_1_PERCENT - 0.05


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_mesh(got, ref):
    return all((g is None and r is None) or (g is not None and r is not None and _same(g, r)) for g, r in zip(got, ref))


def _opt(**kw):
    o = E.default_mesh_clean_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.fixture(scope="module")
def three():
    return K.three_spheres()[:4]


# ---- 1: the labelling -----------------------------------------------------------------------------------------------------------
def _component_case(name):
    """(triangles, n_vertices, expected labels or None = the restatement's)."""
    if name == "three_spheres":
        v, _, _, t = K.three_spheres(colours=False)[:4]
        return t, len(v), None
    if name == "one_triangle":
        return np.array([[2, 0, 1]], np.int32), 3, np.zeros(3, np.int32)
    if name == "no_triangle":
        return np.zeros((0, 3), np.int32), 5, np.arange(5, dtype=np.int32)
    if name == "disjoint":                                         # 20 000 triangles of their own and 1 000 vertices in none
        perm = np.random.default_rng(6).permutation(61000).astype(np.int32)
        return np.ascontiguousarray(perm[:60000].reshape(-1, 3)), 61000, None
    kind, _, variant = name.partition("_")
    assert kind == "strip"
    numbering = "ascending" if variant == "repeat" else variant
    return K.strip(70001, numbering, seed=9, repeat_index=variant == "repeat"), 70001, np.zeros(70001, np.int32)


@pytest.mark.parametrize("name", ["three_spheres", "one_triangle", "no_triangle", "disjoint", "strip_ascending", "strip_descending",
                                  "strip_random", "strip_repeat"])
def test_components_bit_parity(gpu_ctx, name):
    t, n_vertices, expected = _component_case(name)
    labels, count, n = E.mesh_components(t, n_vertices, gpu_ctx)
    r_labels, r_count, r_n = R.components(t, n_vertices)
    if expected is not None:
        assert np.array_equal(r_labels, expected)
    assert n == r_n and _same(labels, r_labels), np.count_nonzero(labels != r_labels)
    assert _same(count, r_count) and count.sum() == len(t)
    if name == "disjoint":
        assert n == 21000 and np.count_nonzero(count == 1) == 20000
    if name.startswith("strip"):
        assert n == 1 and count[0] == 69999 and len(t) // 256 > 200       # one component over many workgroups
    again = E.mesh_components(t, n_vertices, gpu_ctx)
    assert _same(again[0], labels) and _same(again[1], count) and again[2] == n


# ---- 2: the clean-up ------------------------------------------------------------------------------------------------------------
def _ref_opt(o):
    return R.options(o.min_component_triangles, o.min_component_permille, o.smooth_iterations, o.smooth_lambda, o.smooth_mu, o.pin_boundary)


def _check_clean(gpu_ctx, v, rgb, t, o):
    got = E.mesh_clean(v, rgb, t, o, gpu_ctx, return_maps=True)
    ref = R.clean(v, rgb, t, _ref_opt(o))
    assert len(got[0]) == len(ref[0]) and len(got[3]) == len(ref[3]), (len(got[0]), len(ref[0]), len(got[3]), len(ref[3]))
    for name, g, r in zip(("vertices", "normals", "rgb", "triangles", "vertex_map", "triangle_map"), got, ref):
        assert (g is None and r is None) or _same(g, r), (name, np.count_nonzero(_bits(g) != _bits(r)))
    assert _same_mesh(E.mesh_clean(v, rgb, t, o, gpu_ctx, return_maps=True), got)           # twice: identical bytes
    assert _same_mesh(E.mesh_clean(v, rgb, t, o, gpu_ctx), got[:4])                          # the maps are optional
    return got


@pytest.mark.parametrize("iterations", [0, 1, 5])
@pytest.mark.parametrize("pin", [0, 1])
@pytest.mark.parametrize("colours", [False, True], ids=["plain", "rgb"])
def test_clean_three_spheres_bit_parity(gpu_ctx, three, iterations, pin, colours):
    v, _, rgb, t = three
    got = _check_clean(gpu_ctx, v, rgb if colours else None, t, _opt(smooth_iterations=iterations, pin_boundary=pin))
    assert len(got[3]) == sum(K.THREE_COUNTS) and (got[2] is not None) == colours
    assert np.allclose(np.linalg.norm(got[1], axis=1), 1, atol=1e-6)
    assert np.array_equal(_bits(got[0]), _bits(v)) == (iterations == 0)


def test_clean_opened_sphere_bit_parity(gpu_ctx):
    v, _, _, t = K.opened_sphere()
    keep_all = dict(min_component_triangles=1, min_component_permille=0)
    held = _check_clean(gpu_ctx, v, None, t, _opt(pin_boundary=1, **keep_all))
    free = _check_clean(gpu_ctx, v, None, t, _opt(pin_boundary=0, **keep_all))
    pinned = R.adjacency(t, len(v))[2]
    assert pinned.any() and np.array_equal(_bits(held[0][pinned]), _bits(v[pinned])) and np.all(np.any(free[0][pinned] != v[pinned], axis=1))


@pytest.mark.parametrize("min_triangles,permille,kept", [(1, 0, sum(K.THREE_COUNTS)), (300, 0, 4352), (300, 200, 3708), (1, 1000, 3708), (4000, 0, 0)])
def test_clean_filters(gpu_ctx, three, min_triangles, permille, kept):
    v, _, rgb, t = three
    got = _check_clean(gpu_ctx, v, rgb, t, _opt(min_component_triangles=min_triangles, min_component_permille=permille, smooth_iterations=2))
    assert len(got[3]) == kept and (kept > 0 or all(len(a) == 0 for a in got))


def test_clean_degenerate_meshes(gpu_ctx):
    """No triangle at all; unreferenced vertices; a triangle that repeats an index; a triangle that is one vertex three times."""
    v = np.random.default_rng(1).normal(size=(9, 3)).astype(F)
    none = E.mesh_clean(v, None, np.zeros((0, 3), np.int32), None, gpu_ctx, return_maps=True)
    assert [len(a) for a in (none[0], none[1], none[3], none[4], none[5])] == [0] * 5
    t = np.array([[0, 1, 2], [2, 1, 3], [3, 3, 4], [7, 7, 7], [5, 8, 5]], np.int32)
    for pin in (0, 1):
        got = _check_clean(gpu_ctx, v, None, t, _opt(min_component_triangles=1, min_component_permille=0, smooth_iterations=3, pin_boundary=pin))
        assert len(got[0]) == 8 and len(got[3]) == 5                          # vertex 6 is in no triangle


# ---- 3: the chain on the synthetic scene ----------------------------------------------------------------------------------------
def test_chain_on_synthetic_scene(gpu_ctx):
    """The mesh of tests/test_tsdf_gpu.py's chain (GPU sweep, the fusion's mask, the fused mesh call), cleaned with the defaults:
    the restatement's result on the same mesh, bit for bit, and it lies on the true surface."""
    scene = S.make_scene()
    nb, rng, _ = T.chain_plan(scene, M)
    o = E.default_mvs_options()
    o.num_planes = 48
    depth, _ = E.mvs_depth_maps(scene["images"], scene["K4"], scene["poses"], nb, rng, o, gpu_ctx)
    _, _, index = E.mvs_fuse(scene["images"], scene["K4"], scene["poses"], nb, depth, o, gpu_ctx, return_index=True)
    origin, h, dims = T.CHAIN_GRID
    v, _, rgb, t = E.mvs_mesh(scene["images"], scene["K4"], scene["poses"], E.masked_depth(depth, index), E.tsdf_grid(origin, h, dims), None, gpu_ctx)
    assert E.mesh_components(t, len(v), gpu_ctx)[2] == 18
    got = E.mesh_clean(v, rgb, t, None, gpu_ctx, return_maps=True)
    ref = R.clean(v, rgb, t)
    assert (len(got[0]), len(got[3])) == (len(ref[0]), len(ref[3]))
    assert _same_mesh(got, ref)
    kept = E.mesh_components(got[3], len(got[0]), gpu_ctx)[2]
    n, median, share = T.chain_quality(scene, S, got[0])
    n0, median0, share0 = T.chain_quality(scene, S, v)
    print(f"chain: {kept} of 18 components, {len(got[0])} vertices, {len(got[3])} triangles; {n} vertices away from edges: median relative "
          f"depth error {median:.6f} (before {median0:.6f}), {share:.4f} within 1 % (before {share0:.4f})")
    assert (kept, len(got[0]), len(got[3])) == REF_CHAIN_KEPT
    assert n > 5000
    assert median <= MAX_MEDIAN_REL_DEPTH_ERROR and share >= MIN_SHARE_WITHIN_1_PERCENT
