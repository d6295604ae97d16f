"""Surface reconstruction on the GPU against tests/tsdf_ref.py: the integration, the extraction on supplied volumes, the
capacities, the fused call and the whole chain on the synthetic scene.  Outputs are compared as bit patterns: there is no
tolerance."""
import ctypes as C

import numpy as np
import pytest

import easysfm_amd as E
import mvs_ref as M
import mvs_scene as S
import tsdf_ref as T

pytestmark = pytest.mark.gpu
F = np.float32

# Accuracy of the mesh on the synthetic scene, over the vertices whose projection into view 2 lies at least 4 px from an
# occlusion edge: the median of |ray depth - own depth| / ray depth and the share within 1 %.  Computed on the CPU from
# tests/mvs_ref.py depth maps (r 3, D 48), masked with tests/merge_ref.py's fuse_index and fed to tests/tsdf_ref.py -- none of
# them is the code under test: 13 115 vertices and 24 926 triangles, 10 284 of the vertices selected, median 0.001487, 0.9774
# within 1 %.  The GPU gives identical bits, so the margins only leave room for a later change of defaults.
REF_MEDIAN_REL_DEPTH_ERROR = 0.001487
REF_SHARE_WITHIN_1_PERCENT = 0.9774
MAX_MEDIAN_REL_DEPTH_ERROR = 1.5 * REF_MEDIAN_REL_DEPTH_ERROR
MIN_SHARE_WITHIN_1_PERCENT = REF_SHARE_WITHIN_1_PERCENT - 0.05


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_mesh(got, ref):
    return all((g is None and r is None) or _same(g, r) for g, r in zip(got, ref))


def _grid(origin, h, dims):
    return E.tsdf_grid(origin, h, dims)


def _opt(trunc=0.0, min_weight=2):
    o = E.default_tsdf_options()
    o.trunc, o.min_weight = trunc, min_weight
    return o


@pytest.fixture(scope="module")
def scene():
    return S.make_scene()


@pytest.fixture(scope="module")
def crops(scene):
    """Three 37 x 53 exact-depth crops (the image's top-left corner, so K4 stays) with a tenth of the depths zeroed, and a
    fourth view without any depth; grey and 3-channel images of them."""
    rng = np.random.default_rng(5)
    views = [0, 2, 4, 1]
    d = scene["depth"][views, :37, :53].astype(F)
    d[rng.random(d.shape) < 0.1] = 0
    d[3] = 0
    grey = np.ascontiguousarray(scene["images"][views, :37, :53])
    bgr = np.stack([grey, 255 - grey, grey // 2 + 17], -1).astype(np.uint8)
    return dict(K4=scene["K4"][views], poses=scene["poses"][views], depth=d, grey=grey, bgr=bgr)


# ---- 1: integration -------------------------------------------------------------------------------------------------------------
# 24 x 20 x 17 at h 0.4 from z = -0.6: the first z layers lie behind the cameras (p2 <= 0), most of the grid projects outside
# the crops, the rest runs through the surface; 2 x 3 x 2 sits on the surface the three crops share.
INTEGRATION_GRIDS = [((-6.5, -5.0, -0.6), 0.4, (24, 20, 17)), ((-2.4, -2.0, 4.3), 0.25, (2, 3, 2))]


@pytest.mark.parametrize("grid", INTEGRATION_GRIDS, ids=["24x20x17", "2x3x2"])
@pytest.mark.parametrize("images", [None, "grey", "bgr"])
@pytest.mark.parametrize("trunc_voxels", [0.0, 2.5])
def test_integrate_bit_parity(gpu_ctx, crops, grid, images, trunc_voxels):
    origin, h, dims = grid
    trunc = float(F(trunc_voxels) * F(h))
    imgs = crops[images] if images else None
    tsdf, weight, rgb = E.tsdf_integrate(imgs, crops["K4"], crops["poses"], crops["depth"], _grid(origin, h, dims), _opt(trunc), gpu_ctx)
    r_tsdf, r_weight, r_rgb = T.integrate(imgs, crops["K4"], crops["poses"], crops["depth"], origin, h, dims, trunc)
    assert _same(weight, r_weight), np.count_nonzero(weight != r_weight)
    assert _same(tsdf, r_tsdf), np.count_nonzero(_bits(tsdf) != _bits(r_tsdf))
    assert (rgb is None and r_rgb is None) or _same(rgb, r_rgb)
    assert weight.max() == 3 and np.any(tsdf < 0) and np.any((tsdf > 0) & (tsdf < 1))
    if dims[2] > 2:
        assert not weight[:2].any() and np.mean(weight == 0) > 0.5           # behind the cameras; outside the crops
    if rgb is not None:
        assert rgb[weight > 0].any() and not rgb[weight == 0].any()


# ---- 2: extraction on supplied volumes ------------------------------------------------------------------------------------------
def _volume(name):
    """(tsdf, weight, origin, h, min_weight) of a named volume."""
    rng = np.random.default_rng(len(name))
    if name == "sphere":
        f, w, _, _ = T.sphere_volume((14, 15, 16))
        return f, w, (0, 0, 0), 0.1, 2
    if name == "zero_plane":
        K4, poses, depth, origin, h, dims, _ = T.plane_views()
        f, w, _ = T.integrate(None, K4, poses, depth, origin, h, dims)
        return f, w, origin, h, 2
    if name == "invalid_slab":
        f, w, _, _ = T.sphere_volume((14, 15, 16))
        w[:, 6:8, :] = 0
        return f, w, (0, 0, 0), 0.1, 2
    if name == "one_cell_thick":
        return rng.normal(size=(8, 9, 2)).astype(F), np.full((8, 9, 2), 2, np.int32), (0.5, -1.0, 2.0), 0.25, 2
    if name == "random_sign":
        return rng.normal(size=(7, 8, 9)).astype(F), np.full((7, 8, 9), 3, np.int32), (-1.0, 0.25, 3.0), 0.07, 3
    if name == "random_weights":
        f = rng.normal(size=(7, 8, 9)).astype(F)
        f[rng.random(f.shape) < 0.1] = 0
        return f, rng.integers(0, 4, (7, 8, 9)).astype(np.int32), (-1.0, 0.25, 3.0), 0.07, 1
    if name == "sphere_shell":
        f, w, _, _ = T.sphere_volume((70, 66, 40), shell=3.0)
        return f, w, (0, 0, 0), 0.1, 2
    raise KeyError(name)


@pytest.mark.parametrize("name", ["sphere", "zero_plane", "invalid_slab", "one_cell_thick", "random_sign", "random_weights", "sphere_shell"])
def test_extract_bit_parity(gpu_ctx, name):
    f, w, origin, h, min_weight = _volume(name)
    rgb = np.random.default_rng(3).integers(0, 256, f.shape + (3,)).astype(np.uint8)
    ref = T.extract(f, w, rgb, origin, h, min_weight, return_cases=True)
    grid, opt = _grid(origin, h, f.shape[::-1]), _opt(min_weight=min_weight)
    got = E.tsdf_extract(f, w, rgb, grid, opt, gpu_ctx)
    assert len(got[0]) == len(ref[0]) and len(got[3]) == len(ref[3]), (len(got[0]), len(ref[0]), len(got[3]), len(ref[3]))
    assert _same(got[3], ref[3]), np.count_nonzero(got[3] != ref[3])
    for g, r in zip(got[:3], ref[:3]):
        assert _same(g, r), np.count_nonzero(_bits(g) != _bits(r))
    assert len(ref[0]) > 50 and len(ref[3]) > 50
    if name == "random_sign":                                     # every tetrahedron case, hence both windings of each
        assert ref[4] == {(t, m) for t in range(6) for m in range(1, 15)}
    if name == "sphere_shell":                                    # the counts cross many 256-voxel scan blocks
        assert len(ref[0]) > 10000 and f.size // 256 > 700
    # normals NULL and colours NULL leave the other outputs as they are
    bare = E.tsdf_extract(f, w, rgb, grid, opt, gpu_ctx, normals=False, colours=False)
    assert bare[1] is None and bare[2] is None and _same(bare[0], ref[0]) and _same(bare[3], ref[3])
    no_rgb = E.tsdf_extract(f, w, None, grid, opt, gpu_ctx)
    assert no_rgb[2] is None and _same(no_rgb[0], ref[0]) and _same(no_rgb[1], ref[1]) and _same(no_rgb[3], ref[3])


# ---- 3: capacities --------------------------------------------------------------------------------------------------------------
def test_extract_capacity(gpu_ctx, monkeypatch):
    f, w, origin, h, min_weight = _volume("sphere")
    ref = T.extract(f, w, None, origin, h, min_weight)
    nv, nt = len(ref[0]), len(ref[3])
    grid, opt = _grid(origin, h, f.shape[::-1]), _opt()
    p = lambda a: C.c_void_p(a.ctypes.data)
    L = E.lib()

    def run(cap_v, cap_t):
        vertices = np.full((nv + 8, 3), 7.0, F); normals = np.full((nv + 8, 3), 7.0, F); tri = np.full((nt + 8, 3), 7, np.int32)
        cv, ct = C.c_int32(-5), C.c_int32(-5)
        rc = L.esfm_tsdf_extract(gpu_ctx.handle, C.byref(grid), p(f), p(w), None, C.byref(opt), cap_v, cap_t, p(vertices), p(normals), None,
                                 p(tri), C.byref(cv), C.byref(ct))
        return rc, cv.value, ct.value, vertices, normals, tri, L.esfm_last_error().decode()

    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1), (0, 0)):
        rc, cv, ct, vertices, normals, tri, err = run(cap_v, cap_t)
        assert rc == -1 and (cv, ct) == (nv, nt) and str(nv) in err and str(nt) in err, (rc, cv, ct, err)
        assert np.all(vertices == 7.0) and np.all(normals == 7.0) and np.all(tri == 7)
    rc, cv, ct, vertices, normals, tri, _ = run(nv, nt)
    assert rc == 0 and (cv, ct) == (nv, nt)
    assert _same(vertices[:nv], ref[0]) and _same(normals[:nv], ref[1]) and _same(tri[:nt], ref[3])
    assert np.all(vertices[nv:] == 7.0) and np.all(tri[nt:] == 7)
    # a guess of the wrapper's that is too small: it retries once with the reported counts
    import easysfm_amd.mesh as mesh
    monkeypatch.setattr(mesh, "CAPACITY_GUESS", (16, 16))
    retried = E.tsdf_extract(f, w, None, grid, opt, gpu_ctx)
    assert _same(retried[0], ref[0]) and _same(retried[3], ref[3])
    with pytest.raises(E.EsfmError) as ei:
        E.tsdf_extract(f, w, None, grid, opt, gpu_ctx, capacity=(nv - 1, nt))
    assert ei.value.status == -1


# ---- 4: the fused call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("images", [None, "bgr"])
def test_mvs_mesh_equals_two_steps(gpu_ctx, crops, images):
    origin, h, dims = (-2.7, -2.15, 4.15), 0.03, (40, 33, 30)
    grid, opt = _grid(origin, h, dims), _opt()
    imgs = crops[images] if images else None
    args = (imgs, crops["K4"], crops["poses"], crops["depth"])
    volume = E.tsdf_integrate(*args, grid, opt, gpu_ctx)
    two = E.tsdf_extract(*volume, grid, opt, gpu_ctx)
    one = E.mvs_mesh(*args, grid, opt, gpu_ctx)
    assert len(two[0]) > 1000 and len(two[3]) > 1000
    assert _same_mesh(one, two)
    assert (one[2] is not None) == (images is not None)
    r_vol = T.integrate(*args, origin, h, dims)
    assert _same_mesh(one, T.extract(*r_vol, origin, h))


# ---- 5: the chain on the synthetic scene ----------------------------------------------------------------------------------------
def test_chain_on_synthetic_scene(gpu_ctx, scene):
    """GPU sweep (r 3, D 48) of the five views, the fusion's mask, the fused mesh call on the 76 x 61 x 80 grid: the mesh is the
    restatement's on the same masked depths, and it lies on the true surface."""
    nb, rng, _ = T.chain_plan(scene, M)
    o = E.default_mvs_options()
    o.num_planes = 48
    depth, _ = E.mvs_depth_maps(scene["images"], scene["K4"], scene["poses"], nb, rng, o, gpu_ctx)
    _, _, index = E.mvs_fuse(scene["images"], scene["K4"], scene["poses"], nb, depth, o, gpu_ctx, return_index=True)
    masked = E.masked_depth(depth, index)
    assert _same(masked, T.masked_depth(depth, index)) and 0.3 < np.mean(masked > 0) < np.mean(depth > 0)
    origin, h, dims = T.CHAIN_GRID
    got = E.mvs_mesh(scene["images"], scene["K4"], scene["poses"], masked, _grid(origin, h, dims), None, gpu_ctx)
    ref = T.extract(*T.integrate(scene["images"], scene["K4"], scene["poses"], masked, origin, h, dims), origin, h)
    assert len(got[0]) == len(ref[0]) and len(got[3]) == len(ref[3]), (len(got[0]), len(ref[0]), len(got[3]), len(ref[3]))
    assert _same_mesh(got, ref)
    n, median, share = T.chain_quality(scene, S, got[0])
    print(f"chain: {len(got[0])} vertices, {len(got[3])} triangles; {n} vertices away from edges: median relative depth error "
          f"{median:.6f}, {share:.4f} within 1 %")
    assert n > 5000
    assert median <= MAX_MEDIAN_REL_DEPTH_ERROR and share >= MIN_SHARE_WITHIN_1_PERCENT
