"""Dense-cloud merge on the GPU against tests/merge_ref.py: normals, the fusion's pixel indices, the voxel merge and the whole
chain through dense_merge.  Outputs are compared as uint32 / uint64 bit patterns: there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import easysfm_amd as E
import merge_ref as R
import mvs_ref as M
import mvs_scene as S

pytestmark = pytest.mark.gpu
F = np.float32

# Median angle between the merged normals and the true surface normal on the synthetic scene (voxels at least 4 px from an
# occlusion edge in every supporting view), computed on the CPU from tests/mvs_ref.py depth maps (r 3, D 48) fed to
# tests/merge_ref.py -- neither is the code under test: 4.408 degrees over 15 202 voxels (4.179 with D 128).  The GPU gives
# identical bits, so the factor 1.5 only leaves room for a later change of defaults.
REF_MEDIAN_NORMAL_ANGLE_DEG = 4.408
MAX_MEDIAN_NORMAL_ANGLE_DEG = 1.5 * REF_MEDIAN_NORMAL_ANGLE_DEG


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _nopt(**kw):
    o = E.default_mvs_normal_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o, R.normal_options(**kw)


@pytest.fixture(scope="module")
def scene():
    sc = S.make_scene()
    n = len(sc["images"])
    sc["nb"] = np.array([[j for j in range(n) if j != i][:4] for i in range(n)], np.int32)
    # a sparse cloud every view observes: the plan's neighbours and depth ranges come from it
    rng = np.random.default_rng(11)
    ys, xs = rng.integers(20, S.ROWS - 20, 400), rng.integers(20, S.COLS - 20, 400)
    P = sc["poses"][2].reshape(3, 4).astype(np.float64)
    d = sc["depth"][2][ys, xs]
    Xc = np.stack([(xs - S.CX) / S.FX * d, (ys - S.CY) / S.FY * d, d], 1)
    sc["sparse"] = ((Xc - P[:, 3]) @ P[:, :3]).astype(F)
    return sc


@pytest.fixture(scope="module")
def swept(gpu_ctx, scene):
    """Depth maps of the five views (r 3, D 48) from the plan of the sparse cloud: the GPU's, and the restatement's, once."""
    n, m = len(scene["images"]), len(scene["sparse"])
    off = (np.arange(n + 1) * m).astype(np.int32)
    pts = np.tile(np.arange(m, dtype=np.int32), n)
    ro = M.options(num_planes=48)
    nb, rng = M.plan(np.ones(n, bool), scene["poses"], scene["sparse"], off, pts, ro)
    assert np.all(rng[:, 0] > 0) and np.all(nb >= 0)
    o = E.default_mvs_options()
    o.num_planes = 48
    depth, _ = E.mvs_depth_maps(scene["images"], scene["K4"], scene["poses"], nb, rng, o, gpu_ctx)
    ref_depth, _ = M.depth_maps(scene["images"], scene["K4"], scene["poses"], nb, rng, ro)
    assert _same(depth, ref_depth) and np.mean(depth > 0) > 0.5
    return dict(nb=nb, rng=rng, depth=depth, opt=o, ref_opt=ro)


# ---- 1, 2: normals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 53), (180, 240)])
@pytest.mark.parametrize("m,min_taps", [(1, 3), (3, 25), (7, 100)])
def test_normals_bit_parity_exact_depth(gpu_ctx, scene, shape, m, min_taps):
    """Two exact-depth views with a tenth of the depths zeroed, a view without any depth, and a view that holds one row and one
    column of depths (collinear taps: det = 0 with enough taps).  37 x 53 and 180 x 240 are no multiples of the 16-pixel tile."""
    rows, cols = shape
    rng = np.random.default_rng(rows + m)
    d = np.zeros((4, rows, cols), F)
    d[:2] = scene["depth"][[1, 3], :rows, :cols].astype(F)
    d[:2][rng.random((2, rows, cols)) < 0.1] = 0
    d[3, rows // 2, :] = 5.0
    d[3, :, cols // 3] = 5.0
    views = [1, 3, 0, 2]
    o, ro = _nopt(normal_radius=m, normal_min_taps=min_taps)
    got = E.mvs_normals(scene["K4"][views], scene["poses"][views], d, o, gpu_ctx)
    ref = R.normals(scene["K4"][views], scene["poses"][views], d, ro)
    assert _same(got, ref), np.count_nonzero(_bits(got) != _bits(ref))
    has = np.any(got != 0, axis=-1)
    assert has[:2].mean() > 0.5 and not has[2].any()
    assert not has[:2][d[:2] == 0].any()                                     # a hole has no normal
    if min_taps <= 2 * m + 1:                                                # the row's windows hold enough taps: only det rejects them
        assert not has[3, rows // 2, cols // 3 + m + 1:].any()


def test_normals_bit_parity_swept_depth(gpu_ctx, scene, swept):
    got = E.mvs_normals(scene["K4"], scene["poses"], swept["depth"], None, gpu_ctx)
    ref = R.normals(scene["K4"], scene["poses"], swept["depth"])
    assert _same(got, ref), np.count_nonzero(_bits(got) != _bits(ref))
    assert np.any(got != 0, axis=-1).mean() > 0.4


# ---- 3: fusion with pixel indices -----------------------------------------------------------------------------------------------
def test_fuse_ex_matches_fuse(gpu_ctx, scene, swept):
    args = (scene["images"], scene["K4"], scene["poses"], swept["nb"], swept["depth"], swept["opt"], gpu_ctx)
    xyz, rgb = E.mvs_fuse(*args)
    xyz2, rgb2, index = E.mvs_fuse(*args, return_index=True)
    assert len(xyz) > 50000 and _same(xyz, xyz2) and np.array_equal(rgb, rgb2)
    rx, _ = M.fuse(scene["images"], scene["K4"], scene["poses"], swept["nb"], swept["depth"], swept["ref_opt"])
    assert _same(xyz, rx)
    assert index.dtype == np.int32 and np.array_equal(index, R.fuse_index(scene["K4"], scene["poses"], swept["nb"], swept["depth"], swept["ref_opt"]))
    # a NULL pixel_index is accepted and changes nothing
    n, rows, cols = swept["depth"].shape
    p = lambda a: C.c_void_p(a.ctypes.data)
    imgs = np.ascontiguousarray(scene["images"])
    K4, poses, nb, d = (np.ascontiguousarray(a) for a in (scene["K4"], scene["poses"], swept["nb"], swept["depth"]))
    o_xyz = np.zeros((n * rows * cols, 3), F); o_rgb = np.zeros((n * rows * cols, 3), np.uint8); cnt = C.c_int32(0)
    rc = E.lib().esfm_mvs_fuse_ex(gpu_ctx.handle, n, rows, cols, 1, p(imgs), p(K4), p(poses), p(nb), p(d), C.byref(swept["opt"]), p(o_xyz), p(o_rgb),
                                  None, C.byref(cnt))
    assert rc == 0 and cnt.value == len(xyz) and _same(o_xyz[:cnt.value], xyz) and np.array_equal(o_rgb[:cnt.value], rgb)


# ---- 4: voxel merge -------------------------------------------------------------------------------------------------------------
def _cloud(seed, n, spread=3.0):
    rng = np.random.default_rng(seed)
    xyz = (rng.normal(size=(n, 3)) * spread).astype(F)                      # negative coordinates too
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    nrm = rng.normal(size=(n, 3)).astype(F)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), F(1e-6))
    nrm[rng.random(n) < 0.1] = 0
    tags = rng.integers(0, 64, n).astype(np.int32)
    if n >= 1000:
        xyz[::97] = np.nan
        xyz[5::101, 1] = np.inf
        xyz[7::103, 2] = -np.inf
    return xyz, rgb, nrm, tags


def _check_merge(gpu_ctx, xyz, rgb, nrm, tags, h, min_points, min_tags):
    got = E.voxel_merge(xyz, rgb, nrm, tags, h, min_points, min_tags, gpu_ctx)
    ref = R.voxel_merge(xyz, rgb, nrm, tags, h, min_points, min_tags)
    for name, g, r in zip(("xyz", "rgb", "normals", "count", "tagmask"), got, ref):
        assert (g is None) == (r is None), name
        if g is not None:
            assert _same(g, r), (name, g.shape, r.shape, np.count_nonzero(_bits(g) != _bits(r)) if g.shape == r.shape else None)
    return got


@pytest.mark.parametrize("n", [0, 1, 2, 1000, 200000])
def test_voxel_merge_bit_parity_sizes(gpu_ctx, n):
    xyz, rgb, nrm, tags = _cloud(n, n)
    h = 0.37 if n < 200000 else 0.15
    xyz[: n // 4] *= F(0.02)                                                 # a tight cluster: voxels of thousands beside voxels of one
    out = _check_merge(gpu_ctx, xyz, rgb, nrm, tags, h, 1, 0)
    assert out[3].sum() == np.all(np.isfinite(xyz), axis=1).sum()
    if n == 200000:                                                          # the filters, on voxels of one to many members
        assert out[3].max() > 64 and np.mean(out[3] == 1) > 0.1
        a = _check_merge(gpu_ctx, xyz, rgb, nrm, tags, h, 2, 0)
        b = _check_merge(gpu_ctx, xyz, rgb, nrm, tags, h, 1, 2)
        c = _check_merge(gpu_ctx, xyz, rgb, nrm, tags, h, 2, 2)
        assert 0 < len(c[0]) <= len(a[0]) < len(out[0]) and len(b[0]) < len(out[0])


@pytest.mark.parametrize("with_rgb,with_normals,with_tags", [(False, False, False), (True, False, False), (False, True, False),
                                                             (False, False, True), (True, True, False)])
def test_voxel_merge_optional_arrays(gpu_ctx, with_rgb, with_normals, with_tags):
    xyz, rgb, nrm, tags = _cloud(21, 3000)
    out = _check_merge(gpu_ctx, xyz, rgb if with_rgb else None, nrm if with_normals else None, tags if with_tags else None, 0.8, 1,
                       1 if with_tags else 0)
    assert len(out[0]) > 100


def test_voxel_merge_every_point_its_own_voxel(gpu_ctx):
    g = np.arange(17, dtype=F)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * F(1.5) - F(9.0)
    xyz = xyz[np.random.default_rng(2).permutation(len(xyz))]
    _, rgb, nrm, tags = _cloud(22, len(xyz))
    out = _check_merge(gpu_ctx, xyz, rgb, nrm, tags, 1.0, 1, 1)
    assert len(out[0]) == len(xyz) == 4913 and np.all(out[3] == 1)


def test_voxel_merge_one_voxel_holds_everything(gpu_ctx):
    """70 000 points in ONE voxel: its run crosses every wave and workgroup boundary, so all its sums arrive through the atomics."""
    n = 70000
    rng = np.random.default_rng(23)
    xyz = (rng.random((n, 3)) * 0.9 - 0.3).astype(F)
    _, rgb, nrm, tags = _cloud(24, n)
    out = _check_merge(gpu_ctx, xyz, rgb, nrm, tags, 1.0, 1, 0)
    assert len(out[0]) == 1 and out[3][0] == n
    # two voxels of about half the points each (a point within rounding of the cell edge may fall to either side: the
    # restatement decides), the boundary between their runs in the middle of a wave
    xyz[: n // 2 + 13, 0] += F(1.0)
    out = _check_merge(gpu_ctx, xyz, rgb, nrm, tags, 1.0, 1, 0)
    assert len(out[0]) == 2 and out[3].sum() == n and abs(int(out[3][0]) - n // 2) < 100 and out[3][0] % 64 != 0


# ---- 5: rejections ------------------------------------------------------------------------------------------------------------
def test_voxel_merge_rejections_write_nothing(gpu_ctx):
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    n = 4
    xyz = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], F)
    tags = np.zeros(n, np.int32)
    o_xyz = np.full((n, 3), 7.0, F); o_cnt = np.full(n, 7, np.int32); o_msk = np.full(n, 7, np.uint64); n_out = C.c_int32(5)

    def merge(xyz_=xyz, tags_=tags, min_tags=0, mask=o_msk):
        return L.esfm_cloud_voxel_merge(gpu_ctx.handle, n, p(xyz_), None, None, p(tags_), 1.0, 1, min_tags, p(o_xyz), None, None, p(o_cnt),
                                        p(mask), C.byref(n_out))
    far = xyz.copy(); far[2, 1] = 2097152.0                                  # cell index 2^21 on the y axis
    bad = tags.copy(); bad[3] = 64
    for call, message in ((lambda: merge(xyz_=far), "cell index reaches 2^21"), (lambda: merge(tags_=bad), "tag is outside 0..63"),
                          (lambda: merge(tags_=None, min_tags=1, mask=None), "min_tags > 0 needs tags")):
        status = call()
        assert status == -1 and message in L.esfm_last_error().decode(), (status, L.esfm_last_error().decode())
        assert n_out.value == 5 and np.all(o_xyz == 7.0) and np.all(o_cnt == 7) and np.all(o_msk == 7)
    near = xyz.copy(); near[2, 1] = 2097151.0                                # the largest index that fits
    assert merge(xyz_=near) == 0 and n_out.value == 4


# ---- 6: the chain -------------------------------------------------------------------------------------------------------------
def _median_normal_angle(sc, pts, normals, mask):
    """Median angle (degrees) between the normals and the scene's true surface normal over the voxels that lie at least 4 px from
    an occlusion edge in every supporting view; also the number of such voxels."""
    n = len(sc["images"])
    clear = [S.edge_distance_mask(sc["obj"][v], sc["depth"][v], 4) for v in range(n)]
    X = pts.astype(np.float64)
    ok = np.any(normals != 0, axis=1)
    obj = np.full(len(X), -1)
    for v in range(n):
        P = sc["poses"][v].reshape(3, 4).astype(np.float64)
        q = X @ P[:, :3].T + P[:, 3]
        px = np.rint(S.FX * q[:, 0] / q[:, 2] + S.CX).astype(int)
        py = np.rint(S.FY * q[:, 1] / q[:, 2] + S.CY).astype(int)
        ins = (px >= 0) & (px < S.COLS) & (py >= 0) & (py < S.ROWS)
        sup = ((mask >> np.uint64(v)) & np.uint64(1)).astype(bool)
        cl = np.zeros(len(X), bool)
        cl[ins] = clear[v][py[ins], px[ins]]
        ok &= ~sup | cl
        first = sup & ins & (obj < 0)
        obj[first] = sc["obj"][v][py[first], px[first]]
    ok &= obj >= 0
    true = np.where((obj == 1)[:, None], X - S.SPHERE_C, np.broadcast_to(S.PLANE_N, X.shape))   # both face the cameras (z < 0 side)
    true /= np.linalg.norm(true, axis=1, keepdims=True)
    c = np.sum(normals.astype(np.float64) * true, 1) / np.maximum(np.linalg.norm(normals.astype(np.float64), axis=1), 1e-30)
    return float(np.median(np.degrees(np.arccos(np.clip(c[ok], -1, 1))))), int(ok.sum())


def test_dense_merge_chain_bit_parity_and_accuracy(gpu_ctx, scene, swept):
    n = len(scene["images"])
    frames = []
    for v in range(n):
        fr = E.Frame(frame_id=v, rgb_image=scene["images"][v])
        fr.K_cam = np.array([[S.FX, 0, S.CX], [0, S.FY, S.CY], [0, 0, 1]], F)
        fr.pose_cam = np.vstack([scene["poses"][v].reshape(3, 4), [0, 0, 0, 1]]).astype(F)
        fr.unique_pixel_ids = np.arange(len(scene["sparse"]), dtype=np.int64)
        frames.append(fr)
    cloud = E.SparsePointCloud(xyz=scene["sparse"], unique_point_ids=np.arange(len(scene["sparse"]), dtype=np.int64))
    merged, normals, count, mask, dense = E.dense_merge(frames, [False] * n, cloud, swept["opt"], None, gpu_ctx)
    ref, n_fused, h = R.merge_chain(scene["images"], scene["K4"], scene["poses"], swept["nb"], swept["depth"], swept["ref_opt"])
    assert len(dense.xyz) == n_fused
    for name, g, r in zip(("xyz", "rgb", "normals", "count", "tagmask"), (merged.xyz, merged.rgb, normals, count, mask), ref):
        assert _same(g, r), (name, g.shape, r.shape)
    assert 1000 < len(merged.xyz) < len(dense.xyz)                           # fewer points come out than go in
    assert all(bin(int(b)).count("1") >= 2 for b in mask)                    # min_tags = 2 by default
    angle, used = _median_normal_angle(scene, merged.xyz, normals, mask)
    print(f"dense_merge: {len(dense.xyz)} points -> {len(merged.xyz)} voxels at h = {h:.5f}; {np.mean(np.any(normals != 0, axis=1)):.3f} with a "
          f"normal; median normal angle {angle:.3f} deg over {used} voxels")
    assert used > 1000 and angle <= MAX_MEDIAN_NORMAL_ANGLE_DEG
