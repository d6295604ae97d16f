"""Dense-cloud merge without a GPU: the restated rules of tests/merge_ref.py on exact synthetic depth (normal accuracy, the
voxel merge's order independence and reduction), the writer of oriented points, argument checks and no CPU fallback."""
import ctypes as C
import os

import numpy as np
import pytest

import merge_ref as R
import mvs_ref as M
import mvs_scene as S

F = np.float32


@pytest.fixture(scope="module")
def E():
    import easysfm_amd as E
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return E


@pytest.fixture(scope="module")
def scene():
    return S.make_scene()


def _world_points(sc, v):
    P = sc["poses"][v].reshape(3, 4).astype(np.float64)
    ys, xs = np.mgrid[0:S.ROWS, 0:S.COLS].astype(np.float64)
    d = sc["depth"][v]
    Xc = np.stack([(xs - S.CX) / S.FX * d, (ys - S.CY) / S.FY * d, d], -1)
    return (Xc - P[:, 3]) @ P[:, :3], -P[:, :3].T @ P[:, 3]


def _angle_deg(a, b):
    c = np.sum(a * b, -1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


def test_reference_normals_on_exact_depth(scene):
    """View 2, the default window: on pixels at least 4 px from an occlusion edge whose window lies inside the image (36 131 of
    the plane, 2 105 of the sphere) the plane's normals are within 0.1 degrees of the true normal and the sphere's within 2
    degrees (measured 0.0001 and 1.06: the sphere's inverse depth is not linear over the window), and every normal faces its
    camera."""
    v = 2
    depth = scene["depth"].astype(F)
    N = R.normals(scene["K4"][v:v + 1], scene["poses"][v:v + 1], depth[v:v + 1])[0].astype(np.float64)
    X, centre = _world_points(scene, v)
    sel = S.edge_distance_mask(scene["obj"][v], scene["depth"][v], 4)
    sel[:3] = sel[-3:] = False
    sel[:, :3] = sel[:, -3:] = False
    plane, sphere = sel & (scene["obj"][v] == 0), sel & (scene["obj"][v] == 1)
    assert plane.sum() == 36131 and sphere.sum() == 2105
    assert np.all(np.any(N[sel] != 0, axis=-1))                             # every such pixel has a normal
    assert np.allclose(np.linalg.norm(N[sel], axis=-1), 1.0, atol=1e-6)
    assert np.all(np.sum(N[sel] * (centre - X[sel]), -1) > 0)               # facing the camera
    true_plane = S.PLANE_N if S.PLANE_N @ (centre - S.PLANE_P) > 0 else -S.PLANE_N
    a_plane = _angle_deg(N[plane], np.broadcast_to(true_plane, N[plane].shape))
    a_sphere = _angle_deg(N[sphere], X[sphere] - S.SPHERE_C)
    print(f"normals, view {v}: plane {int(plane.sum())} px max {a_plane.max():.4f} deg; sphere {int(sphere.sum())} px "
          f"max {a_sphere.max():.3f} median {np.median(a_sphere):.3f} deg")
    assert a_plane.max() <= 0.1 and a_sphere.max() <= 2.0


def test_reference_normals_exits():
    """No depth, too few taps and a degenerate tap set (one row: det = 0) all give (0, 0, 0)."""
    K4 = np.array([[50, 10, 50, 10]], F)
    P = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F)
    d = np.zeros((1, 21, 21), F)
    d[0, 10, :] = 2.0                                                        # a single row of depths
    o = R.normal_options(normal_radius=3, normal_min_taps=3)
    assert not np.any(R.normals(K4, P, d, o))
    d[0] = 2.0
    N = R.normals(K4, P, d, R.normal_options(normal_radius=1, normal_min_taps=9))
    assert np.all(N[0, 1:-1, 1:-1] == np.array([0, 0, -1], F))              # fronto-parallel plane, facing the camera
    assert not np.any(N[0, 0]) and not np.any(N[0, :, -1])                  # border windows hold 6 or 4 taps < 9
    d[0, 5, 5] = 0
    assert not np.any(R.normals(K4, P, d, R.normal_options(normal_radius=1, normal_min_taps=9))[0, 4:7, 4:7])


def _cloud(seed, n, spread=3.0):
    rng = np.random.default_rng(seed)
    xyz = (rng.normal(size=(n, 3)) * spread).astype(F)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    nrm = rng.normal(size=(n, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[rng.random(n) < 0.1] = 0
    tags = rng.integers(0, 64, n).astype(np.int32)
    return xyz, rgb, nrm, tags


def test_reference_voxel_merge_is_order_free():
    xyz, rgb, nrm, tags = _cloud(3, 20000)
    xyz[::97] = np.nan
    xyz[5::101, 1] = np.inf
    h = F(0.37)
    a = R.voxel_merge(xyz, rgb, nrm, tags, h, 1, 0)
    perm = np.random.default_rng(4).permutation(len(xyz))
    b = R.voxel_merge(xyz[perm], rgb[perm], nrm[perm], tags[perm], h, 1, 0)
    for u, w in zip(a, b):
        assert u.dtype == w.dtype and u.shape == w.shape and u.tobytes() == w.tobytes()
    pts, _, out_n, count, mask, keys = a
    valid = np.all(np.isfinite(xyz), axis=1)
    assert count.sum() == valid.sum() and 1000 < len(pts) < valid.sum()
    assert np.all(np.diff(keys.astype(np.int64)) > 0)                       # ascending, one entry per voxel
    # every output point lies in its voxel to within one quantum: the cell index is floorf of an f32 quotient, so a member can
    # sit below the cell's edge by the rounding of the f32 subtract and divide (2^-23 relative each) -- and the mean with it --
    # and the output adds its own rounding to f32
    o = xyz[valid].min(axis=0).astype(np.float64)
    cell = np.stack([keys & np.uint64(0x1FFFFF), (keys >> np.uint64(21)) & np.uint64(0x1FFFFF), keys >> np.uint64(42)], 1).astype(np.float64)
    t = (pts.astype(np.float64) - o) / np.float64(h) - cell
    quantum = 3 * 2.0 ** -23 * np.maximum(np.abs(pts.astype(np.float64)).max() / np.float64(h), cell.max() + 1)
    assert t.min() >= -quantum and t.max() <= 1 + quantum
    ln = np.linalg.norm(out_n.astype(np.float64), axis=1)
    assert np.all((np.abs(ln - 1) < 1e-6) | (ln == 0))
    # filters: min_points and min_tags select exactly the voxels the full output says they should
    bits = np.array([bin(int(m)).count("1") for m in mask])
    c = R.voxel_merge(xyz, rgb, nrm, tags, h, 2, 2)
    assert np.array_equal(c[5], keys[(count >= 2) & (bits >= 2)])


def test_reference_voxel_merge_small_cases():
    one = np.array([[1.5, -2.0, 3.0]], F)
    pts, rgb, nrm, count, mask, keys = R.voxel_merge(one, np.array([[1, 2, 3]], np.uint8), None, np.array([7]), 0.5, 1, 1)
    assert np.array_equal(pts, one) and np.array_equal(rgb, [[1, 2, 3]]) and nrm is None and count[0] == 1 and mask[0] == 1 << 7 and keys[0] == 0
    two = np.array([[0, 0, 0], [0.25, 0.5, 0.75]], F)
    pts, rgb, _, count, _, _ = R.voxel_merge(two, np.array([[0, 0, 1], [1, 2, 2]], np.uint8), None, None, 1.0, 1, 0)
    assert np.array_equal(pts, [[0.125, 0.25, 0.375]]) and np.array_equal(rgb, [[1, 1, 2]]) and count[0] == 2   # (sum + k / 2) / k
    assert len(R.voxel_merge(np.full((3, 3), np.nan, F), voxel_size=1.0)[0]) == 0
    assert len(R.voxel_merge(np.zeros((0, 3), F), voxel_size=1.0)[0]) == 0
    with pytest.raises(R.Rejected):
        R.voxel_merge(np.array([[0, 0, 0], [2097152.0, 0, 0]], F), voxel_size=1.0)
    assert len(R.voxel_merge(np.array([[0, 0, 0], [2097151.0, 0, 0]], F), voxel_size=1.0)[0]) == 2
    with pytest.raises(R.Rejected):
        R.voxel_merge(one, tags=np.array([64]), voxel_size=1.0)
    with pytest.raises(R.Rejected):
        R.voxel_merge(one, voxel_size=1.0, min_tags=1)


def test_reference_reduction_on_exact_depth(scene):
    """The exact-depth cloud of the five views (every pixel back-projected) at voxel_scale 2: at most half the points remain
    (measured 216 000 into 27 937 voxels), and most voxels are seen by two or more views (measured 74 %), so min_tags = 2 has
    both kinds to separate."""
    n = len(scene["images"])
    depth = scene["depth"].astype(F)
    ys, xs = np.mgrid[0:S.ROWS, 0:S.COLS]
    pts = []
    for v in range(n):
        X = M.backproject(scene["K4"][v], scene["poses"][v], xs.astype(F).ravel(), ys.astype(F).ravel(), depth[v].ravel())
        pts.append(np.stack(X, 1))
    xyz = np.concatenate(pts).astype(F)
    index = np.arange(len(xyz))
    tags = index // (S.ROWS * S.COLS)
    h = R.voxel_size(depth, scene["K4"], index, 2.0)
    out = R.voxel_merge(xyz, None, None, tags, h, 1, 0)
    bits = np.array([bin(int(m)).count("1") for m in out[4]])
    print(f"exact-depth cloud: {len(xyz)} points -> {len(out[0])} voxels at h = {h:.5f}; {np.mean(bits >= 2):.3f} with two or more views")
    assert len(xyz) == 216000 and 2 * len(out[0]) <= len(xyz)
    two = R.voxel_merge(xyz, None, None, tags, h, 1, 2)
    assert len(two[0]) == int(np.sum(bits >= 2)) and 0.5 * len(out[0]) < len(two[0]) < len(out[0])


def test_write_ply_normals_round_trip(E, tmp_path):
    xyz, rgb, nrm, _ = _cloud(5, 50)
    path = str(tmp_path / "m.ply")
    assert E.write_ply_normals(path, E.SparsePointCloud(xyz=xyz, rgb=rgb), nrm)
    head = open(path).read().split("end_header")[0].split("\n")
    assert head[:3] == ["ply", "format ascii 1.0", "element vertex 50"]
    assert [l.split()[-1] for l in head if l.startswith("property")] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    x2, n2, c2 = E.read_ply_normals(path)
    assert np.allclose(x2, xyz, rtol=1e-7) and np.allclose(n2, nrm, rtol=1e-7, atol=1e-9) and np.array_equal(c2, rgb)


def test_merge_voxel_size_matches_reference(E, scene):
    depth = scene["depth"].astype(F)
    index = np.random.default_rng(1).choice(depth.size, 5000, replace=False)
    h = E.merge_voxel_size(depth, scene["K4"], index, E.MergeOptions())
    assert h.dtype == F and h == R.voxel_size(depth, scene["K4"], index, 2.0)
    assert E.merge_voxel_size(depth, scene["K4"], index, E.MergeOptions(voxel_size=0.25)) == F(0.25)


def test_bad_arguments_are_rejected(E):
    """Each bad argument on its own, with its own message.  ctx is NULL: the argument checks come first, so a call with good
    arguments fails only with "ctx is NULL"; nothing is written."""
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    n, rows, cols = 2, 9, 11
    K4 = np.tile(np.array([50, 5, 50, 4], F), (n, 1))
    poses = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (n, 1))
    depth = np.full((n, rows, cols), 2.0, F)
    out = np.full((n, rows, cols, 3), 7.0, F)

    def nopt(**kw):
        o = E.default_mvs_normal_options()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def normals(opt=None, K=K4, rows_=rows):
        return L.esfm_mvs_normals(None, n, rows_, cols, p(K), p(poses), p(depth), C.byref(opt or nopt()), p(out))

    def rejected(call, message):
        status = call()
        err = L.esfm_last_error().decode()
        assert status == -1 and message in err, (status, err, message)

    d = E.default_mvs_normal_options()
    assert (d.normal_radius, d.normal_min_taps) == (3, 25) and d.normal_rel_step == F(0.05)
    badK = K4.copy(); badK[1, 2] = 0
    for call, message in ((normals, "ctx is NULL"), (lambda: normals(nopt(normal_radius=7, normal_min_taps=225)), "ctx is NULL"),
                          (lambda: normals(nopt(normal_radius=0)), "normal_radius"), (lambda: normals(nopt(normal_radius=8)), "normal_radius"),
                          (lambda: normals(nopt(normal_min_taps=2)), "normal_min_taps"), (lambda: normals(nopt(normal_min_taps=50)), "normal_min_taps"),
                          (lambda: normals(nopt(normal_rel_step=0.0)), "normal_rel_step"),
                          (lambda: normals(nopt(normal_rel_step=float("inf"))), "normal_rel_step"),
                          (lambda: normals(K=badK), "K4 must be finite"), (lambda: normals(rows_=0), "image sides")):
        rejected(call, message)
    assert np.all(out == 7.0)

    # fuse_ex shares esfm_mvs_fuse's checks
    imgs = np.zeros((n, rows, cols), np.uint8)
    nb = np.array([[1, -1, -1, -1], [0, -1, -1, -1]], np.int32)
    xyz = np.full((n * rows * cols, 3), 7.0, F); rgb = np.full((n * rows * cols, 3), 7, np.uint8); idx = np.full(n * rows * cols, 7, np.int32)
    cnt = C.c_int32(5)

    def fuse_ex(nb_=nb, index=idx):
        return L.esfm_mvs_fuse_ex(None, n, rows, cols, 1, p(imgs), p(K4), p(poses), p(nb_), p(depth), C.byref(E.default_mvs_options()),
                                  p(xyz), p(rgb), p(index), C.byref(cnt))
    bad_nb = nb.copy(); bad_nb[0, 0] = 0
    rejected(fuse_ex, "ctx is NULL")
    rejected(lambda: fuse_ex(index=None), "ctx is NULL")
    rejected(lambda: fuse_ex(nb_=bad_nb), "neighbour index is out of range or equals its view")
    assert cnt.value == 5 and np.all(xyz == 7.0) and np.all(rgb == 7) and np.all(idx == 7)

    # voxel merge
    m = 6
    pts = np.zeros((m, 3), F); col = np.zeros((m, 3), np.uint8); nrm = np.zeros((m, 3), F); tags = np.zeros(m, np.int32)
    o_xyz = np.full((m, 3), 7.0, F); o_rgb = np.full((m, 3), 7, np.uint8); o_nrm = np.full((m, 3), 7.0, F)
    o_cnt = np.full(m, 7, np.int32); o_msk = np.full(m, 7, np.uint64); n_out = C.c_int32(5)

    def merge(n_=m, xyz_=pts, rgb_=col, nrm_=nrm, tags_=tags, h=1.0, min_points=1, min_tags=0, o_rgb_=o_rgb, o_nrm_=o_nrm, o_msk_=o_msk):
        return L.esfm_cloud_voxel_merge(None, n_, p(xyz_), p(rgb_), p(nrm_), p(tags_), h, min_points, min_tags, p(o_xyz), p(o_rgb_), p(o_nrm_),
                                        p(o_cnt), p(o_msk_), C.byref(n_out))
    bad_tag = tags.copy(); bad_tag[4] = 64
    neg_tag = tags.copy(); neg_tag[0] = -1
    for call, message in ((merge, "ctx is NULL"),
                          (lambda: merge(rgb_=None, nrm_=None, tags_=None, o_rgb_=None, o_nrm_=None, o_msk_=None), "ctx is NULL"),
                          (lambda: merge(n_=-1), "n must be"), (lambda: merge(n_=(1 << 28) + 1), "n must be"),
                          (lambda: merge(xyz_=None), "NULL argument"),
                          (lambda: merge(h=0.0), "voxel_size"), (lambda: merge(h=float("nan")), "voxel_size"), (lambda: merge(h=float("inf")), "voxel_size"),
                          (lambda: merge(min_points=0), "min_points"), (lambda: merge(min_tags=-1), "min_tags"),
                          (lambda: merge(tags_=None, o_msk_=None, min_tags=1), "min_tags > 0 needs tags"),
                          (lambda: merge(rgb_=None), "output array is requested without its input"),
                          (lambda: merge(nrm_=None), "output array is requested without its input"),
                          (lambda: merge(tags_=None), "output array is requested without its input"),
                          (lambda: merge(tags_=bad_tag), "tag is outside 0..63"), (lambda: merge(tags_=neg_tag), "tag is outside 0..63")):
        rejected(call, message)
    assert n_out.value == 5 and np.all(o_xyz == 7.0) and np.all(o_rgb == 7) and np.all(o_nrm == 7.0) and np.all(o_cnt == 7) and np.all(o_msk == 7)


def test_dense_merge_rejects_more_than_64_views(E):
    frames = [E.Frame(frame_id=i) for i in range(65)]
    with pytest.raises(ValueError, match="at most 64 views"):
        E.dense_merge(frames, [False] * 65, E.SparsePointCloud())


def test_merge_has_no_cpu_fallback(E):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    K4 = np.tile(np.array([50, 10, 50, 10], F), (2, 1))
    poses = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (2, 1))
    nb = np.array([[1, -1, -1, -1], [0, -1, -1, -1]], np.int32)
    depth = np.ones((2, 20, 20), F)
    for call in (lambda: E.mvs_normals(K4, poses, depth),
                 lambda: E.mvs_fuse(np.zeros((2, 20, 20), np.uint8), K4, poses, nb, depth, return_index=True),
                 lambda: E.voxel_merge(np.zeros((4, 3), F), voxel_size=1.0)):
        with pytest.raises(E.EsfmError) as ei:
            call()
        assert ei.value.status == -2, ei.value                            # ESFM_ERR_NO_DEVICE
