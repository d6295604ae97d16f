"""Surface reconstruction without a GPU: the restated rules of tests/tsdf_ref.py on analytic volumes (a closed, outward
oriented sphere; the exact-zero plane; holes), the mesh writer, argument checks, no CPU fallback, and the drivers' argument
counts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import tsdf_ref as T

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E():
    import easysfm_amd as E
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return E


@pytest.fixture(scope="module")
def sphere():
    f, w, centre, radius = T.sphere_volume((14, 15, 16))
    return dict(f=f, w=w, centre=centre, radius=radius, h=0.1, mesh=T.extract(f, w, None, (0, 0, 0), 0.1))


def _faces(vertices, triangles):
    p = vertices.astype(np.float64)
    a, b, c = p[triangles[:, 0]], p[triangles[:, 1]], p[triangles[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3


def test_winding_table_is_complete():
    """Every tetrahedron has one triangle for a lone corner and two for a 2 + 2 split, on edges that join an inside to an
    outside corner; the complementary mask cuts the same edges, and a lone corner's triangle comes back with the opposite winding."""
    for t in range(6):
        assert T.tet_triangles(t, 0) == [] and T.tet_triangles(t, 15) == []
        for m in range(1, 15):
            tris = T.tet_triangles(t, m)
            assert len(tris) == (2 if bin(m).count("1") == 2 else 1)
            for tri in tris:
                assert all((m >> a & 1) != (m >> b & 1) for a, b in tri)
            flipped = T.tet_triangles(t, 15 - m)
            assert {frozenset(e) for tri in tris for e in tri} == {frozenset(e) for tri in flipped for e in tri}
            if len(tris) == 1:
                other = flipped[0]
                assert [frozenset(e) for e in tris[0]] == [frozenset(e) for e in (other[0], other[2], other[1])]


def test_sphere_is_closed_oriented_and_accurate(sphere):
    """14 x 15 x 16 exact distances: every directed edge once with its reverse once, V - E + F = 2, every face normal outward,
    vertices within 0.1 h of the sphere (linear interpolation of exact distances across at most a body diagonal; measured
    0.074 h), vertex normals within 3 degrees of radial (measured 1.06), enclosed volume 0.98 of the sphere's."""
    vertices, normals, _, triangles = sphere["mesh"]
    repeated, unpaired, n_edges, overfull = T.mesh_topology(triangles)
    assert (repeated, unpaired, overfull) == (0, 0, 0)
    assert len(vertices) - n_edges + len(triangles) == 2 and len(triangles) == 2 * len(vertices) - 4
    assert np.array_equal(np.unique(triangles), np.arange(len(vertices)))
    fn, centroid = _faces(vertices, triangles)
    assert np.all(np.sum(fn * (centroid - sphere["centre"]), 1) > 0)
    radial = vertices.astype(np.float64) - sphere["centre"]
    dist = np.linalg.norm(radial, axis=1)
    angle = np.degrees(np.arccos(np.clip(np.sum(normals * radial, 1) / dist, -1, 1)))
    a, b, c = (vertices[triangles[:, i]].astype(np.float64) - sphere["centre"] for i in range(3))
    volume = np.sum(np.einsum("ij,ij->i", a, np.cross(b, c))) / 6 / (4 / 3 * np.pi * sphere["radius"] ** 3)
    print(f"sphere: {len(vertices)} vertices, {len(triangles)} triangles; distance max {np.abs(dist - sphere['radius']).max() / sphere['h']:.4f} h; "
          f"normal angle max {angle.max():.3f} deg; volume ratio {volume:.4f}")
    assert np.abs(dist - sphere["radius"]).max() <= 0.1 * sphere["h"]
    assert angle.max() <= 3.0 and np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)
    assert 0.95 < volume < 1.0


def test_plane_through_voxel_centres():
    """Three views of a plane whose depth is exactly a layer of voxel centres: tsdf is exactly 0 on that layer, every vertex lies
    on it, most triangles have zero area and are kept, and the reversed view order gives the same volume and mesh."""
    K4, poses, depth, origin, h, dims, z = T.plane_views()
    tsdf, weight, _ = T.integrate(None, K4, poses, depth, origin, h, dims)
    assert np.all(weight == 3) and np.all(tsdf[7] == 0) and np.all(tsdf[:7] > 0) and np.all(tsdf[8:] < 0)
    vertices, normals, _, triangles = T.extract(tsdf, weight, None, origin, h)
    assert len(vertices) > 0 and np.all(vertices[:, 2] == z)
    fn, _ = _faces(vertices, triangles)
    degenerate = np.all(fn == 0, axis=1)
    assert 0 < degenerate.sum() < len(triangles)
    assert np.all(fn[~degenerate][:, 2] < 0) and np.all(fn[~degenerate][:, :2] == 0)     # towards the cameras: free space
    assert np.all(normals == np.array([0, 0, -1], F))
    # the surface patch is tiled exactly once: the areas add up to the (nx - 1) x (ny - 1) cells' faces
    assert np.isclose(np.sum(np.linalg.norm(fn, axis=1)) / 2, (dims[0] - 1) * (dims[1] - 1) * float(h) ** 2)
    r = T.plane_views(reverse=True)
    tsdf_r, weight_r, _ = T.integrate(None, r[0], r[1], r[2], origin, h, dims)
    assert tsdf_r.tobytes() == tsdf.tobytes() and np.array_equal(weight_r, weight)
    again = T.extract(tsdf_r, weight_r, None, origin, h)
    assert len(again[0]) == len(vertices) and len(again[3]) == len(triangles) and np.array_equal(again[3], triangles)


def test_invalid_slab_opens_the_mesh(sphere):
    """A slab of weight 0 through the sphere: the mesh is open (edges without a reverse), no triangle edge is shared by more than
    two triangles, and no vertex sits on an edge that has no live cell, so none lies inside the slab's span."""
    w = sphere["w"].copy()
    w[:, 6:8, :] = 0
    vertices, _, _, triangles = T.extract(sphere["f"], w, None, (0, 0, 0), sphere["h"])
    repeated, unpaired, _, overfull = T.mesh_topology(triangles)
    assert repeated == 0 and unpaired > 0 and overfull == 0
    assert 0 < len(vertices) < len(sphere["mesh"][0])
    y_lo, y_hi = (5 + 0.5) * sphere["h"], (8 + 0.5) * sphere["h"]        # centres of the valid layers next to the slab
    assert not np.any((vertices[:, 1] > y_lo + 1e-6) & (vertices[:, 1] < y_hi - 1e-6))
    assert np.array_equal(np.unique(triangles), np.arange(len(vertices)))   # every vertex is used
    # an isolated valid voxel pair has a sign change but no live cell: no vertex
    f = np.ones((4, 4, 4), F)
    f[1, 1, 1] = -1
    lone = np.zeros((4, 4, 4), np.int32)
    lone[1, 1, 1:3] = 2
    assert len(T.extract(f, lone, None, (0, 0, 0), 1.0)[0]) == 0


def test_min_weight_is_respected(sphere):
    w = sphere["w"].copy()
    w[:, :, :7] = 1
    full = T.extract(sphere["f"], w, None, (0, 0, 0), sphere["h"], min_weight=1)
    assert all(np.array_equal(a, b) for a, b in zip((full[0], full[1], full[3]), (sphere["mesh"][0], sphere["mesh"][1], sphere["mesh"][3])))
    half = T.extract(sphere["f"], w, None, (0, 0, 0), sphere["h"], min_weight=2)
    assert 0 < len(half[0]) < len(full[0]) and half[0][:, 0].min() >= (7 + 0.5) * sphere["h"] - 1e-6
    with pytest.raises(T.Rejected):
        T.extract(sphere["f"], w, None, (0, 0, 0), sphere["h"], min_weight=0)


def test_colours_interpolate(sphere):
    rgb = np.zeros(sphere["f"].shape + (3,), np.uint8)
    rgb[sphere["f"] < 0] = (200, 100, 0)
    rgb[sphere["f"] >= 0] = (100, 200, 255)
    c = T.extract(sphere["f"], sphere["w"], rgb, (0, 0, 0), sphere["h"])[2]
    assert c.dtype == np.uint8 and np.all((c[:, 0] >= 100) & (c[:, 0] <= 200)) and np.all(c[:, 0].astype(int) + c[:, 1] == 300)


def test_write_ply_mesh_round_trip(E, tmp_path, sphere):
    vertices, normals, _, triangles = sphere["mesh"]
    rgb = np.random.default_rng(2).integers(0, 256, (len(vertices), 3)).astype(np.uint8)
    path = str(tmp_path / "mesh.ply")
    assert E.write_ply_mesh(path, vertices, normals, rgb, triangles)
    head = open(path).read().split("end_header")[0].split("\n")
    assert head[:3] == ["ply", "format ascii 1.0", f"element vertex {len(vertices)}"]
    assert [l.split()[-1] for l in head if l.startswith("property")] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "vertex_indices"]
    assert f"element face {len(triangles)}" in head and "property list uchar int vertex_indices" in head
    v2, n2, c2, t2 = E.read_ply_mesh(path)
    assert np.allclose(v2, vertices, rtol=1e-7) and np.allclose(n2, normals, rtol=1e-7, atol=1e-9)
    assert np.array_equal(c2, rgb) and np.array_equal(t2, triangles) and t2.dtype == np.int32
    with pytest.raises(ValueError):
        E.write_ply_mesh(path, vertices, normals, rgb, triangles + 1)


def test_bad_arguments_are_rejected(E):
    """Each bad argument on its own, with its own message.  ctx is NULL: the argument checks come first, so a call with good
    arguments fails only with "ctx is NULL"; nothing is written."""
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    n, rows, cols = 2, 9, 11
    K4 = np.tile(np.array([50, 5, 50, 4], F), (n, 1))
    poses = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (n, 1))
    depth = np.full((n, rows, cols), 2.0, F)
    imgs = np.zeros((n, rows, cols), np.uint8)
    dims = (4, 3, 2)
    nvox = 24
    tsdf = np.full(nvox, 7.0, F); weight = np.full(nvox, 7, np.int32); rgb = np.full((nvox, 3), 7, np.uint8)
    vtx = np.full((8, 3), 7.0, F); nrm = np.full((8, 3), 7.0, F); col = np.full((8, 3), 7, np.uint8); tri = np.full((8, 3), 7, np.int32)
    nv, nt = C.c_int32(5), C.c_int32(5)

    def grid(origin=(0, 0, 1), h=0.25, d=dims):
        return E.tsdf_grid(origin, h, d)

    def topt(trunc=0.0, min_weight=2):
        o = E.default_tsdf_options()
        o.trunc, o.min_weight = trunc, min_weight
        return o

    d = E.default_tsdf_options()
    assert d.trunc == 0.0 and d.min_weight == 2

    def integrate(g=None, o=None, images=imgs, out_rgb=rgb, K=K4, n_=n, rows_=rows, ch=1):
        return L.esfm_tsdf_integrate(None, n_, rows_, cols, ch, p(images), p(K), p(poses), p(depth), C.byref(g or grid()), C.byref(o or topt()),
                                     p(tsdf), p(weight), p(out_rgb))

    def extract(g=None, o=None, in_rgb=rgb, out_rgb=col, cap_v=8, cap_t=8, out_nrm=nrm):
        return L.esfm_tsdf_extract(None, C.byref(g or grid()), p(tsdf), p(weight), p(in_rgb), C.byref(o or topt()), cap_v, cap_t, p(vtx), p(out_nrm),
                                   p(out_rgb), p(tri), C.byref(nv), C.byref(nt))

    def mesh(g=None, o=None, images=imgs, out_rgb=col, cap_v=8, cap_t=8, n_=n):
        return L.esfm_mvs_mesh(None, n_, rows, cols, 1, p(images), p(K4), p(poses), p(depth), C.byref(g or grid()), C.byref(o or topt()), cap_v,
                               cap_t, p(vtx), p(nrm), p(out_rgb), p(tri), C.byref(nv), C.byref(nt))

    def rejected(call, message):
        status = call()
        err = L.esfm_last_error().decode()
        assert status == -1 and message in err, (status, err, message)

    badK = K4.copy(); badK[1, 0] = np.inf
    for call in (integrate, extract, mesh):
        for kw, message in ((dict(), "ctx is NULL"),
                            (dict(o=topt(trunc=0.25)), "ctx is NULL"), (dict(o=topt(trunc=3.0, min_weight=1)), "ctx is NULL"),
                            (dict(g=grid(d=(2, 2, 2))), "ctx is NULL"), (dict(g=grid(d=(1024, 1024, 128))), "ctx is NULL"),
                            (dict(g=grid(origin=(0, float("nan"), 0))), "origin"), (dict(g=grid(origin=(float("inf"), 0, 0))), "origin"),
                            (dict(g=grid(h=0.0)), "voxel_size"), (dict(g=grid(h=-1.0)), "voxel_size"), (dict(g=grid(h=float("nan"))), "voxel_size"),
                            (dict(g=grid(h=float("inf"))), "voxel_size"),
                            (dict(g=grid(d=(1, 3, 2))), "dims"), (dict(g=grid(d=(4, 3, 1025))), "dims"), (dict(g=grid(d=(4, 0, 2))), "dims"),
                            (dict(g=grid(d=(1024, 1024, 129))), "2^27"),
                            (dict(o=topt(trunc=0.2)), "trunc"), (dict(o=topt(trunc=float("inf"))), "trunc"), (dict(o=topt(trunc=float("nan"))), "trunc"),
                            (dict(o=topt(trunc=-1.0)), "trunc"), (dict(o=topt(min_weight=0)), "min_weight")):
            rejected(lambda: call(**kw), message)
    for call, message in ((lambda: integrate(images=None, out_rgb=None), "ctx is NULL"), (lambda: integrate(out_rgb=None), "ctx is NULL"),
                          (lambda: integrate(images=None), "output array is requested without its input"),
                          (lambda: integrate(n_=0), "n_views"), (lambda: integrate(n_=65), "n_views"), (lambda: integrate(rows_=0), "image sides"),
                          (lambda: integrate(ch=2), "images must be"), (lambda: integrate(K=badK), "K4 must be finite"),
                          (lambda: extract(in_rgb=None, out_rgb=None, out_nrm=None), "ctx is NULL"), (lambda: extract(out_rgb=None), "ctx is NULL"),
                          (lambda: extract(in_rgb=None), "output array is requested without its input"),
                          (lambda: extract(cap_v=-1), "capacities"), (lambda: extract(cap_t=-1), "capacities"),
                          (lambda: mesh(images=None, out_rgb=None), "ctx is NULL"), (lambda: mesh(cap_v=0, cap_t=0), "ctx is NULL"),
                          (lambda: mesh(images=None), "output array is requested without its input"),
                          (lambda: mesh(cap_v=-1), "capacities"), (lambda: mesh(n_=65), "n_views")):
        rejected(call, message)
    assert nv.value == 5 and nt.value == 5
    assert np.all(tsdf == 7.0) and np.all(weight == 7) and np.all(rgb == 7)
    assert np.all(vtx == 7.0) and np.all(nrm == 7.0) and np.all(col == 7) and np.all(tri == 7)


def test_mesh_has_no_cpu_fallback(E):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    K4 = np.tile(np.array([50, 10, 50, 10], F), (2, 1))
    poses = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (2, 1))
    depth = np.ones((2, 20, 20), F)
    grid = E.tsdf_grid((-0.5, -0.5, 0.5), 0.125, (8, 8, 8))
    for call in (lambda: E.tsdf_integrate(None, K4, poses, depth, grid),
                 lambda: E.tsdf_extract(np.zeros((8, 8, 8), F), np.zeros((8, 8, 8), np.int32), None, grid),
                 lambda: E.mvs_mesh(np.zeros((2, 20, 20), np.uint8), K4, poses, depth, grid)):
        with pytest.raises(E.EsfmError) as ei:
            call()
        assert ei.value.status == -2, ei.value                            # ESFM_ERR_NO_DEVICE


def test_dense_mesh_rejects_more_than_64_views(E):
    frames = [E.Frame(frame_id=i) for i in range(65)]
    with pytest.raises(ValueError, match="at most 64 views"):
        E.dense_mesh(frames, [False] * 65, E.SparsePointCloud())


def test_mesh_grid_and_masked_depth(E):
    """The grid holds the 1st..99th percentile box padded by the truncation distance, stays within max_voxels and 1024 per axis
    by enlarging the voxels, and the mask keeps exactly the fusion's pixels."""
    rng = np.random.default_rng(8)
    pts = rng.uniform([-1, -2, 3], [1, 2, 7], (5000, 3)).astype(F)
    pts[:20] *= 100                                                       # blunders outside the percentile box
    g = E.mesh_grid(pts, 0.05, E.MeshOptions())
    s = np.sort(pts.astype(np.float64), axis=0)
    lo, hi = s[int(np.floor(0.01 * (len(s) - 1)))], s[int(np.ceil(0.99 * (len(s) - 1)))]
    origin, dims, h = np.array(g.origin[:]), np.array(g.dims[:]), g.voxel_size
    assert h == F(0.05) and np.all(origin <= lo - 4 * h + 1e-3) and np.all(origin + dims * h >= hi + 4 * h - 1e-3)
    assert np.all(origin + dims * h <= hi + 6 * h) and dims.prod() <= 2 ** 24
    small = E.mesh_grid(pts, 0.05, E.MeshOptions(max_voxels=20000))
    assert small.voxel_size > h and np.prod(small.dims[:]) <= 20000 * 1.05
    thin = E.mesh_grid(pts * np.array([1, 1, 400], F), 0.05, E.MeshOptions(max_voxels=2 ** 27))
    assert max(thin.dims[:]) <= 1024 and thin.voxel_size > 1.0
    depth = rng.uniform(1, 2, (2, 4, 5)).astype(F)
    index = np.array([0, 7, 21, 39])
    m = E.masked_depth(depth, index)
    assert m.dtype == F and np.count_nonzero(m) == 4 and np.array_equal(m.reshape(-1)[index], depth.reshape(-1)[index])
    assert np.array_equal(m, T.masked_depth(depth, index))


def _driver_cmd(driver, tmp_path, E):
    if driver == "python":
        return [sys.executable, os.path.join(ROOT, "bin", "sfm")]
    exe = os.path.join(ROOT, "bin", "sfm_native")
    if not os.path.exists(exe):
        exe = str(tmp_path / "sfm_native")
        cmd = ["g++", "-O2", "-std=c++17", os.path.join(ROOT, "easysfm_amd", "host", "sfm_main.cpp"), "-o", exe,
               os.path.join(ROOT, "easysfm_amd", "libesfm_hip.so"), "-lz", "-pthread", "-Wl,-rpath," + os.path.join(ROOT, "easysfm_amd"),
               "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return [exe]


@pytest.mark.parametrize("driver", ["python", "native"])
def test_drivers_take_a_seventeenth_argument(E, tmp_path, driver):
    """argc 18 passes argument parsing -- the run then ends on the missing image list --, argc 19 is the usage text (status 2)."""
    cmd = _driver_cmd(driver, tmp_path, E)
    args = ["imgs", "list.txt", "K.txt", "none", str(tmp_path / "out.ply"), "S", "100", "1.0", "1", "0", "4", "1", "0", "ratio", "none", "none"]

    def run(extra):
        return subprocess.run(cmd + args + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=str(tmp_path))
    r = run([str(tmp_path / "mesh.ply")])
    assert r.returncode != 2 and "mesh.ply | none" not in r.stdout, r.stdout[-2000:]
    r = run(["none"])
    assert r.returncode != 2, r.stdout[-2000:]
    r = run([str(tmp_path / "mesh.ply"), "extra"])
    assert r.returncode == 2 and "mesh.ply | none" in r.stdout, r.stdout[-2000:]
    assert not (tmp_path / "mesh.ply").exists()
