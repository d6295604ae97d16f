"""Mesh rendering without a GPU: properties of the rule as tests/render_ref.py restates it (include/esfm.h, "Mesh rendering") --
every pixel of a closed surface patch is covered exactly once, the ownership of vertices and edges that run through pixel
centres, the chain mesh's re-render figures --, the package's Python-only helpers (orbit_poses, mesh_render_error), and the
library's host half: argument checks before any device call, the stand-alone check program, no CPU fallback."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mvs_scene as S
import render_cases as RC
import render_ref as R
import texture_cases as TC

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")

# The chain mesh of tests/golden/texture_chain_mesh.npz (1 138 vertices, 2 000 triangles) with the atlas tests/texture_ref.py bakes for
# it (S = 4, 128 x 128 texels), re-rendered by tests/render_ref.py into the scene's five views of 180 x 240 and compared with the
# photographs those views took.  Per view 0 .. 4:
#   vertex-colour error 4.492 4.429 4.368 4.506 4.801;  textured error 3.145 3.081 3.096 3.180 3.390  (grey levels, mean |difference|
#   over the covered pixels and three channels);  covered pixels within 2 % of the scene's exact depth 0.9945 0.9969 0.9968 0.9901
#   0.9743;  coverage 0.1466 0.1493 0.1502 0.1497 0.1440.
# The GPU gives identical bits (tests/test_mesh_render_gpu.py).  The conditions: textured below vertex-colour in every view, the depth
# share at least 0.95; the recorded errors are held with half as much again, which only leaves room for a later change of defaults
# upstream of the renderer.
REF_TEXTURED_ERROR = (3.145, 3.081, 3.096, 3.180, 3.390)


@pytest.fixture(scope="module")
def E():
    import easysfm_amd as E
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return E


# ---- coverage ---------------------------------------------------------------------------------------------------------------------
def test_grid_is_covered_exactly_once():
    v, t, interior = RC.grid_mesh()
    assert len(t) == 242
    K4, P = RC.grid_camera()
    total = R.coverage_count(v, t, K4[0], P[0], RC.ROWS, RC.COLS)
    assert total.max() == 1 and total.sum() == 723, total.sum()        # (the restatement's own count on this grid)
    # a pixel inside or on the rim of an interior quadrilateral has the mesh all around it: it is covered, by exactly one triangle
    tr = R.Tris(v, t, K4[0], P[0], RC.ROWS, RC.COLS)
    closed = np.zeros((RC.ROWS, RC.COLS), bool)
    py, px = np.mgrid[0:RC.ROWS, 0:RC.COLS]
    for k in np.nonzero(interior)[0]:
        s = np.sign(tr.area2[k])
        inside = np.ones(closed.shape, bool)
        for e in range(3):
            e1 = (e + 1) % 3
            dx, dy = int(tr.x[k, e1] - tr.x[k, e]), int(tr.y[k, e1] - tr.y[k, e])
            inside &= s * (dx * (256 * py - int(tr.y[k, e])) - dy * (256 * px - int(tr.x[k, e]))) >= 0
        closed |= inside
    assert closed.sum() > 300 and np.all(total[closed] == 1)
    # the picture's identities say the same
    tid = R.mesh_render(v, t, K4, P, RC.ROWS, RC.COLS)[2][0]
    assert np.array_equal(tid >= 0, total == 1)


def _covered(points_px, tri=((0, 1, 2),)):
    v = RC.pixel_points(points_px, 8, 8, 8.0, 8.0)
    K4, P = RC.pixel_camera(8, 8, 8.0)
    cnt = R.coverage_count(v, np.array(tri, np.int32), K4[0], P[0], 8, 8)
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(cnt))}, cnt


def test_vertices_and_edges_through_pixel_centres_follow_the_ownership_rule():
    """(2, 2), (6, 2), (2, 6), y down: the edge along y = 2 runs in +x with the inside below it (s dy == 0, s dx > 0: not owned), the
    edge along x = 2 runs upwards (s dy < 0: not owned), the diagonal runs downwards (s dy > 0: owned).  So the top row, the left
    column and all three vertices are left to the neighbours, and the diagonal's pixels (5, 3), (4, 4), (3, 5) belong here."""
    expect = {(3, 3), (4, 3), (5, 3), (3, 4), (4, 4), (3, 5)}
    pts = [(2, 2), (6, 2), (2, 6)]
    assert _covered(pts)[0] == expect
    assert _covered(pts, ((0, 2, 1),))[0] == expect                                    # the other winding: the same pixels
    assert _covered(pts, ((1, 2, 0),))[0] == expect and _covered(pts, ((2, 1, 0),))[0] == expect
    # its mirror image across the diagonal owns the bottom row's and the right column's pixels, not the diagonal's
    other, _ = _covered([(6, 2), (6, 6), (2, 6)])
    assert other == {(6, 3), (5, 4), (6, 4), (4, 5), (5, 5), (6, 5), (3, 6), (4, 6), (5, 6), (6, 6)}
    both, cnt = _covered(pts + [(6, 6)], ((0, 1, 2), (1, 3, 2)))
    assert both == expect | other and cnt.max() == 1
    # a fan of eight triangles around a vertex on a pixel centre: that pixel once, every pixel of the closed square once
    ring = [(1, 1), (4, 1), (7, 1), (7, 4), (7, 7), (4, 7), (1, 7), (1, 4)]
    fan = [(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)]
    got, cnt = _covered([(4, 4)] + ring, fan)
    assert cnt[4, 4] == 1 and cnt.max() == 1 and np.all(cnt[2:7, 2:7] == 1)
    assert got == {(x, y) for x in range(1, 8) for y in range(1, 8)} - {(x, 1) for x in range(1, 8)} - {(1, y) for y in range(1, 8)}


def test_depth_order_and_ties():
    K4, P = RC.pixel_camera(8, 8, 8.0)
    pts = [(1, 1), (7, 1.5), (1.5, 7)]
    near, far = RC.pixel_points(pts, 8, 8, 4.0, 8.0), RC.pixel_points(pts, 8, 8, 8.0, 8.0)
    t = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    _, depth, tid = R.mesh_render(np.concatenate([far, near]), t, K4, P, 8, 8)
    assert set(np.unique(tid)) == {-1, 1} and np.abs(depth[tid == 1] - F(4.0)).max() < 4e-6 and np.all(depth[tid < 0] == 0)
    _, _, tid = R.mesh_render(np.concatenate([far, far]), t, K4, P, 8, 8)
    assert set(np.unique(tid)) == {-1, 0}                                               # equal depth: the lower index


# ---- the Python-only helpers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", [(0, -1, 0), (0, 0, 1), (0.3, -0.9, 0.2)])
def test_orbit_poses(E, up):
    rng = np.random.default_rng(5)
    v = (rng.normal(size=(50, 3)) * [2.0, 1.0, 0.5] + [1.0, -2.0, 7.0]).astype(F)
    mid, half = (v.min(0).astype(np.float64) + v.max(0)) / 2, np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)) / 2
    poses = E.orbit_poses(v, 9, elevation_deg=25.0, distance=3.0, up=up)
    assert poses.shape == (9, 12) and poses.dtype == np.float32
    centres = []
    for p in poses.astype(np.float64).reshape(9, 3, 4):
        Rm, tv = p[:, :3], p[:, 3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(Rm) - 1) < 1e-6
        c = Rm @ mid + tv
        assert abs(c[0]) < 1e-4 * half and abs(c[1]) < 1e-4 * half and abs(c[2] - 3.0 * half) < 1e-4 * half  # the principal point, p2 > 0
        centre = -Rm.T @ tv
        centres.append(centre)
        upn = np.asarray(up, np.float64) / np.linalg.norm(up)
        assert abs((centre - mid) @ upn / (3.0 * half) - np.sin(np.deg2rad(25.0))) < 1e-5
        assert (Rm @ upn)[1] < 0                                                        # `up` points up in the picture (y runs down)
    assert len({tuple(np.round(c, 4)) for c in centres}) == 9


def test_mesh_render_error_is_the_direct_sum(E):
    rng = np.random.default_rng(8)
    pic = rng.integers(0, 256, (3, 5, 7, 3)).astype(np.uint8)
    tid = rng.integers(-1, 3, (3, 5, 7)).astype(np.int32)
    bgr = rng.integers(0, 256, (3, 5, 7, 3)).astype(np.uint8)
    grey = rng.integers(0, 256, (3, 5, 7)).astype(np.uint8)
    for images in (bgr, grey):
        total, covered = E.mesh_render_error(pic, tid, images)
        assert total.dtype == np.int64 and total.shape == (3,) and covered.shape == (3,)
        for n in range(3):
            s = c = 0
            for y in range(5):
                for x in range(7):
                    if tid[n, y, x] >= 0:
                        c += 1
                        for ch in range(3):
                            photo = int(images[n, y, x, 2 - ch]) if images.ndim == 4 else int(images[n, y, x])
                            s += abs(int(pic[n, y, x, ch]) - photo)
            assert (int(total[n]), int(covered[n])) == (s, c)
    with pytest.raises(ValueError):
        E.mesh_render_error(pic, tid[:2], bgr)


# ---- the synthetic scene ----------------------------------------------------------------------------------------------------------
def test_chain_mesh_re_render():
    c = RC.chain()
    assert (len(c["v"]), len(c["t"])) == (1138, 2000) and c["atlas"].shape == (128, 128, 3)
    textured, coloured = RC.chain_figures(*c["textured"], c["scene"]), RC.chain_figures(*c["coloured"], c["scene"])
    assert np.array_equal(c["textured"][1], c["coloured"][1]) and np.array_equal(c["textured"][2], c["coloured"][2])
    for view, (a, b) in enumerate(zip(textured, coloured)):
        print(f"view {view}: vertex-colour error {b[0]:.3f}, textured error {a[0]:.3f}, within 2 % depth {a[1]:.4f}, coverage {a[2]:.4f}")
    for view, (a, b) in enumerate(zip(textured, coloured)):
        assert a[0] < b[0] and a[1] >= RC.MIN_DEPTH_SHARE and a[0] <= 1.5 * REF_TEXTURED_ERROR[view], (view, a, b)


def test_restatement_rejections():
    v, t, _ = RC.grid_mesh()
    K4, P = RC.grid_camera()
    uv, atlas = np.zeros((len(t), 3, 2), F), RC.noise_atlas(4, 4)
    bad_uv = uv.copy(); bad_uv[7, 1, 0] = np.inf
    bad_v = v.copy(); bad_v[3, 2] = np.nan
    bad_t = t.copy(); bad_t[0, 0] = len(v)
    for kw in (dict(uv=uv), dict(atlas=atlas), dict(uv=bad_uv, atlas=atlas), dict(uv=uv, atlas=RC.noise_atlas(1, 4)), dict(v=bad_v), dict(t=bad_t), dict(rows=1),
               dict(cols=16385), dict(K4=K4 * F([0, 1, 1, 1])), dict(K4=np.tile(K4, (65, 1)), P=np.tile(P, (65, 1)))):
        with pytest.raises(R.Rejected):
            R.mesh_render(kw.get("v", v), kw.get("t", t), kw.get("K4", K4), kw.get("P", P), kw.get("rows", RC.ROWS), kw.get("cols", RC.COLS), uv=kw.get("uv"),
                          atlas=kw.get("atlas"))


# ---- the library without a GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_host_checks_and_layout(tmp_path, flags):
    """tests/cpp/render_check_main.cpp: the argument checks and the scratch layout of the rendering; host code, g++."""
    exe = str(tmp_path / "render_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "render_check_main.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "render check ok" in r.stdout, r.stdout[-4000:]


def test_bad_arguments_are_rejected(E):
    """ctx is NULL: the argument checks come first, so a call with good arguments fails only with "ctx is NULL"; nothing is written."""
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    v, t, _ = RC.grid_mesh()
    K4, P = RC.grid_camera()
    uv, atlas = np.full((len(t), 3, 2), 0.5, F), RC.noise_atlas(4, 6)
    rgb = np.full((1, RC.ROWS, RC.COLS, 3), 7, np.uint8); depth = np.full((1, RC.ROWS, RC.COLS), 7.0, F); tid = np.full((1, RC.ROWS, RC.COLS), 7, np.int32)
    d = E.default_mesh_render_options()
    assert tuple(d.background) == (0, 0, 0)

    def call(v=v, t=t, uv=uv, atlas=atlas, H=4, W=6, n=1, rows=RC.ROWS, cols=RC.COLS, K=K4, o=d, outs=(rgb, depth, tid)):
        return L.esfm_mesh_render(None, len(v), len(t), p(v), p(t), None, p(uv), H, W, p(atlas), n, rows, cols, p(K), p(P), C.byref(o) if o else None,
                                  p(outs[0]), p(outs[1]), p(outs[2]))
    bad_v = v.copy(); bad_v[3, 1] = np.inf
    bad_t = t.copy(); bad_t[5, 2] = -1
    bad_uv = uv.copy(); bad_uv[2, 2, 1] = np.nan
    for kw, message in ((dict(), "ctx is NULL"), (dict(uv=None, atlas=None), "ctx is NULL"), (dict(outs=(None, None, tid)), "ctx is NULL"), (dict(v=bad_v), "not finite"),
                        (dict(t=bad_t), "triangle index"), (dict(n=0), "n_views"), (dict(n=65), "n_views"), (dict(rows=1), "rows and cols"),
                        (dict(cols=16385), "rows and cols"), (dict(K=K4 * F([1, 1, 0, 1])), "focal length"), (dict(K=np.full_like(K4, np.nan)), "K4"),
                        (dict(uv=None), "both"), (dict(atlas=None), "both"), (dict(uv=bad_uv), "texture coordinate"), (dict(H=1), "atlas"), (dict(W=16385), "atlas"),
                        (dict(o=None), "options are NULL"), (dict(outs=(None, None, None)), "all NULL")):
        status = call(**kw)
        err = L.esfm_last_error().decode()
        assert status == -1 and message in err, (kw, status, err)
    assert np.all(rgb == 7) and np.all(depth == 7.0) and np.all(tid == 7)


@pytest.mark.parametrize("driver", ["python", "native"])
def test_drivers_take_the_render_directory(E, tmp_path, driver):
    """An existing directory or none as the eighteenth argument passes argument parsing -- the run then ends on the missing image
    list --; a directory that does not exist, a directory without a mesh and a nineteenth argument are the usage text (status 2),
    which names the new argument."""
    import sys
    if driver == "python":
        cmd = [sys.executable, os.path.join(ROOT, "bin", "sfm")]
    else:
        exe = os.path.join(ROOT, "bin", "sfm_native")
        assert os.path.exists(exe), "bin/sfm_native not built: run __graft_entry__.build()"
        cmd = [exe]
    (tmp_path / "renders").mkdir()
    args = ["imgs", "list.txt", "K.txt", "none", str(tmp_path / "out.ply"), "S", "100", "1.0", "1", "0", "4", "1", "0", "ratio", "none", "none"]

    def run(extra):
        return subprocess.run(cmd + args + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=str(tmp_path))
    mesh = "clean+simplify+texture:" + str(tmp_path / "mesh.ply")
    for extra in ([mesh, str(tmp_path / "renders")], [mesh, "none"], [str(tmp_path / "mesh.ply"), str(tmp_path / "renders")], ["none", "none"]):
        r = run(extra)
        assert r.returncode != 2 and "render_dir" not in r.stdout, (extra, r.stdout[-2000:])
    for extra in ([mesh, str(tmp_path / "missing")], ["none", str(tmp_path / "renders")], [mesh, str(tmp_path / "renders"), "extra"]):
        r = run(extra)
        assert r.returncode == 2 and "[render_dir | none]" in r.stdout, (extra, r.stdout[-2000:])
    assert sorted(os.listdir(tmp_path)) == ["renders"] and os.listdir(tmp_path / "renders") == []


def test_mesh_render_has_no_cpu_fallback(E):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    v, t, _ = RC.grid_mesh()
    K4, P = RC.grid_camera()
    with pytest.raises(E.EsfmError) as ei:
        E.mesh_render(v, t, K4, P, RC.ROWS, RC.COLS)
    assert ei.value.status == -2, ei.value                                # ESFM_ERR_NO_DEVICE
