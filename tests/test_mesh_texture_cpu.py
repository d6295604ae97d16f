"""Mesh texturing without a GPU: properties of the rule as tests/texture_ref.py restates it (include/esfm.h, "Mesh texturing") --
the atlas layout never bleeds, occlusion, back faces, the image border, ties, rejections, and the two scene figures -- and the
library's host half: argument checks before any device call, the stand-alone check program, no CPU fallback."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mvs_scene as S
import texture_cases as TC
import texture_ref as X

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")

# The chain mesh of tests/golden/texture_chain_mesh.npz (the synthetic scene through the restated dense chain, cleaned and
# simplified: 1 138 vertices, 2 000 triangles) under the scene's five views of 180 x 240, textured by tests/texture_ref.py with the
# default options (min_cos 0.2, occlusion_tol 0.02), the derived chart size S = 4 and a square atlas (32 squares, 128 x 128 texels):
#   (a) 1 985 of 2 000 triangles labelled (0.9925); 0.0081 of them have a centroid that the true surface hides by more than 2 % in
#       their chosen view;
#   (b) over the 8 931 texels inside the charts of labelled triangles: mean |grey level - true texture| 2.999 for the atlas, 4.801 for
#       the barycentric mix of the mesh's vertex colours.
# The GPU gives identical bits (tests/test_mesh_texture_gpu.py), so the margin only leaves room for a later change of defaults.  The
# figures are held by tests/texture_cases.py check_chain, which both tests call.

@pytest.fixture(scope="module")
def E():
    import easysfm_amd as E
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return E


# ---- the layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_", range(4, 65))
def test_no_bleed(S_):
    """Points on a lattice of 3 S steps over both charts, borders and corners included, in exact integer arithmetic (coordinates in
    units of 1 / (6 S)): every texel with a non-zero bilinear weight belongs to the chart's triangle and lies in the square."""
    n = 3 * S_
    k0, k1 = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    k0, k1 = k0[k0 + k1 <= n], k1[k0 + k1 <= n]
    k2 = n - k0 - k1
    owner = X.texel_owner(S_)
    for odd in (0, 1):
        c2 = np.rint(2 * X.chart_corners(S_, odd).astype(np.float64)).astype(np.int64)       # corners in half texels
        assert np.array_equal(c2 / 2.0, X.chart_corners(S_, odd))
        num_x = k0 * c2[0, 0] + k1 * c2[1, 0] + k2 * c2[2, 0] - n                          # (x - 0.5) in units of 1 / (2 n)
        num_y = k0 * c2[0, 1] + k1 * c2[1, 1] + k2 * c2[2, 1] - n
        i0, rx = num_x // (2 * n), num_x % (2 * n)
        j0, ry = num_y // (2 * n), num_y % (2 * n)
        for di in (0, 1):
            for dj in (0, 1):
                touched = (rx != 0 if di else np.ones_like(rx, bool)) & (ry != 0 if dj else np.ones_like(ry, bool))
                i, j = (i0 + di)[touched], (j0 + dj)[touched]
                assert i.min() >= 0 and i.max() <= S_ - 1 and j.min() >= 0 and j.max() <= S_ - 1, (S_, odd, di, dj)
                assert np.all(owner[j, i] == odd), (S_, odd, di, dj)
    assert owner.sum() == S_ * (S_ - 1) // 2


@pytest.mark.parametrize("T_,width,shape", [(0, 3, (0, 15)), (1, 1, (5, 5)), (2, 1, (5, 5)), (3, 1, (10, 5)), (7, 3, (10, 15)), (12, 3, (10, 15)),
                                            (13, 3, (15, 15))])
def test_uv_and_atlas_shape(T_, width, shape):
    S_ = 5
    assert X.atlas_shape(T_, S_, width) == shape
    uv = X.texture_uv(T_, S_, width)
    assert uv.shape == (T_, 3, 2) and uv.dtype == F
    if T_:
        assert uv.min() > 0 and uv.max() < 1
        px = uv.astype(np.float64) * [shape[1], shape[0]]
        for t in range(T_):
            q = t // 2
            local = px[t] - [q % width * S_, q // width * S_]
            assert np.allclose(local, X.chart_corners(S_, t % 2), atol=1e-5)
    # the bake agrees with it, and a texel of a triangle that does not exist is black
    v = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2]], F)
    t = np.tile(np.array([[0, 2, 1]], np.int32), (T_, 1))
    K4, P = TC.front_camera(16, 16, 10.0)
    atlas, uv2 = X.texture_bake(v, None, t, np.full(T_, -1, np.int32), np.zeros((1, 16, 16), np.uint8), K4, P, S_, width)
    assert atlas.shape == shape + (3,) and np.array_equal(uv, uv2)
    if T_:
        own = np.kron(np.ones((shape[0] // S_, width), int), X.texel_owner(S_))
        Y, Xc = np.mgrid[0:shape[0], 0:shape[1]]
        exists = 2 * (Y // S_ * width + Xc // S_) + own < T_
        assert np.all(atlas[exists] == 128) and np.all(atlas[~exists] == 0)


# ---- view choice ------------------------------------------------------------------------------------------------------------------
ROWS, COLS, FOCAL = 64, 96, 60.0
far_grid, chain_mesh, check_chain = TC.far_grid, TC.chain_mesh, TC.check_chain


def test_small_quad_in_front_of_large():
    """A quad at z = 2 over x in [-0.45, 0.45], y in [-0.3, 0.3] shadows |x| < 0.9, |y| < 0.6 of the plane z = 4, and with the
    half-pixel rim and the nearest-pixel look-up |x| < 0.94, |y| < 0.67.  Of the far grid's vertices only (0, 0) lies there, of the centroids of the
    triangles that do not touch it only (0.667, -0.5) and (-0.667, 0.5): exactly the eight triangles of the four central quads
    (numbers 5, 6, 9, 10) are unlabelled.  Without the front quad every far triangle is labelled."""
    fv, ft = far_grid()
    qv, qt = TC.quad(-0.45, 0.45, -0.3, 0.3, 2.0, first=len(fv))
    K4, P = TC.front_camera(ROWS, COLS, FOCAL)
    label, score, buffers = X.texture_views(np.concatenate([fv, qv]), np.concatenate([ft, qt]), ROWS, COLS, K4, P)
    hidden = sorted(2 * q + k for q in (5, 6, 9, 10) for k in (0, 1))
    assert np.nonzero(label[:32] == -1)[0].tolist() == hidden and np.all(score[hidden] == 0)
    assert np.all(label[32:] == 0)
    assert np.allclose(score[[t for t in range(32) if t not in hidden]], 0.5 * 15.0 * 11.25)       # 1 x 0.75 units at 15 px per unit
    assert np.allclose(score[32:], 0.5 * 27.0 * 18.0)
    # the buffer: 1 / 2 on the front quad's pixels (rim included), 1 / 4 on the rest of the far grid, 0 outside
    z = buffers[0].view(F)
    assert z[31, 48] == F(0.5) and z[20, 48] == F(0.25) and z[2, 2] == 0 and set(np.unique(z)) == {F(0), F(0.25), F(0.5)}
    assert (z == F(0.5)).sum() == 28 * 20                  # u in 34 .. 61, w in 22.5 .. 40.5 widened by half a pixel: columns 34 .. 61, rows 22 .. 41
    label2, _, _ = X.texture_views(fv, ft, ROWS, COLS, K4, P)
    assert np.all(label2 == 0)


def test_back_faces_and_the_image_border():
    fv, ft = far_grid()
    K4, P = TC.front_camera(ROWS, COLS, FOCAL)
    label, score, _ = X.texture_views(fv, ft[:, [0, 2, 1]], ROWS, COLS, K4, P)        # the other winding: all back-facing, and they still occlude
    assert np.all(label == -1) and np.all(score == 0)
    # shifted right by 1.4: the last column of quads leaves the image (u up to 98.5), the third ends at u = 83.5 inside
    label, _, _ = X.texture_views(fv + F([1.4, 0, 0]), ft, ROWS, COLS, K4, P)
    out = np.array([c == 3 for r in range(4) for c in range(4) for _ in (0, 1)])
    assert np.array_equal(label == -1, out) and np.all(label[~out] == 0)
    # a vertex exactly one pixel inside the border is admissible, one nearer to it is not (focal 64 at z = 64: one pixel per unit, exact)
    K64, _ = TC.front_camera(ROWS, COLS, 64.0)
    for x0, expect in ((-46.5, 0), (-46.75, -1)):
        one = np.array([[x0, -10, 64], [-20, 10, 64], [-20, -10, 64]], F)
        label, score, _ = X.texture_views(one, [[0, 1, 2]], ROWS, COLS, K64, P)
        assert label[0] == expect and score[0] == (F(0.5 * 26.5 * 20) if expect == 0 else 0), (x0, label, score)
    # behind the camera: skipped
    label, _, buffers = X.texture_views(fv * F([1, 1, -1]), ft, ROWS, COLS, K4, P)
    assert np.all(label == -1) and not buffers.any()


def test_a_tie_goes_to_the_lower_view():
    fv, ft = far_grid()
    K4, P = TC.front_camera(ROWS, COLS, FOCAL)
    label, _, _ = X.texture_views(fv, ft, ROWS, COLS, np.tile(K4, (3, 1)), np.tile(P, (3, 1)))
    assert np.all(label == 0)
    # a view that sees the plane larger wins wherever the triangle is still inside it
    K2 = np.concatenate([K4, K4 * F([1.6, 1, 1.6, 1])])
    label, score, _ = X.texture_views(fv, ft, ROWS, COLS, K2, np.tile(P, (2, 1)))
    inner = np.array([r in (1, 2) and c in (1, 2) for r in range(4) for c in range(4) for _ in (0, 1)])
    assert np.all(label[inner] == 1) and np.all(label[~inner] == 0)


def test_restatement_rejections():
    fv, ft = far_grid()
    K4, P = TC.front_camera(ROWS, COLS, FOCAL)
    img = np.zeros((1, ROWS, COLS), np.uint8)
    lab = np.zeros(len(ft), np.int32)
    bad_v = fv.copy(); bad_v[3, 1] = np.nan
    bad_t = ft.copy(); bad_t[5, 2] = len(fv)
    neg_t = ft.copy(); neg_t[0, 0] = -1
    views = lambda **kw: X.texture_views(kw.get("v", fv), kw.get("t", ft), kw.get("rows", ROWS), kw.get("cols", COLS), kw.get("K4", K4), kw.get("P", P),
                                         kw.get("o"))
    for kw in (dict(v=bad_v), dict(t=bad_t), dict(t=neg_t), dict(K4=np.tile(K4, (65, 1)), P=np.tile(P, (65, 1))), dict(K4=np.zeros((0, 4), F), P=np.zeros((0, 12), F)),
               dict(o=X.options(min_cos=1.0)), dict(o=X.options(min_cos=-0.1)), dict(o=X.options(min_cos=np.nan)), dict(o=X.options(occlusion_tol=1.0)),
               dict(o=X.options(occlusion_tol=-0.01)), dict(rows=1), dict(cols=16385), dict(K4=K4 * F([0, 1, 1, 1])), dict(P=np.full_like(P, np.inf))):
        with pytest.raises(X.Rejected):
            views(**kw)
    bake = lambda **kw: X.texture_bake(kw.get("v", fv), None, kw.get("t", ft), kw.get("lab", lab), kw.get("img", img), K4, P, kw.get("S", 8), kw.get("A", 4),
                                       kw.get("cap"))
    for kw in (dict(v=bad_v), dict(t=bad_t), dict(S=3), dict(S=65), dict(A=0), dict(A=2049), dict(S=64, A=257), dict(A=1, S=64, t=np.tile(ft, (17, 1)), lab=np.tile(lab, 17)),
               dict(lab=lab + 1), dict(lab=lab - 2), dict(img=np.zeros((1, ROWS, COLS, 2), np.uint8)), dict(cap=31)):
        with pytest.raises(X.Rejected):
            bake(**kw)
    with pytest.raises(X.Rejected, match="needs 32 rows"):
        bake(cap=31)
    assert bake(cap=32)[0].shape == (32, 32, 3) and bake(A=2048, S=8)[0].shape == (8, 16384, 3)


# ---- the synthetic scene ----------------------------------------------------------------------------------------------------------
def test_chain_mesh_occlusion_and_fidelity():
    v, rgb, t = chain_mesh()
    assert (len(v), len(t)) == (1138, 2000)
    scene = S.make_scene()
    label, score, _ = X.texture_views(v, t, S.ROWS, S.COLS, scene["K4"], scene["poses"])
    S_ = X.auto_texels(label, score)
    atlas, _ = X.texture_bake(v, rgb, t, label, scene["images"], scene["K4"], scene["poses"], S_, 32)
    assert S_ == 4 and atlas.shape == (128, 128, 3)
    check_chain(v, rgb, t, label, score, atlas, S_, 32, scene)


# ---- the library without a GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_host_checks_and_layout(tmp_path, flags):
    """tests/cpp/texture_check_main.cpp: the argument checks, the uv corners and the scratch layout of the texturing, and the host
    layer's PNG writer through its reader; host code, g++."""
    exe = str(tmp_path / "texture_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "texture_check_main.cpp"), "-o", exe, "-lz"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    (tmp_path / "png").mkdir()
    r = subprocess.run([exe, str(tmp_path / "png")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "texture check ok" in r.stdout, r.stdout[-4000:]


def test_textured_ply_and_png_round_trip(E, tmp_path):
    """write_ply_textured_mesh and its reader; the atlas it writes decodes through the host layer's C++ PNG reader to the same bytes."""
    rng = np.random.default_rng(2)
    v = rng.normal(size=(5, 3)).astype(F); nrm = rng.normal(size=(5, 3)).astype(F)
    t = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 3]], np.int32)
    uv = X.texture_uv(3, 7, 2)
    atlas = rng.integers(0, 256, (14, 14, 3)).astype(np.uint8)
    assert E.write_ply_textured_mesh(str(tmp_path / "m.ply"), v, nrm, t, uv, atlas)
    assert sorted(os.listdir(tmp_path)) == ["m.ply", "m.png"]
    text = (tmp_path / "m.ply").read_text().split("\n")
    assert text[2] == "comment TextureFile m.png" and "property list uchar float texcoord" in text
    assert text[text.index("end_header") + 6].split()[:5] == ["3", "0", "1", "2", "6"] and len(text[text.index("end_header") + 6].split()) == 11
    v2, n2, t2, uv2, name = E.read_ply_textured_mesh(str(tmp_path / "m.ply"))
    assert name == "m.png" and np.array_equal(t2, t) and np.array_equal(v2, v) and np.array_equal(n2, nrm)
    assert np.abs(uv2 - uv).max() <= 2e-7 and uv2.min() >= 0 and uv2.max() <= 1                     # (1 - v twice, 8 digits)
    exe = str(tmp_path / "png_reader")
    r = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "png_reader_main.cpp"), "-o", exe, "-lz"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, str(tmp_path / "m.png"), str(tmp_path / "m.raw")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["14", "14"], r.stdout
    assert np.array_equal(np.fromfile(str(tmp_path / "m.raw"), np.uint8).reshape(14, 14, 3)[..., ::-1], atlas)
    with pytest.raises(ValueError):
        E.write_png_rgb(str(tmp_path / "empty.png"), np.zeros((0, 4, 3), np.uint8))


def test_bad_arguments_are_rejected(E):
    """ctx is NULL: the argument checks come first, so a call with good arguments fails only with "ctx is NULL"; nothing is written,
    except the needed height where only the atlas buffer is too small."""
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    fv, ft = far_grid()
    K4, P = TC.front_camera(ROWS, COLS, FOCAL)
    img = np.zeros((1, ROWS, COLS), np.uint8)
    label = np.full(len(ft), 7, np.int32); score = np.full(len(ft), 7.0, F); buffers = np.full((1, ROWS, COLS), 7, np.uint32)
    d = E.default_mesh_texture_options()
    assert d.min_cos == F(0.2) and d.occlusion_tol == F(0.02)

    def opt(**kw):
        o = E.default_mesh_texture_options()
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def views(v=fv, t=ft, n=1, rows=ROWS, cols=COLS, K=K4, o=None):
        return L.esfm_mesh_texture_views(None, len(v), len(t), p(v), p(t), n, rows, cols, p(K), p(P), C.byref(o or opt()), p(label), p(score), p(buffers))
    bad_v = fv.copy(); bad_v[3, 1] = np.inf
    bad_t = ft.copy(); bad_t[5, 2] = len(fv)
    for kw, message in ((dict(), "ctx is NULL"), (dict(v=bad_v), "not finite"), (dict(t=bad_t), "triangle index"), (dict(n=0), "n_views"), (dict(n=65), "n_views"),
                        (dict(rows=1), "rows and cols"), (dict(cols=16385), "rows and cols"), (dict(K=K4 * F([1, 1, 0, 1])), "focal length"),
                        (dict(K=np.full_like(K4, np.nan)), "K4"), (dict(o=opt(min_cos=1.0)), "min_cos"), (dict(o=opt(min_cos=float("nan"))), "min_cos"),
                        (dict(o=opt(occlusion_tol=-0.5)), "occlusion_tol"), (dict(o=opt(occlusion_tol=1.0)), "occlusion_tol")):
        status = views(**kw)
        err = L.esfm_last_error().decode()
        assert status == -1 and message in err, (kw, status, err)
    assert np.all(label == 7) and np.all(score == 7.0) and np.all(buffers == 7)

    atlas = np.full((32, 32, 3), 7, np.uint8); uv = np.full((len(ft), 3, 2), 7.0, F)
    rows_out = C.c_int32(5)
    lab = np.zeros(len(ft), np.int32)

    def bake(v=fv, t=ft, lab=lab, ch=1, S_=8, A=4, cap=32):
        return L.esfm_mesh_texture_bake(None, len(v), len(t), p(v), None, p(t), p(lab), 1, ROWS, COLS, ch, p(img), p(K4), p(P), S_, A, cap, p(atlas), p(uv),
                                        C.byref(rows_out))
    for kw, message in ((dict(v=bad_v), "not finite"), (dict(t=bad_t), "triangle index"), (dict(S_=3), "texels"), (dict(S_=65), "texels"), (dict(A=0), "atlas_width"),
                        (dict(A=2049), "wider than 16384"), (dict(lab=lab + 1), "label"), (dict(lab=lab - 2), "label"), (dict(ch=2), "channels"),
                        (dict(cap=-1), "max_atlas_rows")):
        status = bake(**kw)
        err = L.esfm_last_error().decode()
        assert status == -1 and message in err and rows_out.value == 5, (kw, status, err)
    assert bake(cap=31) == -1 and "needs 32 rows" in L.esfm_last_error().decode() and rows_out.value == 32
    rows_out.value = 5
    assert bake() == -1 and "ctx is NULL" in L.esfm_last_error().decode() and rows_out.value == 32
    assert np.all(atlas == 7) and np.all(uv == 7.0)


def test_mesh_texture_has_no_cpu_fallback(E):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    fv, ft = far_grid()
    K4, P = TC.front_camera(ROWS, COLS, FOCAL)
    with pytest.raises(E.EsfmError) as ei:
        E.mesh_texture_views(fv, ft, ROWS, COLS, K4, P)
    assert ei.value.status == -2, ei.value                                # ESFM_ERR_NO_DEVICE
    with pytest.raises(E.EsfmError) as ei:
        E.mesh_texture_bake(fv, None, ft, np.zeros(len(ft), np.int32), np.zeros((1, ROWS, COLS), np.uint8), K4, P, 8)
    assert ei.value.status == -2, ei.value


@pytest.mark.parametrize("driver", ["python", "native"])
def test_drivers_take_the_texture_forms(E, tmp_path, driver):
    """texture:mesh.ply and the three +texture forms as the seventeenth argument pass argument parsing -- the run then ends on the
    missing image list --; one more argument is still the usage text (status 2), which names the new forms."""
    import sys
    if driver == "python":
        cmd = [sys.executable, os.path.join(ROOT, "bin", "sfm")]
    else:
        exe = os.path.join(ROOT, "bin", "sfm_native")
        if not os.path.exists(exe):
            exe = str(tmp_path / "sfm_native")
            r = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "easysfm_amd", "host", "sfm_main.cpp"), "-o", exe,
                                os.path.join(ROOT, "easysfm_amd", "libesfm_hip.so"), "-lz", "-pthread", "-Wl,-rpath," + os.path.join(ROOT, "easysfm_amd"),
                                "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 0, r.stdout
        cmd = [exe]
    args = ["imgs", "list.txt", "K.txt", "none", str(tmp_path / "out.ply"), "S", "100", "1.0", "1", "0", "4", "1", "0", "ratio", "none", "none"]

    def run(extra):
        return subprocess.run(cmd + args + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=str(tmp_path))
    for form in ("texture:", "clean+texture:", "simplify+texture:", "clean+simplify+texture:"):
        r = run([form + str(tmp_path / "mesh.ply")])
        assert r.returncode != 2 and "clean+simplify+texture:" not in r.stdout, (form, r.stdout[-2000:])
        r = run([form + str(tmp_path / "mesh.ply"), "extra"])
        assert r.returncode == 2 and "texture:, clean+texture:, simplify+texture:, clean+simplify+texture:" in r.stdout, r.stdout[-2000:]
    assert sorted(os.listdir(tmp_path)) in ([], ["sfm_native"])
