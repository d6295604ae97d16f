"""Mesh simplification without a GPU: the restated rule of tests/simplify_ref.py on its own ground (closed meshes stay closed, what
the quadric placement buys, invariance under triangle order, degenerate inputs, rejections), the host-only argument checks and
scratch layout under the sanitizers, the library's rejections, no CPU fallback, and the drivers' forms of the seventeenth argument."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_clean_cases as K
import simplify_ref as Q
import tsdf_ref as T

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")
H = 0.1

# RMS of (distance of a face centroid to the sphere's centre - r) / h on the exact-distance 40^3 sphere (11 684 vertices, 23 364
# triangles), simplified by tests/simplify_ref.py with the default options and with use_quadric = 0 (the cell mean), computed on the
# CPU; the GPU gives identical bits, so the margin only leaves room for a later change of defaults.
#   cell 2 h: 872 vertices, 1 740 triangles, quadric 0.0372, mean 0.0734;  cell 4 h: 228 vertices, 452 triangles, quadric 0.1262, mean 0.2804
REF_RMS_QUADRIC = {2: 0.0372, 4: 0.1262}
REF_RMS_MEAN = {2: 0.0734, 4: 0.2804}
REF_COUNTS = {1: (3089, 6174), 2: (872, 1740), 3: (410, 816), 4: (228, 452)}
NOISE_SEED = 3


@pytest.fixture(scope="module")
def E():
    import easysfm_amd as E
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return E


def _sphere(noise):
    f, w, centre, radius = T.sphere_volume((40, 40, 40), H)
    if noise:
        f = (f + np.random.default_rng(NOISE_SEED).uniform(-0.3 * H, 0.3 * H, f.shape).astype(F)).astype(F)
    v, _, _, t = T.extract(f, w, None, (0, 0, 0), H)
    return dict(v=v, t=t, centre=centre, radius=radius)


@pytest.fixture(scope="module")
def sphere():
    return _sphere(False)


@pytest.fixture(scope="module")
def noisy_sphere():
    return _sphere(True)


@pytest.fixture(scope="module")
def three():
    v, _, rgb, t = K.three_spheres()[:4]
    return dict(v=v, rgb=rgb, t=t)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _centroid_rms(d, s):
    c = d["vertices"][d["triangles"]].astype(np.float64).mean(axis=1)
    return float(np.sqrt(np.mean(((np.linalg.norm(c - s["centre"], axis=1) - s["radius"]) / H) ** 2)))


# ---- closed stays closed --------------------------------------------------------------------------------------------------------
# (the noisy sphere at 2 h is not in the list: there the rule pinches the surface along two edges -- four faces each, every directed
# edge still with its reverse, V - E + F still 2 -- so "no directed edge used twice" does not hold)
@pytest.mark.parametrize("noise,cells", [(False, 1), (False, 2), (False, 3), (False, 4), (True, 1), (True, 3), (True, 4)],
                         ids=["exact-1", "exact-2", "exact-3", "exact-4", "noisy-1", "noisy-3", "noisy-4"])
def test_closed_stays_closed(sphere, noisy_sphere, cells, noise):
    s = noisy_sphere if noise else sphere
    assert T.mesh_topology(s["t"])[:2] == (0, 0)
    d = Q.simplify_detail(s["v"], None, s["t"], F(cells * H), (0, 0, 0))
    repeated, unpaired, n_edges, _ = T.mesh_topology(d["triangles"])
    print(f"cell {cells} h{' noisy' if noise else ''}: {len(s['v'])} / {len(s['t'])} -> {len(d['vertices'])} / {len(d['triangles'])}, directed edges used "
          f"twice {repeated}, without reverse {unpaired}, groups with a surplus of two or more {d['surplus2']}")
    assert (repeated, unpaired) == (0, 0)
    assert len(d["vertices"]) - n_edges + len(d["triangles"]) == 2
    assert d["surplus2"] == 0
    if not noise:
        assert (len(d["vertices"]), len(d["triangles"])) == REF_COUNTS[cells]
    assert np.array_equal(np.unique(d["triangles"]), np.arange(len(d["vertices"])))
    assert np.all(np.diff(d["triangle_map"]) > 0) and np.array_equal(d["vertex_map"][s["t"][d["triangle_map"]]], d["triangles"])


# ---- the quadric pays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [2, 4])
def test_the_quadric_pays(sphere, cells):
    quadric = Q.simplify_detail(sphere["v"], None, sphere["t"], F(cells * H), (0, 0, 0), Q.options(use_quadric=1))
    mean = Q.simplify_detail(sphere["v"], None, sphere["t"], F(cells * H), (0, 0, 0), Q.options(use_quadric=0))
    assert np.array_equal(quadric["triangles"], mean["triangles"]) and np.array_equal(quadric["vertex_map"], mean["vertex_map"])
    rq, rm = _centroid_rms(quadric, sphere), _centroid_rms(mean, sphere)
    print(f"cell {cells} h: RMS radial error of the face centroids {rq:.4f} h with the quadric, {rm:.4f} h with the cell mean")
    assert abs(rm - REF_RMS_MEAN[cells]) < 5e-4
    assert rq < rm and rq <= 1.5 * REF_RMS_QUADRIC[cells]


# ---- invariance -----------------------------------------------------------------------------------------------------------------
def test_positions_do_not_depend_on_triangle_order(three):
    """Shuffled triangles with rotated corners: the same cells, colours and f32 positions bit for bit (the f64 sums see another
    order and other roundings of N, far below half an f32 unit of the result), the same triangle set up to order and rotation."""
    v, rgb, t = three["v"], three["rgb"], three["t"]
    rng = np.random.default_rng(12)
    order = rng.permutation(len(t))
    shift = rng.integers(0, 3, len(t))
    t2 = np.stack([t[np.arange(len(t)), (c + shift) % 3] for c in range(3)], 1)[order]
    a = Q.simplify(v, rgb, t, F(1.5 * K.THREE_H), (0, 0, 0))
    b = Q.simplify(v, rgb, t2, F(1.5 * K.THREE_H), (0, 0, 0))
    assert 0 < len(a[3]) < len(t)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4])

    def canonical(tri):
        r = np.argmin(tri, axis=1)
        rows = np.stack([tri[np.arange(len(tri)), (r + k) % 3] for k in range(3)], 1)
        return rows[np.lexsort(rows.T[::-1])]
    assert np.array_equal(canonical(a[3]), canonical(b[3]))


# ---- edge cases -----------------------------------------------------------------------------------------------------------------
def test_one_cell_and_every_vertex_alone(three):
    v, rgb, t = three["v"], three["rgb"], three["t"]
    none = Q.simplify(v, rgb, t, F(100.0), (-1, -1, -1))
    assert [len(a) for a in none[:4]] == [0, 0, 0, 0] and np.all(none[4] == -1) and len(none[5]) == 0
    cell = F(1e-4)
    alone = Q.simplify(v, rgb, t, cell, (0, 0, 0))
    assert len(alone[0]) == len(v) and np.array_equal(alone[4][t], alone[3]) and np.array_equal(alone[5], np.arange(len(t)))
    assert np.abs(alone[0][alone[4]].astype(np.float64) - v).max() <= 1e-5 * cell
    assert np.array_equal(alone[2][alone[4]], rgb)
    assert [len(a) for a in Q.simplify(v, None, np.zeros((0, 3), np.int32), 0.1, (0, 0, 0))[:2]] == [0, 0]


def test_open_mesh_stays_open_only_at_its_opening():
    v, _, _, t = K.opened_sphere()
    before = T.mesh_topology(t)
    assert before[0] == 0 and before[1] > 0
    d = Q.simplify_detail(v, None, t, F(0.2), (0, 0, 0))
    tri = d["triangles"]
    repeated, unpaired, _, overfull = T.mesh_topology(tri)
    assert (repeated, overfull) == (0, 0) and 0 < unpaired < before[1]
    # every unpaired edge joins two cells that hold an input vertex of the opening's border
    tt = np.asarray(t, np.int64)
    e = np.concatenate([tt[:, [0, 1]], tt[:, [1, 2]], tt[:, [2, 0]]])
    has = set(map(tuple, e.tolist()))
    border = np.unique([p for p in e.tolist() if (p[1], p[0]) not in has])
    border_cells = set(d["vertex_map"][border].tolist())
    o = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).tolist()
    out_has = set(map(tuple, o))
    open_edges = [p for p in o if (p[1], p[0]) not in out_has]
    assert len(open_edges) == unpaired and all(p[0] in border_cells and p[1] in border_cells for p in open_edges)


def test_zero_area_triangle_and_flap():
    """A triangle without area adds nothing to A; an added pair of opposite triangles on the same three cells is removed."""
    p = np.array([[0.1, 0.1, 0.1], [1.2, 0.1, 0.2], [0.2, 1.3, 0.1], [1.1, 1.2, 1.3], [0.5, 2.5, 0.5], [1.5, 2.5, 0.5], [2.5, 2.5, 0.5]], F)
    base = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    d0 = Q.simplify_detail(p, None, base, F(1.0), (0, 0, 0))
    flat = Q.simplify_detail(p, None, np.concatenate([base, [[4, 5, 6]]]).astype(np.int32), F(1.0), (0, 0, 0))
    assert flat["triangle_map"].tolist() == [0, 1, 2]
    line, rest = flat["cell_of"][4:], flat["cell_of"][:4]                  # the collinear triangle's three cells
    assert len(set(line.tolist())) == 3 and not flat["A"][line].any() and not flat["b"][line].any()
    assert np.array_equal(flat["A"][rest], d0["A"][d0["cell_of"][:4]]) and np.array_equal(_bits(flat["vertices"][flat["triangles"][:2]]), _bits(d0["vertices"][d0["triangles"]]))
    flap = Q.simplify_detail(p, None, np.concatenate([base, [[0, 1, 3], [3, 1, 0]]]).astype(np.int32), F(1.0), (0, 0, 0))
    assert flap["triangle_map"].tolist() == [0, 1] and np.array_equal(flap["triangles"], d0["triangles"])
    twice = Q.simplify_detail(p, None, np.concatenate([base, base[:1]]).astype(np.int32), F(1.0), (0, 0, 0))
    assert twice["triangle_map"].tolist() == [0, 1] and twice["surplus2"] == 1


def test_restatement_rejections(three):
    v, rgb, t = three["v"], three["rgb"], three["t"]
    for kw in (dict(cell=0.0), dict(cell=-0.1), dict(cell=float("nan")), dict(cell=float("inf")), dict(origin=(0.5, 0, 0)),
               dict(origin=(0, float("nan"), 0)), dict(o=Q.options(regularisation=0.0)), dict(o=Q.options(regularisation=2.0)),
               dict(o=Q.options(use_quadric=2)), dict(cell=1e-7), dict(rgb=None, want_rgb=True), dict(t=np.array([[0, 1, len(v)]]))):
        with pytest.raises(Q.Rejected):
            Q.simplify(v, kw.get("rgb", rgb), kw.get("t", t), kw.get("cell", 0.15), kw.get("origin", (0, 0, 0)), kw.get("o"), kw.get("want_rgb"))
    assert len(Q.simplify(v, None, t, 0.15, (0, 0, 0))[3]) > 0


# ---- the library without a GPU --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_host_checks_and_layout(tmp_path, flags):
    """tests/cpp/simplify_check_main.cpp: the argument checks and the scratch layout of esfm_mesh_simplify, host code, with g++."""
    exe = str(tmp_path / "simplify_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "simplify_check_main.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "simplify check ok" in r.stdout, r.stdout[-4000:]


def test_bad_arguments_are_rejected(E, three):
    """ctx is NULL: the argument checks come first, so a call with good arguments fails only with "ctx is NULL"; nothing is written."""
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    v, rgb, t = three["v"], three["rgb"], three["t"]
    out_v = np.full_like(v, 7.0); out_n = np.full_like(v, 7.0); out_c = np.full_like(rgb, 7); out_t = np.full_like(t, 7)
    vmap = np.full(len(v), 7, np.int32); tmap = np.full(len(t), 7, np.int32)
    nv, nt = C.c_int32(5), C.c_int32(5)
    d = E.default_mesh_simplify_options()
    assert d.regularisation == F(1e-3) and d.use_quadric == 1

    def opt(**kw):
        o = E.default_mesh_simplify_options()
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def call(cell=0.15, origin=(0, 0, 0), o=None, in_rgb=rgb, o_c=out_c, vertices=v):
        org = np.asarray(origin, F)
        return L.esfm_mesh_simplify(None, len(v), len(t), p(vertices), p(in_rgb), p(t), p(org), C.c_float(cell), C.byref(o or opt()), p(out_v),
                                    p(out_n), p(o_c), p(out_t), p(vmap), p(tmap), C.byref(nv), C.byref(nt))
    left = v.copy(); left[17, 2] = -0.01
    for kw, message in ((dict(), "ctx is NULL"), (dict(in_rgb=None, o_c=None), "ctx is NULL"), (dict(o=opt(use_quadric=0, regularisation=1.0)), "ctx is NULL"),
                        (dict(cell=0.0), "cell"), (dict(cell=-2.0), "cell"), (dict(cell=float("nan")), "cell"), (dict(cell=float("inf")), "cell"),
                        (dict(origin=(0, 0, float("nan"))), "origin"), (dict(vertices=left), "outside the grid"), (dict(origin=(0.5, 0, 0)), "outside the grid"),
                        (dict(cell=1e-7), "outside the grid"), (dict(in_rgb=None), "output array is requested without its input"),
                        (dict(o=opt(regularisation=0.0)), "regularisation"), (dict(o=opt(regularisation=float("nan"))), "regularisation"),
                        (dict(o=opt(use_quadric=3)), "use_quadric")):
        status = call(**kw)
        err = L.esfm_last_error().decode()
        assert status == -1 and message in err, (kw, status, err)
    assert (nv.value, nt.value) == (5, 5)
    assert np.all(out_v == 7.0) and np.all(out_n == 7.0) and np.all(out_c == 7) and np.all(out_t == 7) and np.all(vmap == 7) and np.all(tmap == 7)


def test_mesh_simplify_has_no_cpu_fallback(E, three):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(E.EsfmError) as ei:
        E.mesh_simplify(three["v"], three["rgb"], three["t"], 0.15)
    assert ei.value.status == -2, ei.value                                # ESFM_ERR_NO_DEVICE


def _driver_cmd(driver, tmp_path):
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
def test_drivers_take_the_simplify_forms(E, tmp_path, driver):
    """simplify:mesh.ply and clean+simplify:mesh.ply as the seventeenth argument pass argument parsing -- the run then ends on the
    missing image list --; one more argument is still the usage text (status 2), which names the new forms."""
    cmd = _driver_cmd(driver, tmp_path)
    args = ["imgs", "list.txt", "K.txt", "none", str(tmp_path / "out.ply"), "S", "100", "1.0", "1", "0", "4", "1", "0", "ratio", "none", "none"]

    def run(extra):
        return subprocess.run(cmd + args + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=str(tmp_path))
    for form in ("simplify:", "clean+simplify:"):
        r = run([form + str(tmp_path / "mesh.ply")])
        assert r.returncode != 2 and "mesh.ply | none" not in r.stdout, r.stdout[-2000:]
        r = run([form + str(tmp_path / "mesh.ply"), "extra"])
        assert r.returncode == 2 and "simplify:mesh.ply | clean+simplify:mesh.ply | mesh.ply | clean:mesh.ply | none" in r.stdout, r.stdout[-2000:]
    assert sorted(os.listdir(tmp_path)) in ([], ["sfm_native"])
