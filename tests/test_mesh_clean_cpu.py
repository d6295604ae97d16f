"""Mesh clean-up without a GPU: the restated rule of tests/mesh_clean_ref.py on its own ground (components against scipy, the
filter, pinning, invariance under triangle order, what smoothing buys), the library's argument checks, no CPU fallback, and
the drivers' clean:mesh.ply form of the seventeenth argument."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_clean_cases as K
import mesh_clean_ref as R
import tsdf_ref as T

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What 10 Taubin iterations at the defaults buy on the three-sphere volume with seeded uniform noise of +-0.3 h on the distances
# (np.random.default_rng(7)), over the large sphere's vertices: the RMS of (distance to the centre - r) / h before and after,
# the enclosed volume after over before, and on the noise-free volume the largest angle between the recomputed normals and the
# radial directions (8.530 degrees before smoothing).  Figures of tests/mesh_clean_ref.py, computed on the CPU; the GPU gives
# identical bits, so the margins only leave room for a later change of defaults.
REF_RMS_BEFORE = 0.1389
REF_RMS_AFTER = 0.1087
REF_VOLUME_RATIO = 1.0046
REF_MAX_NORMAL_ANGLE = 8.480
MAX_RMS_AFTER = 1.1 * REF_RMS_AFTER
MAX_NORMAL_ANGLE = 1.1 * REF_MAX_NORMAL_ANGLE


@pytest.fixture(scope="module")
def E():
    import easysfm_amd as E
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return E


@pytest.fixture(scope="module")
def three():
    vertices, normals, rgb, triangles, centre, radius = K.three_spheres()
    return dict(v=vertices, n=normals, rgb=rgb, t=triangles, centre=centre, radius=radius)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_three_sphere_fixture(three):
    v, t = three["v"], three["t"]
    assert (len(v), len(t)) == (2310, 4608)
    assert T.mesh_topology(t) == (0, 0, 6912, 0)
    labels, count, n = R.components(t, len(v))
    assert n == 3 and tuple(sorted(count[count > 0], reverse=True)) == K.THREE_COUNTS
    start, _, pinned = R.adjacency(t, len(v))
    assert (np.diff(start).min(), np.diff(start).max()) == (4, 10) and not pinned.any()


def test_components_equal_scipy(three):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    cases = [(three["t"], len(three["v"])), (K.strip(5001, "random", 3), 5001), (K.strip(300, "descending", repeat_index=True), 320),
             (np.zeros((0, 3), np.int32), 5)]
    for t, n_vertices in cases:
        labels, count, n = R.components(t, n_vertices)
        a, b = np.r_[t[:, 0], t[:, 0]], np.r_[t[:, 1], t[:, 2]]
        n_sp, part = connected_components(sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(n_vertices, n_vertices)), directed=False)
        assert n == n_sp
        # the same partition, and every label is its component's smallest index
        assert len(set(zip(labels.tolist(), part.tolist()))) == n
        smallest = np.full(n_sp, n_vertices)
        np.minimum.at(smallest, part, np.arange(n_vertices))
        assert np.array_equal(labels, smallest[part])
        assert count.sum() == len(t) and not count[labels != np.arange(n_vertices)].any()


def test_filter_compaction_and_maps(three):
    v, rgb, t = three["v"], three["rgb"], three["t"]
    labels, _, _ = R.components(t, len(v))
    for permille, kept_triangles, kept_components in ((0, 4352, 2), (200, 3708, 1)):         # 644 is 17.4 % of 3 708
        o = R.options(min_component_triangles=300, min_component_permille=permille, smooth_iterations=0)
        pos, nrm, col, tri, vmap, tmap = R.clean(v, rgb, t, o)
        assert len(tri) == kept_triangles
        new_labels, new_count, n = R.components(tri, len(pos))
        assert n == kept_components
        for c in np.nonzero(new_count)[0]:                                                  # each kept piece is a closed sphere
            sel = new_labels[tri[:, 0]] == c
            repeated, unpaired, n_edges, overfull = T.mesh_topology(tri[sel])
            assert (repeated, unpaired, overfull) == (0, 0, 0)
            assert np.count_nonzero(new_labels == c) - n_edges + sel.sum() == 2
        # ascending order survives, the maps index the input, colours and (unsmoothed) positions follow
        assert np.all(np.diff(vmap) > 0) and np.all(np.diff(tmap) > 0)
        assert np.array_equal(_bits(pos), _bits(v[vmap])) and np.array_equal(col, rgb[vmap])
        assert np.array_equal(vmap[tri], t[tmap])
        assert np.array_equal(np.unique(tri), np.arange(len(pos)))
        assert np.allclose(np.linalg.norm(nrm, axis=1), 1, atol=1e-6)
    # everything filtered out, and an empty mesh
    none = R.clean(v, rgb, t, R.options(min_component_triangles=4000))
    assert [len(a) for a in none] == [0] * 6
    assert [len(a) for a in R.clean(v, None, np.zeros((0, 3), np.int32))[:2]] == [0, 0]
    with pytest.raises(R.Rejected):
        R.clean(v, None, np.array([[0, 1, len(v)]]))


def test_pinning():
    """A closed sphere has no pinned vertex; the opened one has, and those stay where they are, bit for bit, unless pin_boundary
    is 0."""
    v, _, _, t = K.opened_sphere()
    assert T.mesh_topology(t)[1] > 0
    _, _, pinned = R.adjacency(t, len(v))
    assert 0 < pinned.sum() < len(v)
    keep_all = dict(min_component_triangles=1, min_component_permille=0, smooth_iterations=5)
    held = R.clean(v, None, t, R.options(pin_boundary=1, **keep_all))
    free = R.clean(v, None, t, R.options(pin_boundary=0, **keep_all))
    assert len(held[0]) == len(v) and np.array_equal(held[3], t)
    assert np.array_equal(_bits(held[0][pinned]), _bits(v[pinned]))
    assert np.all(np.any(held[0][~pinned] != v[~pinned], axis=1))
    assert np.all(np.any(free[0][pinned] != v[pinned], axis=1))


def test_positions_do_not_depend_on_triangle_order(three):
    """Shuffled triangles with rotated corners: positions are bit-identical (the adjacency is a sorted key list); the normals'
    sums run in triangle order by rule, so they agree to rounding."""
    v, t = three["v"], three["t"]
    rng = np.random.default_rng(12)
    order = rng.permutation(len(t))
    shift = rng.integers(0, 3, len(t))
    t2 = np.stack([t[np.arange(len(t)), (c + shift) % 3] for c in range(3)], 1)[order]
    o = R.options(min_component_triangles=1, min_component_permille=0)
    a, b = R.clean(v, None, t, o), R.clean(v, None, t2, o)
    assert np.any(a[0] != v) and np.array_equal(_bits(a[0]), _bits(b[0]))
    assert np.abs(a[1].astype(np.float64) - b[1]).max() <= 1e-5
    assert np.array_equal(b[5], np.sort(b[5])) and np.array_equal(t2, b[3])


def _radial_rms(pos, sel, centre, radius):
    d = np.linalg.norm(pos[sel].astype(np.float64) - centre, axis=1)
    return float(np.sqrt(np.mean(((d - radius) / K.THREE_H) ** 2)))


def _volume(pos, tri, sel, centre):
    tt = tri[sel[tri[:, 0]]]
    a, b, c = (pos[tt[:, i]].astype(np.float64) - centre for i in range(3))
    return float(np.sum(np.einsum("ij,ij->i", a, np.cross(b, c))) / 6)


def test_what_smoothing_buys(three):
    noise = np.random.default_rng(7).uniform(-0.3 * K.THREE_H, 0.3 * K.THREE_H, K.THREE_DIMS[::-1])
    v, _, _, t, centre, radius = K.three_spheres(noise, colours=False)
    labels, count, n = R.components(t, len(v))
    assert n == 3
    big = int(np.argmax(count))
    pos, _, _, tri, vmap, _ = R.clean(v, None, t, R.options(smooth_iterations=10))
    before, after = _radial_rms(v, labels == big, centre, radius), _radial_rms(pos, labels[vmap] == big, centre, radius)
    ratio = _volume(pos, tri, labels[vmap] == big, centre) / _volume(v, t, labels == big, centre)
    clean_pos, clean_nrm, _, _, clean_map, _ = R.clean(three["v"], None, three["t"], R.options(smooth_iterations=10))
    clean_labels, clean_count, _ = R.components(three["t"], len(three["v"]))
    sel = clean_labels[clean_map] == int(np.argmax(clean_count))
    radial = clean_pos[sel].astype(np.float64) - three["centre"]
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    angle = float(np.degrees(np.arccos(np.clip(np.sum(clean_nrm[sel] * radial, 1), -1, 1))).max())
    print(f"smoothing: radial RMS {before:.4f} h -> {after:.4f} h, volume ratio {ratio:.4f}, normal angle max {angle:.3f} deg")
    assert abs(before - REF_RMS_BEFORE) < 5e-4
    assert after <= MAX_RMS_AFTER and after < before
    assert abs(ratio - 1) <= 0.01
    assert angle <= MAX_NORMAL_ANGLE


def test_bad_arguments_are_rejected(E):
    """Each bad argument on its own, with its own message.  ctx is NULL: the argument checks come first, so a call with good
    arguments fails only with "ctx is NULL"; nothing is written."""
    L = E.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    V, Tn = 6, 3
    vertices = np.arange(3 * V, dtype=F).reshape(V, 3)
    rgb = np.full((V, 3), 9, np.uint8)
    tri = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5]], np.int32)
    out_v = np.full((V, 3), 7.0, F); out_n = np.full((V, 3), 7.0, F); out_c = np.full((V, 3), 7, np.uint8)
    out_t = np.full((Tn, 3), 7, np.int32); vmap = np.full(V, 7, np.int32); tmap = np.full(Tn, 7, np.int32)
    labels = np.full(V, 7, np.int32); count = np.full(V, 7, np.int32)
    nv, nt, nc = C.c_int32(5), C.c_int32(5), C.c_int32(5)

    d = E.default_mesh_clean_options()
    assert (d.min_component_triangles, d.min_component_permille, d.smooth_iterations, d.pin_boundary) == (64, 10, 5, 1)
    assert d.smooth_lambda == 0.5 and d.smooth_mu == F(-0.53)

    def opt(**kw):
        o = E.default_mesh_clean_options()
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def clean(o=None, V_=V, T_=Tn, t=tri, v=vertices, in_rgb=rgb, o_v=out_v, o_c=out_c, o_t=out_t, n_v=nv, n_t=nt, null_opt=False):
        return L.esfm_mesh_clean(None, V_, T_, p(v), p(in_rgb), p(t), None if null_opt else C.byref(o or opt()), p(o_v), p(out_n), p(o_c),
                                 p(o_t), p(vmap), p(tmap), C.byref(n_v) if n_v else None, C.byref(n_t) if n_t else None)

    def components(V_=V, T_=Tn, t=tri, lab=labels, n_c=nc):
        return L.esfm_mesh_components(None, V_, T_, p(t), p(lab), p(count), C.byref(n_c) if n_c else None)

    def rejected(call, message):
        status = call()
        err = L.esfm_last_error().decode()
        assert status == -1 and message in err, (status, err, message)

    def bad(i, value):
        t = tri.copy()
        t.reshape(-1)[i] = value
        return t

    inf, nan = float("inf"), float("nan")
    for kw, message in ((dict(), "ctx is NULL"),
                        (dict(o=opt(min_component_triangles=1, min_component_permille=0, smooth_iterations=0, pin_boundary=0)), "ctx is NULL"),
                        (dict(o=opt(min_component_permille=1000, smooth_iterations=1000, smooth_lambda=1.0, smooth_mu=-1.5)), "ctx is NULL"),
                        (dict(o=opt(smooth_mu=0.0)), "ctx is NULL"), (dict(in_rgb=None, o_c=None), "ctx is NULL"), (dict(o_c=None), "ctx is NULL"),
                        (dict(V_=0, T_=0), "ctx is NULL"), (dict(T_=0), "ctx is NULL"),
                        (dict(o=opt(min_component_triangles=0)), "min_component_triangles"), (dict(o=opt(min_component_triangles=-3)), "min_component_triangles"),
                        (dict(o=opt(min_component_permille=-1)), "min_component_permille"), (dict(o=opt(min_component_permille=1001)), "min_component_permille"),
                        (dict(o=opt(smooth_iterations=-1)), "smooth_iterations"), (dict(o=opt(smooth_iterations=1001)), "smooth_iterations"),
                        (dict(o=opt(smooth_lambda=0.0)), "smooth_lambda"), (dict(o=opt(smooth_lambda=-0.5)), "smooth_lambda"),
                        (dict(o=opt(smooth_lambda=1.5)), "smooth_lambda"), (dict(o=opt(smooth_lambda=nan)), "smooth_lambda"),
                        (dict(o=opt(smooth_lambda=inf)), "smooth_lambda"),
                        (dict(o=opt(smooth_mu=0.1)), "smooth_mu"), (dict(o=opt(smooth_mu=-1.6)), "smooth_mu"), (dict(o=opt(smooth_mu=nan)), "smooth_mu"),
                        (dict(o=opt(smooth_mu=-inf)), "smooth_mu"),
                        (dict(o=opt(pin_boundary=2)), "pin_boundary"), (dict(o=opt(pin_boundary=-1)), "pin_boundary"),
                        (dict(null_opt=True), "options are NULL"),
                        (dict(t=bad(4, V)), "triangle index"), (dict(t=bad(0, -1)), "triangle index"), (dict(t=bad(8, 2 ** 31 - 1)), "triangle index"),
                        (dict(V_=5), "triangle index"),
                        (dict(V_=-1), "n_vertices"), (dict(V_=2 ** 30 + 1, T_=0), "n_vertices"), (dict(T_=-1), "n_triangles"),
                        (dict(T_=2 ** 28 + 1, t=None), "n_triangles"),
                        (dict(v=None), "NULL argument"), (dict(t=None), "NULL argument"), (dict(o_v=None), "NULL argument"),
                        (dict(o_t=None), "NULL argument"), (dict(n_v=None), "NULL argument"), (dict(n_t=None), "NULL argument"),
                        (dict(in_rgb=None), "output array is requested without its input")):
        rejected(lambda: clean(**kw), message)
    for kw, message in ((dict(), "ctx is NULL"), (dict(T_=0), "ctx is NULL"), (dict(V_=0, T_=0), "ctx is NULL"),
                        (dict(t=bad(4, V)), "triangle index"), (dict(t=bad(7, -2)), "triangle index"), (dict(V_=3), "triangle index"),
                        (dict(V_=-1), "n_vertices"), (dict(T_=-1), "n_triangles"), (dict(T_=2 ** 28 + 1, t=None), "n_triangles"),
                        (dict(t=None), "NULL argument"), (dict(lab=None), "NULL argument"), (dict(n_c=None), "NULL argument")):
        rejected(lambda: components(**kw), message)
    assert (nv.value, nt.value, nc.value) == (5, 5, 5)
    assert np.all(out_v == 7.0) and np.all(out_n == 7.0) and np.all(out_c == 7) and np.all(out_t == 7) and np.all(vmap == 7) and np.all(tmap == 7)
    assert np.all(labels == 7) and np.all(count == 7)


def test_mesh_clean_has_no_cpu_fallback(E, three):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for call in (lambda: E.mesh_components(three["t"], len(three["v"])), lambda: E.mesh_clean(three["v"], three["rgb"], three["t"])):
        with pytest.raises(E.EsfmError) as ei:
            call()
        assert ei.value.status == -2, ei.value                            # ESFM_ERR_NO_DEVICE


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
def test_drivers_take_the_clean_form(E, tmp_path, driver):
    """clean:mesh.ply as the seventeenth argument passes argument parsing -- the run then ends on the missing image list --; one
    more argument is still the usage text (status 2), which names the new form next to the old ones."""
    cmd = _driver_cmd(driver, tmp_path, E)
    args = ["imgs", "list.txt", "K.txt", "none", str(tmp_path / "out.ply"), "S", "100", "1.0", "1", "0", "4", "1", "0", "ratio", "none", "none"]

    def run(extra):
        return subprocess.run(cmd + args + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=str(tmp_path))
    r = run(["clean:" + str(tmp_path / "mesh.ply")])
    assert r.returncode != 2 and "mesh.ply | none" not in r.stdout, r.stdout[-2000:]
    r = run(["clean:" + str(tmp_path / "mesh.ply"), "extra"])
    assert r.returncode == 2 and "mesh.ply | clean:mesh.ply | none" in r.stdout, r.stdout[-2000:]
    assert not (tmp_path / "mesh.ply").exists() and not (tmp_path / "clean:mesh.ply").exists()
