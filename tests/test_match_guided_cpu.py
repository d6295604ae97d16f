"""Epipolar-guided matching (esfm_match_guided_*, include/esfm.h "Epipolar-guided matching") without a GPU: the ABI surface, no CPU
fallback, the numpy restatement (tests/guided_ref.py) against the oracle's RANSAC mask, property (b), what the guided pass buys
on the repeated-structure scene, and the drivers' handling of the new filter names.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guided_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUIDED_SYMBOLS = ("esfm_match_guided_pairs_dev", "esfm_match_guided_pairs", "esfm_knn2_guided_pairs_dev", "esfm_match_guided_l2_f32",
                  "esfm_match_guided_hamming")


def _built_lib():
    import easysfm_amd as E
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return E


def test_guided_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "esfm.h")).read()
    from easysfm_amd._lib import EXPORTED_SYMBOLS
    assert "Epipolar-guided matching" in hdr
    for s in GUIDED_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in EXPORTED_SYMBOLS, s
    L = _built_lib().lib()
    for s in GUIDED_SYMBOLS:
        assert hasattr(L, s), s
    from easysfm_amd import MATCH_FILTERS
    assert MATCH_FILTERS[:3] == ("ratio", "cross", "ratio+cross")
    assert set(MATCH_FILTERS[3:]) == {"ratio+guided", "cross+guided", "ratio+cross+guided"}


def test_guided_entry_points_have_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    E = _built_lib()
    q = np.zeros((3, 64), np.float32); t = np.zeros((4, 64), np.float32)
    kq = np.zeros((3, 2), np.float32); kt = np.zeros((4, 2), np.float32)
    Em = np.eye(3); K4 = np.array([700, 380, 700, 250], np.float32)
    for call in (lambda: E.match_guided_l2(q, kq, t, kt, Em, K4, 1.0, 0.5),
                 lambda: E.match_guided_l2(q, kq, t, kt, Em, K4, 1.0, None, True),
                 lambda: E.match_guided_hamming(np.zeros((3, 32), np.uint8), kq, np.zeros((4, 32), np.uint8), kt, Em, K4, 1.0, 0.8),
                 lambda: E.match_guided_pairs_host([q, t], [kq, kt], [(0, 1)], [Em], [K4], 1.0, 0.5)):
        with pytest.raises(E.EsfmError) as ei:
            call()
        assert ei.value.status == -2, ei.value          # ESFM_ERR_NO_DEVICE: the context cannot be created


def test_l2_rows_is_the_oracles_canonical_sum(oracle_lib):
    rng = np.random.default_rng(5)
    for dim in (64, 128, 20, 7):
        a = rng.standard_normal((40, dim)).astype(np.float32); b = rng.standard_normal((40, dim)).astype(np.float32)
        want = np.array([np.sqrt(np.float32(oracle_lib.l2sqr(a[i], b[i]))) for i in range(40)], np.float32)
        assert G.l2_rows(a, b).tobytes() == want.tobytes(), dim


def test_guided_table_on_a_hand_built_pair():
    """E = [t]x for a sideways translation: the epipolar line of a query is its own image row, so adm is |dv| within the threshold."""
    E = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)
    K4 = np.array([100, 0, 100, 0], np.float32)
    kq = np.array([[10, 10], [10, 50], [10, 90]], np.float32)
    kt = np.array([[30, 10.2], [40, 10.4], [50, 50.1], [60, 70], [70, np.nan]], np.float32)
    dq = np.zeros((3, 8), np.float32)
    dt = np.zeros((5, 8), np.float32); dt[:, 0] = [3, 3, 1, 0, 0]
    adm = G.admissible(kq, kt, E, K4, 1.0)
    assert adm.tolist() == [[True, True, False, False, False], [False, False, True, False, False], [False] * 5]
    idx, dist, n_adm, ridx, rdist = G.knn2_guided(G.L2, dq, kq, dt, kt, E, K4, 1.0)
    assert idx.tolist() == [[0, 1], [2, -1], [-1, -1]]                  # the tie between rows 0 and 1 goes to the lower index
    assert dist[0].tolist() == [3.0, 3.0] and dist[1, 0] == 1.0 and dist[1, 1] == G.FLT_MAX and dist[2, 0] == G.FLT_MAX
    assert n_adm.tolist() == [2, 1, 0]
    assert ridx.tolist() == [[0, -1], [0, -1], [1, -1], [-1, -1], [-1, -1]]
    # ratio: a query with one admissible row emits nothing; q0's 3.0 < 0.5 * 3.0 fails
    assert len(G.filter_lists(idx, dist, ridx, rdist, 0.5, False)[0]) == 0
    # cross alone: q0 <-> t0 and q1 <-> t2 are mutual; t1's nearest is q0 but q0's is t0
    q, t, d = G.filter_lists(idx, dist, ridx, rdist, None, True)
    assert q.tolist() == [0, 1] and t.tolist() == [0, 2] and d.tolist() == [3.0, 1.0]
    # +inf admits every finite row, never the NaN keypoint
    assert G.admissible(kq, kt, E, K4, np.inf).tolist() == [[True, True, True, True, False]] * 3


@pytest.fixture(scope="module")
def scene_runs(oracle_lib):
    """Per filter, per pair (i, j < i) of the scene with an essential matrix: the plain list, the oracle's RANSAC (E, mask), the
    restatement's guided list at 1 px and the union."""
    frames, K, _, _ = G.scene()
    K4 = G.k4_of(K)
    runs = {}
    for name, (ratio, cross) in G.FILTERS.items():
        rows = []
        for i in range(len(frames)):
            for j in range(i):
                fi, fj = frames[i], frames[j]
                q, t, d = G.plain_lists(oracle_lib, fi["descriptors"], fj["descriptors"], ratio, cross)
                if len(q) <= 20:
                    continue
                ok, E, mask, _, _ = oracle_lib.find_essential_ransac(fi["keypoints"][q], fj["keypoints"][t], K4, 0.99, 1.0)
                if not ok:
                    continue
                guided = G.match_guided(G.L2, fi["descriptors"], fi["keypoints"], fj["descriptors"], fj["keypoints"], E, K4, 1.0, ratio, cross)
                rows.append(dict(i=i, j=j, plain=(q, t, d), E=E, mask=mask, guided=guided, union=G.union((q[mask], t[mask], d[mask]), guided)))
        runs[name] = rows
    return frames, K4, runs


def _true(frames, i, j, q, t):
    a = frames[i]["point_id"][q]; b = frames[j]["point_id"][t]
    return int(((a == b) & (a >= 0)).sum())


def test_predicate_is_the_oracles_ransac_mask(scene_runs):
    frames, K4, runs = scene_runs
    n = 0
    for rows in runs.values():
        assert len(rows) == 28
        for r in rows:
            q, t, _ = r["plain"]
            adm = G.admissible_rows(frames[r["i"]]["keypoints"][q], frames[r["j"]]["keypoints"][t], r["E"], K4, 1.0)
            assert np.array_equal(adm, r["mask"]), (r["i"], r["j"], int((adm != r["mask"]).sum()))
            n += len(q)
    assert n > 10000


def test_property_b_on_the_restatement(scene_runs):
    """A plain inlier (q, t): if q emits anything under the guided filter it emits the same t; the union has one train row per
    query, and with a cross filter one query per train row."""
    _, _, runs = scene_runs
    for name, rows in runs.items():
        for r in rows:
            q, t, _ = r["plain"]
            emitted = dict(zip(r["guided"][0].tolist(), r["guided"][1].tolist()))
            for a, b in zip(q[r["mask"]].tolist(), t[r["mask"]].tolist()):
                assert emitted.get(a, b) == b, (name, r["i"], r["j"], a)
            uq, ut, _ = r["union"]
            assert len(np.unique(uq)) == len(uq) and np.all(np.diff(uq) > 0)
            if G.FILTERS[name][1]:
                assert len(np.unique(ut)) == len(ut), (name, r["i"], r["j"])


def test_guided_pass_on_the_repeated_structure_scene(scene_runs):
    frames, _, runs = scene_runs
    fig = {}
    for name, rows in runs.items():
        plain = sum(int(r["mask"].sum()) for r in rows)
        uni = sum(len(r["union"][0]) for r in rows)
        uni_true = sum(_true(frames, r["i"], r["j"], r["union"][0], r["union"][1]) for r in rows)
        lst = sum(len(r["plain"][0]) for r in rows)
        lst_true = sum(_true(frames, r["i"], r["j"], r["plain"][0], r["plain"][1]) for r in rows)
        fig[name] = dict(plain=plain, union=uni, precision=uni_true / uni, list_precision=lst_true / lst)
        print(name, fig[name])
    for name in ("ratio", "ratio+cross"):
        assert fig[name]["union"] >= 3 * fig[name]["plain"], fig[name]
        assert fig[name]["precision"] >= 0.99, fig[name]              # the junk cap of 1 %
    # cross alone keeps its junk with or without the guided pass: only not below the plain cross list's precision
    assert fig["cross"]["precision"] >= fig["cross"]["list_precision"], fig["cross"]


@pytest.mark.parametrize("driver", ["python", "native"])
def test_drivers_and_the_guided_filter_names(tmp_path, driver):
    """"guided" alone is no filter (status 2, the usage text); "ratio+guided" passes argument parsing -- the run then ends on the
    missing image list, not on the filter."""
    def run(match_filter):
        args = ["imgs", "list.txt", "K.txt", "none", str(tmp_path / "out.ply"), "S", "100", "1.0", "1", "0", "4", "1", "0", match_filter]
        if driver == "python":
            cmd = [sys.executable, os.path.join(ROOT, "bin", "sfm")] + args
        else:
            exe = os.path.join(ROOT, "bin", "sfm_native")
            if not os.path.exists(exe):
                _built_lib()
                exe = str(tmp_path / "sfm_native")
                if not os.path.exists(exe):
                    cmd = ["g++", "-O2", "-std=c++17", os.path.join(ROOT, "easysfm_amd", "host", "sfm_main.cpp"), "-o", exe,
                           os.path.join(ROOT, "easysfm_amd", "libesfm_hip.so"), "-lz", "-pthread", "-Wl,-rpath," + os.path.join(ROOT, "easysfm_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                    assert r.returncode == 0, r.stdout
            cmd = [exe] + args
        return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=str(tmp_path))
    r = run("guided")
    assert r.returncode == 2, r.stdout[-2000:]
    assert "match_filter" in r.stdout and "ratio+cross+guided" in r.stdout
    r = run("ratio+guided")
    assert r.returncode != 2, r.stdout[-2000:]
    assert "ratio+cross+guided" not in r.stdout                     # not the usage text
    assert not (tmp_path / "out.ply").exists()
