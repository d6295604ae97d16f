"""Pair selection through the pipeline on the MI355X (esfm.h "Image retrieval"): run_sfm's pair_selection option on the synthetic
scene of the pipeline test -- None changes nothing; RetrievalOptions(top_k=3, window=1) matches only the listed pairs and still
registers every camera within the all-pairs run's bound -- and the "+retrieval" token of both drivers."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _similarity(A, B):
    """Least-squares s, R, t with B ~ s R A + t (Umeyama)."""
    ma, mb = A.mean(0), B.mean(0)
    Ac, Bc = A - ma, B - mb
    U, S, Vt = np.linalg.svd(Bc.T @ Ac / len(A))
    D = np.eye(3); D[2, 2] = np.sign(np.linalg.det(U @ Vt))
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / (Ac ** 2).sum() * len(A)
    return s, R, mb - s * R @ ma


SELECTION = dict(top_k=3, window=1)


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """run_sfm on synth.sfm_scene() three times: without the argument, with pair_selection=None, with RetrievalOptions(top_k=3, window=1)"""
    data, K, poses, pts = synth.sfm_scene()
    out = {}
    for tag, kw in (("plain", {}), ("none", dict(pair_selection=None)), ("selected", dict(pair_selection=E.RetrievalOptions(**SELECTION)))):
        frames = []
        for i, f in enumerate(data):
            fr = E.Frame(frame_id=i, keypoints=f["keypoints"], descriptors=f["descriptors"])
            fr.K_cam = K.copy()
            frames.append(fr)
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            cloud, filtered, graph = E.run_sfm(frames, None, "S", 1.0, True, 0.0, 4, gpu_ctx, verbose=True, **kw)
        out[tag] = (frames, cloud, filtered, graph, log.getvalue())
    return data, poses, out


def _match_lists(graph):
    return [[(m.queryIdx, m.trainIdx, m.distance) for m in g.matches] for row in graph for g in row]


def test_none_changes_nothing(runs):
    """the cloud, the filtered cloud and every match list equal those of a call that does not pass the argument"""
    _, _, out = runs
    fa, ca, la, ga, text_a = out["plain"]
    fb, cb, lb, gb, text_b = out["none"]
    for a, b in ((ca, cb), (la, lb)):
        assert a.xyz.tobytes() == b.xyz.tobytes() and np.array_equal(a.unique_point_ids, b.unique_point_ids) and np.array_equal(a.rgb, b.rgb)
    assert _match_lists(ga) == _match_lists(gb)
    for a, b in zip(fa, fb):
        assert a.pose_cam.tobytes() == b.pose_cam.tobytes()
    assert text_a == text_b and "Pair selection:" not in text_a


def test_selected_run(runs, gpu_ctx):
    """only listed pairs carry matches; the list has at most 8 * 4 entries and holds every (i, i - 1); all 8 cameras end registered;
    the camera-centre error after similarity alignment stays below 0.05, the bound of the all-pairs run in tests/test_pipeline_gpu.py
    (the chain of adjacent pairs lets propagate_track_ids build the same full-length tracks)"""
    data, poses, out = runs
    frames, cloud, filtered, graph, text = out["selected"]
    n = len(frames)
    assert n == 8
    pairs = E.select_pairs([f["descriptors"] for f in data], E.ESFM_L2_F32, E.RetrievalOptions(**SELECTION), gpu_ctx)
    listed = {tuple(p) for p in pairs}
    lines = [l for l in text.splitlines() if l.startswith("Pair selection:")]
    print("\n".join(lines))
    d = data[0]["descriptors"].shape[1]
    assert lines == [f"Pair selection: [{len(pairs)}] of [28] pairs, [3] nearest of [8] images, window [1], codebook [64] x [{d}]"]
    assert len(pairs) <= 8 * 4 and all((i, i - 1) in listed for i in range(1, n))
    carrying = {(i, j) for i in range(n) for j in range(i) if graph[i][j].matches}
    assert carrying <= listed and all((i, i - 1) in carrying for i in range(1, n))
    for i in range(n):
        for j in range(i):
            if (i, j) not in listed:
                g = graph[i][j]
                assert not g.matches and g.appro_depth == 1.0 and np.array_equal(g.T_21, np.eye(4, dtype=np.float32))
    shown = {(int(l.split()[2]), int(l.split()[4])) for l in text.splitlines() if l.startswith("Pair (")}
    assert shown == carrying
    assert [l for l in text.splitlines() if l.startswith("Progress:")][-1] == "Progress: [ 8 / 8 ]"
    C_gt = np.array([-T[:3, :3].T @ T[:3, 3] for T in poses])
    C_est = np.array([-f.pose_cam[:3, :3].astype(np.float64).T @ f.pose_cam[:3, 3].astype(np.float64) for f in frames])
    s, R, t = _similarity(C_est, C_gt)
    err = np.linalg.norm((s * (R @ C_est.T).T + t) - C_gt, axis=1)
    print(f"selected {len(pairs)} of 28 pairs; largest camera-centre error {err.max():.5f}; {len(cloud.xyz)} points")
    assert err.max() < 0.05, err
    assert len(cloud.xyz) > 500 and 0 < len(filtered.xyz) <= len(cloud.xyz)


def test_pair_list_argument(gpu_ctx):
    """match_and_verify_all_pairs with a list: the listed pairs' results equal the all-pairs call's, the others stay default"""
    data, K, _, _ = synth.sfm_scene()

    def frames():
        out = []
        for i, f in enumerate(data[:5]):
            fr = E.Frame(frame_id=i, keypoints=f["keypoints"], descriptors=f["descriptors"])
            fr.K_cam = K.copy()
            out.append(fr)
        return out
    full = E.match_and_verify_all_pairs(frames(), "S", 1.0, 20, gpu_ctx)
    chosen = np.array([(1, 0), (3, 1), (4, 3)], np.int32)
    part = E.match_and_verify_all_pairs(frames(), "S", 1.0, 20, gpu_ctx, pairs=chosen)
    for i in range(5):
        for j in range(i):
            a, b = full[i][j], part[i][j]
            if (i, j) in {(1, 0), (3, 1), (4, 3)}:
                assert [(m.queryIdx, m.trainIdx) for m in a.matches] == [(m.queryIdx, m.trainIdx) for m in b.matches] and len(b.matches) > 20
                assert a.T_21.tobytes() == b.T_21.tobytes() and a.appro_depth == b.appro_depth
            else:
                assert not b.matches and b.appro_depth == 1.0
    empty = E.match_and_verify_all_pairs(frames(), "S", 1.0, 20, gpu_ctx, pairs=np.zeros((0, 2), np.int32))
    assert not any(g.matches for row in empty for g in row)
    for bad in ([(0, 1)], [(5, 0)], [(1, 0), (1, 0)]):
        with pytest.raises(ValueError):
            E.match_and_verify_all_pairs(frames(), "S", 1.0, 20, gpu_ctx, pairs=np.array(bad, np.int32))


def _fountain_files(tmp_path, count=6):
    PIL = pytest.importorskip("PIL.Image")
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    img_dir = tmp_path / "images"; img_dir.mkdir()
    names = []
    for i, img in enumerate(z["images"][:count]):
        names.append(f"{i:04d}.png")
        PIL.fromarray(np.stack([img] * 3, axis=2)).save(str(img_dir / names[-1]))
    (tmp_path / "image_list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "K.txt").write_text(f"{689.87 / 2} 0 {380.17 / 2}\n0 {691.04 / 2} {251.70 / 2}\n0 0 1\n")
    exe = os.path.join(ROOT, "bin", "sfm_native")
    if not os.path.exists(exe):
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "easysfm_amd", "csrc"), "../../bin/sfm_native"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
    return exe, [str(img_dir), str(tmp_path / "image_list.txt"), str(tmp_path / "K.txt"), "none"]


def test_both_drivers_with_ratio_retrieval3(tmp_path):
    """bin/sfm_native and bin/sfm with "ratio+retrieval3" on six fountain images: status 1, the same "Pair selection:" line, the same
    "Pair ( i , j )" lines; the native driver's pair-by-pair loop walks the same list; an ill-formed token gives the usage message"""
    exe, args = _fountain_files(tmp_path)
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0"]
    python = [sys.executable, os.path.join(ROOT, "bin", "sfm")]
    logs = {}
    for tag, cmd, env in (("native", [exe], {}), ("python", python, {}), ("native-pair-by-pair", [exe], {"ESFM_PAIR_BY_PAIR": "1"})):
        out = tmp_path / tag / "cloud.ply"
        r = subprocess.run(cmd + args + [str(out)] + tail + ["ratio+retrieval3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                           env=dict(os.environ, **env))
        assert r.returncode == 1, (tag, r.stdout[-3000:])
        assert "Output ply file done." in r.stdout
        xyz = E.read_ply_vertices(str(out))[0]
        assert len(xyz) > 200 and np.all(np.isfinite(xyz))
        logs[tag] = r.stdout

    def lines(text, key):
        return [l.strip() for l in text.splitlines() if l.startswith(key)]
    selection = lines(logs["native"], "Pair selection:")
    print("\n".join(selection))
    assert len(selection) == 1 and selection[0].endswith("pairs, [3] nearest of [6] images, window [0], codebook [64] x [64]")
    assert lines(logs["python"], "Pair selection:") == selection and lines(logs["native-pair-by-pair"], "Pair selection:") == selection
    shown = lines(logs["native"], "Pair (")
    assert len(shown) >= 5 and lines(logs["python"], "Pair (") == shown and lines(logs["native-pair-by-pair"], "Pair (") == shown
    n_selected = int(selection[0].split("[")[1].split("]")[0])
    assert len(shown) <= n_selected <= 15
    for bad in ("ratio+retrieval0", "ratio+retrieval+tracks", "ratio+retrieval1000", "ratio+retrieval3x", "+retrieval"):
        for cmd in ([exe], python):
            r = subprocess.run(cmd + args + [str(tmp_path / "never.ply")] + tail + [bad], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
            assert r.returncode == 2 and "retrieval" in r.stdout and "image_folder" in r.stdout, (bad, cmd, r.stdout[-500:])
    assert not os.path.exists(str(tmp_path / "never.ply"))
