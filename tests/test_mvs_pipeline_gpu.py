"""Dense reconstruction end to end on the half-resolution fountain: run_sfm(dense_output_file=...) against the sparse cloud,
and both drivers with the fifteenth argument."""
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_HALF = np.array([[689.87 / 2, 0, 380.17 / 2], [0, 691.04 / 2, 251.70 / 2], [0, 0, 1]], np.float32)
DENSE_FLOOR = 167000       # about half of the first measured count, 335 270 (dense reconstruction)


def test_run_sfm_dense_fountain(gpu_ctx, tmp_path):
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    frames = []
    for i, img in enumerate(z["images"]):
        fr = E.Frame(frame_id=i, rgb_image=img)
        fr.K_cam = K_HALF.copy()
        E.detectFeaturesSURF(fr, 100, ctx=gpu_ctx)
        frames.append(fr)
    dense_file = str(tmp_path / "dense.ply")
    cloud, _, _ = E.run_sfm(frames, str(tmp_path / "sparse.ply"), "S", 1.0, True, 0.0, 4, gpu_ctx, dense_output_file=dense_file)
    xyz, rgb, _ = E.read_ply_vertices(dense_file)
    print(f"fountain dense: {len(xyz)} points")
    assert len(xyz) >= DENSE_FLOOR and np.all(np.isfinite(xyz))
    dense, nb, rng, depth, cost = E.dense_reconstruction(frames, [False] * len(frames), cloud, ctx=gpu_ctx)
    assert len(dense.xyz) == len(xyz) and np.sum(rng[:, 0] > 0) >= 9
    # the sparse points each view observes, projected into it, against the depth map where it has an estimate
    from easysfm_amd.mvs import observations
    off, pts = observations(frames, cloud)
    track = np.bincount(pts, minlength=len(cloud.xyz))                     # views that observe each sparse point
    rel, tracks = [], []
    for v, f in enumerate(frames):
        P, K = f.pose_cam[:3, :4].astype(np.float64), f.K_cam.astype(np.float64)
        idx = pts[off[v]:off[v + 1]]
        p = cloud.xyz[idx].astype(np.float64) @ P[:, :3].T + P[:, 3]
        front = p[:, 2] > 0
        idx, p = idx[front], p[front]
        u = np.rint(K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2]).astype(int)
        w = np.rint(K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]).astype(int)
        ins = (u >= 0) & (u < depth.shape[2]) & (w >= 0) & (w < depth.shape[1])
        d = depth[v][w[ins], u[ins]]
        has = d > 0
        rel.append(np.abs(d[has] - p[ins][has, 2]) / p[ins][has, 2])
        tracks.append(track[idx[ins][has]])
    rel, tracks = np.concatenate(rel), np.concatenate(tracks)
    long = tracks >= 3
    print(f"fountain dense vs sparse: {len(rel)} points, median {np.median(rel):.4f}, within 3 % {np.mean(rel < 0.03):.3f}; "
          f"points seen by 3+ views: {int(long.sum())}, median {np.median(rel[long]):.4f}, within 3 % {np.mean(rel[long] < 0.03):.3f}")
    # all observed points (measured 1.47 %, 76.2 %): most are two-view points, whose own depth is the noisier side;
    # the points three or more views triangulate hold the issue's 1 % (measured 0.58 %, 90.7 %)
    assert len(rel) > 500 and np.median(rel) <= 0.02 and np.mean(rel < 0.03) >= 0.6
    assert long.sum() > 200 and np.median(rel[long]) <= 0.01 and np.mean(rel[long] < 0.03) >= 0.6


def _dense_line(text):
    return [l for l in text.splitlines() if l.startswith("Dense reconstruction:")]


def test_both_drivers_write_dense_cloud(tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    exe = os.path.join(ROOT, "bin", "sfm_native")
    if not os.path.exists(exe):
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "easysfm_amd", "csrc"), "../../bin/sfm_native"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    img_dir = tmp_path / "images"; img_dir.mkdir()
    names = []
    for i, img in enumerate(z["images"][:6]):
        names.append(f"{i:04d}.png")
        PIL.fromarray(np.stack([img, np.roll(img, 1, 1), img // 2 + 60], axis=2)).save(str(img_dir / names[-1]))
    (tmp_path / "image_list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "K.txt").write_text(f"{689.87 / 2} 0 {380.17 / 2}\n0 {691.04 / 2} {251.70 / 2}\n0 0 1\n")
    args = [str(img_dir), str(tmp_path / "image_list.txt"), str(tmp_path / "K.txt"), "none"]
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0", "ratio"]
    counts = []
    for name, cmd in (("c", [exe]), ("p", [sys.executable, os.path.join(ROOT, "bin", "sfm")])):
        dense = tmp_path / name / "dense.ply"
        r = subprocess.run(cmd + args + [str(tmp_path / name / "cloud.ply")] + tail + [str(dense)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 1, r.stdout[-3000:]
        line = _dense_line(r.stdout)
        assert len(line) == 1, r.stdout[-3000:]
        xyz, rgb, _ = E.read_ply_vertices(str(dense))
        assert line[0].endswith(f"[{len(xyz)}] points.")
        assert len(xyz) > 5000 and np.all(np.isfinite(xyz))
        assert np.any(rgb[:, 0] != rgb[:, 2])                           # coloured (the channels differ)
        if name == "c":
            assert "dense seconds:" in r.stdout
        counts.append(len(xyz))
    print("dense points: native", counts[0], "python", counts[1])
    assert abs(counts[0] - counts[1]) <= 0.15 * max(counts)
    r = subprocess.run([exe] + args + [str(tmp_path / "n" / "cloud.ply")] + tail + ["none"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 1 and not _dense_line(r.stdout) and "dense seconds" not in r.stdout
    assert sorted(os.listdir(tmp_path / "n")) == ["cloud.ply"]
