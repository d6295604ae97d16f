"""Feature type I (SIFT) through both drivers: ./bin/sfm_native and ./bin/sfm agree on every stage before the first bundle
adjustment and build a cloud; run_sfm takes SIFT frames with the ratio+cross filter."""
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stages(text):
    keys = ("verified matches", "total unique feature point number", "Initialization frames", "Triangulate [")
    return [l.strip() for l in text.splitlines() if any(k in l for k in keys)]


def test_both_drivers_run_sift(tmp_path):
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
    tail = ["I", "0", "1.0", "1", "0", "4", "1", "0"]
    out_c, out_p = tmp_path / "c" / "cloud.ply", tmp_path / "p" / "cloud.ply"
    rc = subprocess.run([exe] + args + [str(out_c)] + tail, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert rc.returncode == 1, rc.stdout[-3000:]
    assert "Wrong feature input" not in rc.stdout and "Output ply file done." in rc.stdout
    rp = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "sfm")] + args + [str(out_p)] + tail, stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT, text=True, timeout=600)
    assert rp.returncode == 1, rp.stdout[-3000:]
    assert "Wrong feature input" not in rp.stdout
    sc_, sp_ = _stages(rc.stdout), _stages(rp.stdout)
    assert len(sc_) > 10 and sc_ == sp_
    for out in (out_c, out_p):
        xyz, rgb, _ = E.read_ply_vertices(str(out))
        assert len(xyz) > 200 and np.all(np.isfinite(xyz))


def test_run_sfm_sift_ratio_cross(gpu_ctx):
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    K = np.array([[689.87 / 2, 0, 380.17 / 2], [0, 691.04 / 2, 251.70 / 2], [0, 0, 1]], np.float32)
    frames = []
    for i, img in enumerate(z["images"][:5]):
        f = E.Frame(frame_id=i, rgb_image=np.ascontiguousarray(np.stack([img] * 3, axis=2)))
        f.K_cam = K.copy()
        assert E.detectFeaturesSIFT(f, 0, ctx=gpu_ctx)
        assert f.descriptors.shape[1] == 128 and f.descriptors.dtype == np.float32
        frames.append(f)
    cloud, filtered, graph = E.run_sfm(frames, None, "I", 1.0, ctx=gpu_ctx, match_filter="ratio+cross")
    assert len(filtered.xyz) > 100
    assert sum(len(graph[i][j].matches) for i in range(len(frames)) for j in range(i)) > 200
