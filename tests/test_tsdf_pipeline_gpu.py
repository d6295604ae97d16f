"""The surface mesh end to end on the half-resolution fountain: both drivers with the seventeenth argument, against their own
runs without it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(text, start):
    return [l for l in text.splitlines() if l.startswith(start)]


def test_both_drivers_write_mesh(tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    exe = os.path.join(ROOT, "bin", "sfm_native")
    assert os.path.exists(exe), "bin/sfm_native not built: run __graft_entry__.build()"
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
        out = {}
        for run, extra in (("with", ["mesh.ply"]), ("without", [])):
            d = tmp_path / name / run
            r = subprocess.run(cmd + args + [str(d / "cloud.ply")] + tail + [str(d / "dense.ply"), str(d / "merged.ply")] + [str(d / e) for e in extra],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            assert r.returncode == 1, r.stdout[-3000:]
            out[run] = r.stdout
            assert len(_line(r.stdout, "Dense merge:")) == 1, r.stdout[-3000:]
        # the new argument changes none of the clouds, and without it nothing new is printed or written
        for f in ("cloud.ply", "dense.ply", "merged.ply"):
            assert (tmp_path / name / "with" / f).read_bytes() == (tmp_path / name / "without" / f).read_bytes(), (name, f)
        assert not _line(out["without"], "Dense mesh:") and sorted(os.listdir(tmp_path / name / "without")) == ["cloud.ply", "dense.ply", "merged.ply"]
        line = _line(out["with"], "Dense mesh:")
        assert len(line) == 1, out["with"][-3000:]
        vertices, normals, rgb, triangles = E.read_ply_mesh(str(tmp_path / name / "with" / "mesh.ply"))
        assert line[0].startswith(f"Dense mesh: [{len(vertices)}] vertices, [{len(triangles)}] triangles from ["), line[0]
        assert len(triangles) > 1000 and triangles.min() >= 0 and triangles.max() < len(vertices) and np.all(np.isfinite(vertices))
        has = np.any(normals != 0, axis=1)
        assert has.any() and np.all(np.abs(np.linalg.norm(normals[has].astype(np.float64), axis=1) - 1) <= 1e-6)   # (8 digits written)
        assert np.any(rgb[:, 0] != rgb[:, 2])                           # coloured
        # every triangle edge is shared by at most two triangles
        t = triangles.astype(np.int64)
        e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        _, shared = np.unique(np.minimum(e[:, 0], e[:, 1]) * len(vertices) + np.maximum(e[:, 0], e[:, 1]), return_counts=True)
        assert shared.max() <= 2
        print(f"{name}: {line[0]}  closed edges {np.mean(shared == 2):.3f}")
        counts.append(len(triangles))
    print("mesh triangles: native", counts[0], "python", counts[1])
    # the drivers differ before the mesh (image decoding aside, their sparse reconstructions are not the same run): the bound is
    # the one tests/test_mvs_pipeline_gpu.py holds their dense clouds to, which the volumes are made from
    assert abs(counts[0] - counts[1]) <= 0.15 * max(counts)
