"""The cleaned surface mesh end to end on the half-resolution fountain: both drivers with clean:mesh.ply as the seventeenth
argument, and the Python driver's plain form next to it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E
import mesh_clean_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(text, start):
    return [l for l in text.splitlines() if l.startswith(start)]


def test_both_drivers_write_a_cleaned_mesh(tmp_path):
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
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0", "ratio", "none", "none"]
    python = [sys.executable, os.path.join(ROOT, "bin", "sfm")]

    def run(name, cmd, mesh_arg):
        d = tmp_path / name
        r = subprocess.run(cmd + args + [str(d / "cloud.ply")] + tail + [mesh_arg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=600)
        assert r.returncode == 1, r.stdout[-3000:]
        return r.stdout

    dense_lines = {}
    for name, cmd in (("c", [exe]), ("p", python)):
        out = run(name, cmd, "clean:" + str(tmp_path / name / "mesh.ply"))
        dense_lines[name] = _line(out, "Dense mesh:")
        line = _line(out, "Mesh clean:")
        assert len(dense_lines[name]) == 1 and len(line) == 1, out[-3000:]
        assert sorted(os.listdir(tmp_path / name)) == ["cloud.ply", "mesh.ply"]
        vertices, normals, rgb, triangles = E.read_ply_mesh(str(tmp_path / name / "mesh.ply"))
        m = re.fullmatch(r"Mesh clean: \[(\d+)\] of \[(\d+)\] components kept, \[(\d+)\] vertices, \[(\d+)\] triangles\.", line[0])
        assert m, line[0]
        kept, before, nv, nt = (int(g) for g in m.groups())
        labels, count, n = R.components(triangles, len(vertices))
        assert (kept, nv, nt) == (n, len(vertices), len(triangles)) and 1 <= kept <= before
        m = re.match(r"Dense mesh: \[(\d+)\] vertices, \[(\d+)\] triangles", dense_lines[name][0])
        assert nv <= int(m.group(1)) and nt <= int(m.group(2))
        # every piece of the written mesh has 64 triangles or more and at least 1 % of the largest
        sizes = count[count > 0]
        assert len(sizes) == n and sizes.min() >= 64 and 1000 * int(sizes.min()) >= 10 * int(sizes.max())
        assert len(triangles) > 1000 and triangles.min() >= 0 and triangles.max() < len(vertices) and np.all(np.isfinite(vertices))
        has = np.any(normals != 0, axis=1)
        assert has.any() and np.all(np.abs(np.linalg.norm(normals[has].astype(np.float64), axis=1) - 1) <= 1e-6)   # (8 digits written)
        assert np.any(rgb[:, 0] != rgb[:, 2])                           # coloured
        t = triangles.astype(np.int64)
        e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        _, shared = np.unique(np.minimum(e[:, 0], e[:, 1]) * len(vertices) + np.maximum(e[:, 0], e[:, 1]), return_counts=True)
        assert shared.max() <= 2
        print(f"{name}: {dense_lines[name][0]}  {line[0]}  closed edges {np.mean(shared == 2):.3f}")
    # without the prefix (run_sfm's dense_mesh_clean=None) the same mesh is extracted and nothing new is printed
    out = run("plain", python, str(tmp_path / "plain" / "mesh.ply"))
    assert not _line(out, "Mesh clean:") and _line(out, "Dense mesh:") == dense_lines["p"]
