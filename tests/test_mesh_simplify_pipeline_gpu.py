"""The simplified surface mesh end to end on the half-resolution fountain: both drivers with clean+simplify:mesh.ply as the
seventeenth argument next to clean:mesh.ply -- fewer triangles, the printed counts agree with the file, and everything before the
simplification is what it was."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(text, start):
    return [l for l in text.splitlines() if l.startswith(start)]


@pytest.fixture(scope="module")
def fountain(tmp_path_factory):
    PIL = pytest.importorskip("PIL.Image")
    root = tmp_path_factory.mktemp("fountain")
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    img_dir = root / "images"; img_dir.mkdir()
    names = []
    for i, img in enumerate(z["images"][:6]):
        names.append(f"{i:04d}.png")
        PIL.fromarray(np.stack([img, np.roll(img, 1, 1), img // 2 + 60], axis=2)).save(str(img_dir / names[-1]))
    (root / "image_list.txt").write_text("\n".join(names) + "\n")
    (root / "K.txt").write_text(f"{689.87 / 2} 0 {380.17 / 2}\n0 {691.04 / 2} {251.70 / 2}\n0 0 1\n")
    return root


@pytest.mark.parametrize("driver", ["native", "python"])
def test_driver_writes_a_simplified_mesh(fountain, tmp_path, driver):
    exe = os.path.join(ROOT, "bin", "sfm_native")
    assert os.path.exists(exe), "bin/sfm_native not built: run __graft_entry__.build()"
    cmd = [exe] if driver == "native" else [sys.executable, os.path.join(ROOT, "bin", "sfm")]
    args = [str(fountain / "images"), str(fountain / "image_list.txt"), str(fountain / "K.txt"), "none"]
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0", "ratio"]

    def run(name, prefix):
        d = tmp_path / name
        r = subprocess.run(cmd + args + [str(d / "cloud.ply")] + tail + [str(d / "dense.ply"), str(d / "merged.ply"), prefix + str(d / "mesh.ply")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 1, r.stdout[-3000:]
        assert sorted(os.listdir(d)) == ["cloud.ply", "dense.ply", "merged.ply", "mesh.ply"]
        return r.stdout

    out_c, out_s = run("clean", "clean:"), run("both", "clean+simplify:")
    assert not _line(out_c, "Mesh simplify:")
    line = _line(out_s, "Mesh simplify:")
    assert len(line) == 1, out_s[-3000:]
    # everything before the simplification is what it was
    for start in ("Dense reconstruction:", "Dense merge:", "Dense mesh:", "Mesh clean:"):
        assert len(_line(out_c, start)) == 1 and _line(out_c, start) == _line(out_s, start), start
    for name in ("cloud.ply", "dense.ply", "merged.ply"):
        assert (tmp_path / "clean" / name).read_bytes() == (tmp_path / "both" / name).read_bytes(), name
    cv, _, _, ct = E.read_ply_mesh(str(tmp_path / "clean" / "mesh.ply"))
    vertices, normals, rgb, triangles = E.read_ply_mesh(str(tmp_path / "both" / "mesh.ply"))
    m = re.fullmatch(r"Mesh simplify: \[(\d+)\] vertices, \[(\d+)\] triangles into \[(\d+)\] vertices, \[(\d+)\] triangles, cells of \[([0-9.e+-]+)\]\.", line[0])
    assert m, line[0]
    assert tuple(int(g) for g in m.groups()[:4]) == (len(cv), len(ct), len(vertices), len(triangles))
    voxel = float(re.search(r"voxels of \[([0-9.e+-]+)\]", _line(out_s, "Dense mesh:")[0]).group(1))
    assert abs(float(m.group(5)) - 2 * voxel) <= 1e-4 * voxel
    assert 0 < len(triangles) < len(ct) and 0 < len(vertices) < len(cv)
    assert triangles.min() == 0 and triangles.max() == len(vertices) - 1 and np.all(np.isfinite(vertices))
    assert np.array_equal(np.unique(triangles), np.arange(len(vertices)))
    lo, hi = cv.min(axis=0) - 2 * voxel, cv.max(axis=0) + 2 * voxel
    assert np.all(vertices >= lo) and np.all(vertices <= hi)
    has = np.any(normals != 0, axis=1)
    assert has.any() and np.all(np.abs(np.linalg.norm(normals[has].astype(np.float64), axis=1) - 1) <= 1e-6)   # (8 digits written)
    assert np.any(rgb[:, 0] != rgb[:, 2])                           # coloured
    print(f"{driver}: {_line(out_s, 'Mesh clean:')[0]}  {line[0]}")
