"""Seam levelling end to end on the half-resolution fountain: both drivers with clean+simplify+texture+level:mesh.ply as the
seventeenth argument next to clean+simplify+texture:mesh.ply -- a "Mesh texture level:" line of the stated form whose counts fit the
driver's own "Mesh texture:" line, an atlas that differs, and without +level every file and every printed line what it is with it,
the atlas and that one line aside."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTURE = r"Mesh texture: \[(\d+)\] triangles, \[(\d+)\] labelled from \[(\d+)\] views, charts of \[(\d+)\] texels, atlas \[(\d+)\] x \[(\d+)\]\."
LEVEL = r"Mesh texture level: \[(\d+)\] nodes, \[(\d+)\] seam vertices, \[(\d+)\] iterations"


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


@pytest.fixture(scope="module")
def runs(fountain, tmp_path_factory):
    """Each driver once with +texture and once with +texture+level: {driver: (directory, stdout of the first, stdout of the second)}."""
    exe = os.path.join(ROOT, "bin", "sfm_native")
    assert os.path.exists(exe), "bin/sfm_native not built: run __graft_entry__.build()"
    args = [str(fountain / "images"), str(fountain / "image_list.txt"), str(fountain / "K.txt"), "none"]
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0", "ratio"]
    out = {}
    for driver, cmd in (("native", [exe]), ("python", [sys.executable, os.path.join(ROOT, "bin", "sfm")])):
        root = tmp_path_factory.mktemp(driver)
        texts = []
        for name, prefix in (("textured", "clean+simplify+texture:"), ("levelled", "clean+simplify+texture+level:")):
            d = root / name
            r = subprocess.run(cmd + args + [str(d / "cloud.ply")] + tail + [str(d / "dense.ply"), str(d / "merged.ply"), prefix + str(d / "mesh.ply")],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            assert r.returncode == 1, r.stdout[-3000:]
            texts.append(r.stdout)
        out[driver] = (root, texts[0], texts[1])
    return out


@pytest.mark.parametrize("driver", ["native", "python"])
def test_driver_levels_the_texture(runs, driver):
    root, out_t, out_l = runs[driver]
    files = ["cloud.ply", "dense.ply", "merged.ply", "mesh.ply", "mesh.png"]
    assert sorted(os.listdir(root / "textured")) == files and sorted(os.listdir(root / "levelled")) == files
    # the line, its form, and its counts against the driver's own "Mesh texture:" line
    line = _line(out_l, "Mesh texture level:")
    assert len(line) == 1, out_l[-3000:]
    m = re.fullmatch(LEVEL, line[0])
    assert m, line[0]
    nodes, seam_vertices, iterations = (int(g) for g in m.groups())
    t = re.fullmatch(TEXTURE, _line(out_l, "Mesh texture:")[0])
    assert t, _line(out_l, "Mesh texture:")
    labelled = int(t.group(2))
    v = E.read_ply_textured_mesh(str(root / "levelled" / "mesh.ply"))[0]
    # every labelled triangle takes part with three corners; a seam vertex has two nodes or more; a vertex has a node per label it meets
    assert 0 < seam_vertices <= nodes // 2 and 3 <= nodes <= 3 * labelled and nodes - seam_vertices >= 3 and nodes <= len(v) + 63 * seam_vertices
    assert 0 < iterations <= 200
    out_lines = out_l.splitlines()
    assert out_lines.index(line[0]) < out_lines.index(_line(out_l, "Mesh texture:")[0])
    # without +level: no such line, and every other line and file is the same; only the atlas differs
    assert not _line(out_t, "Mesh texture level:")
    timed = lambda l: "seconds" in l                                  # the drivers' wall-clock lines
    assert [l.replace("levelled", "textured") for l in out_lines if l != line[0] and not timed(l)] == [l for l in out_t.splitlines() if not timed(l)]
    for name in ("cloud.ply", "dense.ply", "merged.ply", "mesh.ply"):
        assert (root / "textured" / name).read_bytes() == (root / "levelled" / name).read_bytes(), name
    assert (root / "textured" / "mesh.png").read_bytes() != (root / "levelled" / "mesh.png").read_bytes()
    print(f"{driver}: {line[0]}")
