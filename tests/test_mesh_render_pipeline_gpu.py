"""The re-render of the surface mesh end to end on the half-resolution fountain: both drivers with a directory as the eighteenth
argument -- one PNG per registered frame, a "Mesh render:" line in the stated form, the textured mesh nearer to the photographs
than the same driver's vertex-coloured one -- and the same build run without it writes the same bytes to every other file and prints
the same stage lines (a run of seventeen arguments against a run of eighteen; the parent commit itself is not run here)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_mesh_texture_pipeline_gpu import fountain, png_reader  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = r"Mesh render: \[(\d+)\] views, \[(\d+)\] covered pixels, mean absolute error \[(\d+\.\d{3})\]"
STAGES = ("Dense reconstruction:", "Dense merge:", "Dense mesh:", "Mesh clean:", "Mesh simplify:", "Mesh texture:")


def _line(text, start):
    return [l for l in text.splitlines() if l.startswith(start)]


@pytest.fixture(scope="module")
def runs(fountain, tmp_path_factory):  # noqa: F811
    """Each driver three times: textured without the eighteenth argument, textured with it, vertex-coloured with it:
    {driver: (directory, the three stdouts)}."""
    exe = os.path.join(ROOT, "bin", "sfm_native")
    assert os.path.exists(exe), "bin/sfm_native not built: run __graft_entry__.build()"
    args = [str(fountain / "images"), str(fountain / "image_list.txt"), str(fountain / "K.txt"), "none"]
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0", "ratio"]
    out = {}
    for driver, cmd in (("native", [exe]), ("python", [sys.executable, os.path.join(ROOT, "bin", "sfm")])):
        root = tmp_path_factory.mktemp(driver)
        texts = []
        for name, prefix, render in (("before", "clean+simplify+texture:", False), ("textured", "clean+simplify+texture:", True), ("coloured", "clean+simplify:", True)):
            d = root / name
            extra = []
            if render:
                (d / "renders").mkdir(parents=True)
                extra = [str(d / "renders")]
            r = subprocess.run(cmd + args + [str(d / "cloud.ply")] + tail + [str(d / "dense.ply"), str(d / "merged.ply"), prefix + str(d / "mesh.ply")] + extra,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            assert r.returncode == 1, r.stdout[-3000:]
            texts.append(r.stdout)
        out[driver] = (root, texts)
    return out


def _parse(text):
    line = _line(text, "Mesh render:")
    assert len(line) == 1, text[-3000:]
    m = re.fullmatch(LINE, line[0])
    assert m, line[0]
    return int(m.group(1)), int(m.group(2)), float(m.group(3))


@pytest.mark.parametrize("driver", ["native", "python"])
def test_driver_re_renders_the_mesh(runs, png_reader, driver):  # noqa: F811
    root, (before, textured, coloured) = runs[driver]
    names = [f"render_{i:04d}.png" for i in range(6)]
    assert sorted(os.listdir(root / "textured" / "renders")) == names and sorted(os.listdir(root / "coloured" / "renders")) == names
    # without the eighteenth argument nothing of it shows; with it every other file and stage line is that of the run without
    assert not _line(before, "Mesh render:") and sorted(os.listdir(root / "before")) == ["cloud.ply", "dense.ply", "merged.ply", "mesh.ply", "mesh.png"]
    for name in ("cloud.ply", "dense.ply", "merged.ply", "mesh.ply", "mesh.png"):
        assert (root / "before" / name).read_bytes() == (root / "textured" / name).read_bytes(), name
    for start in STAGES:
        assert len(_line(before, start)) == 1 and _line(before, start) == _line(textured, start), start
    views_t, covered_t, error_t = _parse(textured)
    views_c, covered_c, error_c = _parse(coloured)
    print(f"{driver}: textured {_line(textured, 'Mesh render:')[0]}\n{driver}: coloured {_line(coloured, 'Mesh render:')[0]}")
    assert views_t == views_c == 6 and covered_t == covered_c                         # one mesh, one coverage
    assert 0.3 * 6 * 256 * 384 < covered_t < 6 * 256 * 384
    assert 0 < error_t < error_c < 40
    # a picture through the host layer's PNG reader: the photographs' size, the background black, the rest not
    raw = str(root / "textured" / "render.raw")
    r = subprocess.run([png_reader, str(root / "textured" / "renders" / names[2]), raw], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["256", "384"], r.stdout
    picture = np.fromfile(raw, np.uint8).reshape(256, 384, 3)
    assert 0.3 < picture.any(axis=2).mean() <= 1.0 and picture.std() > 10


def test_drivers_agree_on_the_render_line(runs):
    """Both drivers print the line in one form with integer sums behind it.  Their sparse reconstructions are not the same run
    (tests/test_mesh_texture_pipeline_gpu.py says why), so they draw two meshes of the same surface: held here are the same views, a
    coverage within 5 % and a textured error within 15 % of each other -- means over some 200 000 pixels of the same six
    photographs."""
    n, p = _parse(runs["native"][1][1]), _parse(runs["python"][1][1])
    print("native:", n, "python:", p)
    assert n[0] == p[0] == 6
    assert abs(n[1] - p[1]) <= 0.05 * max(n[1], p[1]) and abs(n[2] - p[2]) <= 0.15 * max(n[2], p[2])
