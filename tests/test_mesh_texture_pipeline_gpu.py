"""The textured surface mesh end to end on the half-resolution fountain: both drivers with clean+simplify+texture:mesh.ply as the
seventeenth argument next to clean+simplify:mesh.ply -- a .ply with texture coordinates and its atlas as a .png that read back
consistently, "Mesh texture:" lines that agree as far as two drivers can, and everything before the texturing is what it was."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E
import texture_ref as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = r"Mesh texture: \[(\d+)\] triangles, \[(\d+)\] labelled from \[(\d+)\] views, charts of \[(\d+)\] texels, atlas \[(\d+)\] x \[(\d+)\]\."


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
def png_reader(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("png") / "png_reader")
    r = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "png_reader_main.cpp"), "-o", exe, "-lz"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


@pytest.fixture(scope="module")
def runs(fountain, tmp_path_factory):
    """Each driver once without and once with +texture: {driver: (directory, stdout of the plain run, stdout of the textured run)}."""
    exe = os.path.join(ROOT, "bin", "sfm_native")
    assert os.path.exists(exe), "bin/sfm_native not built: run __graft_entry__.build()"
    args = [str(fountain / "images"), str(fountain / "image_list.txt"), str(fountain / "K.txt"), "none"]
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0", "ratio"]
    out = {}
    for driver, cmd in (("native", [exe]), ("python", [sys.executable, os.path.join(ROOT, "bin", "sfm")])):
        root = tmp_path_factory.mktemp(driver)
        texts = []
        for name, prefix in (("plain", "clean+simplify:"), ("textured", "clean+simplify+texture:")):
            d = root / name
            r = subprocess.run(cmd + args + [str(d / "cloud.ply")] + tail + [str(d / "dense.ply"), str(d / "merged.ply"), prefix + str(d / "mesh.ply")],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            assert r.returncode == 1, r.stdout[-3000:]
            texts.append(r.stdout)
        out[driver] = (root, texts[0], texts[1])
    return out


@pytest.mark.parametrize("driver", ["native", "python"])
def test_driver_writes_a_textured_mesh(runs, png_reader, driver):
    root, out_p, out_t = runs[driver]
    assert sorted(os.listdir(root / "plain")) == ["cloud.ply", "dense.ply", "merged.ply", "mesh.ply"]
    assert sorted(os.listdir(root / "textured")) == ["cloud.ply", "dense.ply", "merged.ply", "mesh.ply", "mesh.png"]
    # without +texture nothing of it shows; everything before the texturing is what it was
    assert not _line(out_p, "Mesh texture:")
    for start in ("Dense reconstruction:", "Dense merge:", "Dense mesh:", "Mesh clean:", "Mesh simplify:"):
        assert len(_line(out_p, start)) == 1 and _line(out_p, start) == _line(out_t, start), start
    for name in ("cloud.ply", "dense.ply", "merged.ply"):
        assert (root / "plain" / name).read_bytes() == (root / "textured" / name).read_bytes(), name
    pv, pn, _, pt = E.read_ply_mesh(str(root / "plain" / "mesh.ply"))
    v, n, t, uv, texture = E.read_ply_textured_mesh(str(root / "textured" / "mesh.ply"))
    assert np.array_equal(v, pv) and np.array_equal(n, pn) and np.array_equal(t, pt) and texture == "mesh.png"
    line = _line(out_t, "Mesh texture:")
    assert len(line) == 1, out_t[-3000:]
    m = re.fullmatch(LINE, line[0])
    assert m, line[0]
    T_, labelled, views, S_, W, H = (int(g) for g in m.groups())
    A = E.mesh.default_atlas_width(T_)
    assert T_ == len(t) and 0.5 * T_ < labelled <= T_ and views == 6 and 4 <= S_ <= 64 and (H, W) == X.atlas_shape(T_, S_, A)
    # the texture coordinates: inside [0, 1], and the layout's within the 8 digits written
    assert uv.min() >= 0 and uv.max() <= 1 and np.abs(uv - X.texture_uv(T_, S_, A)).max() <= 2e-7
    # the atlas through the host layer's PNG reader: the stated size, texels of labelled triangles from the images
    raw = str(root / "textured" / "mesh.raw")
    r = subprocess.run([png_reader, str(root / "textured" / "mesh.png"), raw], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(H), str(W)], r.stdout
    atlas = np.fromfile(raw, np.uint8).reshape(H, W, 3)[..., ::-1]
    used = atlas[:(T_ + 1) // 2 // A * S_]                       # the full rows of squares
    assert used.std() > 10 and np.any(used[..., 0] != used[..., 2])
    print(f"{driver}: {line[0]}")


def test_drivers_agree_on_the_texture_line(runs):
    """The two drivers' "Mesh texture:" lines agree as far as two drivers' lines can.  Their sparse reconstructions are not the same
    run (tests/test_pipeline_gpu.py: the stages are equal up to the first bundle adjustment and no further), so they texture two
    meshes of the same surface -- DESIGN 8f: 9 044 and 9 088 triangles on these six views -- and the lines read
      native: Mesh texture: [9044] triangles, [8934] labelled from [6] views, charts of [4] texels, atlas [272] x [268].
      python: Mesh texture: [9088] triangles, [8960] labelled from [6] views, charts of [4] texels, atlas [272] x [268].
    Held here: the same form; the same views; the same derived chart size (the median triangle's leg is below the clamp of 4 texels
    on both); each driver's triangle count is that of its own "Mesh simplify:" line and its atlas the layout's for that count; the
    triangle counts within the 15 % that tests/test_tsdf_pipeline_gpu.py holds the two drivers' meshes to; at least 90 % labelled
    on both sides (the condition of the synthetic scene) and the two shares within 0.01 of each other -- the labelled share is a
    mean over some 9 000 triangles of the same surface under the same six photographs."""
    parsed = {}
    for driver in ("native", "python"):
        line = _line(runs[driver][2], "Mesh texture:")
        assert len(line) == 1
        m = re.fullmatch(LINE, line[0])
        assert m, line[0]
        parsed[driver] = T_, labelled, views, S_, W, H = tuple(int(g) for g in m.groups())
        kept = re.search(r"into \[\d+\] vertices, \[(\d+)\] triangles", _line(runs[driver][2], "Mesh simplify:")[0])
        assert T_ == int(kept.group(1)) and (H, W) == X.atlas_shape(T_, S_, E.mesh.default_atlas_width(T_))
        assert labelled >= 0.9 * T_
    n, p = parsed["native"], parsed["python"]
    assert n[2] == p[2] == 6 and n[3] == p[3]
    assert abs(n[0] - p[0]) <= 0.15 * max(n[0], p[0])
    assert abs(n[1] / n[0] - p[1] / p[0]) <= 0.01
    print("native:", n, "python:", p)
