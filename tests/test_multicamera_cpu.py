"""Multiple-camera mode in front of the solver, the parts that need no GPU (easysfm_amd/cameras.py and both drivers' arguments):
the `+cameras` token with every existing suffix combination, the `9 G + N` calibration file and the distortion file with their
error cases, the remap of keypoints into the canonical camera's pixels, and the scene generator with per-camera intrinsics."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth
from easysfm_amd.cameras import (canonical_camera, cameras_line, check_one_image_size, pair_stage_view, parse_camera_distort, parse_camera_file,
                                 remap_keypoints, split_cameras_token)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ["ratio", "cross", "ratio+cross", "ratio+guided", "cross+guided", "ratio+cross+guided"]
EVERY_FILTER = [f + t + r for f, t, r in itertools.product(FILTERS, ["", "+tracks"], ["", "+retrieval", "+retrieval4"])]
K_A = np.array([[690.0, 0, 380.0], [0, 691.0, 252.0], [0, 0, 1]], np.float32)
K_B = np.array([[552.0, 0, 381.5], [0, 552.8, 250.0], [0, 0, 1]], np.float32)


def _k_text(*Ks):
    return "\n".join(" ".join(repr(float(v)) for v in K.ravel()) for K in Ks)


@pytest.mark.parametrize("head", EVERY_FILTER)
def test_cameras_token_is_stripped_first_and_leaves_the_grammar_alone(head):
    assert split_cameras_token(head + "+cameras") == (head, True)
    assert split_cameras_token(head) == (head, False)


def test_cameras_token_only_at_the_very_end():
    assert split_cameras_token("+cameras") == ("+cameras", False)                    # a filter must stand in front of it
    assert split_cameras_token("ratio+cameras+tracks") == ("ratio+cameras+tracks", False)
    assert split_cameras_token("ratio+cameras+cameras") == ("ratio+cameras", True)   # ... which the driver then refuses


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("multicamera_args")
    (d / "list.txt").write_text("a.png\nb.png\nc.png\n")
    (d / "K_ok.txt").write_text(_k_text(K_A, K_B) + "\n0 1 0\n")
    (d / "K_index.txt").write_text(_k_text(K_A, K_B) + "\n0 2 0\n")
    (d / "K_count.txt").write_text(_k_text(K_A, K_B) + "\n0 1\n")
    (d / "D_bad.txt").write_text("0.1 0.2 0.3\n")
    return d


def _drivers():
    return {"native": [os.path.join(ROOT, "bin", "sfm_native")], "python": [sys.executable, os.path.join(ROOT, "bin", "sfm")]}


def _run(driver, d, k_file, distort, match_filter):
    r = subprocess.run(_drivers()[driver] + [str(d), str(d / "list.txt"), str(d / k_file), distort if distort == "none" else str(d / distort),
                                             str(d / "out.ply"), "S", "100", "1.0", "1", "0", "4", "1", "0", match_filter],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    return r.returncode, r.stdout


@pytest.mark.parametrize("driver,filters", [("native", EVERY_FILTER), ("python", ["ratio", "ratio+guided+tracks+retrieval4"])])
def test_drivers_accept_the_token_behind_every_filter(run_dir, driver, filters):
    """A well-formed filter with +cameras gets past the usage check (exit status 2) to the camera file, whose bad index ends the run
    with status 3 and a message -- before any image is looked at."""
    for f in filters:
        rc, out = _run(driver, run_dir, "K_index.txt", "none", f + "+cameras")
        assert rc == 3 and "camera file" in out and "[0, 2)" in out, (f, rc, out[-500:])


@pytest.mark.parametrize("driver", ["native", "python"])
def test_drivers_refuse_malformed_camera_arguments(run_dir, driver):
    for bad in ("ratio+cameras+tracks", "ratio+cameras+cameras", "+cameras", "ratio+camera"):
        assert _run(driver, run_dir, "K_ok.txt", "none", bad)[0] == 2, bad
    rc, out = _run(driver, run_dir, "K_count.txt", "none", "ratio+cameras")
    assert rc == 3 and "expected 9 G + 3" in out, out[-500:]
    rc, out = _run(driver, run_dir, "K_ok.txt", "D_bad.txt", "ratio+cameras")
    assert rc == 3 and "distortion file" in out and "expected 4 (all cameras) or 8" in out, out[-500:]
    rc, out = _run(driver, run_dir, "K_ok.txt", "none", "ratio+cameras")           # the files are fine: one line, then the images are missing
    assert rc != 2 and "Cameras: 2 models, 2 / 1 images" in out, out[-500:]


def test_camera_file_parser():
    K, idx = parse_camera_file(_k_text(K_A, K_B) + "\n0 1 1 0 1\n", 5)
    assert K.dtype == np.float32 and K.shape == (2, 3, 3) and np.array_equal(K[0], K_A) and np.array_equal(K[1], K_B)
    assert idx.dtype == np.int32 and idx.tolist() == [0, 1, 1, 0, 1]
    assert cameras_line(idx, 2) == "Cameras: 2 models, 2 / 3 images"
    K, idx = parse_camera_file(_k_text(K_A) + " 0 0 0", 3)                         # one camera, every index 0
    assert K.shape == (1, 3, 3) and idx.tolist() == [0, 0, 0] and cameras_line(idx, 1) == "Cameras: 1 models, 3 images"
    for text, n in ((_k_text(K_A, K_B) + " 0 1", 3),            # an index short
                    (_k_text(K_A, K_B) + " 0 1 0 1", 3),        # one too many
                    (_k_text(K_A), 3),                          # no indices at all
                    ("0 1 0", 3),                               # no matrix
                    (_k_text(K_A, K_B) + " 0 2 0", 3),          # index out of range
                    (_k_text(K_A, K_B) + " 0 -1 0", 3),
                    (_k_text(K_A, K_B) + " 0 0.5 0", 3),        # not an integer
                    (_k_text(K_A, K_B) + " 0 x 0", 3)):
        with pytest.raises(ValueError, match="camera file"):
            parse_camera_file(text, n)


def test_camera_distortion_parser(tmp_path):
    assert not parse_camera_distort(None, 3).any() and parse_camera_distort(None, 3).shape == (3, 4)
    # four numbers: every camera, stored exactly as the one-camera reader stores them
    p = tmp_path / "d.txt"; p.write_text("-0.1 0.02 0.001 -0.002\n")
    one = E.import_distort(str(p))
    both = parse_camera_distort(p.read_text(), 2)
    assert both[0].tobytes() == one.tobytes() and both[1].tobytes() == one.tobytes()
    per = parse_camera_distort("-0.1 0.02 0.001 -0.002  0.3 0 0 0.004", 2)
    assert per[0].tobytes() == one.tobytes() and per[1].view(np.float32)[:4].tolist() == np.array([0.3, 0, 0, 0.004], np.float32).tolist()
    for text in ("0.1 0.2 0.3", "1 2 3 4 5 6 7 8 9 10 11 12", "1 2 3 x"):
        with pytest.raises(ValueError, match="distortion file"):
            parse_camera_distort(text, 2)


def test_remap_is_the_identity_for_equal_K_and_a_projection_otherwise():
    rng = np.random.default_rng(5)
    kp = rng.uniform(0, 760, (500, 2)).astype(np.float32)
    assert remap_keypoints(kp, K_A, K_A.copy()) is kp                              # bitwise equal K: the same array object
    out = remap_keypoints(kp, K_B, K_A)
    assert out.dtype == np.float32 and out is not kp
    # against a float64 projection: the rays of camera B's pixels, seen by the canonical camera
    Kb, Ka = K_B.astype(np.float64), K_A.astype(np.float64)
    rays = np.concatenate([kp.astype(np.float64), np.ones((len(kp), 1))], 1) @ np.linalg.inv(Kb).T
    want = (rays / rays[:, 2:3]) @ Ka.T
    assert np.abs(out - want[:, :2]).max() <= 2e-4                                 # one float32 rounding at <= 1024 px: 6e-5
    # and points of the scene project into B and A so that the remap joins them
    X = rng.uniform(-1, 1, (200, 3)) + [0, 0, 6.0]
    ub = (X / X[:, 2:3]) @ Kb.T; ua = (X / X[:, 2:3]) @ Ka.T
    assert np.abs(remap_keypoints(ub[:, :2].astype(np.float32), K_B, K_A) - ua[:, :2]).max() <= 3e-4


def _frames(Ks, ids):
    frames = []
    for i, (K, cid) in enumerate(zip(Ks, ids)):
        fr = E.Frame(frame_id=i, keypoints=np.full((4, 2), 100.0 + i, np.float32))
        fr.K_cam = K.copy(); fr.camera_id = cid
        frames.append(fr)
    return frames


def test_pair_stage_view_swaps_and_restores():
    frames = _frames([K_B, K_A, K_B, K_A], [1, 0, 1, 0])
    assert np.array_equal(canonical_camera(frames), K_A)                          # camera_id 0's, not frame 0's
    before = [(f.keypoints, f.K_cam) for f in frames]
    with pair_stage_view(frames) as active:
        assert active
        assert all(np.array_equal(f.K_cam, K_A) for f in frames)
        assert frames[1].keypoints is before[1][0] and frames[3].keypoints is before[3][0]       # camera 0's frames: untouched
        assert np.allclose(frames[0].keypoints[:, 0], (100.0 - 381.5) * 690.0 / 552.0 + 380.0, atol=1e-4)
    assert all(f.keypoints is kp and f.K_cam is K for f, (kp, K) in zip(frames, before))
    with pytest.raises(RuntimeError):                                              # restored on the way out of a failure too
        with pair_stage_view(frames):
            raise RuntimeError("pair stage failed")
    assert all(f.keypoints is kp and f.K_cam is K for f, (kp, K) in zip(frames, before))
    # one K for all frames, whatever the ids say: nothing is touched
    same = _frames([K_A] * 3, [0, 1, 2])
    before = [(f.keypoints, f.K_cam) for f in same]
    with pair_stage_view(same) as active:
        assert not active and all(f.keypoints is kp and f.K_cam is K for f, (kp, K) in zip(same, before))


def test_dense_outputs_need_one_image_size():
    frames = _frames([K_A, K_B], [0, 1])
    frames[0].rgb_image = np.zeros((48, 64, 3), np.uint8); frames[1].rgb_image = np.zeros((48, 64, 3), np.uint8)
    check_one_image_size(frames)                                                   # different intrinsics at one size are fine
    frames[1].rgb_image = np.zeros((40, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="one size"):
        check_one_image_size(frames)


def two_camera_scene():
    """sfm_scene(8, 900, seed 7000) with the odd frames taken by a second camera of 0.8 x the focal lengths, same principal point."""
    K0 = np.array([[synth.FOUNTAIN_K4[0], 0, synth.FOUNTAIN_K4[1]], [0, synth.FOUNTAIN_K4[2], synth.FOUNTAIN_K4[3]], [0, 0, 1]], np.float32)
    K1 = K0.copy(); K1[0, 0] *= np.float32(0.8); K1[1, 1] *= np.float32(0.8)
    Ks = [K0 if c % 2 == 0 else K1 for c in range(8)]
    return synth.sfm_scene(8, 900, seed=7000, K_per_cam=Ks), Ks


def test_two_camera_scene_loses_no_visible_point():
    one = synth.sfm_scene(8, 900, seed=7000)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(one[0], synth.sfm_scene(8, 900, seed=7000, K_per_cam=None)[0]) for k in a)
    (data, K, poses, pts), Ks = two_camera_scene()
    assert np.array_equal(K, Ks[0]) and np.array_equal(poses, one[2]) and np.array_equal(pts, one[3])
    for c, (f1, f2) in enumerate(zip(one[0], data)):
        seen1, seen2 = set(f1["point_id"][f1["point_id"] >= 0].tolist()), set(f2["point_id"][f2["point_id"] >= 0].tolist())
        assert np.array_equal(f2["K"], Ks[c])
        if c % 2 == 0:
            assert seen1 == seen2 and np.array_equal(f1["keypoints"], f2["keypoints"])
        else:
            # the wider camera sees at least what the first sees (the detector's 10 % misses are separate draws per frame: compare
            # what is IN VIEW, which the smaller focal length can only enlarge)
            Xc = pts @ poses[c][:3, :3].T + poses[c][:3, 3]
            def in_view(Kc):
                u = Xc[:, 0] / Xc[:, 2] * Kc[0, 0] + Kc[0, 2]; v = Xc[:, 1] / Xc[:, 2] * Kc[1, 1] + Kc[1, 2]
                return (Xc[:, 2] > 1) & (u > 5) & (u < 763) & (v > 5) & (v < 507)
            assert np.all(in_view(Ks[c])[in_view(Ks[0])])
            assert len(seen2) >= 0.85 * np.count_nonzero(in_view(Ks[0]))
