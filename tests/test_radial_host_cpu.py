"""Free radial distortion, the host side that needs no GPU: the inverse model in cameras.py, the +radial token, the packing of the
BundleAdjustment mirror, and the native driver's refusal of the mode."""
import os
import subprocess

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import cameras, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pinhole_keypoints_inverts_the_model():
    """20 fixed-point steps at |k1| r^2 <= 0.12 x 0.6 contract by that factor per step: 0.072^20, far below f64; what is left is the
    float32 rounding of the pixel, 3e-5 at u ~ 700: bar 1e-4 px"""
    K = np.array([[700, 0, 380], [0, 690, 250], [0, 0, 1]], np.float32)
    x = np.random.default_rng(0).uniform(-0.55, 0.55, (2000, 2))
    for k1, k2 in ((-0.12, 0.03), (0.05, 0.0), (-0.10, 0.0)):
        r2 = (x ** 2).sum(1); L = 1 + k1 * r2 + k2 * r2 * r2
        raw = np.stack([700 * x[:, 0] * L + 380, 690 * x[:, 1] * L + 250], 1).astype(np.float32)
        pin = cameras.pinhole_keypoints(raw, K, (k1, k2))
        assert pin.dtype == np.float32 and np.abs(pin - np.stack([700 * x[:, 0] + 380, 690 * x[:, 1] + 250], 1)).max() < 1e-4
    raw = np.float32([[1.5, 2.5], [300, 200]])
    same = cameras.pinhole_keypoints(raw, K, (0.0, 0.0))
    assert same.tobytes() == raw.tobytes() and same is not raw
    # the optical axis maps to itself
    assert np.array_equal(cameras.pinhole_keypoints(np.float32([[380, 250]]), K, (-0.1, 0.02)), np.float32([[380, 250]]))


def test_radial_token():
    assert cameras.split_radial_token("ratio+radial") == ("ratio", True)
    assert cameras.split_radial_token("ratio+guided+tracks+retrieval4+radial") == ("ratio+guided+tracks+retrieval4", True)
    assert cameras.split_radial_token("ratio") == ("ratio", False) and cameras.split_radial_token("+radial") == ("+radial", False)
    # in front of +cameras when both are given: +cameras is stripped first
    f, multi = cameras.split_cameras_token("ratio+radial+cameras")
    assert multi and cameras.split_radial_token(f) == ("ratio", True)
    assert cameras.RADIAL_TOKEN_TOLERANCE == 1.0


def _frames(camera_ids):
    sc = synth.ba_scene(len(camera_ids), 120, 3, seed=9)
    frames = []
    for c, cid in enumerate(camera_ids):
        sel = np.nonzero(sc.cam_idx == c)[0]
        fr = E.Frame(frame_id=c, keypoints=sc.uv[sel])
        fr.unique_pixel_ids = sc.pt_idx[sel].astype(np.int64)
        fr.unique_pixel_has_match = np.ones(len(sel), bool)
        fr.K_cam = np.array([[2000.0 + c, 0, 700 + c], [0, 2100.0 + c, 500 + c], [0, 0, 1]], np.float32)
        fr.camera_id = cid
        fr.radial_cam = (-0.01 * (c + 1), 0.001 * (c + 1))
        frames.append(fr)
    cloud = E.SparsePointCloud(xyz=sc.pts0.astype(np.float32), unique_point_ids=np.arange(sc.n_pt))
    ba = E.BundleAdjustment.__new__(E.BundleAdjustment); ba._ctx = None; ba.options = None; ba.initBA()
    return ba, frames, cloud, sc


def test_setBAProblem_packs_one_radial_block_per_camera_id():
    assert E.Frame().radial_cam == (0.0, 0.0) and E.Frame().keypoints_raw is None
    ids, process = [7, 3, 7, 3, 5, 7], [False, True, False, False, False, False]       # frame 1 is not processed
    ba, frames, cloud, sc = _frames(ids)
    frames[2].keypoints_raw = frames[2].keypoints + np.float32(1.0)                  # a frame with raw pixels: those are observed
    ba.setBAProblem(frames, process, cloud, 25.0, 0, 0.5)
    assert ba.group_camera_ids_ == [7, 3, 5] and ba.camera_group_.tolist() == [0, 0, 1, 2, 0] and ba.radial_tolerance_ == 0.5
    n0 = 6 * 5 + 3 * sc.n_pt
    assert ba.num_parameters_ == n0 + 4 * 3 + 2 * 3
    first = {7: 0, 3: 3, 5: 4}
    for g, cid in enumerate(ba.group_camera_ids_):
        fr = frames[first[cid]]
        K = fr.K_cam
        assert ba.parameters_[n0 + 4 * g:][:4].tolist() == [K[0, 0], K[0, 2], K[1, 1], K[1, 2]]
        assert ba.parameters_[n0 + 12 + 2 * g:][:2].tolist() == [fr.radial_cam[0], fr.radial_cam[1]]
    cam1 = ba.camera_index_ == 1                                                       # frame 2 is processed camera 1
    rows = lambda a: sorted(map(tuple, np.asarray(a).tolist()))
    assert rows(ba.points_2d_[cam1]) == rows(frames[2].keypoints_raw) and rows(ba.points_2d_[cam1]) != rows(frames[2].keypoints)
    assert rows(ba.points_2d_[ba.camera_index_ == 0]) == rows(frames[0].keypoints)          # no raw pixels: the keypoints
    # solveBA takes the tolerance too, positive exactly when the problem was set up with radial blocks
    for args in ((25.0,), (25.0, 0.0)):
        with pytest.raises(ValueError, match="radial_tolerance"):
            ba.solveBA(*args)
    # ONE camera id still opens a (radial) block; with fixed pinhole intrinsics too
    ba1, frames1, cloud1, _ = _frames([4] * 6)
    ba1.setBAProblem(frames1, process, cloud1, 0.0, 0, 0.5)
    assert ba1.group_camera_ids_ == [4] and ba1.camera_group_.tolist() == [0] * 5 and ba1.num_parameters_ == n0 + 4 + 2
    # radial_tolerance 0 (and the argument left out): the packing as before, camera ids and radial_cam play no part
    for args in ((25.0, 0), (25.0, 0, 0.0)):
        ba2, frames2, cloud2, _ = _frames(ids)
        ba2.setBAProblem(frames2, process, cloud2, *args)
        assert ba2.num_parameters_ == n0 + 4 * 3 and ba2.radial_tolerance_ == 0.0
        with pytest.raises(ValueError, match="radial_tolerance"):
            ba2.solveBA(25.0, 0.5)
    ba3, frames3, cloud3, _ = _frames(ids)
    for fr in frames3:
        fr.radial_cam = (0.0, 0.0)
    ba3.setBAProblem(frames3, process, cloud3, 25.0, 0)
    assert ba3.parameters_.tobytes() == ba2.parameters_.tobytes() and ba3.points_2d_.tobytes() == ba2.points_2d_.tobytes()


def test_native_driver_refuses_the_radial_token(tmp_path):
    exe = os.path.join(ROOT, "bin", "sfm_native")
    for flt in ("ratio+radial", "ratio+guided+radial+cameras"):
        r = subprocess.run([exe, str(tmp_path), "list.txt", "K.txt", "none", str(tmp_path / "o.ply"), "S", "400", "1.0", "1", "0", "4", "0", "0", flt],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0 and r.stderr.count("\n") == 1 and "+radial" in r.stderr, (r.returncode, r.stderr)


def test_cpp_mirror_packs_one_radial_block_per_camera_id(tmp_path):
    """tests/cpp/ba_radial_host_check.cpp: setBAProblem of the esfm_host.hpp mirror with a radial tolerance, the assertions of the Python
    test above; a stand-alone host program, g++."""
    exe = str(tmp_path / "ba_radial_host_check")
    lib_dir = os.path.join(ROOT, "easysfm_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "ba_radial_host_check.cpp"), "-o", exe, os.path.join(lib_dir, "libesfm_hip.so"), "-lz",
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ba radial host check ok" in r.stdout, r.stdout[-4000:]
