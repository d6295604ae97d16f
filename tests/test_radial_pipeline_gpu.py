"""The incremental pipeline with free radial distortion (run_sfm's ba_radial_tolerance) on the synthetic scene of
tests/test_pipeline_gpu.py, seen through a lens with k1 = -0.10.

That scene is keypoints and descriptors, not pictures, so what is warped here is the keypoints: every detected pixel goes through
the forward model (x, y) -> (x, y) (1 + k1 r^2) in float64.  (The inverse the pipeline applies to them is cameras.pinhole_keypoints, 20
fixed-point steps.)  At the corner of the 768 x 512 image that is 17 pixels.  The parts that need pictures -- the undistortion in front
of the dense chain, and bin/sfm's +radial token end to end -- run on the fountain images."""
import contextlib
import copy
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import cameras, synth
from easysfm_amd.pipeline import undistort_registered_images

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1_TRUE = -0.10


def _frames(distort):
    data, K, poses, pts = synth.sfm_scene(8, 900, seed=7000)
    frames = []
    for i, f in enumerate(data):
        kp = f["keypoints"]
        if distort:
            Kd = K.astype(np.float64)
            x = (kp[:, 0].astype(np.float64) - Kd[0, 2]) / Kd[0, 0]; y = (kp[:, 1].astype(np.float64) - Kd[1, 2]) / Kd[1, 1]
            L = 1.0 + K1_TRUE * (x * x + y * y)
            kp = np.stack([x * L * Kd[0, 0] + Kd[0, 2], y * L * Kd[1, 1] + Kd[1, 2]], 1).astype(np.float32)
        fr = E.Frame(frame_id=i, keypoints=kp, descriptors=f["descriptors"])
        fr.K_cam = K.copy()
        frames.append(fr)
    return frames


def _cost_of_the_final_state(frames, cloud, ctx, radial):
    """what a bundle adjustment of the run's own kind starts from at the state the run left: the cost its last one ended at (up to
    the float write-back).  On COPIES: the frames and the cloud the run returned stay as it left them."""
    ba = E.BundleAdjustment(ctx)
    ba.doSFMBA(copy.deepcopy(frames), [False] * len(frames), copy.deepcopy(cloud), 0.0, -1, 1.0 if radial else 0.0)
    return ba.summary.initial_cost, ba.num_observations_


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """the distorted scene with and without the option: (frames, cloud before the filter, cost at the final state, observations, what
    the run printed)"""
    out = {}
    for radial in (False, True):
        frames = _frames(True)
        kw = dict(ba_radial_tolerance=1.0) if radial else {}
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            cloud, filtered, graph = E.run_sfm(frames, None, "S", 1.0, True, 0.0, 4, gpu_ctx, **kw)
        state = [(f.K_cam.tobytes(), f.radial_cam, f.keypoints.tobytes()) for f in frames]
        cost, n_obs = _cost_of_the_final_state(frames, cloud, gpu_ctx, radial)
        assert state == [(f.K_cam.tobytes(), f.radial_cam, f.keypoints.tobytes()) for f in frames]
        out[radial] = (frames, cloud, cost, n_obs, printed.getvalue())
    return out


def test_free_radial_distortion_lowers_the_cost_and_finds_k1(runs):
    frames, cloud, cost, n_obs, printed = runs[True]
    _, cloud0, cost0, n_obs0, printed0 = runs[False]
    k = [f.radial_cam for f in frames]
    print(f"\n[radial pipeline] pinhole: cost {cost0:.6g} over {n_obs0} observations, {len(cloud0.xyz)} points; radial: cost {cost:.6g} over {n_obs} "
          f"observations, {len(cloud.xyz)} points, k1 {k[0][0]:.6f} k2 {k[0][1]:.6f}")
    assert all(kk == k[0] for kk in k)                                    # one camera: every frame carries its coefficients
    assert all(f.K_cam.tobytes() == frames[0].K_cam.tobytes() for f in frames)          # ... and its K
    assert all(f.keypoints_raw is not None and not np.array_equal(f.keypoints_raw, f.keypoints) for f in frames)
    assert cost / n_obs < cost0 / n_obs0 and cost < cost0
    assert abs(k[0][0] - K1_TRUE) < abs(K1_TRUE) / 2.0                    # closer to the truth than the start, by at least half
    # keypoints is the pinhole-equivalent pixel of the final model, for every frame
    for f in frames:
        assert np.array_equal(f.keypoints, cameras.pinhole_keypoints(f.keypoints_raw, f.K_cam, f.radial_cam))
    # one "Distortion:" line, with the coefficients the frames carry
    lines = [ln for ln in printed.splitlines() if ln.startswith("Distortion:")]
    assert lines == [f"Distortion: camera 0: k1 [{k[0][0]:.6g}] k2 [{k[0][1]:.6g}]"] and lines[0] == cameras.distortion_line(frames)
    # without the option nothing of it shows
    assert all(f.keypoints_raw is None and f.radial_cam == (0.0, 0.0) for f in runs[False][0]) and "Distortion:" not in printed0


def test_option_absent_and_none_write_the_same_bytes(gpu_ctx, tmp_path):
    files = []
    for tag, kw in (("absent", {}), ("none", dict(ba_radial_tolerance=None))):
        out_file = str(tmp_path / f"{tag}.ply")
        E.run_sfm(_frames(False), out_file, "S", 1.0, True, 0.0, 4, gpu_ctx, **kw)
        files.append(open(out_file, "rb").read())
    assert files[0] == files[1] and len(files[0]) > 1000
    with pytest.raises(ValueError):
        E.run_sfm(_frames(False), None, "S", 1.0, True, 0.0, 4, gpu_ctx, ba_radial_tolerance=0.0)


def _fountain():
    return np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))["images"]


def test_registered_images_are_undistorted_with_their_cameras_k1_k2(gpu_ctx):
    """The step in front of the dense chain: each registered frame's image through esfm_undistort with ITS K_cam and (k1, k2, 0, 0) --
    not (k2, k1), not another frame's K; frames to be registered, frames without coefficients and frames without an image are
    left alone."""
    imgs = _fountain()[:4]
    K = np.array([[689.87 / 2, 0, 380.17 / 2], [0, 691.04 / 2, 251.70 / 2], [0, 0, 1]], np.float32)
    frames = []
    for i, img in enumerate(imgs):
        fr = E.Frame(frame_id=i, rgb_image=np.ascontiguousarray(np.stack([img] * 3, axis=2)))
        fr.K_cam = K.copy(); fr.K_cam[0, 0] += 10.0 * i
        fr.radial_cam = (-0.10 - 0.01 * i, 0.03)
        frames.append(fr)
    frames[2].radial_cam = (0.0, 0.0)
    before = [f.rgb_image.copy() for f in frames]
    todo = [False, False, False, True]
    undistort_registered_images(frames, todo, gpu_ctx)
    for i in (0, 1):
        want = E.undistort(before[i], frames[i].K_cam, np.array([frames[i].radial_cam[0], frames[i].radial_cam[1], 0.0, 0.0]), gpu_ctx)
        assert np.array_equal(frames[i].rgb_image, want) and not np.array_equal(want, before[i])
        swapped = E.undistort(before[i], frames[i].K_cam, np.array([frames[i].radial_cam[1], frames[i].radial_cam[0], 0.0, 0.0]), gpu_ctx)
        other_K = E.undistort(before[i], frames[1 - i].K_cam, np.array([frames[i].radial_cam[0], frames[i].radial_cam[1], 0.0, 0.0]), gpu_ctx)
        assert not np.array_equal(swapped, want) and not np.array_equal(other_K, want)
    assert np.array_equal(frames[2].rgb_image, before[2]) and np.array_equal(frames[3].rgb_image, before[3])
    no_image = [E.Frame(frame_id=0)]
    no_image[0].radial_cam = (-0.1, 0.0)
    undistort_registered_images(no_image, [False], gpu_ctx)
    assert no_image[0].rgb_image is None


def test_bin_sfm_radial_token_end_to_end(tmp_path):
    """./bin/sfm with ratio+radial as the match filter and a dense cloud as the 15th argument, on six fountain images: the reference's
    success code, one "Distortion:" line, the sparse and the dense .ply; and bin/sfm_native refuses the same filter."""
    PIL = pytest.importorskip("PIL.Image")
    img_dir = tmp_path / "images"; img_dir.mkdir()
    names = []
    for i, img in enumerate(_fountain()[:6]):
        names.append(f"{i:04d}.png")
        PIL.fromarray(np.stack([img] * 3, axis=2)).save(str(img_dir / names[-1]))
    (tmp_path / "image_list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "K.txt").write_text(f"{689.87 / 2} 0 {380.17 / 2}\r\n0 {691.04 / 2} {251.70 / 2}\r\n0 0 1")
    out, dense = tmp_path / "output" / "cloud.ply", tmp_path / "output" / "dense.ply"
    args = [str(img_dir), str(tmp_path / "image_list.txt"), str(tmp_path / "K.txt"), "none", str(out), "S", "100", "1.0", "1", "0", "4", "1", "0", "ratio+radial",
            str(dense)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "sfm")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 1, r.stdout[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Distortion:")]
    assert len(lines) == 1 and lines[0].startswith("Distortion: camera 0: k1 ["), r.stdout[-2000:]
    print("\n[radial pipeline] bin/sfm:", lines[0])
    xyz, rgb, cam = E.read_ply_vertices(str(out))
    assert len(xyz) > 200 and np.all(np.isfinite(xyz))
    dxyz, _, _ = E.read_ply_vertices(str(dense))
    assert len(dxyz) > 1000 and np.all(np.isfinite(dxyz))
    r = subprocess.run([os.path.join(ROOT, "bin", "sfm_native")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode != 0 and "+radial" in r.stderr and r.stderr.count("\n") == 1
