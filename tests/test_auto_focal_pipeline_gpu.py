"""The uncalibrated start end to end (esfm.h "Fundamental-matrix RANSAC"; run_sfm's auto_focal): the free-hand scene reconstructed
without a calibration matrix against the same run given the true one, and the arc scene, where the focal length cannot be told."""
import numpy as np
import pytest

import easysfm_amd as E

import fundamental_cases as Cs
from test_pipeline_gpu import _similarity

pytestmark = pytest.mark.gpu

TOLERANCE_BA = 50.0


def _frames(data, K):
    frames = []
    for i, f in enumerate(data):
        fr = E.Frame(frame_id=i, keypoints=f["keypoints"], descriptors=f["descriptors"])
        if K is not None:
            fr.K_cam = K.copy()
        frames.append(fr)
    return frames


def _measures(data, pts, frames, cloud, f_true):
    """(final focal error: |mean of fx, fy over the frames - f_true|, median cloud error after the similarity that maps the cloud's
    points onto their scene points, frames without a pose)"""
    focal = float(np.mean([[f.K_cam[0, 0], f.K_cam[1, 1]] for f in frames]))
    id_to_pt = {}
    for f, fr in zip(data, frames):
        for k, uid in enumerate(fr.unique_pixel_ids):
            if f["point_id"][k] >= 0:
                id_to_pt.setdefault(int(uid), int(f["point_id"][k]))
    keep = [k for k, u in enumerate(cloud.unique_point_ids) if int(u) in id_to_pt]
    P = cloud.xyz.astype(np.float64)[keep]
    Q = pts[[id_to_pt[int(cloud.unique_point_ids[k])] for k in keep]]
    s, R, t = _similarity(P, Q)
    d = np.linalg.norm((s * (R @ P.T).T + t) - Q, axis=1)
    unposed = sum(bool(np.array_equal(f.pose_cam, np.eye(4, dtype=np.float32))) for f in frames)
    return abs(focal - f_true), float(np.median(d)), unposed, focal, len(d)


def test_auto_focal_on_the_free_hand_scene_against_the_known_K_run(gpu_ctx, capsys):
    """run_sfm(auto_focal=AutoFocalOptions(), fix_calib_tolerance_BA=50) registers every frame and prints `estimated`; its final focal
    error and its median cloud error stay within 2 x those of the same run given the true K (for the focal error the grid step, 1.8 %
    of f, if the known-K run's own error is zero to rounding)."""
    data, K, poses, pts = Cs.freehand_scene(0)
    known = _frames(data, K)
    cloud_k, _, _ = E.run_sfm(known, None, "S", 1.0, True, TOLERANCE_BA, 4, gpu_ctx)
    fe_k, ce_k, unposed_k, focal_k, n_k = _measures(data, pts, known, cloud_k, Cs.FREEHAND_F)
    capsys.readouterr()
    auto = _frames(data, None)
    cloud_a, filtered, _ = E.run_sfm(auto, None, "S", 1.0, True, TOLERANCE_BA, 4, gpu_ctx,
                                     auto_focal=E.AutoFocalOptions(image_size=(Cs.WIDTH, Cs.HEIGHT)))
    out = capsys.readouterr().out
    fe_a, ce_a, unposed_a, focal_a, n_a = _measures(data, pts, auto, cloud_a, Cs.FREEHAND_F)
    lines = [l for l in out.splitlines() if l.startswith("Auto focal:")]
    with capsys.disabled():
        print(f"\n[auto focal] known K: final f {focal_k:.3f} (error {fe_k:.3f}), median cloud error {ce_k:.5f} over {n_k} points, {unposed_k} frame(s) at the identity")
        print(f"[auto focal] auto:    final f {focal_a:.3f} (error {fe_a:.3f}), median cloud error {ce_a:.5f} over {n_a} points, {unposed_a} frame(s) at the identity")
        print("[auto focal] " + " | ".join(lines))
    assert len(lines) == 1 and "estimated" in lines[0]
    assert unposed_k <= 1 and unposed_a <= 1                      # the first frame of the initial pair keeps the identity
    assert n_a > 500 and len(filtered.xyz) > 0
    bar_f = 2.0 * fe_k if fe_k > 1e-3 else 0.018 * Cs.FREEHAND_F
    assert fe_a <= bar_f, (fe_a, bar_f)
    assert ce_a <= 2.0 * ce_k, (ce_a, ce_k)


def test_auto_focal_on_the_arc_scene_falls_back_and_finishes(gpu_ctx, capsys):
    """cameras equidistant from the point they fixate: the cost curve is flat, the run says `fallback`, takes 1.2 x the longer side and
    still reconstructs"""
    data, K, poses, pts = Cs.arc_scene()
    frames = _frames(data, None)
    cloud, filtered, _ = E.run_sfm(frames, None, "S", 1.0, True, TOLERANCE_BA, 4, gpu_ctx,
                                   auto_focal=E.AutoFocalOptions(image_size=(Cs.WIDTH, Cs.HEIGHT)))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Auto focal:")]
    assert len(lines) == 1 and "fallback" in lines[0] and "estimated" not in lines[0]
    assert f"[{1.2 * Cs.WIDTH:.2f}]" in lines[0]
    assert len(cloud.xyz) > 100 and len(filtered.xyz) > 0


def test_calibrate_hook_sees_the_matches_once(gpu_ctx):
    """match_and_verify_all_pairs calls `calibrate` once, before K_cam is read, with the matched pixels of the pairs it will verify; a
    hook that changes nothing leaves every output as without it"""
    data, K, poses, pts = Cs.freehand_scene(0)
    calls = []

    def hook(pairs, sel, off, p1, p2):
        calls.append((len(pairs), len(sel), int(off[-1]), p1.shape, p2.shape))

    g0 = E.match_and_verify_all_pairs(_frames(data[:4], K), "S", 1.0, 20, gpu_ctx)
    g1 = E.match_and_verify_all_pairs(_frames(data[:4], K), "S", 1.0, 20, gpu_ctx, calibrate=hook)
    assert len(calls) == 1 and calls[0][0] == 6 and calls[0][3] == (calls[0][2], 2) == calls[0][4]
    for i in range(4):
        for j in range(i):
            assert [(m.queryIdx, m.trainIdx) for m in g0[i][j].matches] == [(m.queryIdx, m.trainIdx) for m in g1[i][j].matches]
            assert np.array_equal(g0[i][j].T_21, g1[i][j].T_21)


def test_bin_sfm_with_auto_as_the_calibration_file(tmp_path):
    """./bin/sfm with the word auto in place of K.txt on six fountain images: the image size comes from the pictures, one "Auto focal:"
    line names the verdict (either one: nothing is known about these photographs' focal cost curve), exit status 1 and a cloud."""
    import os
    import subprocess
    import sys
    PIL = pytest.importorskip("PIL.Image")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    z = np.load(os.path.join(root, "tests", "golden", "fountain11_half_gray.npz"))
    img_dir = tmp_path / "images"; img_dir.mkdir()
    names = []
    for i, img in enumerate(z["images"][:6]):
        names.append(f"{i:04d}.png")
        PIL.fromarray(np.stack([img] * 3, axis=2)).save(str(img_dir / names[-1]))
    (tmp_path / "image_list.txt").write_text("\n".join(names) + "\n")
    out = tmp_path / "output" / "cloud.ply"
    r = subprocess.run([sys.executable, os.path.join(root, "bin", "sfm"), str(img_dir), str(tmp_path / "image_list.txt"), "auto", "none",
                        str(out), "S", "100", "1.0", "1", "50", "4", "1", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("Auto focal:")]
    print("\n[auto focal] bin/sfm: " + " | ".join(lines))
    assert r.returncode == 1, r.stdout[-2000:]
    assert len(lines) == 1 and ("estimated" in lines[0] or "fallback" in lines[0]) and "ba_calib_change_tolerance is 0" not in r.stdout
    assert "No calibration file" in r.stdout and "Output ply file done." in r.stdout
    xyz, rgb, cam = E.read_ply_vertices(str(out))
    assert len(xyz) > 100 and np.all(np.isfinite(xyz))
