"""A data set taken with two cameras, end to end: run_sfm on the synthetic scene with every odd frame taken by a
camera of 0.8 x the focal lengths, against ground truth; both drivers with `+cameras` on images written to disk; and a one-camera
run given as `+cameras`, which must write the same .ply byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E

from test_multicamera_cpu import two_camera_scene
from test_pipeline_gpu import _similarity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reconstruct(data, Ks, ctx, out_file):
    frames = []
    for i, f in enumerate(data):
        fr = E.Frame(frame_id=i, keypoints=f["keypoints"], descriptors=f["descriptors"])
        fr.K_cam = Ks[i].copy(); fr.camera_id = i % 2
        frames.append(fr)
    cloud, filtered, graph = E.run_sfm(frames, out_file, "S", 1.0, True, 0.0, 4, ctx)
    return frames, cloud, filtered, graph


def _centre_errors(frames, poses):
    C_gt = np.array([-T[:3, :3].T @ T[:3, 3] for T in poses])
    C_est = np.array([-f.pose_cam[:3, :3].astype(np.float64).T @ f.pose_cam[:3, 3].astype(np.float64) for f in frames])
    s, R, t = _similarity(C_est, C_gt)
    return np.linalg.norm((s * (R @ C_est.T).T + t) - C_gt, axis=1), (s, R, t)


def test_run_sfm_with_two_cameras_against_ground_truth(gpu_ctx, tmp_path):
    """The measures of test_incremental_sfm_on_synthetic_scene with its bounds widened by 1.25 (at equal pixel noise the second
    camera's angular noise is 1 / 0.8 of the first's): centres < 0.0625, median point error < 0.0375, 97 % of the points within 0.2.
    Control: the same data with camera 0's K on every frame must miss the centre bound, or the scene would test nothing."""
    (data, K, poses, pts), Ks = two_camera_scene()
    frames, cloud, filtered, graph = _reconstruct(data, Ks, gpu_ctx, str(tmp_path / "two.ply"))
    kp_before = [f["keypoints"] for f in data]
    assert all(np.array_equal(fr.keypoints, kp) and np.array_equal(fr.K_cam, Kc) for fr, kp, Kc in zip(frames, kp_before, Ks))   # own pixels, own K afterwards
    assert all(len(graph[i][i - 1].matches) > 100 for i in range(1, 8))           # neighbouring pairs (one frame of each camera) are verified
    for i in range(1, 8):
        m = graph[i][i - 1].matches
        same = sum(data[i]["point_id"][a.queryIdx] == data[i - 1]["point_id"][a.trainIdx] and data[i]["point_id"][a.queryIdx] >= 0 for a in m)
        assert same >= 0.98 * len(m)
    err, (s, R, t) = _centre_errors(frames, poses)
    print(f"\n[multicamera] centre errors {np.round(err, 4)}")
    assert err.max() < 0.0625, err
    P = s * (R @ cloud.xyz.astype(np.float64).T).T + t
    id_to_pt = {}
    for f, fr in zip(data, frames):
        for k, uid in enumerate(fr.unique_pixel_ids):
            if f["point_id"][k] >= 0:
                id_to_pt.setdefault(int(uid), int(f["point_id"][k]))
    d = np.array([np.linalg.norm(P[k] - pts[id_to_pt[int(u)]]) for k, u in enumerate(cloud.unique_point_ids) if int(u) in id_to_pt])
    print(f"[multicamera] {len(d)} points, median error {np.median(d):.4f}, within 0.2: {np.mean(d < 0.2):.4f}")
    assert len(d) > 500 and np.median(d) < 0.0375 and np.mean(d < 0.2) > 0.97
    assert 0 < len(filtered.xyz) <= len(cloud.xyz)
    # control: one K for every frame
    try:
        wrong, _, _, _ = _reconstruct(data, [Ks[0]] * 8, gpu_ctx, str(tmp_path / "one.ply"))
        err_wrong, _ = _centre_errors(wrong, poses)
    except Exception as e:             # a reconstruction that falls apart misses the bound as well
        print(f"[multicamera] control failed outright: {e!r}")
        err_wrong = np.array([np.inf])
    print(f"[multicamera] control (camera 0's K everywhere): centre errors {np.round(err_wrong, 4)}")
    assert not err_wrong.max() < 0.0625


def _write_images(tmp_path, n=6):
    """The fountain images, the odd ones re-taken by a camera of 0.8 x the focal lengths about the same principal point at the same
    image size (an affine resampling: what that camera would see, with an empty border)."""
    PIL = pytest.importorskip("PIL.Image")
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    K0 = np.array([[689.87 / 2, 0, 380.17 / 2], [0, 691.04 / 2, 251.70 / 2], [0, 0, 1]])
    K1 = K0.copy(); K1[0, 0] *= 0.8; K1[1, 1] *= 0.8
    img_dir = tmp_path / "images"; img_dir.mkdir()
    names = []
    for i, img in enumerate(z["images"][:n]):
        names.append(f"{i:04d}.png")
        col = PIL.fromarray(np.stack([img, np.roll(img, 1, 1), img // 2 + 60], axis=2))
        if i % 2 == 1:          # output pixel (u', v') shows input pixel ((u' - cx) / 0.8 + cx, (v' - cy) / 0.8 + cy)
            cx, cy = K0[0, 2], K0[1, 2]
            col = col.transform(col.size, PIL.AFFINE, (1 / 0.8, 0, cx - cx / 0.8, 0, 1 / 0.8, cy - cy / 0.8), resample=PIL.BILINEAR)
        col.save(str(img_dir / names[-1]))
    (tmp_path / "image_list.txt").write_text("\n".join(names) + "\n")
    rows = lambda K: "\n".join(" ".join(repr(float(v)) for v in r) for r in K)
    (tmp_path / "K.txt").write_text(rows(K0) + "\n")
    (tmp_path / "K_one.txt").write_text(rows(K0) + "\n" + " ".join("0" for _ in names) + "\n")
    (tmp_path / "K_two.txt").write_text(rows(K0) + "\n" + rows(K1) + "\n" + " ".join(str(i % 2) for i in range(n)) + "\n")
    return [str(img_dir), str(tmp_path / "image_list.txt")]


def _drive(driver, args, k_file, out, match_filter):
    exe = [os.path.join(ROOT, "bin", "sfm_native")] if driver == "native" else [sys.executable, os.path.join(ROOT, "bin", "sfm")]
    r = subprocess.run(exe + args + [str(k_file), "none", str(out), "S", "100", "1.0", "1", "0", "4", "1", "0", match_filter],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 1, r.stdout[-3000:]
    assert "Output ply file done." in r.stdout
    return r.stdout


def test_both_drivers_with_two_cameras_agree_stage_by_stage(tmp_path):
    args = _write_images(tmp_path)
    out_c, out_p = tmp_path / "c" / "cloud.ply", tmp_path / "p" / "cloud.ply"
    text_c = _drive("native", args, tmp_path / "K_two.txt", out_c, "ratio+cameras")
    text_p = _drive("python", args, tmp_path / "K_two.txt", out_p, "ratio+cameras")
    assert "Cameras: 2 models, 3 / 3 images" in text_c and "Cameras: 2 models, 3 / 3 images" in text_p

    def stages(text):          # as test_native_sfm_matches_the_python_driver: everything up to the first bundle adjustment
        keys = ("verified matches", "total unique feature point number", "Initialization frames", "Triangulate [")
        return [l.strip() for l in text.splitlines() if any(k in l for k in keys)]
    sc_, sp_ = stages(text_c), stages(text_p)
    print("\n[multicamera drivers]", sc_)
    assert len(sc_) > 6 and sc_ == sp_
    assert any("Pair ( 1 , 0 )" in l for l in sc_)                                # a pair across the two cameras is verified
    xc, _, _ = E.read_ply_vertices(str(out_c)); xp, _, _ = E.read_ply_vertices(str(out_p))
    assert len(xc) > 100 and np.all(np.isfinite(xc)) and abs(len(xc) - len(xp)) <= 0.05 * len(xp)


@pytest.mark.parametrize("driver", ["native", "python"])
def test_one_camera_given_as_cameras_writes_the_same_ply(tmp_path, driver):
    args = _write_images(tmp_path)
    # (the images stay the two-camera ones: what matters is that both runs get the same input and one K)
    plain, token = tmp_path / "plain" / "cloud.ply", tmp_path / "token" / "cloud.ply"
    text_a = _drive(driver, args, tmp_path / "K.txt", plain, "ratio")
    text_b = _drive(driver, args, tmp_path / "K_one.txt", token, "ratio+cameras")
    assert "Cameras:" not in text_a and "Cameras: 1 models, 6 images" in text_b
    assert plain.read_bytes() == token.read_bytes()
