"""Track triangulation through the pipeline on the MI355X (esfm.h "Track triangulation"): run_sfm's track_refine option on the
synthetic scene of the pipeline test -- None changes nothing, TrackOptions() leaves a cloud whose every point passes the
verdict, no more gross errors and cameras no worse -- and the "+tracks" token of both drivers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _similarity(A, B):
    """Least-squares s, R, t with B ~ s R A + t (Umeyama)."""
    ma, mb = A.mean(0), B.mean(0)
    Ac, Bc = A - ma, B - mb
    U, S, Vt = np.linalg.svd(Bc.T @ Ac / len(A))
    D = np.eye(3); D[2, 2] = np.sign(np.linalg.det(U @ Vt))
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / (Ac ** 2).sum() * len(A)
    return s, R, mb - s * R @ ma


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """run_sfm on synth.sfm_scene() three times: without the argument, with track_refine=None, with TrackOptions()"""
    import contextlib
    import io
    data, K, poses, pts = synth.sfm_scene()
    out = {}
    for tag, kw in (("plain", {}), ("none", dict(track_refine=None)), ("refine", dict(track_refine=E.TrackOptions()))):
        frames = []
        for i, f in enumerate(data):
            fr = E.Frame(frame_id=i, keypoints=f["keypoints"], descriptors=f["descriptors"])
            fr.K_cam = K.copy()
            frames.append(fr)
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            cloud, filtered, _ = E.run_sfm(frames, None, "S", 1.0, True, 0.0, 4, gpu_ctx, **kw)
        out[tag] = (frames, cloud, filtered, log.getvalue())
    return data, poses, pts, out


def _errors(data, poses, pts, frames, cloud):
    """camera-centre errors and point errors against the truth after the similarity of the camera centres (the pipeline test's)"""
    C_gt = np.array([-T[:3, :3].T @ T[:3, 3] for T in poses])
    C_est = np.array([-f.pose_cam[:3, :3].astype(np.float64).T @ f.pose_cam[:3, 3].astype(np.float64) for f in frames])
    s, R, t = _similarity(C_est, C_gt)
    cam_err = np.linalg.norm((s * (R @ C_est.T).T + t) - C_gt, axis=1)
    P = s * (R @ cloud.xyz.astype(np.float64).T).T + t
    id_to_pt = {}
    for f, fr in zip(data, frames):
        for k, uid in enumerate(fr.unique_pixel_ids):
            if f["point_id"][k] >= 0:
                id_to_pt.setdefault(int(uid), int(f["point_id"][k]))
    d = np.array([np.linalg.norm(P[k] - pts[id_to_pt[int(u)]]) for k, u in enumerate(np.asarray(cloud.unique_point_ids)) if int(u) in id_to_pt])
    return cam_err, d


def test_none_changes_nothing(runs):
    _, _, _, out = runs
    fa, ca, la, text_a = out["plain"]
    fb, cb, lb, text_b = out["none"]
    for a, b in ((ca, cb), (la, lb)):
        assert a.xyz.tobytes() == b.xyz.tobytes() and np.array_equal(a.unique_point_ids, b.unique_point_ids) and np.array_equal(a.rgb, b.rgb)
    for a, b in zip(fa, fb):
        assert a.pose_cam.tobytes() == b.pose_cam.tobytes() and np.array_equal(a.unique_pixel_has_match, b.unique_pixel_has_match)
    assert "Track refine:" not in text_a and "Track refine:" not in text_b


def test_refined_run(runs, gpu_ctx):
    """With TrackOptions(): one "Track refine:" line per call (one before each of the four bundle adjustments of eight frames at
    frequency 4, one after the last); every point of the unfiltered cloud passes the verdict under the final poses; against the
    None run, after the pipeline test's similarity alignment:
      points farther from the truth than 10 x the None run's median error   None 1 of 906, refined 1 of 906 (required: not more)
      largest camera-centre error                                         None 0.00369, refined 0.00367 (required: not larger)"""
    data, poses, pts, out = runs
    frames, cloud, filtered, text = out["refine"]
    lines = [l for l in text.splitlines() if l.startswith("Track refine:")]
    print("\n".join(lines))
    assert len(lines) == 5 and lines[-1].split("] re-triangulated")[0].endswith("[0")
    cam_idx, pt_idx, uv, K4, Rt, _, _ = E.track_observations(frames, [False] * len(frames), cloud)
    ev = E.track_evaluate(cam_idx, pt_idx, uv, K4, Rt, cloud.xyz.astype(np.float64), E.TrackOptions(), gpu_ctx)
    assert len(cloud.xyz) > 500 and np.all(ev.status == 0)
    cam0, d0 = _errors(data, poses, pts, *out["none"][:2])
    cam1, d1 = _errors(data, poses, pts, frames, cloud)
    far0, far1 = int(np.count_nonzero(d0 > 10 * np.median(d0))), int(np.count_nonzero(d1 > 10 * np.median(d0)))
    print(f"points beyond 10 x the None run's median ({np.median(d0):.5f}): None {far0} of {len(d0)}, refined {far1} of {len(d1)} "
          f"(beyond 10 x its own median {np.median(d1):.5f}: {int(np.count_nonzero(d1 > 10 * np.median(d1)))}); "
          f"largest camera-centre error: None {cam0.max():.5f}, refined {cam1.max():.5f}")
    assert far1 <= far0
    assert cam1.max() <= cam0.max()


def _fountain_files(tmp_path, count=6):
    PIL = pytest.importorskip("PIL.Image")
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    img_dir = tmp_path / "images"; img_dir.mkdir()
    names = []
    for i, img in enumerate(z["images"][:count]):
        names.append(f"{i:04d}.png")
        PIL.fromarray(np.stack([img] * 3, axis=2)).save(str(img_dir / names[-1]))
    (tmp_path / "image_list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "K.txt").write_text(f"{689.87 / 2} 0 {380.17 / 2}\n0 {691.04 / 2} {251.70 / 2}\n0 0 1\n")
    exe = os.path.join(ROOT, "bin", "sfm_native")
    if not os.path.exists(exe):
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "easysfm_amd", "csrc"), "../../bin/sfm_native"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
    return exe, [str(img_dir), str(tmp_path / "image_list.txt"), str(tmp_path / "K.txt"), "none"]


def test_both_drivers_with_ratio_tracks(tmp_path):
    """bin/sfm_native and bin/sfm with "ratio+tracks" on six fountain images: status 1, the same stage lines up to the first bundle
    adjustment, identical "Track refine:" lines, and the same cloud in the .ply -- compared the way the driver-agreement test of the
    pipeline compares two drivers' clouds (size within 5 %); without the token no such line is printed."""
    exe, args = _fountain_files(tmp_path)
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0"]
    logs, clouds = {}, {}
    for tag, cmd, flt in (("native", [exe], ["ratio+tracks"]), ("python", [sys.executable, os.path.join(ROOT, "bin", "sfm")], ["ratio+tracks"]),
                          ("native-plain", [exe], [])):
        out = tmp_path / tag / "cloud.ply"
        r = subprocess.run(cmd + args + [str(out)] + tail + flt, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 1, (tag, r.stdout[-3000:])
        assert "Output ply file done." in r.stdout
        clouds[tag] = E.read_ply_vertices(str(out))[0]
        assert len(clouds[tag]) > 200 and np.all(np.isfinite(clouds[tag]))
        logs[tag] = r.stdout

    def stages(text, keys=("verified matches", "total unique feature point number", "Initialization frames", "Triangulate [")):
        return [l.strip() for l in text.splitlines() if any(k in l for k in keys)]
    assert len(stages(logs["native"])) > 10 and stages(logs["native"]) == stages(logs["python"])
    tn, tp = stages(logs["native"], ("Track refine:",)), stages(logs["python"], ("Track refine:",))
    print("\n".join(tn))
    assert len(tn) == 4 and tn == tp                                 # six frames at frequency 4: three bundle adjustments, and the filter
    assert not stages(logs["native-plain"], ("Track refine:",))
    assert abs(len(clouds["native"]) - len(clouds["python"])) <= 0.05 * len(clouds["python"])
    from scipy.spatial import cKDTree
    a_all, b_all = clouds["native"].astype(np.float64), clouds["python"].astype(np.float64)
    tree = cKDTree(b_all)
    sc, R, t = 1.0, np.eye(3), np.zeros(3)
    for _ in range(15):
        d, idx = tree.query(sc * (R @ a_all.T).T + t)
        keep = d <= np.percentile(d, 80)
        sc, R, t = _similarity(a_all[keep], b_all[idx[keep]])
    d, _ = tree.query(sc * (R @ a_all.T).T + t)
    extent = np.linalg.norm(b_all - b_all.mean(0), axis=1).mean()
    print(f"clouds: {len(a_all)} and {len(b_all)} points, scale {sc:.4f}, median closest-point distance {np.median(d) / extent:.2e} of the extent")
    assert abs(sc - 1) < 0.15 and np.median(d) < 0.1 * extent
