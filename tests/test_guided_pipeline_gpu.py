"""The "+guided" match filters through the pipeline on the MI355X: run_sfm on the repeated-structure scene of tests/guided_ref.py
("ratio" against "ratio+guided"), the fountain images with SURF, and the native driver against the Python one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd.pipeline import match_and_verify_all_pairs

import guided_ref as G

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


def _frames_of(data, K):
    frames = []
    for i, f in enumerate(data):
        fr = E.Frame(frame_id=i, keypoints=f["keypoints"], descriptors=f["descriptors"])
        fr.K_cam = K.copy()
        frames.append(fr)
    return frames


def _lists(matches):
    return (np.array([m.queryIdx for m in matches], np.int32), np.array([m.trainIdx for m in matches], np.int32),
            np.array([m.distance for m in matches], np.float32))


def _first_pass(frames, ctx, ratio=0.5, reproj=1.0, num_min_pair=20):
    """The pipeline's first pass once more, keeping what run_sfm does not return: per pair (i, j) with a model its plain inlier
    list and the essential matrix the GPU's RANSAC returned (the RANSAC's sample stream is fixed: the same input gives the same E)."""
    n = len(frames)
    pairs = np.array([(i, j) for i in range(n) for j in range(i)], np.int32)
    pm = E.PairMatcher(E.DescriptorBank([f.descriptors for f in frames], E.ESFM_L2_F32, device=f"cuda:{ctx.device}"), pairs, ctx)
    res = pm.match(ratio).to_host()
    pm.close()
    sel = [k for k in range(len(pairs)) if len(res[k][0]) > num_min_pair]
    off = np.concatenate([[0], np.cumsum([len(res[k][0]) for k in sel])]).astype(np.int32)
    p1 = np.concatenate([np.asarray(frames[pairs[k][0]].keypoints, np.float32).reshape(-1, 2)[res[k][0]] for k in sel])
    p2 = np.concatenate([np.asarray(frames[pairs[k][1]].keypoints, np.float32).reshape(-1, 2)[res[k][1]] for k in sel])
    K4 = np.array([G.k4_of(frames[pairs[k][0]].K_cam) for k in sel], np.float32)
    Es, mask, status, _ = E.find_essential_pairs(off, p1, p2, K4, 0.99, reproj, ctx)
    out = {}
    for s, k in enumerate(sel):
        if status[s]:
            m = mask[off[s]:off[s + 1]]
            q, t, d = res[k]
            out[(int(pairs[k][0]), int(pairs[k][1]))] = dict(inliers=(q[m], t[m], d[m]), E=Es[s], K4=K4[s])
    return out


def test_run_sfm_ratio_against_ratio_guided(gpu_ctx, tmp_path):
    data, K, poses, pts = G.scene()
    first = _first_pass(_frames_of(data, K), gpu_ctx)
    assert len(first) == 28
    results = {}
    for flt in ("ratio", "ratio+guided"):
        frames = _frames_of(data, K)
        cloud, filtered, graph = E.run_sfm(frames, str(tmp_path / (flt.replace("+", "_") + ".ply")), "S", 1.0, True, 0.0, 4, gpu_ctx, match_filter=flt)
        results[flt] = (frames, cloud, graph)
    # every pair's guided matches are the restatement's union, computed from the E the GPU returned
    n_plain = n_guided = n_true = 0
    for (i, j), f in first.items():
        _, _, gp = results["ratio"]
        _, _, gg = results["ratio+guided"]
        got_plain, got = _lists(gp[i][j].matches), _lists(gg[i][j].matches)
        for a, b in zip(got_plain, f["inliers"]):
            assert a.tobytes() == b.astype(a.dtype).tobytes(), (i, j, "plain")
        guided = G.match_guided(G.L2, data[i]["descriptors"], data[i]["keypoints"], data[j]["descriptors"], data[j]["keypoints"], f["E"], f["K4"], 1.0, 0.5, False)
        want = G.union(f["inliers"], guided)
        for a, b in zip(got, want):
            assert a.tobytes() == b.astype(a.dtype).tobytes(), (i, j, "guided")
        n_plain += len(got_plain[0]); n_guided += len(got[0])
        n_true += int(((data[i]["point_id"][got[0]] == data[j]["point_id"][got[1]]) & (data[i]["point_id"][got[0]] >= 0)).sum())
    print(f"scene: verified matches plain {n_plain}, guided {n_guided} ({n_guided / n_plain:.2f} x), true {n_true / n_guided:.4f}")
    assert n_guided >= 3 * n_plain and n_true >= 0.99 * n_guided
    # all eight frames registered in both runs, camera centres within the synthetic pipeline test's bound
    C_gt = np.array([-T[:3, :3].T @ T[:3, 3] for T in poses])
    for flt, (frames, cloud, _) in results.items():
        C_est = np.array([-f.pose_cam[:3, :3].astype(np.float64).T @ f.pose_cam[:3, 3].astype(np.float64) for f in frames])
        gaps = np.linalg.norm(C_est[:, None] - C_est[None], axis=2) + np.eye(8)
        assert gaps.min() > 1e-3, (flt, "a frame was left at another frame's pose")
        s, R, t = _similarity(C_est, C_gt)
        err = np.linalg.norm((s * (R @ C_est.T).T + t) - C_gt, axis=1)
        print(flt, "camera centre error", np.round(err, 4), "cloud", len(cloud.xyz))
        assert err.max() < 0.05, (flt, err)
    # the ratio test alone can only triangulate the uniquely described points; the guided pass reaches the repeated ones
    assert len(results["ratio+guided"][1].xyz) >= 2 * len(results["ratio"][1].xyz)


def test_fountain_surf_guided(gpu_ctx):
    """The fountain images at half resolution, SURF: every verified pair's guided list holds the plain inliers, every added match
    passes the predicate of the pair's essential matrix.  The gain on real images is printed, not asserted."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    K = np.array([[689.87 / 2, 0, 380.17 / 2], [0, 691.04 / 2, 251.70 / 2], [0, 0, 1]], np.float32)
    frames = []
    for i, img in enumerate(z["images"]):
        fr = E.Frame(frame_id=i, rgb_image=img)
        fr.K_cam = K.copy()
        E.detectFeaturesSURF(fr, 100, ctx=gpu_ctx)
        frames.append(fr)
    first = _first_pass(frames, gpu_ctx)
    plain = match_and_verify_all_pairs(frames, "S", 1.0, 20, gpu_ctx, "ratio")
    guided = match_and_verify_all_pairs(frames, "S", 1.0, 20, gpu_ctx, "ratio+guided")
    n_plain = n_guided = n_pairs = 0
    for i in range(len(frames)):
        for j in range(i):
            p, g = _lists(plain[i][j].matches), _lists(guided[i][j].matches)
            if (i, j) not in first:
                assert len(p[0]) == 0 and len(g[0]) == 0
                continue
            f = first[(i, j)]
            for a, b in zip(p, f["inliers"]):
                assert a.tobytes() == b.astype(a.dtype).tobytes(), (i, j)
            held = dict(zip(g[0].tolist(), g[1].tolist()))
            assert len(held) == len(g[0]) and np.all(np.diff(g[0]) > 0)
            assert all(held.get(a) == b for a, b in zip(p[0].tolist(), p[1].tolist())), (i, j)
            kq = np.asarray(frames[i].keypoints, np.float32).reshape(-1, 2); kt = np.asarray(frames[j].keypoints, np.float32).reshape(-1, 2)
            assert np.all(G.admissible_rows(kq[g[0]], kt[g[1]], f["E"], f["K4"], 1.0)), (i, j)
            assert np.allclose(guided[i][j].T_21, plain[i][j].T_21) and guided[i][j].appro_depth == plain[i][j].appro_depth
            n_plain += len(p[0]); n_guided += len(g[0]); n_pairs += 1
    print(f"fountain (11 half-resolution images, SURF 100): {n_pairs} verified pairs, verified matches plain {n_plain}, guided {n_guided} "
          f"({n_guided / max(n_plain, 1):.2f} x)")
    assert n_pairs >= 10 and n_guided >= n_plain


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


def _stages(text, keys=("verified matches", "total unique feature point number", "Initialization frames", "Triangulate [")):
    return [l.strip() for l in text.splitlines() if any(k in l for k in keys)]


def test_native_driver_agrees_with_python_on_ratio_guided(tmp_path):
    """bin/sfm_native and bin/sfm with "ratio+guided" on six fountain images: status 1, a .ply each, and -- everything up to the
    first bundle adjustment being a deterministic function of the images -- the same verified-match counts per pair, the same
    number of tracks, the same initial pair and the same triangulation counts.  The guided pass adds matches over "ratio"."""
    exe, args = _fountain_files(tmp_path)
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0"]
    logs = {}
    for tag, cmd, flt in (("native", [exe], "ratio+guided"), ("python", [sys.executable, os.path.join(ROOT, "bin", "sfm")], "ratio+guided"),
                          ("native-plain", [exe], "ratio")):
        out = tmp_path / tag / "cloud.ply"
        r = subprocess.run(cmd + args + [str(out)] + tail + [flt], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 1, (tag, r.stdout[-3000:])
        assert "Output ply file done." in r.stdout
        xyz, _, _ = E.read_ply_vertices(str(out))
        assert len(xyz) > 200 and np.all(np.isfinite(xyz))
        logs[tag] = r.stdout
    sn, sp = _stages(logs["native"]), _stages(logs["python"])
    assert len(sn) > 10 and sn == sp

    def verified(text):
        return sum(int(l.split("[")[1].split("]")[0]) for l in _stages(text, ("verified matches",)))
    print("six fountain images, verified matches: ratio", verified(logs["native-plain"]), "ratio+guided", verified(logs["native"]))
    assert verified(logs["native"]) >= verified(logs["native-plain"])


def test_native_batched_guided_equals_pair_by_pair(tmp_path):
    """The native driver's batched guided call (esfm_match_guided_pairs) and ESFM_PAIR_BY_PAIR=1 (esfm_match_guided_l2_f32 per pair)
    give the same per-pair lines, tracks, initial pair and triangulation counts, with the cross filter's reverse table in play."""
    exe, args = _fountain_files(tmp_path)
    logs = {}
    for tag in ("batched", "pairwise"):
        env = dict(os.environ)
        env.pop("ESFM_PAIR_BY_PAIR", None)
        if tag == "pairwise":
            env["ESFM_PAIR_BY_PAIR"] = "1"
        r = subprocess.run([exe] + args + [str(tmp_path / tag / "cloud.ply"), "S", "100", "1.0", "1", "0", "4", "1", "0", "ratio+cross+guided"], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 1, r.stdout[-3000:]
        logs[tag] = r.stdout
    keys = ("inlier matches from", "verified matches", "total unique feature point number", "Initialization frames", "Triangulate [")
    sb, sp = sorted(_stages(logs["batched"], keys)), sorted(_stages(logs["pairwise"], keys))
    assert len(sb) > 10 and sb == sp
