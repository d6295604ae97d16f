"""Dense reconstruction on the GPU: depth and cost maps bit for bit against tests/mvs_ref.py (synthetic scene, BGR input, a crop
of the half-resolution fountain), fusion bit for bit, and accuracy against the synthetic scene's exact depth."""
import os

import numpy as np
import pytest

import easysfm_amd as E
import mvs_ref as M
import mvs_scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scene():
    sc = S.make_scene()
    n = len(sc["images"])
    sc["nb"] = np.array([[j for j in range(n) if j != i][:4] for i in range(n)], np.int32)
    d = sc["depth"].reshape(n, -1)
    sc["range"] = np.stack([d.min(1) / 1.1, d.max(1) * 1.1], 1).astype(np.float32)
    return sc


def _opts(**kw):
    o = E.default_mvs_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o, M.options(**kw)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("r,D,best_k", [(1, 3, 1), (3, 48, 2), (1, 48, 2), (3, 3, 1), (3, 48, 1)])
def test_sweep_bit_parity_synthetic(gpu_ctx, scene, r, D, best_k):
    o, ro = _opts(window_radius=r, num_planes=D, best_k=best_k)
    depth, cost = E.mvs_depth_maps(scene["images"], scene["K4"], scene["poses"], scene["nb"], scene["range"], o, gpu_ctx)
    rd, rc = M.depth_maps(scene["images"], scene["K4"], scene["poses"], scene["nb"], scene["range"], ro)
    assert _same(depth, rd), np.count_nonzero(depth.view(np.uint32) != rd.view(np.uint32))
    assert _same(cost, rc), np.count_nonzero(cost.view(np.uint32) != rc.view(np.uint32))
    if D == 48:
        assert np.mean(depth > 0) > 0.5


@pytest.mark.parametrize("r", [2, 4, 5, 6, 7])
def test_sweep_and_fuse_bit_parity_tile_tails_and_radii(gpu_ctx, scene, r):
    """173 x 235: neither side a multiple of the 16-pixel tile, so both tails and the halo reads past the right and bottom
    edges are compared; the radii the other cases leave out (r = 7 is the instance with the widest unrolled window)."""
    imgs = np.ascontiguousarray(scene["images"][:, :173, :235])
    o, ro = _opts(window_radius=r, num_planes=8, best_k=2)
    depth, cost = E.mvs_depth_maps(imgs, scene["K4"], scene["poses"], scene["nb"], scene["range"], o, gpu_ctx)
    rd, rc = M.depth_maps(imgs, scene["K4"], scene["poses"], scene["nb"], scene["range"], ro)
    assert _same(depth, rd), np.count_nonzero(depth.view(np.uint32) != rd.view(np.uint32))
    assert _same(cost, rc), np.count_nonzero(cost.view(np.uint32) != rc.view(np.uint32))
    assert np.mean(depth > 0) > 0.2 and np.any(depth[:, 160:173 - r, 224:235 - r] > 0)   # estimates inside the tail tiles
    xyz, rgb = E.mvs_fuse(imgs, scene["K4"], scene["poses"], scene["nb"], depth, o, gpu_ctx)
    rx, rr = M.fuse(imgs, scene["K4"], scene["poses"], scene["nb"], depth, ro)
    assert len(xyz) > 1000 and _same(xyz, rx) and np.array_equal(rgb, rr)


def test_sweep_and_fuse_bit_parity_bgr(gpu_ctx, scene):
    g = scene["images"]
    bgr = np.ascontiguousarray(np.stack([g, np.roll(g, 3, axis=2), (g // 2 + 60).astype(np.uint8)], axis=3))
    rng = scene["range"].copy()
    rng[4] = 0                                                            # one view without a depth map
    nb = scene["nb"].copy()
    nb[1, 3] = -1                                                         # a padded neighbour list
    o, ro = _opts(num_planes=40, best_k=2)
    depth, cost = E.mvs_depth_maps(bgr, scene["K4"], scene["poses"], nb, rng, o, gpu_ctx)
    rd, rc = M.depth_maps(bgr, scene["K4"], scene["poses"], nb, rng, ro)
    assert _same(depth, rd) and _same(cost, rc)
    assert np.all(depth[4] == 0) and np.all(np.isinf(cost[4]))
    xyz, rgb = E.mvs_fuse(bgr, scene["K4"], scene["poses"], nb, depth, o, gpu_ctx)
    rx, rr = M.fuse(bgr, scene["K4"], scene["poses"], nb, depth, ro)
    assert len(xyz) > 10000 and _same(xyz, rx) and np.array_equal(rgb, rr)
    assert not np.array_equal(rgb[:, 0], rgb[:, 2])                      # BGR turned into RGB
    # grey input, other fusion settings
    o2, ro2 = _opts(fuse_min_views=1, fuse_reproj_px=0.5, fuse_rel_depth=0.005, max_neighbours=4)
    xyz, rgb = E.mvs_fuse(scene["images"], scene["K4"], scene["poses"], scene["nb"], depth, o2, gpu_ctx)
    rx, rr = M.fuse(scene["images"], scene["K4"], scene["poses"], scene["nb"], depth, ro2)
    assert _same(xyz, rx) and np.array_equal(rgb, rr)


def test_accuracy_against_ground_truth(gpu_ctx, scene):
    o = E.default_mvs_options()
    r = o.window_radius
    depth, cost = E.mvs_depth_maps(scene["images"], scene["K4"], scene["poses"], scene["nb"], scene["range"], o, gpu_ctx)
    n = len(depth)
    n_px = n_est = n_good = 0
    for v in range(n):
        gt = scene["depth"][v]
        sel = (S.visible_count(scene, v, scene["nb"][v]) >= 2) & S.edge_distance_mask(scene["obj"][v], gt, r + 1)
        d = depth[v][sel]
        est = d > 0
        n_px += int(sel.sum()); n_est += int(est.sum())
        n_good += int(np.sum(np.abs(d[est] - gt[sel][est]) < 0.01 * gt[sel][est]))
    print(f"synthetic: {n_px} pixels, {n_est / n_px:.4f} estimated, {n_good / max(n_est, 1):.4f} of those within 1 %")
    assert n_est >= 0.9 * n_px and n_good >= 0.95 * n_est
    # fused points: each view alone as reference, so every point's view is known
    total = close = 0
    for v in range(n):
        nb = np.full_like(scene["nb"], -1)
        nb[v] = scene["nb"][v]
        xyz, _ = E.mvs_fuse(scene["images"], scene["K4"], scene["poses"], nb, depth, o, gpu_ctx)
        true, own = S.ray_depth(scene, v, xyz)
        total += len(xyz); close += int(np.sum(np.abs(own - true) < 0.01 * true))
    print(f"synthetic: {total} fused points, {close / total:.4f} within 1 %")
    assert total > 50000 and close >= 0.95 * total


@pytest.fixture(scope="module")
def fountain(gpu_ctx):
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    K = np.array([[689.87 / 2, 0, 380.17 / 2], [0, 691.04 / 2, 251.70 / 2], [0, 0, 1]], np.float32)
    frames = []
    for i, img in enumerate(z["images"]):
        fr = E.Frame(frame_id=i, rgb_image=img)
        fr.K_cam = K.copy()
        E.detectFeaturesSURF(fr, 100, ctx=gpu_ctx)
        frames.append(fr)
    cloud, _, _ = E.run_sfm(frames, None, "S", 1.0, True, 0.0, 4, gpu_ctx)
    return frames, cloud


def test_sweep_bit_parity_fountain_crop(gpu_ctx, fountain):
    frames, cloud = fountain
    nb_all, rng_all = E.mvs_plan(frames, [False] * len(frames), cloud)
    views = [4, 5, 6]
    assert np.all(rng_all[views, 0] > 0)
    y0, x0, h, w = 48, 80, 144, 208
    imgs = np.stack([np.asarray(frames[v].rgb_image)[y0:y0 + h, x0:x0 + w] for v in views])
    K4 = np.array([[f.K_cam[0, 0], f.K_cam[0, 2] - x0, f.K_cam[1, 1], f.K_cam[1, 2] - y0] for f in (frames[v] for v in views)], np.float32)
    poses = np.stack([frames[v].pose_cam[:3, :4].reshape(12) for v in views]).astype(np.float32)
    nb = np.array([[1, 2, -1, -1], [0, 2, -1, -1], [0, 1, -1, -1]], np.int32)
    rng = rng_all[views]
    o, ro = _opts(num_planes=48)
    depth, cost = E.mvs_depth_maps(imgs, K4, poses, nb, rng, o, gpu_ctx)
    rd, rc = M.depth_maps(imgs, K4, poses, nb, rng, ro)
    assert _same(depth, rd) and _same(cost, rc)
    assert np.mean(depth > 0) > 0.2
    xyz, rgb = E.mvs_fuse(imgs, K4, poses, nb, depth, o, gpu_ctx)
    rx, rr = M.fuse(imgs, K4, poses, nb, depth, ro)
    assert len(xyz) > 1000 and _same(xyz, rx) and np.array_equal(rgb, rr)
