"""SIFT on the GPU (esfm_sift_detect_and_compute, feature type 'I'): keypoints and descriptors bit-identical to the CPU
restatement tests/sift_ref/sift_ref.c, invariance to a 90-degree rotation, and the hand-off to the 128-float L2 matcher and
the essential-matrix RANSAC."""
import os

import numpy as np
import pytest

import easysfm_amd as E
from sift_ref import SiftRef

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return SiftRef(tmp_path_factory.mktemp("sift_ref"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_equal(got, ref):
    kg, dg = got
    kr, dr = ref
    assert kg.shape == kr.shape, (kg.shape, kr.shape)
    assert np.array_equal(_bits(kg), _bits(kr))
    assert np.array_equal(_bits(dg), _bits(dr))


def _synthetic(rng, rows, cols, n_blobs):
    """Gaussian blobs of random size, sign and contrast on a gradient, plus mild noise: extrema at many scales."""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img = 100 + 30 * x / cols + 20 * y / rows
    for _ in range(n_blobs):
        cy, cx, s = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(1.5, 10)
        img += rng.choice([-1, 1]) * rng.uniform(30, 90) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    img += rng.normal(0, 2, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def test_sift_fountain_pair_bitexact(gpu_ctx, sref):
    z = np.load(os.path.join(GOLD, "fountain_pair_half.npz"))
    for name in ("img0", "img1"):
        bgr = z[name]
        ref = sref.detect(bgr)
        assert len(ref[0]) > 100
        _check_equal(E.sift_detect_and_compute(bgr, 0, None, gpu_ctx), ref)                   # BGR in: the gray conversion runs on the GPU
        _check_equal(E.sift_detect_and_compute(sref.gray(bgr), 0, None, gpu_ctx), ref)
    kp, d = E.sift_detect_and_compute(z["img0"], 0, None, gpu_ctx)
    assert np.all(d == np.rint(d)) and d.min() >= 0 and d.max() <= 255 and d.shape[1] == 128
    assert np.all(kp[:, 6] == -1) and np.all((kp[:, 3] >= 0) & (kp[:, 3] < 360))


def test_sift_fullsize_and_nfeatures_bitexact(gpu_ctx, sref):
    img = np.load(os.path.join(GOLD, "fountain11_gray.npz"))["images"][0]
    assert img.shape == (512, 768)
    full = sref.detect(img)
    got = E.sift_detect_and_compute(img, 0, None, gpu_ctx)
    _check_equal(got, full)
    for nf in (100, 800):
        ref = sref.detect(img, nf)
        _check_equal(E.sift_detect_and_compute(img, nf, None, gpu_ctx), ref)
        assert len(ref[0]) >= min(nf, len(full[0]))
        thr = np.sort(full[0][:, 4])[::-1][nf - 1]
        assert np.all(ref[0][:, 4] >= thr)
    # max_keypoints returns a prefix of the full list
    k2, d2 = E.sift_detect_and_compute(img, 0, 57, gpu_ctx)
    assert np.array_equal(_bits(k2), _bits(got[0][:57])) and np.array_equal(_bits(d2), _bits(got[1][:57]))


@pytest.mark.parametrize("rows,cols,seed", [(33, 40, 0), (97, 131, 1), (240, 320, 2)])
def test_sift_synthetic_bitexact(gpu_ctx, sref, rows, cols, seed):
    img = _synthetic(np.random.default_rng(seed), rows, cols, 6 if rows < 50 else 40)
    ref = sref.detect(img)
    _check_equal(E.sift_detect_and_compute(img, 0, None, gpu_ctx), ref)
    if rows >= 240:
        assert len(ref[0]) > 20


def test_sift_rotation_invariance_and_matching(gpu_ctx):
    """np.rot90 maps pixel (x, y) to (y, W - 1 - x) and turns every gradient with it, so the keypoint angle drops by 90 degrees.
    Reported points sit 0.25 px right of and below the true ones (the x2 INTER_LINEAR phase, test_sift_ref_cpu.py), so a
    reported (x, y) maps to (y, W - 0.5 - x).  The pyramid's sampling grids map onto themselves only up to that phase, so the
    test asks for most keypoints, not all."""
    g0 = np.load(os.path.join(GOLD, "fountain_pair_half.npz"))["img0"]
    g0 = (g0[..., 0] * 0.114 + g0[..., 1] * 0.587 + g0[..., 2] * 0.299).round().astype(np.uint8)
    W = g0.shape[1]
    kp, d = E.sift_detect_and_compute(g0, 0, None, gpu_ctx)
    kr, dr = E.sift_detect_and_compute(np.ascontiguousarray(np.rot90(g0)), 0, None, gpu_ctx)
    mapped = np.stack([kp[:, 1], W - 0.5 - kp[:, 0]], axis=1)
    from scipy.spatial import cKDTree
    dist, idx = cKDTree(kr[:, :2]).query(mapped, k=8)
    found = 0
    for a in range(len(kp)):
        for dd, b in zip(dist[a], idx[a]):
            if dd <= 0.5 and b < len(kr):
                da = (kr[b, 3] - kp[a, 3] + 90.0 + 180.0) % 360.0 - 180.0
                if abs(da) <= 2.0:
                    found += 1
                    break
    assert found >= 0.8 * len(kp), (found, len(kp))
    q, t, _ = E.match_l2(d, dr, 0.7, gpu_ctx)
    ok = np.linalg.norm(kr[t, :2] - mapped[q], axis=1) <= 2.0
    assert len(q) > 0.3 * len(kp) and ok.mean() >= 0.9, (len(q), ok.mean())


def test_sift_hands_off_to_matcher_and_ransac(gpu_ctx, sref, oracle_lib):
    z = np.load(os.path.join(GOLD, "fountain_pair_half.npz"))
    k0, d0 = E.sift_detect_and_compute(z["img0"], 0, None, gpu_ctx)
    k1, d1 = E.sift_detect_and_compute(z["img1"], 0, None, gpu_ctx)
    qi, ti, dist = E.match_l2(d1, d0, 0.7, gpu_ctx)
    rq, rt, rd = oracle_lib.match_l2(d1, d0, 0.7)
    assert np.array_equal(qi, rq) and np.array_equal(ti, rt) and np.array_equal(_bits(dist), _bits(rd))
    assert len(qi) >= 30
    K = (689.87 / 2, 380.17 / 2, 691.04 / 2, 251.70 / 2)
    Em, mask, _ = E.find_essential_mat(k1[qi, :2], k0[ti, :2], K, 0.99, 1.0, gpu_ctx)
    assert mask.sum() >= max(15, 0.3 * len(qi)), (mask.sum(), len(qi))
