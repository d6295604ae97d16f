"""Parity of the HIP ORB detector + descriptor (ORB half; reference
FeatureMatching::detectFeaturesORB, cpp_code/src/feature_matching.cpp:14-41) through the C ABI against the CPU oracle
(oracle/orb_ref.c, pinned to its rule list by tests/orb_ref.py; OpenCV absent, own test point pairs): keypoints and descriptors bit for bit -- the image
arithmetic is integer, the few float expressions keep their operation order, cos / sin come from the host's libm on both sides.
Then the properties an ORB implementation must have and the hand-off to the Hamming matcher."""
import os

import numpy as np
import pytest

import easysfm_amd as E

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _check_equal(gpu, ref):
    (kg, dg), (kr, dr) = gpu, ref
    assert len(kg) == len(kr) and len(kg) > 50
    assert np.array_equal(kg.view(np.uint32), kr.view(np.uint32))
    assert np.array_equal(dg, dr)


@pytest.mark.parametrize("nfeatures", [500, 8000])
def test_orb_fountain_bitexact(gpu_ctx, oracle_lib, nfeatures):
    imgs = np.load(os.path.join(GOLD, "fountain11_gray.npz"))["images"]
    for k in (0, 5):
        _check_equal(E.orb_detect_and_compute(imgs[k], nfeatures, None, gpu_ctx), oracle_lib.orb(imgs[k], nfeatures))
    kp, d = E.orb_detect_and_compute(imgs[0], nfeatures, None, gpu_ctx)
    assert d.dtype == np.uint8 and d.shape[1] == 32
    # level by level, strongest first inside a level; OpenCV's keypoint fields
    lv = kp[:, 5].astype(int)
    assert np.all(np.diff(lv) >= 0) and lv.max() <= 7
    for l in np.unique(lv):
        assert np.all(np.diff(kp[lv == l, 4]) <= 0)
    assert np.allclose(kp[:, 2], 31.0 * 1.2 ** lv, rtol=1e-6) and np.all((kp[:, 3] >= 0) & (kp[:, 3] <= 360)) and np.all(kp[:, 6] == -1)
    # the per-level quota of cv::ORB (geometric, remainder to the last level); retainBest may keep ties
    f = 1 / 1.2
    nd = nfeatures * (1 - f) / (1 - f ** 8)
    for l in range(7):
        assert (lv == l).sum() <= round(nd) + 8
        nd *= f


def test_orb_bgr_input_and_small_images(gpu_ctx, oracle_lib):
    z = np.load(os.path.join(GOLD, "fountain_pair_half.npz"))
    bgr = z["img0"]
    gray = oracle_lib.bgr2gray(bgr)
    ref = oracle_lib.orb(gray, 1000)
    _check_equal(E.orb_detect_and_compute(bgr, 1000, None, gpu_ctx), ref)        # the gray conversion runs on the GPU
    _check_equal(E.orb_detect_and_compute(gray, 1000, None, gpu_ctx), ref)
    rng = np.random.default_rng(3)
    for rows, cols in ((97, 131), (64, 300), (40, 40)):                          # levels that get smaller than the border are skipped
        img = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        img = np.clip(np.kron(img[::4, ::4], np.ones((4, 4))) [:rows, :cols] + rng.integers(-8, 9, (rows, cols)), 0, 255).astype(np.uint8)
        kg, dg = E.orb_detect_and_compute(img, 300, None, gpu_ctx)
        kr, dr = oracle_lib.orb(img, 300)
        assert np.array_equal(kg.view(np.uint32), kr.view(np.uint32)) and np.array_equal(dg, dr)
    kg, dg = E.orb_detect_and_compute(np.full((120, 160), 77, np.uint8), 500, None, gpu_ctx)    # flat image: nothing
    assert len(kg) == 0


def test_orb_rotation_and_matching(gpu_ctx, oracle_lib):
    """np.rot90 of the image maps the FAST ring, the Harris block and the orientation disc onto themselves: the same corners come
    back (rotated) with the same responses; descriptors of two fountain views match through the Hamming matcher with the
    reference's ratio 0.8 and the matches are geometrically consistent."""
    imgs = np.load(os.path.join(GOLD, "fountain11_gray.npz"))["images"]
    img = imgs[0][:, :512]                                    # square crop: every pyramid level stays square under rotation
    kp, d = E.orb_detect_and_compute(img, 2000, None, gpu_ctx)
    kr, dr = E.orb_detect_and_compute(np.ascontiguousarray(np.rot90(img)), 2000, None, gpu_ctx)
    l0, l0r = kp[kp[:, 5] == 0], kr[kr[:, 5] == 0]
    a = {(int(x), int(y)) for x, y in l0[:, :2]}
    b = {(511 - int(y), int(x)) for x, y in l0r[:, :2]}       # rot90 (counter-clockwise) sends (x, y) to (y, W - 1 - x): invert it
    assert len(a & b) >= 0.95 * min(len(a), len(b))
    k0, d0 = E.orb_detect_and_compute(imgs[0], 8000, None, gpu_ctx)
    k1, d1 = E.orb_detect_and_compute(imgs[1], 8000, None, gpu_ctx)
    q, t, dist = E.match_hamming(d1, d0, 0.8, gpu_ctx)
    rq, rt, rd = oracle_lib.match_hamming(d1, d0, 0.8)
    assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(dist, rd) and len(q) > 500
    flow = k1[q, :2] - k0[t, :2]
    med = np.median(flow, axis=0)
    assert np.mean(np.linalg.norm(flow - med, axis=1) < 40) > 0.8


def test_feature_matching_mirror_orb(gpu_ctx, oracle_lib):
    imgs = np.load(os.path.join(GOLD, "fountain11_gray.npz"))["images"]
    fr = E.Frame(frame_id=0, rgb_image=np.stack([imgs[2]] * 3, axis=2))
    assert E.FeatureMatching(gpu_ctx).detectFeaturesORB(fr, 3000) is True
    rk, rd = oracle_lib.orb(imgs[2], 3000)      # B = G = R: the 14-bit gray conversion returns the value itself
    assert np.array_equal(fr.descriptors, rd) and np.array_equal(fr.keypoints, rk[:, :2])
