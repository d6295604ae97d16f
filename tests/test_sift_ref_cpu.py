"""CPU checks of the SIFT restatement (tests/sift_ref/sift_ref.c) that esfm_sift_detect_and_compute must reproduce to the bit:
the pyramid against an independent separable filter, the written-out exp / exp2 / sin / cos against libm, a known answer on
Gaussian blobs, the descriptor format and the nfeatures rule; and the C ABI entry point itself."""
import math
import os

import numpy as np
import pytest
from scipy.ndimage import correlate1d

from sift_ref import SiftRef

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return SiftRef(tmp_path_factory.mktemp("sift_ref"))


def test_pyramid_matches_an_independent_filter(sref):
    """Each layer i >= 1 is layer i-1 filtered with the taps of sig[i] (rows, then columns, mirror = BORDER_REFLECT_101, which
    scipy also repeats for kernels wider than the image); layer 0 of octave o+1 is every second pixel of layer 3 of octave o."""
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (37, 52), dtype=np.uint8)
    pyr = sref.pyramid(img)
    sig = sref.sigmas()
    assert len(pyr) == round(math.log2(74) - 2) + 1
    worst = 0.0
    for o, layers in enumerate(pyr):
        if o > 0:
            assert np.array_equal(layers[0], pyr[o - 1][3][0::2, 0::2][:layers[0].shape[0], :layers[0].shape[1]])
        for i in range(1, 6):
            w = sref.taps(sig[i]).astype(np.float64)
            exp = correlate1d(correlate1d(layers[i - 1].astype(np.float64), w, axis=1, mode="mirror"), w, axis=0, mode="mirror")
            err = np.abs(layers[i] - exp) / np.maximum(np.abs(exp), 1.0)
            worst = max(worst, float(err.max()))
    assert worst <= 1e-5, worst


def test_octave_count_and_taps(sref):
    assert len(sref.octave_shapes(512, 768)) == 9
    assert [len(sref.taps(s)) for s in sref.sigmas()] == [11, 11, 13, 17, 21, 27]
    for s in sref.sigmas():
        w = sref.taps(s)
        assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6 and np.array_equal(w, w[::-1])


def _ulp_err(got, exact):
    got = np.asarray(got, np.float32)
    ref32 = np.asarray(exact, np.float64)
    ulp = np.spacing(np.abs(ref32.astype(np.float32))).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref32) / ulp


def test_math_routines_within_two_ulp(sref):
    rng = np.random.default_rng(1)
    # exp: the orientation and descriptor weights (arguments down to about -25)
    x = np.concatenate([rng.uniform(-30.0, 0.0, 4000), np.linspace(-25.0, 0.0, 1001)]).astype(np.float32)
    assert _ulp_err(sref.fn("sift_exp", x), [math.exp(float(v)) for v in x]).max() <= 2
    # exp2: the keypoint size, 2^((layer + xi) / 3)
    x = np.concatenate([rng.uniform(0.0, 1.5, 2000), np.linspace(-1.0, 2.0, 601)]).astype(np.float32)
    assert _ulp_err(sref.fn("sift_exp2", x), [2.0 ** float(v) for v in x]).max() <= 2
    # sin / cos: the descriptor rotation, ori * pi/180 for ori in [0, 360]
    ang = np.concatenate([rng.uniform(0.0, 360.0, 3000), np.arange(0, 361, 1.0)]).astype(np.float32)
    x = (ang * np.float32(math.pi / 180)).astype(np.float32)
    for name, f in (("sift_sin", math.sin), ("sift_cos", math.cos)):
        ref = np.array([f(float(v)) for v in x])
        got = sref.fn(name, x)
        tiny = np.abs(ref) < 1e-30
        assert _ulp_err(got[~tiny], ref[~tiny]).max() <= 2, name


@pytest.mark.parametrize("s", [2.0, 3.0, 5.0, 8.0])
def test_gaussian_blob_known_answer(sref, s):
    """A blob A exp(-r^2 / 2 s^2) on a flat field.  SIFT assumes its input carries a blur of 0.5 px (1 px in the x2 base), so
    at nominal scale t (base pixels) the blob's variance is (2s)^2 - 1 + t^2.  Its DoG response at the centre,
    L(k t) - L(t) with L(t) = A b^2 / (b^2 + t^2), b^2 = 4 s^2 - 1, is extremal where d/dt [t^2 / ((b^2 + k^2 t^2)(b^2 + t^2))]
    = 0, i.e. t = b / sqrt(k), k = 2^(1/3).  The keypoint's size (input pixels, after the firstOctave halving) is that t.
    Position: INTER_LINEAR puts input pixel k at base coordinate 2k + 0.5 and the firstOctave halving maps base u to u / 2, so
    OpenCV's SIFT (and this restatement) reports a point at (x + 0.25, y + 0.25)."""
    n = int(12 * s) + 41
    cy, cx = n / 2 + 0.3, n / 2 - 0.2
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    img = np.rint(60 + 150 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))).astype(np.uint8)
    kp, d = sref.detect(img)
    assert len(kp) >= 1
    best = kp[np.argmax(kp[:, 4])]
    assert math.hypot(best[0] - (cx + 0.25), best[1] - (cy + 0.25)) <= 0.1, (best[:2], (cx, cy))
    predicted = math.sqrt(4 * s * s - 1) / 2 ** (1 / 6)
    assert abs(best[2] / predicted - 1) <= 0.15, (best[2], predicted)
    # every keypoint at the dominant location shares its position and size: one blob, one location (orientations may repeat)
    strong = kp[kp[:, 4] >= 0.5 * best[4]]
    assert np.all(np.hypot(strong[:, 0] - best[0], strong[:, 1] - best[1]) < 1e-3)


def test_descriptor_format_and_keypoint_fields(sref):
    z = np.load(os.path.join(GOLD, "fountain_pair_half.npz"))
    kp, d = sref.detect(z["img0"])
    assert len(kp) > 100 and d.shape == (len(kp), 128) and kp.shape[1] == 7
    assert np.all(d == np.rint(d)) and d.min() >= 0 and d.max() <= 255
    assert np.all(d.max(axis=1) > 0)
    assert np.all(kp[:, 6] == -1) and np.all((kp[:, 3] >= 0) & (kp[:, 3] < 360)) and np.all(kp[:, 4] > 0)
    oc = kp[:, 5].astype(np.int64)
    assert np.all(oc == kp[:, 5]) and np.all(oc < 2 ** 24)
    octave = oc & 255
    octave = np.where(octave < 128, octave, octave - 256)
    layer = (oc >> 8) & 255
    assert set(np.unique(octave)) <= set(range(-1, 8)) and set(np.unique(layer)) <= {1, 2, 3}
    # no two keypoints share (x, y, size, angle)
    keys = {tuple(r) for r in kp[:, :4].view(np.uint32)}
    assert len(keys) == len(kp)


def test_nfeatures_keeps_ties_in_scan_order(sref):
    z = np.load(os.path.join(GOLD, "fountain_pair_half.npz"))
    kp, d = sref.detect(z["img1"])
    resp = np.sort(kp[:, 4])[::-1]
    # a candidate with several orientation peaks gives keypoints of equal response: cut right inside such a group
    tied = [i for i in range(1, len(resp) - 1) if resp[i] == resp[i + 1]]
    assert tied, "no orientation group to cut"
    for nf in (tied[0] + 1, 50, len(kp) - 1):
        kn, dn = sref.detect(z["img1"], nf)
        thr = resp[nf - 1]
        sel = kp[:, 4] >= thr
        assert np.array_equal(kn, kp[sel]) and np.array_equal(dn, d[sel])
        assert len(kn) >= nf
    kn, _ = sref.detect(z["img1"], tied[0] + 1)
    assert len(kn) > tied[0] + 1                     # the tie with the n-th response is kept
    km, dm = sref.detect(z["img1"], 0, 10)
    assert np.array_equal(km, kp[:10]) and np.array_equal(dm, d[:10])


def test_abi_entry_point_exported_and_needs_a_device():
    import easysfm_amd as E
    from easysfm_amd._lib import EXPORTED_SYMBOLS
    L = E.lib()
    assert "esfm_sift_detect_and_compute" in EXPORTED_SYMBOLS and hasattr(L, "esfm_sift_detect_and_compute")
    assert "esfm_sift_detect_and_compute" in open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "esfm.h")).read()
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(E.EsfmError) as ei:
        E.sift_detect_and_compute(np.zeros((40, 40), np.uint8))
    assert ei.value.status == -2
