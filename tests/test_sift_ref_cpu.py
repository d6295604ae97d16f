"""CPU checks of the SIFT restatement (tests/sift_ref/sift_ref.c) that esfm_sift_detect_and_compute must reproduce to the bit:
the pyramid against an independent separable filter, the written-out exp / exp2 / sin / cos against libm, a known answer on
Gaussian blobs, the descriptor format and the nfeatures rule; and the C ABI entry point itself.

Second half: the restatement against tests/sift_np.py, the independent float64 statement of SIFT -- `verify` on its output for
every case of feature_cases.SIFT_CASES, hand-written answers for every stage of sift_np itself, and the tampers `verify` must
catch.  tests/test_feature_ref_gpu.py runs the same `verify`, with the same cap and tolerance, on the library's output."""
import functools
import math
import os

import numpy as np
import pytest
from scipy.ndimage import correlate1d

import feature_cases as F
import sift_np as S
from sift_ref import SiftRef
from surf_ref import fast_atan2_deg

UNDECIDED_CAP = 0.02                     # the cap of tests/test_feature_ref_gpu.py

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


# ============================================================================================================================
# the restatement against the independent statement tests/sift_np.py
@functools.lru_cache(maxsize=None)
def _case(name, form):
    _, make, n = next(c for c in F.SIFT_CASES if c[0] == name)
    img = make() if form == "bgr" else S.as_gray(make())
    return img, n, S.Stages(img)


@pytest.mark.parametrize("form", ["gray", "bgr"])
@pytest.mark.parametrize("name", [c[0] for c in F.SIFT_CASES])
def test_verify_passes_on_restatement(sref, name, form):
    img, n, st = _case(name, form)
    kp, d = sref.detect(img)
    assert len(kp) == n
    rep = S.verify(img, {"nfeatures": 0}, kp, d, st)
    print(name, form, rep, "undecided share %.4f" % rep.undecided_share(), rep.undecided)
    assert rep.ok, rep.errors[:10]
    assert rep.undecided_share() <= UNDECIDED_CAP
    assert rep.n_reference > 0 and rep.n_described >= min(len(kp), 150) - len(rep.undecided) and rep.max_desc_distance <= S.DESC_TOL
    if name in ("fountain256x320", "blobs240x320"):
        assert rep.n_reported > 100
    if name == "blob24":
        assert rep.n_clipped_radius >= 1
    if name == "border150x203":
        assert rep.n_partial_disc >= 10
    if name == "blob11":                                   # the octave of side 11 has one searchable position
        assert {(f.o, f.ref.r, f.ref.c) for f in st.finals.values()} == {(1, 5, 5)} and st.G[1].shape[1:] == (11, 11)
    if name == "checker168":
        resp, counts = np.unique(kp[:, 4], return_counts=True)
        assert (counts - 1).sum() == 488                    # keypoints whose response an earlier one already has


def test_symmetric_blob_is_listed_not_decided(sref):
    """feature_cases.blob11_symmetric, the 11 x 11 blob centred exactly on a pixel: one keypoint in the octave of side 11.  The
    picture equals its transpose, its diagonal samples sit on fastAtan2's jump across a bin edge, and which histogram peaks
    exist turns on float32 round-off: the restatement reports 1 orientation, float64 finds 3, every one of the four within the
    histogram's error radius.  `verify` must neither fail the output nor call it decided (measured: 3 claims undecided of 3)."""
    img = F.blob11_symmetric()
    assert np.array_equal(img, img.T)
    kp, d = sref.detect(img)
    assert len(kp) == 1
    rep = S.verify(img, {"nfeatures": 0}, kp, d)
    assert rep.ok, rep.errors
    assert len(rep.undecided) >= 1 and rep.n_clipped_radius == 1


def test_pyramid_bound_holds(sref):
    """Every pixel of every Gaussian layer of the float32 restatement lies within sift_np's bound of the float64 pyramid, and
    every DoG pixel within its bound: the model of round-off behind `blur_error` holds on every case."""
    worst = 0.0
    for name, make, _ in F.SIFT_CASES:
        gray = S.as_gray(make())
        G, D, EG, ED = S.build_pyramid(gray)
        P = sref.pyramid(gray)
        assert len(P) == len(G)
        for o in range(len(G)):
            L = np.stack(P[o])
            assert L.shape == G[o].shape
            for i in range(6):
                e = float(np.abs(L[i].astype(np.float64) - G[o][i]).max())
                worst = max(worst, e / EG[o][i])
                assert e <= EG[o][i], (name, o, i, e, EG[o][i])
            dog = L[1:] - L[:-1]                                                   # float32 differences, as the restatement takes them
            for i in range(5):
                e = float(np.abs(dog[i].astype(np.float64) - D[o][i]).max())
                assert e <= ED[o][i] + 3 * S.U * float(np.abs(D[o][i]).max()), (name, o, i, e, ED[o][i])
    print("largest error / bound of a Gaussian pixel: %.3f" % worst)


# ---- hand-written answers for every stage of sift_np -----------------------------------------------------------------------
def test_stage_upsample_of_a_ramp():
    """INTER_LINEAR x2 reads the source at (k + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25, 1.75, 2.25; replicated edges clamp the
    first and last to 0 and 2.  A ramp 10 x + 30 y is reproduced exactly by linear interpolation."""
    ramp = np.array([[0, 10, 20], [30, 40, 50], [60, 70, 80]], np.uint8)
    at = np.array([0, 0.25, 0.75, 1.25, 1.75, 2.0])
    want = 10 * at[None, :] + 30 * at[:, None]
    assert want[0].tolist() == [0, 2.5, 7.5, 12.5, 17.5, 20] and want[1, 1] == 10.0 and want[5, 5] == 80.0
    assert np.array_equal(S.upsample2(ramp), want)
    assert S.as_gray(np.dstack([ramp, ramp, ramp])).tolist() == ramp.tolist()


def test_stage_pyramid_plan():
    sig = S.layer_sigmas()
    k = 2 ** (1 / 3)
    assert abs(sig[0] - math.sqrt(1.56)) < 1e-15 and abs(sig[1] - 1.6 * math.sqrt(k * k - 1)) < 1e-15 and abs(sig[3] / sig[2] - k) < 1e-12
    assert [len(S.gaussian_taps(x)) for x in sig] == [11, 11, 13, 17, 21, 27]
    assert [S.n_octaves(r, c) for r, c in ((512, 768), (11, 11), (24, 24), (1, 200), (2, 2), (3, 3), (5, 5), (6, 200))] == [9, 3, 5, 0, 1, 2, 2, 3]
    w = S.gaussian_taps(2.0)
    assert abs(w.sum() - 1) < 1e-15 and abs(w[9] / w[8] - math.exp(-0.125)) < 1e-12       # x = 1 over x = 0 of a 17-tap kernel


def test_stage_dog_of_a_gaussian_blob():
    """A blob A exp(-r^2 / 2 s^2) (not rounded to uint8) centred on a base pixel.  The x2 linear interpolation reads the source at
    -0.25 (weight 0.75) and +0.75 (0.25) pixels: a kernel of variance 0.1875 source^2 = 0.75 base^2 per axis.  Layer i then holds
    the blob at variance v_i = (2 s)^2 + 0.75 + (1.6 k^i)^2 - 1, centre value A (2 s)^2 / v_i, and DoG_i = A (2 s)^2 (1 / v_(i+1)
    - 1 / v_i).  Tolerance 1 %: the taps end at 4 sigma, which takes 0.1 % off the added variance, about 5e-3 of a DoG value."""
    s, A, n = 5.0, 150.0, 101
    cx = cy = 50.25                                           # base coordinate 2 * 50.25 + 0.5 = 101, a pixel centre
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    img = A * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    base = S.upsample2(img)
    sig = S.layer_sigmas()
    layers = [S.blur(base, sig[0])]
    for i in range(1, 6):
        layers.append(S.blur(layers[-1], sig[i]))
    k = 2 ** (1 / 3)
    v = [(2 * s) ** 2 + 0.75 + (1.6 * k ** i) ** 2 - 1 for i in range(6)]
    for i in range(5):
        want = A * (2 * s) ** 2 * (1 / v[i + 1] - 1 / v[i])
        got = layers[i + 1][101, 101] - layers[i][101, 101]
        assert abs(got / want - 1) <= 0.01, (i, got, want)


def _quadratic_field(p, A, v0, shape=(5, 15, 15)):
    """D(s, y, x) = 255 (v0 + q' A q / 2), q = (x, y, s) - p."""
    s, y, x = np.mgrid[0:shape[0], 0:shape[1], 0:shape[2]].astype(np.float64)
    q = np.stack([x - p[0], y - p[1], s - p[2]], axis=-1)
    return 255 * (v0 + 0.5 * np.einsum("...i,ij,...j->...", q, A, q))


def test_stage_refine_on_a_quadratic_field():
    """Central differences are exact on a quadratic, so one round lands on its extremum: offset = p - sample, contrast = the
    field's value there (D + g . x / 2 is exact for a quadratic).  From a sample more than half a pixel away the walk moves first."""
    A = -np.array([[0.02, 0.004, 0.001], [0.004, 0.03, -0.002], [0.001, -0.002, 0.025]])
    p, v0 = (7.3, 6.8, 2.1), 0.07
    D = _quadratic_field(p, A, v0)
    for start, rounds in (((2, 7, 7), 1), ((2, 8, 6), 2), ((3, 6, 8), 2)):
        ref = S.refine(D, *start)
        assert ref.status == "kept" and (ref.layer, ref.r, ref.c) == (2, 7, 7) and ref.rounds == rounds
        assert np.allclose(ref.offset, [0.3, -0.2, 0.1], rtol=0, atol=1e-12) and abs(ref.contrast - v0) <= 1e-12
    x, yy, size, resp, packed = S.keypoint_fields(2, 2, ref.offset, 7, 7, ref.contrast)
    assert abs(x - 7.3 * 4 / 2) < 1e-11 and abs(yy - 6.8 * 4 / 2) < 1e-11 and abs(size - 1.6 * 2 ** (2.1 / 3) * 4) < 1e-11 and abs(resp - 0.07) < 1e-12
    assert S.unpack_octave(packed) == (2, 2, 153) and packed == 1 + (2 << 8) + (153 << 16)        # (0.1 + 0.5) 255 = 153
    # the extremum half a pixel beyond layer 3: the move leaves the layers; a weak one fails the contrast test
    assert S.refine(_quadratic_field((7.3, 6.8, 3.6), A, v0), 3, 7, 7).why == ["left the layers or the border"]
    assert S.refine(_quadratic_field(p, A, 0.0133), 2, 7, 7).why == ["contrast"] and S.refine(_quadratic_field(p, A, 0.0134), 2, 7, 7).status == "kept"


def test_stage_edge_threshold():
    """dxx = 10 dyy, dxy = 0 gives tr^2 / det = 121 / 10 exactly: the threshold itself is rejected (10 tr^2 >= 121 det), a ratio
    just above too, just below kept; det <= 0 rejected whatever the trace."""
    assert not S.edge_ok(-10.0, -1.0, 0.0) and not S.edge_ok(-10.01, -1.0, 0.0) and S.edge_ok(-9.99, -1.0, 0.0)
    assert not S.edge_ok(1.0, -1.0, 0.0) and not S.edge_ok(-1.0, -1.0, 1.0) and S.edge_ok(-1.0, -1.0, 0.5)
    for ratio, status in ((9.9, "kept"), (10.1, "rejected")):
        A = -np.diag([0.002 * ratio, 0.002, 0.01])
        ref = S.refine(_quadratic_field((7.0, 7.0, 2.0), A, 0.05), 2, 7, 7)
        assert ref.status == status and (status == "kept" or ref.why == ["edge"])


def _slopes(theta, m=3.0):
    """m (cos, sin) of theta on a grid of 2^-30, so that every pixel of the plane and every difference of two is exact (at 45
    degrees the two components are then equal to the bit, as fastAtan2's branch at |dx| = |dy| needs)."""
    return round(m * math.cos(math.radians(theta)) * 2 ** 30) / 2 ** 30, round(m * math.sin(math.radians(theta)) * 2 ** 30) / 2 ** 30


def _plane(theta, m=3.0, side=41):
    """dx = I(x + 1) - I(x - 1) = 2 m cos(theta), dy = I(y - 1) - I(y + 1) = 2 m sin(theta) everywhere."""
    y, x = np.mgrid[0:side, 0:side].astype(np.float64)
    gx, gy = _slopes(theta, m)
    return 100 + gx * x - gy * y


@pytest.mark.parametrize("theta,angle", [(0.0, 0.0), (45.0, 320.0), (95.0, 270.0), (359.9, 0.0)])
def test_stage_orientation_of_a_constant_gradient(theta, angle):
    """Every sample has the same direction, so all mass falls into bin round(fastAtan2 / 10) and the smoothed histogram is
    symmetric about it: one peak, no parabola offset, angle 360 - 10 bin.  45 degrees: fastAtan2 gives 44.990, bin 4.  359.9: bin
    36 = 0 and the angle 360 folds to 0.  95 lies on the edge of bins 9 and 10 and the polynomial decides: c = tan 5 = 0.0874887,
    p(c) = 57.29578 (0.99978784 c - 0.3258084 c^3 + 0.1555787 c^5) = 4.99921, angle 180 - (90 - 4.99921) = 94.99921, bin 9."""
    scl = 2.0
    ori = S.orientation(_plane(theta), 20, 20, scl)
    assert ori.radius == 9 and ori.n_samples == 19 * 19 and ori.n_skipped == 0
    assert [p.angle for p in ori.peaks] == [angle]
    b = int(round((360 - angle) / 10)) % 36
    i, j = np.mgrid[-9:10, -9:10]
    mass = 2 * math.hypot(*_slopes(theta)) * np.exp(-(i * i + j * j) / (2 * 3.0 ** 2)).sum()
    assert abs(ori.raw[b] / mass - 1) < 1e-12 and np.count_nonzero(ori.raw) == 1
    # near the border the disc is cut: samples strictly inside only
    cut = S.orientation(_plane(theta), 3, 38, scl)
    assert cut.n_samples == (3 + 9) * (9 + 2) and cut.n_skipped == 19 * 19 - cut.n_samples and [p.angle for p in cut.peaks] == [angle]


def test_stage_orientation_parabola_and_threshold():
    """Raw mass 3 in bin 9 and 1 in bin 10: smoothed (x 16) 3, 13, 22, 18, 7, 1 in bins 7..12.  Bin 9 is the one peak; the parabola
    moves it by 0.5 (13 - 18) / (13 - 44 + 18) = 5 / 26 of a bin: angle 360 - 10 (9 + 5 / 26).  A second hump of 0.79 of the
    first is no peak, one of 0.81 is; equal neighbours are no peak (strictly above both)."""
    raw = np.zeros(36); raw[9], raw[10] = 3.0, 1.0
    hist = S.smooth(raw)
    assert np.allclose(hist[7:13] * 16, [3, 13, 22, 18, 7, 1], rtol=0, atol=1e-12)
    peaks = S.peaks_of(hist)
    assert len(peaks) == 1 and peaks[0].bin == 9 and abs(peaks[0].angle - (360 - 10 * (9 + 5 / 26))) < 1e-12
    for share, n in ((0.79, 1), (0.81, 2)):
        raw = np.zeros(36); raw[9], raw[25] = 1.0, share
        assert len(S.peaks_of(S.smooth(raw))) == n
    raw = np.zeros(36); raw[9] = raw[10] = 1.0
    assert S.peaks_of(S.smooth(raw)) == []
    raw = np.zeros(36); raw[0], raw[35] = 3.0, 1.0                    # the wrap: bin -5 / 26 folds to 36 - 5 / 26, angle 10 * 5 / 26
    peaks = S.peaks_of(S.smooth(raw))
    assert len(peaks) == 1 and abs(peaks[0].angle - 50 / 26) < 1e-12


@pytest.mark.parametrize("theta", [0.0, 45.0, 95.0, 359.9])
def test_stage_descriptor_of_a_constant_gradient(theta):
    """With the keypoint's angle set to 360 - fastAtan2 of the gradient, every sample's obin is 0: all mass lies in orientation bin
    0 of every cell.  The spatial profile is then a plain double sum, written out here sample by sample: magnitude 2 m times the
    window exp(-(c_rot^2 + r_rot^2) / 8), split bilinearly between the four cells around (rbin, cbin)."""
    m, scl, xo, yo = 3.0, 1.3, 20.2, 19.7
    img = _plane(theta, m)
    gx, gy = _slopes(theta, m)
    F_ = float(fast_atan2_deg(2 * gy, 2 * gx))
    angle = (360.0 - F_) % 360.0
    hist = S.descriptor_histogram(img, xo, yo, scl, angle)
    radius, clipped = S.descriptor_geometry(img.shape, scl)
    assert radius == round(3 * 1.3 * math.sqrt(2) * 2.5) == 14 and not clipped
    ori = math.radians(360.0 - angle)
    want = np.zeros((4, 4))
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            c_rot = (j * math.cos(ori) - i * math.sin(ori)) / (3 * scl)
            r_rot = (j * math.sin(ori) + i * math.cos(ori)) / (3 * scl)
            rbin, cbin = r_rot + 1.5, c_rot + 1.5
            if not (-1 < rbin < 4 and -1 < cbin < 4):
                continue
            r0, c0 = math.floor(rbin), math.floor(cbin)
            for rr, wr in ((r0, 1 - (rbin - r0)), (r0 + 1, rbin - r0)):
                for cc, wc in ((c0, 1 - (cbin - c0)), (c0 + 1, cbin - c0)):
                    if 0 <= rr < 4 and 0 <= cc < 4:
                        want[rr, cc] += 2 * math.hypot(gx, gy) * math.exp(-(c_rot ** 2 + r_rot ** 2) / 8) * wr * wc
    total = want.sum()
    assert np.abs(hist[:, :, 0] - want).max() <= 1e-9 * total
    assert np.abs(hist[:, :, 1:]).max() <= 1e-9 * total
    # finish: clip at 0.2 of the norm, rescale to 512; 16 equal-ish values of one bin: nothing is clipped unless a cell exceeds 0.2
    v = want.ravel() / np.linalg.norm(want)
    v = np.minimum(v, 0.2)
    pre = S.descriptor(img, xo, yo, scl, angle).reshape(4, 4, 8)
    assert np.abs(pre[:, :, 0].ravel() - np.minimum(512 * v / np.linalg.norm(v), 255)).max() <= 1e-6


def test_stage_descriptor_wrap_clip_and_saturation():
    """Orientation 7.5 bins splits between bins 7 and 0 (8 folds onto 0); one dominant value is clipped at 0.2 of the norm and
    the rest rescaled to a norm of 512; a lone value saturates at 255."""
    img = _plane(0.0)
    hist = S.descriptor_histogram(img, 20.0, 20.0, 1.3, 360.0 - 22.5)      # ori = 22.5: obin = (0 - 22.5) 8 / 360 = -0.5
    tot = hist.sum(axis=(0, 1))
    assert abs(tot[7] / tot[0] - 1) < 1e-9 and np.abs(tot[1:7]).max() <= 1e-12 * tot[0]
    h = np.zeros((4, 4, 8)); h[0, 0, 0], h[1, 2, 3] = 10.0, 1.0
    pre = S.descriptor_finish(h).reshape(4, 4, 8)
    thr = 0.2 * math.sqrt(101)
    assert abs(pre[0, 0, 0] - 255.0) < 1e-9 and abs(pre[1, 2, 3] - min(512 / math.hypot(thr, 1.0), 255)) < 1e-9
    h = np.full((4, 4, 8), 1.0); h[0, 0, 0] = 4.0
    pre = S.descriptor_finish(h)
    c = min(4.0, 0.2 * math.sqrt(127 + 16))
    assert abs(pre[0] - 512 * c / math.sqrt(127 + c * c)) < 1e-9 and abs(pre[1] - 512 / math.sqrt(127 + c * c)) < 1e-9
    assert S.descriptor_distance(np.array([10.4, 20.6]), [10, 21]) == 0.0 and abs(S.descriptor_distance(np.array([10.4, 20.6]), [11, 21]) - 0.1) < 1e-12


def test_stage_extrema_rule():
    """|v| > 1 strictly; >= all 26 neighbours for a maximum (a tie with a neighbour keeps both), <= for a minimum; border 5."""
    D = np.zeros((5, 20, 20))
    D[2, 7, 7] = 2.0                      # a maximum
    D[2, 5, 5] = -1.5                     # a minimum on the first searchable position
    D[2, 4, 10] = 5.0                     # inside the border: not searched
    D[2, 10, 10] = 1.0                    # not above 1
    D[1, 9, 5] = D[2, 9, 6] = 3.0         # equal neighbours in adjacent layers: both pass >=
    D[3, 11, 8], D[2, 12, 9] = 2.0, 2.5   # the larger one wins
    got = {i: list(zip(*[a.tolist() for a in S.extrema(D, i)[:2]])) for i in (1, 2, 3)}
    assert got == {1: [(9, 5)], 2: [(5, 5), (7, 7), (9, 6), (12, 9)], 3: []}
    assert len(S.extrema(np.zeros((5, 10, 30)), 2)[0]) == 0


# ---- the tolerance, measured against sift_np itself -------------------------------------------------------------------------
def test_descriptor_tolerance_measured(sref):
    """DESC_F32_DISTANCE is the largest distance between sift_np's descriptor in float32 arithmetic (pyramid included) and in
    float64 over the sampled keypoints of every case; the reversed / transposed tampers of the same keypoints lie far beyond
    DESC_TOL, and a single element moved by 1 away from the float64 value at 0.5 or more."""
    worst, t_min = (0.0, None), np.inf
    for name, make, _ in F.SIFT_CASES:
        img, _, st = _case(name, "gray")
        st32 = S.Stages(img, np.float32)
        kp, d = sref.detect(img)
        for k in S.sample_indices(kp):
            o, layer, xo, yo, scl = S.octave_position(kp[k])
            a = S.descriptor(st.G[o][layer], xo, yo, scl, kp[k, 3])
            b = S.descriptor(st32.G[o][layer], xo, yo, scl, kp[k, 3], np.float32)
            dist = float(np.linalg.norm(a - b))
            worst = max(worst, (dist, name))
            cells = d[k].reshape(4, 4, 8)
            t_min = min(t_min, S.descriptor_distance(a, cells[:, :, ::-1].reshape(128)), S.descriptor_distance(a, cells.transpose(1, 0, 2).reshape(128)))
            e = int(np.argmax((d[k] > 0) & (d[k] < 255)))
            one = d[k].copy(); one[e] += 1.0 if d[k][e] >= a[e] else -1.0
            t_min = min(t_min, S.descriptor_distance(a, one))
    print("largest float32 distance %.3g (%s), smallest tamper distance %.3g" % (worst + (t_min,)))
    assert 0.5 * S.DESC_F32_DISTANCE <= worst[0] <= S.DESC_F32_DISTANCE
    assert S.DESC_TOL == 4 * S.DESC_F32_DISTANCE and t_min >= S.DESC_TAMPER_MIN and S.DESC_TOL < S.DESC_TAMPER_MIN / 2


# ---- the cuts ---------------------------------------------------------------------------------------------------------------
def _cut_inside_a_group(kp):
    """The first nfeatures whose n-th and (n + 1)-th largest responses are equal: a cut inside one candidate's orientations."""
    resp = np.sort(kp[:, 4])[::-1]
    return next(i + 1 for i in range(1, len(resp) - 1) if resp[i] == resp[i + 1])


def test_verify_follows_both_cuts(sref):
    img, n, st = _case("fountain256x320", "gray")
    full = sref.detect(img)
    tied = _cut_inside_a_group(full[0])
    for nf in (1, tied, n - 1, n, n + 5):
        kp, d = sref.detect(img, nf)
        rep = S.verify(img, {"nfeatures": nf}, kp, d, st)
        assert rep.ok and len(kp) >= min(nf, n), (nf, rep.errors[:5])
        if nf == tied:
            assert len(kp) > nf
        # the same list under another nfeatures is not what the rule gives
        if nf < n - 1:
            assert not S.verify(img, {"nfeatures": nf}, *full, st).ok
    for cap in (0, 1, 57, n):
        kp, d = sref.detect(img, 0, cap)
        assert len(kp) == cap and S.verify(img, {"nfeatures": 0, "max_keypoints": cap}, kp, d, st).ok
    assert not S.verify(img, {"nfeatures": 0, "max_keypoints": 57}, full[0][1:58], full[1][1:58], st).ok      # 57 keypoints, but no prefix


# ---- tampers `verify` must catch ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fountain_output(sref):
    img, n, st = _case("fountain256x320", "gray")
    kp, d = sref.detect(img)
    rep = S.verify(img, {"nfeatures": 0}, kp, d, st)
    assert rep.ok
    loose = {u[1] for u in rep.undecided if u[0] == "reported"} | {u[1] for u in rep.undecided if u[0] == "descriptor rounding"}
    # decided keypoints of three octaves, each the only orientation of its candidate and with a distinct successor
    single = [k for k in range(1, n - 1) if k not in loose and not np.array_equal(kp[k, :3], kp[k - 1, :3]) and not np.array_equal(kp[k, :3], kp[k + 1, :3])]
    octave = lambda k: S.unpack_octave(kp[k, 5])[0]
    picks = [next(k for k in single if octave(k) == o) for o in (0, 1, 3)]
    return img, st, kp, d, picks


def _tamper(kind, kp, d, k, img, st):
    kp, d = kp.copy(), d.copy()
    o = S.unpack_octave(kp[k, 5])[0]
    if kind == "dropped":
        return np.delete(kp, k, 0), np.delete(d, k, 0)
    if kind == "invented":
        row = kp[k].copy(); row[0] += 3.0
        return np.insert(kp, k + 1, row, 0), np.insert(d, k + 1, d[k], 0)
    if kind == "x shifted 0.05 px of its octave":
        kp[k, 0] += 0.05 * 2.0 ** o / 2
    elif kind == "size x 1.02":
        kp[k, 2] *= 1.02
    elif kind == "angle + 10":
        kp[k, 3] = (kp[k, 3] + 10.0) % 360.0
    elif kind == "angle mirrored":
        assert abs((2 * kp[k, 3] + 180.0) % 360.0 - 180.0) > 20.0
        kp[k, 3] = (360.0 - kp[k, 3]) % 360.0
    elif kind == "response x 1.01":
        kp[k, 4] *= 1.01
    elif kind == "layer byte + 1":
        kp[k, 5] += 256.0
    elif kind == "layer byte - 1":
        kp[k, 5] -= 256.0
    elif kind == "swapped":
        kp[[k, k + 1]], d[[k, k + 1]] = kp[[k + 1, k]], d[[k + 1, k]]
    elif kind == "orientation bins reversed":
        d[k] = d[k].reshape(4, 4, 8)[:, :, ::-1].reshape(128)
    elif kind == "cells transposed":
        d[k] = d[k].reshape(4, 4, 8).transpose(1, 0, 2).reshape(128)
    elif kind == "one element by one":
        _, layer, xo, yo, scl = S.octave_position(kp[k])
        pre = S.descriptor(st.G[o][layer], xo, yo, scl, kp[k, 3])
        e = int(np.argmax((d[k] > 0) & (d[k] < 255)))
        d[k, e] += 1.0 if d[k, e] >= pre[e] else -1.0          # the smallest change an integer descriptor can take, away from the value
        assert S.descriptor_distance(pre, d[k]) > S.DESC_TOL
    elif kind == "duplicate put back":
        return np.insert(kp, k + 3, kp[k], 0), np.insert(d, k + 3, d[k], 0)
    return kp, d


TAMPERS = ["dropped", "invented", "x shifted 0.05 px of its octave", "size x 1.02", "angle + 10", "angle mirrored", "response x 1.01", "layer byte + 1",
           "layer byte - 1", "swapped", "orientation bins reversed", "cells transposed", "one element by one", "duplicate put back"]


@pytest.mark.parametrize("kind", TAMPERS)
def test_verify_catches_tamper(fountain_output, kind):
    """Each tamper is applied to one decided keypoint of octave -1, of octave 0 and of octave 2 in turn; every one must fail."""
    img, st, kp, d, picks = fountain_output
    for k in picks:
        if kind == "angle mirrored" and abs((2 * kp[k, 3] + 180.0) % 360.0 - 180.0) <= 20.0:
            k = next(q for q in range(k + 1, len(kp)) if abs((2 * kp[q, 3] + 180.0) % 360.0 - 180.0) > 20.0)
        tk, td = _tamper(kind, kp, d, k, img, st)
        rep = S.verify(img, {"nfeatures": 0, "describe": [k]}, tk, td, st)
        assert not rep.ok, (kind, k)
        assert len(rep.errors) <= 3, (kind, k, rep.errors)                     # and nothing but the tampered keypoint is blamed


def test_verify_catches_a_dropped_tie_below_the_cut(sref, fountain_output):
    """nfeatures cuts inside one candidate's orientations: the keypoints that share the n-th response are kept.  Dropping one of
    them leaves a list that still has nfeatures entries and fails."""
    img, st, kp, d, _ = fountain_output
    nf = _cut_inside_a_group(kp)
    kn, dn = sref.detect(img, nf)
    assert len(kn) > nf and S.verify(img, {"nfeatures": nf}, kn, dn, st).ok
    tied = np.flatnonzero(kn[:, 4] == kn[:, 4].min())
    assert len(tied) >= 2
    for k in tied:
        assert len(kn) - 1 >= nf and not S.verify(img, {"nfeatures": nf}, np.delete(kn, k, 0), np.delete(dn, k, 0), st).ok
