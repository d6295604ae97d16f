"""Pins the CPU restatement oracle/surf_ref.c to the independent statement tests/surf_ref.py (no GPU): the oracle's output passes
`surf_ref.verify` claim by claim on images that reach every rule, the reference's stages give hand-written known answers, the
descriptor tolerance is measured against the reference itself, and the verifier rejects every tampered output."""
import functools

import numpy as np
import pytest

import feature_cases as F
import surf_ref as R

UNDECIDED_CAP = 0.02


@functools.lru_cache(maxsize=None)
def _case(name):
    _, make, thr = next(c for c in F.SURF_CASES if c[0] == name)
    return make(), thr, R.Stages(make(), thr)


@functools.lru_cache(maxsize=None)
def _oracle_out(name):
    import oracle
    oracle.build()
    img, thr, _ = _case(name)
    return oracle.surf(R.bgr2gray(img), thr)


def test_gray_and_integral(oracle_lib):
    img = F.fountain_crop()
    g = R.bgr2gray(img)
    assert np.array_equal(oracle_lib.bgr2gray(img), g)
    assert np.array_equal(R.bgr2gray(np.stack([g] * 3, axis=2)), g)          # the weights sum to 2^14: B = G = R stays itself
    S = R.integral(g)
    assert S.shape == (257, 321) and S[-1, -1] == int(g.astype(np.int64).sum()) and S[10, 20] == int(g[:10, :20].astype(np.int64).sum())
    assert S[-1, -1] < 2 ** 31


@pytest.mark.parametrize("name", [c[0] for c in F.SURF_CASES])
def test_oracle_passes_verifier(oracle_lib, name):
    img, thr, st = _case(name)
    kp, d = _oracle_out(name)
    rep = R.verify(img, {"hessian_threshold": thr}, kp, d, st)
    octs = np.bincount(kp[:, 5].astype(int), minlength=4)
    print(name, rep, "undecided share %.4f" % rep.undecided_share(), "octaves", octs)
    for u in rep.undecided:
        print("   undecided:", u)
    assert rep.ok, rep.errors[:10]
    assert rep.undecided_share() <= UNDECIDED_CAP
    assert rep.n_described == min(len(kp), 150) and rep.max_desc_distance <= R.DESC_TOL
    if name == "blobs240x320":
        assert np.all(octs > 0) and len(kp) > 200                           # every octave yields keypoints
    if name == "blobs33x40":
        # all of octave 0 fits (33 <= 33); of octave 1 only 18 and 30 do, so its middle layer 30 has no layer above it and nothing comes from there
        assert len(kp) > 0 and [l[3] for l in st.layers[:10]] == [True] * 7 + [False] * 3 and octs[1:].sum() == 0
    if name == "border150x203":
        assert rep.n_clamped >= 10 and rep.n_partial_disc >= 10             # the clamped-pixel rule and the points that do not fit are both used
    assert R.verify(R.bgr2gray(img), {"hessian_threshold": thr, "describe": [0]}, kp, d, st).ok      # gray in: same claims


# ---- stage known answers, written down by hand ---------------------------------------------------------------------------
def test_known_answer_gaussian_blob():
    """The paper's 9 x 9 filter stands for sigma 1.2, so a Gaussian blob of standard deviation 2.8 = 1.2 * 21 / 9 belongs to the
    21 x 21 filter; boxes are not Gaussians, so the size is asked to lie within one layer spacing of it (15 .. 27).  One keypoint,
    in octave 0, at the blob's centre.  A bright blob has a negative Laplacian, a dark one a positive: class_id -1 / +1, same
    determinant.  A blob twice as wide is the same picture at twice the scale: its strongest keypoint has about twice the size."""
    def strongest(sigma, sign, rows, cols):
        yy, xx = np.mgrid[0:rows, 0:cols]
        img = np.rint(120 + sign * 100.0 * np.exp(-((yy - rows // 2) ** 2 + (xx - cols // 2) ** 2) / (2 * sigma ** 2))).astype(np.uint8)
        st = R.Stages(img, 500.0)
        kept = sorted(st.kept(), key=st.sort_key)
        assert abs(kept[0].x - cols // 2) < 0.5 and abs(kept[0].y - rows // 2) < 0.5 and kept[0].class_id == -sign
        return kept
    bright, dark = strongest(2.8, 1, 81, 91), strongest(2.8, -1, 81, 91)
    assert len(bright) == 1 and len(dark) == 1 and bright[0].octave == 0 and 15 <= bright[0].size <= 27
    assert dark[0].size == bright[0].size and abs(dark[0].response - bright[0].response) < 0.02 * bright[0].response
    wide = strongest(5.6, 1, 161, 181)
    assert 1.7 <= wide[0].size / bright[0].size <= 2.3
    assert len(R.disc_points()[0]) == 113                                    # i^2 + j^2 <= 36 on the 13 x 13 grid: 169 - 4 * 14


def test_known_answer_layers_and_flat():
    """Filter sizes 9 15 21 27 33, then doubled per octave, steps 1 2 4 8.  A constant image has zero determinant everywhere and a
    ramp too (second differences of a linear function vanish, the box areas being symmetric)."""
    assert [(t[2], t[3]) for t in R.layer_table()] == [((9 + 6 * k) * 2 ** o, 2 ** o) for o in range(4) for k in range(5)]
    for img in (np.full((70, 90), 131, np.uint8), np.tile(np.arange(90, dtype=np.uint8) * 2, (70, 1))):
        S = R.integral(img)
        for size, st in ((9, 1), (15, 1), (36, 2)):
            det, trace, err, valid = R._layer(S, size, st)
            assert valid and np.all(det == 0) and np.all(trace == 0)
    # a vertical step edge: Dxx responds, Dyy and Dxy do not, so the determinant is zero and the trace is not
    img = np.zeros((60, 60), np.uint8); img[:, 30:] = 200
    det, trace, _, _ = R._layer(R.integral(img), 9, 1)
    assert np.all(det == 0) and np.abs(trace).max() > 50


def test_known_answer_orientation_and_descriptor_of_a_ramp():
    """I = 3 x: every Haar sample has X > 0 (right half brighter), Y = 0, so the angle is 0; rot90 turns the picture towards -y
    (y down): 270, 180, 90.  The descriptor of a ramp along the window's own column axis holds only sum dx = sum |dx| > 0."""
    ramp = np.tile((3 * np.arange(81)).astype(np.uint8), (81, 1))
    for turns, want in ((0, 0.0), (1, 270.0), (2, 180.0), (3, 90.0)):
        img = np.ascontiguousarray(np.rot90(ramp, turns))
        o = R.orientation(R.integral(img), 40.25, 40.25, 15.0)                # off the half-pixel grid: no sample corner on a rounding tie
        assert o.n_fit == 113 and not o.undecided and abs((o.angle - want + 180) % 360 - 180) <= o.bound + 1e-9
        v = R.describe(img, 40.0, 40.0, 15.0, want).reshape(16, 4)
        assert np.all(v[:, 0] > 0) and np.allclose(v[:, 0], v[:, 2]) and np.abs(v[:, 1]).max() < 0.02 and abs(np.linalg.norm(v) - 1) < 1e-12
    assert R.window_size(15.0) == 42 and R.window_size(20.0) == 56 and R.window_size(16.0) == 44          # floor(2.8 size)
    A = R._area_matrix(42, 21, np.float64)
    assert np.allclose(A.sum(axis=1), 1) and np.allclose(A[0, :3], [0.5, 0.5, 0])
    A = R._area_matrix(25, 21, np.float64)                                   # 25 / 21: the first cell takes pixel 0 and 4 / 21 of pixel 1
    assert np.allclose(A.sum(axis=1), 1) and np.allclose(A[0, :3], [21 / 25, 4 / 25, 0])


# ---- the descriptor tolerance, measured --------------------------------------------------------------------------------------
def test_descriptor_tolerance_measured(oracle_lib):
    """float64 run against float32 run (sample, shrink and gradient arithmetic in numpy float32) on the sampled keypoints of every
    case; the tamper distances on the same keypoints.  Asserts what the header of tests/surf_ref.py records."""
    worst, tamper_shift, tamper_angle = 0.0, np.inf, np.inf
    for name, _, _ in F.SURF_CASES:
        img, thr, st = _case(name)
        kp, _ = _oracle_out(name)
        for k in R.sample_indices(kp):
            x, y, size, angle = (float(t) for t in kp[k, :4])
            worst = max(worst, R.descriptor_distance(st.gray, x, y, size, angle, R.describe(st.gray, x, y, size, angle, np.float32))[0])
            tamper_shift = min(tamper_shift, R.descriptor_distance(st.gray, x, y, size, angle, R.describe(st.gray, x + 1, y, size, angle))[0])
            tamper_angle = min(tamper_angle, R.descriptor_distance(st.gray, x, y, size, angle, R.describe(st.gray, x, y, size, angle + 2))[0])
    print("float32 against float64: %.3g; tolerance %.3g; smallest tamper distance: shift %.3g, angle %.3g" % (worst, R.DESC_TOL, tamper_shift, tamper_angle))
    assert worst <= R.DESC_F32_DISTANCE and R.DESC_TOL == 4 * R.DESC_F32_DISTANCE
    assert min(tamper_shift, tamper_angle) >= R.DESC_TAMPER_MIN and R.DESC_TOL < R.DESC_TAMPER_MIN / 2


# ---- tamper tests ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good(oracle_lib):
    img, thr, st = _case("blobs240x320")
    kp, d = _oracle_out("blobs240x320")
    return img, thr, st, kp, d


def _run(good, kp, d, describe):
    img, thr, st = good[:3]
    return R.verify(img, {"hessian_threshold": thr, "describe": describe}, kp, d, st)


def _decided(good):
    """Index of a reported keypoint none of whose decisions is undecided."""
    base = _run(good, good[3], good[4], [0])
    assert base.ok
    bad = {u[1] for u in base.undecided if u[0] == "orientation"}
    und = [(c.x, c.y) for c in good[2].cands if c.undecided]
    return next(k for k in range(20, len(good[3])) if k not in bad and k + 1 not in bad and all(abs(good[3][k, 0] - x) + abs(good[3][k, 1] - y) > 1 for x, y in und))


def test_tamper_moved_one_level_pixel(good):
    for k in (5, int(np.argmax(good[3][:, 5]))):          # an octave-0 keypoint and one of the top octave
        kp = good[3].copy()
        kp[k, 0] += 2.0 ** kp[k, 5]
        rep = _run(good, kp, good[4], [k])
        assert not rep.ok and any("matches no maximum" in e for e in rep.errors)


def test_tamper_angle(good):
    k = _decided(good)
    kp = good[3].copy()
    kp[k, 3] = (kp[k, 3] + 2.0) % 360.0
    rep = _run(good, kp, good[4], [])
    assert not rep.ok and any("angle" in e for e in rep.errors)


def test_tamper_response(good):
    kp = good[3].copy()
    kp[7, 4] *= np.float32(1 + 1e-4)
    rep = _run(good, kp, good[4], [])
    assert not rep.ok and any("response" in e for e in rep.errors)


def test_tamper_dropped_duplicated_swapped(good):
    img, thr, st, kp, d = good
    k = _decided(good)
    keep = np.arange(len(kp)) != k
    rep = _run(good, kp[keep], d[keep], [])
    assert not rep.ok and any("missing" in e for e in rep.errors)
    idx = np.insert(np.arange(len(kp)), k, k)
    rep = _run(good, kp[idx], d[idx], [])
    assert not rep.ok and any("twice" in e for e in rep.errors)
    idx = np.arange(len(kp)); idx[[k, k + 1]] = idx[[k + 1, k]]
    rep = _run(good, kp[idx], d[idx], [])
    assert not rep.ok and any("order" in e for e in rep.errors)


def test_tamper_descriptor(good):
    """Descriptors recomputed with the window shifted by one pixel, and with the angle off by 2 degrees, at the keypoints where
    that changes the descriptor least (the largest one, and the sampled one nearest to its own tampered form)."""
    img, thr, st, kp, d = good
    for k in sorted({int(np.argmax(kp[:, 2])), 3, len(kp) - 1}):
        x, y, size, angle = (float(t) for t in kp[k, :4])
        for bad in (R.describe(st.gray, x + 1, y, size, angle), R.describe(st.gray, x, y + 1, size, angle), R.describe(st.gray, x, y, size, angle + 2)):
            dd = d.copy(); dd[k] = bad
            rep = _run(good, kp, dd, [k])
            assert not rep.ok and any("descriptor" in e for e in rep.errors)
            assert R.descriptor_distance(st.gray, x, y, size, angle, bad)[0] > 2 * R.DESC_TOL
