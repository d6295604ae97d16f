"""Pins the CPU restatement oracle/orb_ref.c to the independent statement tests/orb_ref.py (no GPU): the oracle's output passes
`orb_ref.verify` claim by claim, the reference's stages give hand-written known answers, and the verifier rejects every tampered
output -- so the tolerances it grants are tight enough to notice one level pixel, 2 degrees, 1e-4 of a response or one bit."""
import functools

import numpy as np
import pytest

import feature_cases as F
import orb_ref as O

UNDECIDED_CAP = 0.02


@functools.lru_cache(maxsize=None)
def _case(name):
    _, make, n = next(c for c in F.ORB_CASES if c[0] == name)
    return make(), n, O.Stages(make(), n)


@pytest.fixture(scope="module")
def good(oracle_lib):
    img, n, st = _case("fountain256x320")
    kp, d = oracle_lib.orb(O.bgr2gray(img), n)
    assert O.verify(img, {"nfeatures": n}, kp, d, st).ok
    return img, n, st, kp, d


def test_pattern_matches_independent_generator(oracle_lib):
    p = O.pattern()
    assert np.array_equal(oracle_lib.orb_pattern(), p)
    assert np.abs(p).max() <= 13 and not np.any((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])) and 5.0 < p.std() < 6.5


def test_gray_conversion(oracle_lib):
    img = F.fountain_crop()
    assert np.array_equal(oracle_lib.bgr2gray(img), O.bgr2gray(img))


@pytest.mark.parametrize("name", [c[0] for c in F.ORB_CASES])
def test_oracle_passes_verifier(oracle_lib, name):
    img, n, st = _case(name)
    gray = O.bgr2gray(img)
    kp, d = oracle_lib.orb(gray, n)
    rep = O.verify(img, {"nfeatures": n}, kp, d, st)
    print(name, rep, "undecided share %.4f" % rep.undecided_share(), "levels", np.bincount(kp[:, 5].astype(int), minlength=8))
    assert rep.ok, rep.errors[:10]
    assert rep.n_reference > 100 and rep.undecided_share() <= UNDECIDED_CAP
    used = [min(l.shape) > 2 * O.EDGE for l in st.levels]
    if name == "fountain256x320":
        assert all(used) and all(np.bincount(kp[:, 5].astype(int), minlength=8) > 0)       # every level yields keypoints
    else:
        assert not all(used) and kp[:, 5].max() == sum(used) - 1                           # the upper levels are skipped
    assert O.verify(gray, {"nfeatures": n}, kp, d, st).ok                                   # gray in: same claims


@pytest.mark.parametrize("nfeatures", [0, 1, 7])
def test_oracle_small_quotas(oracle_lib, nfeatures):
    """Levels whose quota is 0 keep nothing; the last level takes the remainder."""
    img, _, _ = _case("fountain256x320")
    q = O.quotas(nfeatures)
    # by hand: N * (1 - f) / (1 - f^8) = 0.2172 N; for N = 7 that is 1.52, 1.27, 1.06, 0.88, 0.73, 0.61, 0.51 -- every one rounds up,
    # the first seven levels already take 8 and the last level's remainder is clamped to 0
    assert q == {0: [0] * 8, 1: [0] * 7 + [1], 7: [2, 1, 1, 1, 1, 1, 1, 0]}[nfeatures]
    kp, d = oracle_lib.orb(O.bgr2gray(img), nfeatures)
    rep = O.verify(img, {"nfeatures": nfeatures}, kp, d)
    assert rep.ok, rep.errors[:10]
    assert len(kp) >= nfeatures and (nfeatures > 0 or len(kp) == 0)


# ---- stage known answers, written down by hand ---------------------------------------------------------------------------
def test_known_answer_bright_square():
    """A 200-bright 20 x 20 square on black.  At a corner pixel of the square 11 contiguous ring pixels lie outside (darker by 200),
    5 inside: a corner for every t < 200, score 199.  At the middle of an edge only 7 ring pixels lie outside: no corner.  Harris:
    positive at the corner, negative on the edge (one gradient direction only: -0.04 b^2), zero on flat ground."""
    img = np.zeros((80, 80), np.uint8)
    img[30:50, 30:50] = 200
    s = O.fast_score(img)
    for y, x in ((30, 30), (30, 49), (49, 30), (49, 49)):
        assert s[y, x] == 199
    assert s[30, 40] == 0 and s[40, 30] == 0 and s[40, 40] == 0 and s[10, 10] == 0
    assert s[29, 29] == 0                                      # the dark pixel diagonally outside sees 3 bright ring pixels only
    a, b, c = O.harris_sums(img)
    h, e = O.harris(a, b, c)
    assert h[30, 30] > e[30, 30] and h[49, 49] > e[49, 49]
    assert a[30, 40] == 0 and b[30, 40] > 0 and h[30, 40] == -0.04 * float(b[30, 40]) ** 2 * O.HARRIS_K4 < 0
    assert h[10, 10] == 0 and h[40, 40] == 0


def test_known_answer_ramp_orientation():
    """I = 4 x: all mass to the right, m01 = 0, angle 0.  np.rot90 turns the picture counter-clockwise on the screen, i.e. towards
    -y (y points down): 270, 180, 90 degrees for one, two, three turns."""
    ramp = np.tile((4 * np.arange(41)).astype(np.uint8), (41, 1))
    for turns, want in ((0, 0.0), (1, 270.0), (2, 180.0), (3, 90.0)):
        m01, m10 = O.moments(np.ascontiguousarray(np.rot90(ramp, turns)), 20, 20)
        assert (m01 == 0) == (want in (0.0, 180.0)) and (m10 == 0) == (want in (90.0, 270.0))
        assert O.fast_atan2_deg(float(m01), float(m10)) == want
    m = O.disc_mask()
    # rows 0, +-1 .. +-15 hold 2 umax + 1 pixels: 31 + 2 * (2 * (187 - 15) + 15) = 749, close to the area of a radius-15.5 disc
    assert m.sum() == 749 and np.array_equal(m, m.T) and np.array_equal(m, m[::-1, ::-1])
    assert abs(m.sum() - np.pi * 15.5 ** 2) < 10


def test_known_answer_constant_image():
    """Blur weights sum to 256 and the resize weights of a row to 256: a constant image stays the constant, at every size."""
    img = np.full((67, 83), 173, np.uint8)
    assert O.gauss7().sum() == 256 and np.array_equal(O.gauss7(), O.gauss7()[::-1]) and np.array_equal(O.blur7(img), img)
    for lv in O.pyramid(img):
        assert np.all(lv == 173)
    assert [l.shape for l in O.pyramid(img)][:3] == [(67, 83), (56, 69), (47, 58)]              # 67 / 1.2 = 55.8, 83 / 1.2 = 69.2, / 1.44 = 46.5, 57.6
    # a ramp survives a bilinear shrink as a ramp: interior samples lie on the line (x + 0.5) s - 0.5 within the 1/256 weights
    ramp = np.tile(np.arange(120, dtype=np.uint8), (8, 1))
    out = O.resize(ramp, 8, 100).astype(float)
    assert np.abs(out[0, 1:-1] - ((np.arange(1, 99) + 0.5) * 1.2 - 0.5)).max() <= 0.5 + 1 / 256


# ---- tamper tests ----------------------------------------------------------------------------------------------------------
def _run(good, kp, d):
    img, n, st = good[:3]
    return O.verify(img, {"nfeatures": n}, kp, d, st)


def test_tamper_descriptor_bit(good):
    kp, d = good[3].copy(), good[4].copy()
    d[17, 5] ^= 0x10
    rep = _run(good, kp, d)
    assert not rep.ok and any("descriptor" in e for e in rep.errors)


def test_tamper_moved_one_level_pixel(good):
    for k in (3, len(good[3]) - 1):                     # a level-0 keypoint and one of the top level
        kp = good[3].copy()
        kp[k, 0] += np.float32(1.2 ** int(kp[k, 5]))
        assert not _run(good, kp, good[4]).ok


def test_tamper_angle(good):
    kp = good[3].copy()
    kp[40, 3] = (kp[40, 3] + 2.0) % 360.0
    rep = _run(good, kp, good[4])
    assert not rep.ok and any("angle" in e for e in rep.errors)


def test_tamper_response(good):
    kp = good[3].copy()
    kp[0, 4] *= np.float32(1 + 1e-4)
    rep = _run(good, kp, good[4])
    assert not rep.ok and any("response" in e for e in rep.errors)


def test_tamper_dropped_duplicated_swapped(good):
    img, n, st, kp, d = good
    und = {u[1:] for u in _run(good, kp, d).undecided}
    k = next(i for i in range(5, len(kp)) if (int(kp[i, 5]), round(kp[i, 1] / 1.2 ** kp[i, 5]), round(kp[i, 0] / 1.2 ** kp[i, 5])) not in und)
    keep = np.arange(len(kp)) != k
    rep = _run(good, kp[keep], d[keep])
    assert not rep.ok and any("missing" in e for e in rep.errors)
    idx = np.insert(np.arange(len(kp)), k, k)
    rep = _run(good, kp[idx], d[idx])
    assert not rep.ok and any("twice" in e for e in rep.errors)
    idx = np.arange(len(kp)); idx[[k, k + 1]] = idx[[k + 1, k]]
    assert kp[k, 4] != kp[k + 1, 4] or kp[k, 5] != kp[k + 1, 5]
    rep = _run(good, kp[idx], d[idx])
    assert not rep.ok and any("order" in e for e in rep.errors)
