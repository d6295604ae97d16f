"""The HIP ORB, SURF and SIFT detectors against the independent statements tests/orb_ref.py, tests/surf_ref.py and
tests/sift_np.py -- the same `verify` and the same caps that pin the CPU oracle in tests/test_orb_ref_cpu.py /
tests/test_surf_ref_cpu.py / tests/test_sift_ref_cpu.py, run on the library's output directly, in gray and in BGR form -- and
the host-side selection paths the bit-parity tests leave out, bit for bit against the CPU oracle: small and zero quotas,
max_keypoints, massive ties, minimum image sizes, SURF's candidate read-back past its first chunk, keypoints whose window and
orientation disc leave the image, and for SIFT the smallest octaves, empty results and both cuts."""
import functools
import os
import re

import numpy as np
import pytest

import easysfm_amd as E
import feature_cases as F
import orb_ref as O
import sift_np as N
import surf_ref as R
from sift_ref import SiftRef

pytestmark = pytest.mark.gpu
UNDECIDED_CAP = 0.02


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    (kg, dg), (kw, dw) = got, want
    assert len(kg) == len(kw) and np.array_equal(_bits(kg), _bits(kw))
    assert dg.dtype == dw.dtype and np.array_equal(dg.view(np.uint8), dw.view(np.uint8))


@functools.lru_cache(maxsize=None)
def _orb_stages(name):
    _, make, n = next(c for c in F.ORB_CASES if c[0] == name)
    return make(), n, O.Stages(make(), n)


@functools.lru_cache(maxsize=None)
def _surf_stages(name):
    _, make, thr = next(c for c in F.SURF_CASES if c[0] == name)
    return make(), thr, R.Stages(make(), thr)


# ---- the same verifier on the library's output -------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["gray", "bgr"])
@pytest.mark.parametrize("name", [c[0] for c in F.ORB_CASES])
def test_orb_library_passes_verifier(gpu_ctx, name, form):
    img, n, st = _orb_stages(name)
    kp, d = E.orb_detect_and_compute(img if form == "bgr" else O.bgr2gray(img), n, None, gpu_ctx)
    rep = O.verify(img, {"nfeatures": n}, kp, d, st)
    print(name, form, rep, "undecided share %.4f" % rep.undecided_share())
    assert rep.ok, rep.errors[:10]
    assert rep.n_reported > 100 and rep.undecided_share() <= UNDECIDED_CAP


@pytest.mark.parametrize("form", ["gray", "bgr"])
@pytest.mark.parametrize("name", [c[0] for c in F.SURF_CASES])
def test_surf_library_passes_verifier(gpu_ctx, name, form):
    img, thr, st = _surf_stages(name)
    kp, d = E.surf_detect_and_compute(img if form == "bgr" else R.bgr2gray(img), thr, None, gpu_ctx)
    rep = R.verify(img, {"hessian_threshold": thr}, kp, d, st)
    print(name, form, rep, "undecided share %.4f" % rep.undecided_share())
    assert rep.ok, rep.errors[:10]
    assert rep.n_reported > 0 and rep.undecided_share() <= UNDECIDED_CAP
    assert rep.n_described == min(len(kp), 150) and rep.max_desc_distance <= R.DESC_TOL
    if name == "border150x203":
        assert rep.n_clamped >= 10 and rep.n_partial_disc >= 10


# ---- ORB selection edges, bit for bit against the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("nfeatures", [0, 1, 7])
def test_orb_small_quotas(gpu_ctx, oracle_lib, nfeatures):
    """nfeatures 0: every quota is 0.  1: seven levels have quota 0 and the last takes the remainder.  7: the first seven levels
    already take 8, the last level's remainder is clamped to 0."""
    gray = O.bgr2gray(F.fountain_crop())
    got = E.orb_detect_and_compute(gray, nfeatures, None, gpu_ctx)
    _same(got, oracle_lib.orb(gray, nfeatures))
    lv = np.bincount(got[0][:, 5].astype(int), minlength=8)
    assert np.all((lv > 0) == (np.array(O.quotas(nfeatures)) > 0))
    assert O.verify(gray, {"nfeatures": nfeatures}, *got).ok


def test_orb_max_keypoints(gpu_ctx, oracle_lib):
    """A cap below the result returns the prefix of the uncapped output (levels ascending, strongest first inside a level); a cap
    equal to the count changes nothing; 0 returns nothing."""
    gray = O.bgr2gray(F.fountain_crop())
    full = E.orb_detect_and_compute(gray, 500, None, gpu_ctx)
    n = len(full[0])
    assert n > 300
    for cap in (1, 113, n - 1):                       # 113 ends inside level 1: later levels are cut off entirely
        got = E.orb_detect_and_compute(gray, 500, cap, gpu_ctx)
        _same(got, (full[0][:cap], full[1][:cap]))
        _same(got, oracle_lib.orb(gray, 500, cap))
    _same(E.orb_detect_and_compute(gray, 500, n, gpu_ctx), full)
    kp, d = E.orb_detect_and_compute(gray, 500, 0, gpu_ctx)
    assert len(kp) == 0 and len(d) == 0


def test_orb_massive_ties(gpu_ctx, oracle_lib):
    """A periodic picture: the same corner in every period, so hundreds of candidates share FAST score and Harris sums.  Both
    retainBest rules keep every tie with the last kept one: level 0 ends with more than its quota, in (y, x) order inside ties."""
    img = F.checker()
    assert img.shape[0] >= 160 and img.shape[1] >= 160
    n = 100
    st = O.Stages(img, n)
    quota = O.quotas(n)[0]
    cand = O.candidates(st.score[0])
    assert len(cand) > 200 and len(st.first[0]) > 2 * quota and len(st.final[0]) > quota       # both tie rules keep more than they were asked for
    got = E.orb_detect_and_compute(img, n, None, gpu_ctx)
    _same(got, oracle_lib.orb(img, n))
    kp = got[0]
    l0 = kp[kp[:, 5] == 0]
    assert len(l0) == len(st.final[0]) > quota
    resp, counts = np.unique(l0[:, 4], return_counts=True)
    assert counts.max() >= 9                                                                    # one corner, once per period
    for r in resp:
        tie = l0[l0[:, 4] == r]
        order = np.lexsort((tie[:, 0], tie[:, 1]))                                              # by y, then x
        assert np.array_equal(order, np.arange(len(tie)))
    rep = O.verify(img, {"nfeatures": n}, *got, st)
    assert rep.ok and rep.undecided_share() <= UNDECIDED_CAP, (rep.errors[:10], rep.undecided)


def test_orb_minimum_sizes(gpu_ctx, oracle_lib):
    """A level is searched at positions 31 <= x < cols - 31.  62 x 62 has none.  63 x 63 has exactly one, its centre pixel (31, 31):
    the result is empty unless that one pixel is a corner, which it is not in this texture (the oracle agrees); a second 63 x 63
    picture puts a corner exactly there and must return it.  64 x 64 and 69 x 69 search a 2 x 2 and a 7 x 7 patch of level 0 only.
    One-row and one-column images run every kernel on a degenerate pyramid and return nothing."""
    for side in (62, 63):
        gray = O.bgr2gray(F.blocks(side, side, 11))
        kp, d = E.orb_detect_and_compute(gray, 300, None, gpu_ctx)
        assert len(kp) == 0 and len(d) == 0
        assert len(oracle_lib.orb(gray, 300)[0]) == 0
    corner = np.full((63, 63), 40, np.uint8)
    corner[:32, :32] = 200                                  # the bright square's corner pixel is (31, 31)
    corner[31, 31] = 230                                    # and it alone is the strict maximum of the score
    got = E.orb_detect_and_compute(corner, 300, None, gpu_ctx)
    _same(got, oracle_lib.orb(corner, 300))
    assert len(got[0]) == 1 and tuple(got[0][0, :2]) == (31.0, 31.0) and O.verify(corner, {"nfeatures": 300}, *got).ok
    for side, seed in ((64, 11), (69, 11), (69, 12)):
        gray = O.bgr2gray(F.blocks(side, side, seed))
        got = E.orb_detect_and_compute(gray, 300, None, gpu_ctx)
        _same(got, oracle_lib.orb(gray, 300))
        assert O.verify(gray, {"nfeatures": 300}, *got).ok
    for shape in ((1, 200), (200, 1), (1, 1)):
        line = (np.arange(shape[0] * shape[1]) * 37 % 256).astype(np.uint8).reshape(shape)
        kp, d = E.orb_detect_and_compute(line, 300, None, gpu_ctx)
        assert len(kp) == 0 and len(d) == 0
        assert len(oracle_lib.orb(line, 300)[0]) == 0


# ---- SURF read-back and border -----------------------------------------------------------------------------------------------
def _first_chunk():
    src = open(os.path.join(os.path.dirname(E.__file__), "csrc", "surf_api.cpp")).read()
    return int(re.search(r"constexpr\s+int\s+kFirstCand\s*=\s*(\d+)\s*;", src).group(1))


def test_surf_candidates_past_first_chunk(gpu_ctx, oracle_lib):
    """White noise under a threshold near zero holds a maximum at about every 28th pixel: 296 x 390 is about the smallest image
    whose candidate list outgrows the first read-back chunk, so the rest comes in a second transfer.  Full and capped calls."""
    first = _first_chunk()
    img = F.white_noise(296, 390, 7)
    want = oracle_lib.surf(img, 0.001)
    assert first < len(want[0]) < 1.1 * first           # every reported keypoint was a candidate: the list is longer than the chunk
    got = E.surf_detect_and_compute(img, 0.001, None, gpu_ctx)
    _same(got, want)
    for cap in (100, first, first + 1):
        capped = E.surf_detect_and_compute(img, 0.001, cap, gpu_ctx)
        _same(capped, (want[0][:cap], want[1][:cap]))
        _same(capped, oracle_lib.surf(img, 0.001, cap))


def test_surf_border_keypoints(gpu_ctx, oracle_lib):
    """Keypoints as close to the border as the detector allows, in an image whose width is no multiple of 4: descriptor windows
    and orientation discs leave the image (the verifier counts both)."""
    img, thr, st = _surf_stages("border150x203")
    gray = R.bgr2gray(img)
    assert gray.shape[1] % 4 != 0
    got = E.surf_detect_and_compute(gray, thr, None, gpu_ctx)
    _same(got, oracle_lib.surf(gray, thr))
    kp = got[0]
    edge = np.minimum(np.minimum(kp[:, 0], gray.shape[1] - 1 - kp[:, 0]), np.minimum(kp[:, 1], gray.shape[0] - 1 - kp[:, 1]))
    half_window = np.array([R.window_size(s) for s in kp[:, 2]]) / 2
    assert (edge < half_window).sum() >= 10 and (edge < 6 * kp[:, 2] * 1.2 / 9).sum() >= 10


# ---- SIFT: the same verifier on the library's output ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return SiftRef(tmp_path_factory.mktemp("sift_ref"))


@functools.lru_cache(maxsize=None)
def _sift_stages(name):
    _, make, n = next(c for c in F.SIFT_CASES if c[0] == name)
    return make(), n, N.Stages(make())


@pytest.mark.parametrize("form", ["gray", "bgr"])
@pytest.mark.parametrize("name", [c[0] for c in F.SIFT_CASES])
def test_sift_library_passes_verifier(gpu_ctx, name, form):
    img, n, st = _sift_stages(name)
    kp, d = E.sift_detect_and_compute(img if form == "bgr" else N.as_gray(img), 0, None, gpu_ctx)
    rep = N.verify(img, {"nfeatures": 0}, kp, d, st)
    print(name, form, rep, "undecided share %.4f" % rep.undecided_share())
    assert rep.ok, rep.errors[:10]
    assert rep.n_reported == n and rep.undecided_share() <= UNDECIDED_CAP
    assert rep.n_described >= min(len(kp), 150) - len(rep.undecided) and rep.max_desc_distance <= N.DESC_TOL
    if name in ("fountain256x320", "blobs240x320"):
        assert rep.n_reported > 100
    if name == "blob24":
        assert rep.n_clipped_radius >= 1
    if name == "border150x203":
        assert rep.n_partial_disc >= 10


# ---- SIFT bit for bit on the pictures tests/test_sift_gpu.py leaves out ----------------------------------------------------
def _sift_same(got, want):
    (kg, dg), (kw, dw) = got, want
    assert kg.shape == kw.shape, (kg.shape, kw.shape)
    assert np.array_equal(_bits(kg), _bits(kw)) and np.array_equal(_bits(dg), _bits(dw))


def test_sift_smallest_octaves_and_ties(gpu_ctx, sref):
    """11 x 11: the keypoint lies in the octave of side 11, whose only searchable position is (5, 5), and its orientation disc and
    descriptor window cover the whole octave (the symmetric blob, whose peaks turn on float32 round-off alone, and the one moved
    off its axes).  24 x 24: descriptor radius 36 clipped to the octave's diagonal 33.  checker: 537 keypoints, 488 of which
    repeat an earlier response.  White noise: 479 keypoints of the finest layers."""
    for img, n in ((F.blob11_symmetric(), 1), (F.single_blob(11, 100, 2.5, 5.1, 4.95), 2), (F.single_blob(24, 60, 4.0, 11.8, 12.3), 5),
                   (F.checker(), 537), (F.white_noise(296, 390, 7), 479)):
        want = sref.detect(img)
        assert len(want[0]) == n
        _sift_same(E.sift_detect_and_compute(img, 0, None, gpu_ctx), want)
    kp = sref.detect(F.single_blob(24, 60, 4.0, 11.8, 12.3))[0]
    assert len(np.unique(kp[:, :3], axis=0)) == 1 and len(np.unique(kp[:, 3])) == 5           # five orientations of one point


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 3), (5, 5), (6, 200), (200, 6), (1, 200), (200, 1), (40, 40)])
def test_sift_empty_results(gpu_ctx, sref, shape):
    """No octave at all (one row or column), octaves narrower than the border of 5, taps wider than the image, and a constant
    picture: every kernel runs on a degenerate pyramid and both sides return nothing, without an error."""
    img = np.full(shape, 77, np.uint8) if shape == (40, 40) else (np.arange(shape[0] * shape[1]) * 37 % 256).astype(np.uint8).reshape(shape)
    for im in (img, np.repeat(img[:, :, None], 3, axis=2)):
        kp, d = E.sift_detect_and_compute(im, 0, None, gpu_ctx)
        assert kp.shape == (0, 7) and d.shape == (0, 128)
    kw, dw = sref.detect(img)
    assert len(kw) == 0 and len(dw) == 0


def test_sift_selection_edges(gpu_ctx, sref):
    """nfeatures 1; a cut inside one candidate's orientations (the tie is kept); n - 1; n and beyond; 0 (all).  max_keypoints 0, 1
    and n are prefixes of the full result.  All bit-equal to the CPU restatement, and the cut lists pass the verifier."""
    img, n, st = _sift_stages("fountain256x320")
    gray = N.as_gray(img)
    full = E.sift_detect_and_compute(gray, 0, None, gpu_ctx)
    _sift_same(full, sref.detect(gray))
    assert len(full[0]) == n
    resp = np.sort(full[0][:, 4])[::-1]
    tied = next(i + 1 for i in range(1, n - 1) if resp[i] == resp[i + 1])
    for nf in (1, tied, n - 1, n, n + 7):
        got = E.sift_detect_and_compute(gray, nf, None, gpu_ctx)
        _sift_same(got, sref.detect(gray, nf))
        sel = full[0][:, 4] >= resp[min(nf, n) - 1]
        _sift_same(got, (full[0][sel], full[1][sel]))
        assert len(got[0]) >= min(nf, n) and N.verify(gray, {"nfeatures": nf}, *got, st).ok
    assert len(E.sift_detect_and_compute(gray, tied, None, gpu_ctx)[0]) > tied
    for cap in (0, 1, n):
        got = E.sift_detect_and_compute(gray, 0, cap, gpu_ctx)
        _sift_same(got, (full[0][:cap], full[1][:cap]))
        _sift_same(got, sref.detect(gray, 0, cap))
        assert N.verify(gray, {"nfeatures": 0, "max_keypoints": cap}, *got, st).ok
    got = E.sift_detect_and_compute(gray, tied, 5, gpu_ctx)                                  # both cuts: the prefix of the nfeatures list
    _sift_same(got, sref.detect(gray, tied, 5))
