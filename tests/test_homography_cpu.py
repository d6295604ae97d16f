"""The homography model without a GPU (esfm.h "Homography RANSAC"): the host build of easysfm_amd/csrc/homography_core.hpp against the
Python restatement (tests/homography_ref.py route (a), bit for bit) and against the independent SVD route (route (b), to a tolerance
measured from that route's own sensitivity), the sample stream with its subset check, the initial-pair guard, and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import homography_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    from easysfm_amd import motion
    return motion


@pytest.fixture(scope="module")
def samples():
    return R.solver_samples()


@pytest.fixture(scope="module")
def host_models(M, samples):
    return M.homography_models(samples[0], samples[1], host=True)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _one_ulp(x, rng):
    """every coordinate moved by one unit in the last place, up or down at random"""
    return np.nextafter(x, np.where(rng.random(x.shape) < 0.5, -np.inf, np.inf))


def _rel(H, Hb):
    return float(np.max(np.abs(H - Hb)) / np.max(np.abs(Hb)))


def test_host_build_equals_the_restatement_bit_for_bit(samples, host_models):
    """esfm_homography_models_host == route (a) on 4 096 sampled 4-subsets of a plane, a rotation and general relief with 30 % outliers,
    plus the hand-made degenerate samples: H and the model flag."""
    q1, q2 = samples
    H, has = host_models
    assert len(q1) == 4096 + 6
    ref = [R.minimal_solve(q1[i], q2[i]) for i in range(len(q1))]
    Ha = np.array([r[0] for r in ref]).reshape(-1, 3, 3); ha = np.array([r[1] for r in ref])
    assert np.array_equal(has, ha)
    assert np.array_equal(_bits(H), _bits(Ha))
    assert has[:4096].mean() > 0.99
    # the degenerate ones: four identical points, a correspondence at infinity and a collapsed second image give no model and zeros;
    # coordinates of 1e6 give one; three collinear points give whatever the arithmetic gives -- the same on both sides (above)
    assert not has[-6] and not has[-3] and not has[-1] and has[-2]
    assert not H[-6].any() and not H[-3].any() and not H[-1].any()
    assert np.all(H[has][:, 2, 2] == 1.0)


def test_host_build_against_the_svd_route(samples, host_models):
    """Route (b) on the same samples.  Kept: samples whose normalised 8 x 9 system has sigma_8 / sigma_1 >= 1e-4 (at most 2 % may be
    left out; measured: 6 of 4 102, the six degenerate ones).  B = the largest relative change of route (b)'s own H when every
    input coordinate moves by one ulp = 6.6e-10 on these samples; the host build must be within 16 B of route (b) (measured: 4.6e-10)."""
    q1, q2 = samples
    H, has = host_models
    rng = np.random.default_rng(42)
    kept, B, worst = 0, 0.0, 0.0
    for i in range(len(q1)):
        if not (np.all(np.isfinite(q1[i])) and np.all(np.isfinite(q2[i]))):
            continue
        with np.errstate(all="ignore"):
            Hb, cond = R.svd_solve(q1[i], q2[i])
        if not (cond >= 1e-4):
            continue
        kept += 1
        assert has[i]
        Hp, _ = R.svd_solve(_one_ulp(q1[i], rng), _one_ulp(q2[i], rng))
        B = max(B, _rel(Hp, Hb))
        worst = max(worst, _rel(H[i], Hb))
    print(f"kept {kept} of {len(q1)}, B = {B:.3e}, host build vs route (b) = {worst:.3e}")
    assert len(q1) - kept <= 0.02 * len(q1)
    assert B > 0.0
    assert worst <= 16.0 * B


@pytest.fixture(scope="module")
def refit_cases():
    """the three correspondence sets with the RANSAC masks of route (a), threshold 1"""
    out = []
    for name, (a, b) in R.correspondence_sets().items():
        H, mask, _, _ = R.find_homography(a, b, 1.0)
        assert H is not None and mask.sum() >= 4
        out.append((name, a, b, mask))
    return out


def test_refit_host_equals_the_restatement_bit_for_bit(M, refit_cases):
    """esfm_homography_refit_host == route (a)'s re-fit: 256 virtual lanes, halving tree, Jacobi eigenvector."""
    for name, a, b, mask in refit_cases:
        Ha, ok = R.refit(a, b, mask)
        assert ok
        assert np.array_equal(_bits(M.homography_refit_host(a, b, mask)).reshape(9), _bits(Ha)), name
    # more than one point per lane, and an unmasked call
    a, b = R.ransac_case(513, 0.0)
    Ha, ok = R.refit(a, b)
    assert ok and np.array_equal(_bits(M.homography_refit_host(a, b)).reshape(9), _bits(Ha))


def test_refit_host_against_the_svd_route(M, refit_cases):
    """The least-squares form on the inliers, same scheme: B = route (b)'s largest relative change under one ulp per coordinate =
    7.6e-14, the host re-fit within 16 B of it (measured: 9.9e-14).  For n = 4 the re-fit and the minimal solve agree to the same bound
    (measured: 1.3e-13)."""
    rng = np.random.default_rng(43)
    B, worst = 0.0, 0.0
    cases = [(a[mask].astype(np.float64), b[mask].astype(np.float64), M.homography_refit_host(a, b, mask)) for _, a, b, mask in refit_cases]
    a4, b4 = R.ransac_case(4, 0.0)
    H4 = M.homography_refit_host(a4, b4)
    Hmin, has = M.homography_models(a4.astype(np.float64), b4.astype(np.float64), host=True)
    assert has[0]
    cases.append((a4.astype(np.float64), b4.astype(np.float64), H4))
    for a, b, H in cases:
        Hb, _ = R.svd_solve(a, b)
        for _ in range(8):
            B = max(B, _rel(R.svd_solve(_one_ulp(a, rng), _one_ulp(b, rng))[0], Hb))
        worst = max(worst, _rel(H, Hb))
    four = _rel(H4, Hmin[0])
    print(f"B = {B:.3e}, host re-fit vs route (b) = {worst:.3e}, re-fit vs minimal solve at n = 4: {four:.3e}")
    assert worst <= 16.0 * B
    assert four <= 16.0 * B


def test_float_scoring_array_form_equals_scalar_form():
    a, b = R.ransac_case(65, 0.3)
    H, _ = R.minimal_solve(a[:4].astype(np.float64), b[:4].astype(np.float64))
    err = R.transfer_errors(H, a, b)
    for i in range(len(a)):
        assert err[i] == R.transfer_error_scalar(H, a[i, 0], a[i, 1], b[i, 0], b[i, 1])
        assert isinstance(R.transfer_error_scalar(H, a[i, 0], a[i, 1], b[i, 0], b[i, 1]), np.float32)


def test_sample_stream_with_subset_check(M):
    """esfm_homography_sample_stream == route (a)'s sampler.  60 % of the points lie on one line, so subsets with a collinear triple are
    drawn and redrawn; every emitted subset passes the check."""
    rng = np.random.default_rng(9)
    n = 50
    a = np.stack([rng.uniform(5, 763, n), rng.uniform(5, 507, n)], 1).astype(np.float32)
    on_line = np.arange(n) < 30
    a[on_line, 0] = rng.permutation(700)[:30] + 10.0                        # whole numbers: y = x / 2 + 20 is exact, the line is a line in float too
    a[on_line, 1] = (0.5 * a[on_line, 0] + 20.0).astype(np.float32)
    b = (a * np.float32(1.02) + np.float32(3.0)).astype(np.float32)
    idx, redraws = M.homography_sample_stream(a, b, 300)
    ref, ref_redraws = R.sample_stream(a, b, 300)
    assert np.array_equal(idx, ref) and redraws == ref_redraws
    assert redraws > 0
    p1, p2 = R._as_lists(a), R._as_lists(b)
    for s in idx:
        assert len(set(s.tolist())) == 4 and R.check_subset(p1, p2, s.tolist())
        assert on_line[s].sum() <= 2
    # without rejections the stream is the plain distinct-index draw
    a2, b2 = R.ransac_case(64, 0.0)
    idx2, redraws2 = M.homography_sample_stream(a2, b2, 64)
    assert np.array_equal(idx2, R.sample_stream(a2, b2, 64)[0])
    with pytest.raises(Exception):
        M.homography_sample_stream(a[:3], b[:3], 1)


def test_route_a_separates_the_synthetic_pairs():
    """What the GPU classification test asserts, on route (a) alone: the returned model's inliers are at most 0.2 of the correspondences
    on general pairs and at least 0.8 on planar and rotation-only pairs (0.2 px noise, threshold 1).  (Dividing by the essential matrix's
    inliers instead of all correspondences can only raise a ratio, and by at most 1 / 0.5 on these scenes.)"""
    pairs, _ = R.scene_pairs()
    for kind, lst in pairs.items():
        for a, b, _, _, _ in lst:
            H, mask, _, _ = R.find_homography(a, b, 1.0)
            frac = 0.0 if H is None else float(np.count_nonzero(R.inlier_mask(H.reshape(9), a, b, 1.0))) / len(a)
            print(kind, len(a), round(frac, 3))
            assert frac <= 0.1 if kind == "general" else frac >= 0.8


def _table():
    from easysfm_amd.pipeline import FramePair
    T = np.zeros((4, 22), bool)
    T[2:4, 0:10] = True; T[1:3, 10:16] = True; T[0:2, 16:22] = True          # scores: (3,2) = 20, (2,1) = 12, (1,0) = 12
    graph = [[FramePair(i, j, appro_depth=5.0, h_inlier_ratio=0.05) for j in range(i)] for i in range(4)]
    graph[3][2].h_inlier_ratio = 0.95
    return T, graph


def test_init_pair_guard():
    """findInitializeFramePair(max_h_inlier_ratio=...) on a hand-made 4-frame table: the best-scoring pair is skipped when its ratio exceeds
    the limit, ties still go to the later pair, the depth guard comes first, None changes nothing."""
    import easysfm_amd as E
    fm = E.FeatureMatching.__new__(E.FeatureMatching)
    T, graph = _table()
    frames = [None] * 4
    assert fm.findInitializeFramePair(T, frames, graph, min_track_num_init=5) == (True, 3, 2, 5.0)
    stats = {}
    assert fm.findInitializeFramePair(T, frames, graph, min_track_num_init=5, max_h_inlier_ratio=None, h_stats=stats) == (True, 3, 2, 5.0)
    assert stats == {"candidates": 0, "skipped": 0}
    depths = [[p.appro_depth for p in row] + [0.0] * (4 - len(row)) for row in graph]
    assert fm.findInitializeFramePair(T, frames, depths, min_track_num_init=5) == (True, 3, 2, 5.0)                    # plain depths, as before
    assert fm.findInitializeFramePair(T, frames, depths, min_track_num_init=5, max_h_inlier_ratio=0.8) == (True, 3, 2, 5.0)   # no field: ratio 0
    assert fm.findInitializeFramePair(T, frames, graph, min_track_num_init=5, max_h_inlier_ratio=0.8, h_stats=stats) == (True, 2, 1, 5.0)    # tie -> the later pair
    assert stats == {"candidates": 6, "skipped": 1}
    assert fm.findInitializeFramePair(T, frames, graph, min_track_num_init=5, max_h_inlier_ratio=0.95)[1:3] == (3, 2)   # `>`: at the limit it stays
    graph[2][1].appro_depth = 60.0
    assert fm.findInitializeFramePair(T, frames, graph, min_track_num_init=5, max_h_inlier_ratio=0.8, h_stats=stats)[1:3] == (1, 0)
    assert stats == {"candidates": 5, "skipped": 1}
    graph[2][1].appro_depth = 5.0
    graph[1][0].h_inlier_ratio = graph[2][1].h_inlier_ratio = 0.9
    assert fm.findInitializeFramePair(T, frames, graph, min_track_num_init=5, max_h_inlier_ratio=0.8, h_stats=stats) == (False, 1, 0, None)
    assert stats["skipped"] == 3


def test_frame_pair_defaults():
    from easysfm_amd.pipeline import FramePair
    p = FramePair(1, 0)
    assert p.h_inliers == 0 and p.h_inlier_ratio == 0.0 and p.appro_depth == 1.0


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_cpp_mirror_and_host_header(tmp_path, flags):
    """tests/cpp/homography_check_main.cpp: the esfm_host.hpp mirror of the initial-pair guard on the same table, homography_core.hpp's
    host build against constants printed by route (a), the subset check; a stand-alone host program, g++."""
    exe = str(tmp_path / "homography_check")
    lib_dir = os.path.join(ROOT, "easysfm_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "homography_check_main.cpp"), "-o", exe, os.path.join(lib_dir, "libesfm_hip.so"), "-lz",
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "homography check ok" in r.stdout, r.stdout[-4000:]


def test_bad_arguments(M):
    """the host-only entry points refuse what they cannot use; the GPU ones check their arguments before the device"""
    import ctypes as C
    from easysfm_amd import _lib
    L = _lib.lib()
    a, b = R.ransac_case(8, 0.0)
    H = np.zeros(9); mask = np.zeros(8, np.uint8)
    p = lambda x: C.c_void_p(x.ctypes.data)
    assert L.esfm_find_homography(None, p(a), p(b), 3, 1.0, 0.995, p(H), p(mask), None) == _lib.ESFM_ERR_UNSUPPORTED         # ESFM_ERR_UNSUPPORTED before anything else
    assert L.esfm_find_homography(None, p(a), p(b), 8, 1.0, 0.995, p(H), p(mask), None) == _lib.ESFM_ERR_INVALID_ARG          # ctx is NULL
    assert L.esfm_find_homography(None, p(a), p(b), -1, 1.0, 0.995, p(H), p(mask), None) == _lib.ESFM_ERR_INVALID_ARG
    assert L.esfm_homography_refit_host(p(a), p(b), 3, None, p(H)) == _lib.ESFM_ERR_NUMERIC and not H.any()
    assert L.esfm_homography_models_host(None, None, 1, None, None) == _lib.ESFM_ERR_INVALID_ARG
