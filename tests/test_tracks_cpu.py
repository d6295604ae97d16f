"""Track triangulation without a GPU (esfm.h "Track triangulation"): the host build of easysfm_amd/csrc/track_core.hpp
(esfm_track_triangulate_host / esfm_track_evaluate_host) against the Python restatement (tests/track_ref.py), bit for bit, at the
track-length edges, on degenerate geometry and at the options' edges; and what the estimator is for -- outliers flagged, clean
observations kept, points nearer the truth than a plain all-observation refit -- on both."""
import os
import subprocess

import numpy as np
import pytest

import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E():
    import easysfm_amd
    return easysfm_amd


@pytest.fixture(scope="module")
def edge():
    """the edge-length case and the restatement's answer to it (default options), computed once"""
    case = R.ring_case(R.EDGE_LENGTHS)
    return case, R.run(*case[:6], R.Options())


def host(E, case, o, xyz_in=None):
    return E.track_triangulate(*case[:5], case[5], xyz_in, E.TrackOptions(**o.kw), host=True)


def test_default_options(E):
    s = E._lib.TrackOptionsStruct()
    E.lib().esfm_track_options_default(s)
    d = E.TrackOptions()
    assert (s.max_reproj_error_px, s.min_angle_deg, s.min_views, s.max_hypotheses, s.refine_iterations) == (4.0, 1.5, 2, 64, 5)
    assert s.cos_min_angle == d.cos_min_angle == R.Options().cos_min_angle


def test_track_length_edges(E, edge):
    """lengths 0 (first, middle and last point), 1, 2, 3, 11 (55 pairs: all used), 12 (66 pairs: the stride rule's first use), 63,
    64, 65, 129 and 300 (above the staging cap of 256), interleaved in the input"""
    case, ref = edge
    got = host(E, case, R.Options())
    R.assert_same(got, ref)
    n = np.array(R.EDGE_LENGTHS)
    assert np.all(ref.status[n < 2] == R.TOO_FEW) and np.all(ref.status[n >= 2] == R.KEPT)
    assert not ref.xyz[n < 2].any()
    # the displaced observations (every fifth of the longer tracks) are flagged, and the points sit at the truth
    assert np.all(ref.n_inliers[n >= 5] == (n - n // 5)[n >= 5])
    assert np.max(np.linalg.norm(ref.xyz[n >= 2] - case[6][n >= 2], axis=1)) < 0.05


def test_stride_rule():
    """12 observations: 66 pairs, hypothesis h uses pair floor(66 h / 64); 11: all 55"""
    assert R.hypothesis_pairs(11, 64) == [(a, b) for a in range(11) for b in range(a + 1, 11)]
    every = [(a, b) for a in range(12) for b in range(a + 1, 12)]
    assert R.hypothesis_pairs(12, 64) == [every[h * 66 // 64] for h in range(64)]
    assert R.pair_from_number(65534 * 65535 // 2 - 1, 65535) == (65533, 65534)


@pytest.mark.parametrize("kw", [dict(min_views=3), dict(refine_iterations=0), dict(max_hypotheses=1), dict(max_reproj_error_px=1.0, min_angle_deg=8.0)])
def test_options_edges(E, edge, kw):
    case = R.ring_case([0, 2, 3, 7, 12, 40], seed=11)
    o = R.Options(**kw)
    ref = R.run(*case[:6], o)
    R.assert_same(host(E, case, o), ref, kw)
    if "min_views" in kw:
        assert ref.status[1] == R.FEW_INLIERS                      # a two-view track under min_views = 3


def test_layouts(E):
    o = R.Options()
    for lengths in ([3], [0], [0, 0, 4, 0]):                       # n_pt = 1; n_obs = 0; unobserved first and last points
        case = R.ring_case(lengths, seed=3)
        R.assert_same(host(E, case, o), R.run(*case[:6], o), lengths)
    got = E.track_triangulate(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), case[3], case[4], 0, host=True)
    assert len(got.status) == 0 and got.xyz.shape == (0, 3)
    # xyz_in comes back for the points that are not kept
    case = R.ring_case([0, 1, 5], seed=5)
    xin = np.arange(9, dtype=np.float64).reshape(3, 3) + 0.5
    got = host(E, case, o, xin)
    R.assert_same(got, R.run(*case[:6], o, xyz_in=xin))
    assert np.array_equal(got.xyz[:2], xin[:2]) and got.status[2] == R.KEPT and not np.array_equal(got.xyz[2], xin[2])


def test_degenerate_geometry_and_scoring(E):
    case = R.degenerate_case()
    o = R.Options()
    ref = R.run(*case[:6], o)
    got = host(E, case, o)
    R.assert_same(got, ref)
    assert list(ref.status[[0, 1, 4, 5, 6]]) == [R.NO_HYPOTHESIS, R.NO_HYPOTHESIS, R.NON_FINITE, R.NON_FINITE, R.KEPT]
    assert ref.status[2] != R.KEPT                                  # every pair an outlier pair
    assert ref.status[3] == R.KEPT and ref.n_inliers[3] == 3        # the duplicates tie; the lower hypothesis index wins on both sides
    assert np.all(np.isinf(ref.obs_err2[np.isin(case[1], [0, 1, 4, 5])]))
    # judged as given points: the point behind its cameras has no inlier (depth sign), a NaN point is status 5
    xyz = case[6].copy()
    xyz[1] = R.behind_point(case[0][case[1] == 1], case[4])
    xyz[6, 0] = np.nan
    ev = R.run(*case[:6], o, xyz_in=xyz, evaluate=True)
    R.assert_same(E.track_evaluate(*case[:5], xyz, E.TrackOptions(), host=True), ev)
    assert ev.status[1] == R.FEW_INLIERS and ev.n_inliers[1] == 0 and ev.status[6] == R.NON_FINITE and ev.status[0] != R.NON_FINITE


def test_permutation_keeps_every_bit(E, edge):
    """any order of the observation list that keeps each track's internal order gives the same outputs"""
    case, ref = edge
    for perm in (np.argsort(case[1], kind="stable"), np.argsort(-case[1], kind="stable")):
        got = E.track_triangulate(case[0][perm], case[1][perm], case[2][perm], case[3], case[4], case[5], host=True)
        assert np.array_equal(R.bits(got.xyz), R.bits(ref.xyz)) and np.array_equal(got.status, ref.status)
        assert np.array_equal(R.bits(got.min_cos), R.bits(ref.min_cos)) and np.array_equal(R.bits(got.mse), R.bits(ref.mse))
        assert np.array_equal(got.obs_inlier, ref.obs_inlier[perm])
        assert np.array_equal(got.obs_err2.view(np.uint32), ref.obs_err2[perm].view(np.uint32))


def test_evaluate_reproduces_the_triangulation(E, edge):
    case, ref = edge
    ev = E.track_evaluate(*case[:5], ref.xyz, E.TrackOptions(), host=True)
    assert ev.xyz is None
    R.assert_same(ev, R.run(*case[:6], R.Options(), xyz_in=ref.xyz, evaluate=True))
    kept = ref.status == R.KEPT
    assert np.array_equal(ev.status[kept], ref.status[kept]) and np.array_equal(ev.n_inliers[kept], ref.n_inliers[kept])
    assert np.array_equal(R.bits(ev.min_cos[kept]), R.bits(ref.min_cos[kept])) and np.array_equal(R.bits(ev.mse[kept]), R.bits(ref.mse[kept]))
    on_kept = kept[case[1]]
    assert np.array_equal(ev.obs_inlier[on_kept], ref.obs_inlier[on_kept])
    assert np.array_equal(ev.obs_err2[on_kept].view(np.uint32), ref.obs_err2[on_kept].view(np.uint32))


def test_arguments(E):
    case = R.ring_case([3], seed=3)
    for bad in (dict(min_views=1), dict(max_hypotheses=0), dict(max_hypotheses=5000), dict(refine_iterations=-1), dict(max_reproj_error_px=0.0),
                dict(max_reproj_error_px=float("nan"))):
        with pytest.raises(E.EsfmError) as ei:
            E.track_triangulate(*case[:5], 1, None, E.TrackOptions(**bad), host=True)
        assert ei.value.status == -1, bad
    for cam, pt in ((case[0] + 160, case[1]), (case[0], case[1] + 1), (case[0], case[1] - 1)):
        with pytest.raises(E.EsfmError) as ei:
            E.track_triangulate(cam, pt, case[2], case[3], case[4], 1, host=True)
        assert ei.value.status == -1


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_host_code_stand_alone(tmp_path, flags):
    """tests/cpp/track_check_main.cpp: track_api.cpp's host path and track_core.hpp compiled into a stand-alone program with g++, on the
    edge cases, against the library's own build of the same entry points, bit for bit"""
    exe = str(tmp_path / "track_check")
    lib_dir = os.path.join(ROOT, "easysfm_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "track_check_main.cpp"), "-o", exe, os.path.join(lib_dir, "libesfm_hip.so"), "-ldl",
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, os.path.join(lib_dir, "libesfm_hip.so")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "track check ok" in r.stdout, r.stdout[-4000:]


def test_without_a_device(E):
    """the device entry points need a context, and creating one reports ESFM_ERR_NO_DEVICE; the host forms work (every other test here)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    case = R.ring_case([3], seed=3)
    for call in (lambda: E.track_triangulate(*case[:5], 1), lambda: E.track_evaluate(*case[:5], case[6])):
        with pytest.raises(E.EsfmError) as ei:
            call()
        assert ei.value.status == -2, ei.value


def test_robustness(E):
    """ba_scene(8, 400, 6, uv_noise=0.5, outlier_frac=0.1), seed 4000, ground-truth cameras, default options -- on the restatement
    and on the host build alike (they agree to the bit, asserted first).
    (a) every injected outlier displaced by more than 3 x 4 px, on a track that keeps three clean observations, is flagged;
    (b) at most 2 % of the clean observations are flagged and at most 2 % of the points are not kept -- conditions, chosen before
        any measurement; the restatement gives 0.00 % (0 of 2 160) and 0.00 % (0 of 400);
    (c) the median distance of the kept points to the truth is below that of the all-observation refit measured here
        (restatement: 0.00618 against 0.01120; DESIGN.md records both)."""
    sc, Rt, injected, clean = R.scene(8, 400, 6)
    o = R.Options()
    ref = R.run(sc.cam_idx, sc.pt_idx, sc.uv, sc.K4, Rt, sc.n_pt, o)
    got = E.track_triangulate(sc.cam_idx, sc.pt_idx, sc.uv, sc.K4, Rt, sc.n_pt, host=True)
    R.assert_same(got, ref)
    base = R.all_observation_refit(sc.cam_idx, sc.pt_idx, sc.uv, sc.K4, Rt, sc.n_pt, o)
    clean_per_track = np.bincount(sc.pt_idx[~injected], minlength=sc.n_pt)
    far = injected & (np.linalg.norm(sc.uv.astype(np.float64) - clean.uv, axis=1) > 3 * 4.0) & (clean_per_track[sc.pt_idx] >= 3)
    assert injected.sum() == 240 and far.sum() > 150
    for r in (ref, got):
        kept = r.status == R.KEPT
        flagged_clean = np.count_nonzero(~r.obs_inlier & ~injected) / np.count_nonzero(~injected)
        not_kept = np.count_nonzero(~kept) / sc.n_pt
        d_robust = float(np.median(np.linalg.norm(r.xyz[kept] - sc.pts_gt[kept], axis=1)))
        d_base = float(np.median(np.linalg.norm(base[kept] - sc.pts_gt[kept], axis=1)))
        print(f"clean observations flagged {flagged_clean:.4%}, points not kept {not_kept:.4%}, median distance {d_robust:.5f} against {d_base:.5f}")
        assert not r.obs_inlier[far].any()
        assert flagged_clean <= 0.02 and not_kept <= 0.02
        assert d_robust < d_base
