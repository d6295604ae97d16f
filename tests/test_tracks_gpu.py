"""Track triangulation on the GPU (esfm.h "Track triangulation"): the kernels against the host build of the same header and
against the Python restatement (tests/track_ref.py), bit for bit (f64 compared as uint64), on the CPU tests' edge list, at the
edges of the 256-wide grouping kernels and on a 3 000-point scene in shuffled order."""
import numpy as np
import pytest

import track_ref as R
from track_ref import assert_same, bits, degenerate_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import easysfm_amd
    return easysfm_amd


def three_ways(E, ctx, case, o=None, xyz_in=None, ref=True):
    """kernels == host build (== restatement unless ref is False); returns the kernels' result"""
    o = o or R.Options()
    opt = E.TrackOptions(**o.kw)
    dev = E.track_triangulate(*case[:5], case[5], xyz_in, opt, ctx)
    assert_same(dev, E.track_triangulate(*case[:5], case[5], xyz_in, opt, host=True), "host")
    if ref:
        assert_same(dev, R.run(*case[:6], o, xyz_in=xyz_in), "restatement")
    return dev


def test_track_length_edges(E, gpu_ctx):
    """lengths 0, 1, 2, 3, 11, 12, 63, 64, 65, 129 and 300 (the global-memory path above the staging cap), interleaved"""
    case = R.ring_case(R.EDGE_LENGTHS)
    dev = three_ways(E, gpu_ctx, case)
    n = np.array(R.EDGE_LENGTHS)
    assert np.all(dev.status[n < 2] == R.TOO_FEW) and np.all(dev.status[n >= 2] == R.KEPT)
    # ... and judged as given points
    ev = E.track_evaluate(*case[:5], dev.xyz, E.TrackOptions(), gpu_ctx)
    assert_same(ev, E.track_evaluate(*case[:5], dev.xyz, E.TrackOptions(), host=True), "host")
    assert_same(ev, R.run(*case[:6], R.Options(), xyz_in=dev.xyz, evaluate=True), "restatement")
    kept = dev.status == R.KEPT
    assert np.array_equal(ev.n_inliers[kept], dev.n_inliers[kept]) and np.array_equal(bits(ev.mse[kept]), bits(dev.mse[kept]))


@pytest.mark.parametrize("kw", [dict(min_views=3), dict(refine_iterations=0), dict(max_hypotheses=1), dict(max_reproj_error_px=1.0, min_angle_deg=8.0)])
def test_options_edges(E, gpu_ctx, kw):
    three_ways(E, gpu_ctx, R.ring_case([0, 2, 3, 7, 12, 40], seed=11), R.Options(**kw))


def test_degenerate_geometry_layouts_and_permutation(E, gpu_ctx):
    case = degenerate_case()
    dev = three_ways(E, gpu_ctx, case)
    assert list(dev.status[[0, 1, 4, 5, 6]]) == [R.NO_HYPOTHESIS, R.NO_HYPOTHESIS, R.NON_FINITE, R.NON_FINITE, R.KEPT]
    xyz = case[6].copy(); xyz[6, 0] = np.nan
    assert_same(E.track_evaluate(*case[:5], xyz, E.TrackOptions(), gpu_ctx), R.run(*case[:6], R.Options(), xyz_in=xyz, evaluate=True))
    for lengths in ([3], [0], [0, 0, 4, 0]):                       # n_pt = 1; n_obs = 0; unobserved first and last points
        three_ways(E, gpu_ctx, R.ring_case(lengths, seed=3))
    xin = np.arange(9, dtype=np.float64).reshape(3, 3) + 0.5
    three_ways(E, gpu_ctx, R.ring_case([0, 1, 5], seed=5), xyz_in=xin)
    got = E.track_triangulate(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), case[3], case[4], 0, ctx=gpu_ctx)
    assert len(got.status) == 0
    # grouped, reversed-grouped and interleaved inputs give the same bits
    case = R.ring_case([5, 0, 9, 2, 70], seed=9)
    ref = E.track_triangulate(*case[:5], case[5], ctx=gpu_ctx)
    for perm in (np.argsort(case[1], kind="stable"), np.argsort(-case[1], kind="stable")):
        got = E.track_triangulate(case[0][perm], case[1][perm], case[2][perm], case[3], case[4], case[5], ctx=gpu_ctx)
        assert np.array_equal(bits(got.xyz), bits(ref.xyz)) and np.array_equal(bits(got.min_cos), bits(ref.min_cos))
        assert np.array_equal(got.obs_inlier, ref.obs_inlier[perm])


@pytest.mark.parametrize("lengths", [[2], [3] * 255, [3] * 256, [3] * 257, [2] * 127 + [1], [2] * 128, [2] * 127 + [3], [0] * 300 + [4]],
                         ids=["1pt", "255pt", "256pt", "257pt", "255obs", "256obs", "257obs", "300empty"])
def test_block_edges(E, gpu_ctx, lengths):
    """the grouping kernels work in blocks of 256 observations (keys, run heads) and 256 points (defaults); one workgroup per track"""
    three_ways(E, gpu_ctx, R.ring_case(lengths, seed=13, outliers=False))


def test_shuffled_scene(E, gpu_ctx):
    """3 000 points, six observations each, 10 % outliers, in a random order of the observation list: kernels == host build on all of
    it, == restatement on every tenth track (a track's outputs depend on its own observations alone)"""
    sc, Rt, injected, _ = R.scene(8, 3000, 6, seed=4100)
    perm = np.random.default_rng(2).permutation(sc.n_obs)
    cam, pt, uv = sc.cam_idx[perm], sc.pt_idx[perm], sc.uv[perm]
    dev = three_ways(E, gpu_ctx, (cam, pt, uv, sc.K4, Rt, sc.n_pt), ref=False)
    sel = pt % 10 == 0
    sub = R.run(cam[sel], pt[sel] // 10, uv[sel], sc.K4, Rt, sc.n_pt // 10, R.Options())
    assert np.array_equal(bits(dev.xyz[::10]), bits(sub.xyz)) and np.array_equal(dev.status[::10], sub.status)
    assert np.array_equal(bits(dev.min_cos[::10]), bits(sub.min_cos)) and np.array_equal(bits(dev.mse[::10]), bits(sub.mse))
    assert np.array_equal(dev.obs_inlier[sel], sub.obs_inlier) and np.array_equal(dev.obs_err2[sel].view(np.uint32), sub.obs_err2.view(np.uint32))
    assert np.count_nonzero(dev.status == R.KEPT) >= 0.98 * sc.n_pt
    ev = E.track_evaluate(cam, pt, uv, sc.K4, Rt, dev.xyz, E.TrackOptions(), gpu_ctx)
    assert_same(ev, E.track_evaluate(cam, pt, uv, sc.K4, Rt, dev.xyz, E.TrackOptions(), host=True))
    kept = dev.status == R.KEPT
    assert np.array_equal(ev.obs_inlier[kept[pt]], dev.obs_inlier[kept[pt]]) and np.array_equal(ev.status[kept], dev.status[kept])
