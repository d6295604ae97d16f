"""Parity of the HIP 3-D/2-D registration (reference cv::solvePnPRansac with SOLVEPNP_EPNP at
cpp_code/src/estimate_motion.cpp:161-162) through the C ABI against the CPU oracle.

Both sides replay the same cv::RNG sample stream and bookkeeping: iteration counts and inlier masks must agree exactly.  The pose:
the EPnP re-fit on the inliers runs on the HOST in the oracle's summation order for inlier sets up to 8 192 (round 6; 1 024 before) --
every frame this pipeline can meet -- and is then BIT-IDENTICAL to the CPU restatement's, rvec and tvec included; beyond that the
four one-workgroup device reductions (pnp_moment_sums / pnp_mtm_sums / pnp_rt_sums / pnp_reproj_sums_kernel) take over and agree to the
re-fit's own sensitivity to the order of its sums.  tests/stress_pnp.py has no set that large (4 000 points at most): the device
re-fit is tested HERE, by two sets beyond 8 192 inliers and, with ESFM_PNP_HOST_REFIT=0 (the threshold, read on each call), by small
ones at the sizes where a 256-thread strided reduction can go wrong."""

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth

pytestmark = pytest.mark.gpu
K4 = np.array(synth.FOUNTAIN_K4, np.float32)


def _scene(rng, n, frac, noise=0.5):
    R = synth.aa_to_R(rng.normal(0, 0.3, 3)); t = np.array([0.3, -0.2, 6.0]) + rng.normal(0, 0.2, 3)
    X = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    Xc = X.astype(np.float64) @ R.T + t
    pix = np.stack([Xc[:, 0] / Xc[:, 2] * K4[0] + K4[1], Xc[:, 1] / Xc[:, 2] * K4[2] + K4[3]], 1) + rng.normal(0, noise, (n, 2))
    bad = rng.choice(n, int(frac * n), replace=False)
    pix[bad] += rng.uniform(-80, 80, (len(bad), 2))
    return X, pix.astype(np.float32), R, t, bad


@pytest.mark.parametrize("n,frac,iters,seed", [(600, 0.33, 50000, 0), (60, 0.5, 50000, 1), (3000, 0.2, 50000, 2), (25, 0.2, 100, 3), (6, 0.0, 100, 4)])
def test_solve_pnp_ransac_matches_oracle(gpu_ctx, oracle_lib, n, frac, iters, seed):
    rng = np.random.default_rng(seed)
    X, pix, R, t, bad = _scene(rng, n, frac)
    ok, Rr, tr, rvr, mr, itr = oracle_lib.solve_pnp_ransac(X, pix, K4, iters, 2.5, 0.99)
    assert ok
    rv, tv, Rg, mg, itg = E.solve_pnp_ransac(X, pix, K4, iters, 2.5, 0.99, gpu_ctx)
    assert itg == itr and np.array_equal(mg, mr)
    assert np.array_equal(Rg, Rr) and np.array_equal(tv, tr) and np.array_equal(rv, rvr)
    if n >= 60:
        assert np.allclose(Rg, R, atol=5e-3) and np.allclose(tv, t, atol=0.05) and mg[bad].sum() <= 0.05 * len(bad) + 2
        assert abs(np.linalg.det(Rg) - 1) < 1e-9


@pytest.mark.parametrize("n,frac,seed", [(800, 0.6, 21), (400, 0.65, 22), (1500, 0.55, 23)])
def test_solve_pnp_ransac_many_iterations_through_the_deferred_hypotheses(gpu_ctx, oracle_lib, n, frac, seed):
    """Hundreds of RANSAC iterations (55 - 65 % gross outliers): about one hypothesis in a hundred stalls in the 12 x 12 Jacobi
    diagonalisation; the first pass gives up on those after twelve sweeps and the replay has them solved in full when it reaches them
    (pnp_api.cpp) -- with this many iterations it does.  Iteration counts and masks exact, as everywhere."""
    rng = np.random.default_rng(seed)
    X, pix, R, t, bad = _scene(rng, n, frac)
    ok, Rr, tr, rvr, mr, itr = oracle_lib.solve_pnp_ransac(X, pix, K4, 50000, 2.5, 0.99)
    assert ok and itr > 150
    rv, tv, Rg, mg, itg = E.solve_pnp_ransac(X, pix, K4, 50000, 2.5, 0.99, gpu_ctx)
    assert itg == itr and np.array_equal(mg, mr)
    assert np.array_equal(Rg, Rr) and np.array_equal(tv, tr) and np.array_equal(rv, rvr)


def test_pnp_exactly_five_and_too_few(gpu_ctx, oracle_lib):
    rng = np.random.default_rng(9)
    X, pix, R, t, _ = _scene(rng, 5, 0.0, noise=0.0)
    rv, tv, Rg, mg, it = E.solve_pnp_ransac(X, pix, K4, 100, 2.5, 0.99, gpu_ctx)
    ok, Rr, tr, rvr, mr, itr = oracle_lib.solve_pnp_ransac(X, pix, K4, 100, 2.5, 0.99)
    assert ok and np.all(mg) and np.allclose(Rg, Rr, atol=1e-6) and np.allclose(Rg, R, atol=1e-4)
    with pytest.raises(E.EsfmError):
        E.solve_pnp_ransac(X[:4], pix[:4], K4, 100, 2.5, 0.99, gpu_ctx)


def test_mirror_estimate2D3D(gpu_ctx):
    """estimate2D3D_P3P_RANSAC (estimate_motion.cpp:99-232): id join, pose write-back, the reference's inlier bookkeeping."""
    rng = np.random.default_rng(13)
    X, pix, R, t, bad = _scene(rng, 300, 0.2)
    K = np.array([[K4[0], 0, K4[1]], [0, K4[2], K4[3]], [0, 0, 1]], np.float32)
    fr = E.Frame(frame_id=5, keypoints=np.concatenate([pix, rng.uniform(0, 700, (50, 2)).astype(np.float32)])); fr.K_cam = K
    fr.unique_pixel_ids = np.concatenate([np.arange(100, 400), np.arange(9000, 9050)])
    far = np.array([[500.0, 0, 0]], np.float32)                      # beyond the +-300 gate
    cloud = E.SparsePointCloud(xyz=np.concatenate([X, far]), rgb=np.zeros((301, 3), np.uint8),
                               unique_point_ids=np.concatenate([np.arange(100, 400), [9001]]), is_inlier=np.ones(301, np.int32))
    me = E.MotionEstimator(gpu_ctx)
    assert me.estimate2D3D_P3P_RANSAC(fr, cloud)
    assert fr.pose_cam.dtype == np.float32 and np.allclose(fr.pose_cam[:3, :3], R, atol=5e-3) and np.allclose(fr.pose_cam[:3, 3], t, atol=0.05)
    # every correspondence except the first is flagged is_inlier = 0; the gated far point is untouched
    assert cloud.is_inlier[0] == 1 and not cloud.is_inlier[1:300].any() and cloud.is_inlier[300] == 1


# ---- the device EPnP re-fit (pnp_api.cpp, past the host re-fit threshold) -------------------------------------------------------------
def _refit_scene(seed, m, n_out, noise, out_first=False, coplanar=False, out0=False):
    """m correspondences with `noise` px of Gaussian noise + n_out gross outliers (40 .. 120 px off), at random places or in front"""
    rng = np.random.default_rng(seed)
    n = m + n_out
    R = synth.aa_to_R(rng.normal(0, 0.3, 3)); t = np.array([0.3, -0.2, 6.0]) + rng.normal(0, 0.2, 3)
    X = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    if coplanar:
        X[:, 2] = X[0, 2]                                      # exactly, as tests/stress_pnp.py builds its coplanar sets
    Xc = X.astype(np.float64) @ R.T + t
    pix = np.stack([Xc[:, 0] / Xc[:, 2] * K4[0] + K4[1], Xc[:, 1] / Xc[:, 2] * K4[2] + K4[3]], 1) + rng.normal(0, noise, (n, 2))
    bad = np.arange(n_out) if out_first else rng.choice(n, n_out, replace=False)
    if out0 and 0 not in bad:
        bad[0] = 0
    pix[bad] += rng.choice([-1.0, 1.0], (len(bad), 2)) * rng.uniform(40, 120, (len(bad), 2))
    return X, pix.astype(np.float32)


def _pose_diff(Ra, ta, Rb, tb):
    return max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max())


def _refit_spread(oracle_lib, X, pix, mask):
    """How far the re-fit itself depends on the order of its sums: oracle.epnp on the same inliers in eight seeded permutations; the
    largest pose difference between any two of them."""
    Xi = X[mask].astype(np.float64); pi = pix[mask].astype(np.float64)
    rng = np.random.default_rng(77)
    orders = [rng.permutation(len(Xi)) for _ in range(8)]
    runs = [oracle_lib.epnp(Xi[p], pi[p], K4)[:2] for p in orders]
    return max(_pose_diff(*a, *b) for a in runs for b in runs)


def _check_device_refit(gpu_ctx, oracle_lib, X, pix, inliers=None, first_inlier=None):
    ok, Rr, tr, rvr, mr, itr = oracle_lib.solve_pnp_ransac(X, pix, K4, 50000, 2.5, 0.99)
    assert ok
    if inliers is not None:
        assert int(mr.sum()) == inliers                        # (the case is what its name says)
    if first_inlier is not None:
        assert int(np.argmax(mr)) == first_inlier
    rv, tv, Rg, mg, itg = E.solve_pnp_ransac(X, pix, K4, 50000, 2.5, 0.99, gpu_ctx)
    assert itg == itr and np.array_equal(mg, mr)
    spread = _refit_spread(oracle_lib, X, pix, mr)
    diff = _pose_diff(Rg, tv, Rr, tr)
    print(f"n {len(X)}, inliers {int(mr.sum())}: device re-fit off by {diff:.3g}, spread of the re-fit over 8 orders {spread:.3g}")
    assert diff <= max(16.0 * spread, 1e-12)                   # 16 x: a ninth order outside the range of eight; floor: a few ulps of t ~ 6
    assert diff < 1e-7                                         # what DESIGN.md section 6.3 documents, in any case
    assert abs(np.linalg.det(Rg) - 1) < 1e-9
    return int(mr.sum())


# measured on the MI355X (device re-fit off by / spread over 8 orders): see DESIGN.md section 6.3
@pytest.mark.parametrize("m,n_out,seed,out0", [(10800, 1200, 31, False),       # 12 000 points, 10 % outliers: 5 iterations
                                                (9000, 1003, 32, True)])        # n = 10 003 = 39 x 256 + 19; point 0 an outlier: the `first` search
def test_device_refit_beyond_the_host_threshold(gpu_ctx, oracle_lib, monkeypatch, m, n_out, seed, out0):
    monkeypatch.delenv("ESFM_PNP_HOST_REFIT", raising=False)
    X, pix = _refit_scene(seed, m, n_out, 0.5, out0=out0)
    assert _check_device_refit(gpu_ctx, oracle_lib, X, pix, first_inlier=1 if out0 else 0) > 8192


@pytest.mark.parametrize("m", [5, 6, 63, 64, 65, 255, 256, 257, 1000])
def test_device_refit_small_sets(gpu_ctx, oracle_lib, monkeypatch, m):
    """ESFM_PNP_HOST_REFIT=0: every inlier set goes through the four reduction kernels -- one wave partly filled, one wave, one wave and
    a lane, one pass of the 256 threads less one, exactly one, one and a lane, four passes"""
    monkeypatch.setenv("ESFM_PNP_HOST_REFIT", "0")
    X, pix = _refit_scene(40 + m, m, 0 if m == 5 else max(2, m // 4), 0.05)
    _check_device_refit(gpu_ctx, oracle_lib, X, pix, inliers=m)


def test_device_refit_inliers_in_the_last_partial_block(gpu_ctx, oracle_lib, monkeypatch):
    """511 points: the first pass of the 256 threads meets outliers only, the 255 inliers are the second, partial one"""
    monkeypatch.setenv("ESFM_PNP_HOST_REFIT", "0")
    X, pix = _refit_scene(51, 255, 256, 0.05, out_first=True)
    _check_device_refit(gpu_ctx, oracle_lib, X, pix, inliers=255, first_inlier=256)


def test_device_refit_coplanar(gpu_ctx, oracle_lib, monkeypatch):
    """An EXACTLY coplanar set: the scatter matrix has a zero eigenvalue, the fourth control point falls on the centroid and the
    pseudo-inverse of control_points_from_scatter drops its axis -- a well-posed fit (spread of the oracle's re-fit over 8 orders:
    2.4e-14).  A plane that holds only to float rounding (z = a x + b y + c stored as floats) is another matter: the axis survives at
    1e-8 of the others, EPnP takes the rounding for structure, and the ORACLE's own poses over 8 orders are 1.4e-4 apart -- an
    ill-posed fit that says nothing about the sums, so it is not a case here."""
    monkeypatch.setenv("ESFM_PNP_HOST_REFIT", "0")
    X, pix = _refit_scene(52, 400, 100, 0.05, coplanar=True)
    _check_device_refit(gpu_ctx, oracle_lib, X, pix, inliers=400)


def test_host_refit_threshold_default_still_bit_identical(gpu_ctx, oracle_lib, monkeypatch):
    """variable unset: 8 192 inliers or fewer are re-fitted on the host, bit for bit the oracle's pose -- the same sets that the
    variable sends through the kernels above"""
    monkeypatch.delenv("ESFM_PNP_HOST_REFIT", raising=False)
    for m in (257, 1000):
        X, pix = _refit_scene(40 + m, m, m // 4, 0.05)
        ok, Rr, tr, rvr, mr, itr = oracle_lib.solve_pnp_ransac(X, pix, K4, 50000, 2.5, 0.99)
        rv, tv, Rg, mg, itg = E.solve_pnp_ransac(X, pix, K4, 50000, 2.5, 0.99, gpu_ctx)
        assert ok and itg == itr and np.array_equal(mg, mr)
        assert np.array_equal(Rg, Rr) and np.array_equal(tv, tr) and np.array_equal(rv, rvr)
