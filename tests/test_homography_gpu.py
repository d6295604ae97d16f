"""Homography RANSAC on the GPU (esfm.h "Homography RANSAC") against the Python restatement of tests/homography_ref.py, bit for bit: the
4-point solve, the whole RANSAC at the sizes where a lane stride, a wave edge or the refit's tree can go wrong, the batched form
against the per-pair calls, the planar / panoramic statistic on synthetic pairs and what the re-fit gains."""
import numpy as np
import pytest

import homography_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    from easysfm_amd import motion
    return motion


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_models_gpu_equals_host_build(M, gpu_ctx):
    """esfm_homography_models == esfm_homography_models_host on the 4 096 sampled 4-subsets and the degenerate samples, bit for bit."""
    q1, q2 = R.solver_samples()
    Hg, hg = M.homography_models(q1, q2, gpu_ctx)
    Hh, hh = M.homography_models(q1, q2, host=True)
    assert np.array_equal(hg, hh) and hg[:4096].mean() > 0.99
    assert np.array_equal(_bits(Hg), _bits(Hh))


def _case(name):
    if name == "all_inliers":
        return R.ransac_case(200, 0.0) + (1.0,)
    if name == "outliers_80":
        return R.ransac_case(100, 0.8) + (1.0,)
    if name == "outliers_50":
        return R.ransac_case(120, 0.5) + (1.0,)
    if name == "no_model":
        # threshold 0: a point is an inlier only where the float error is exactly 0, which not even a sample's own four points reach
        rng = np.random.default_rng(77)
        return (rng.uniform(5, 763, (12, 2)).astype(np.float32), rng.uniform(5, 507, (12, 2)).astype(np.float32), 0.0)
    n = int(name)
    return R.ransac_case(n, 0.0 if n <= 5 else 0.2) + (1.0,)


@pytest.mark.parametrize("name", ["4", "5", "63", "64", "65", "255", "256", "257", "513", "all_inliers", "outliers_50", "outliers_80", "no_model"])
def test_find_homography_equals_the_restatement(M, gpu_ctx, name):
    """H, mask and iteration count of esfm_find_homography == route (a): one possible sample (n = 4), n = 5, the wave edge (63, 64, 65),
    the refit's lane stride and tree and the scoring stride (255, 256, 257, 513), 100 % inliers (the count collapses inside the first
    chunk), 50 % outliers (the count ends inside a later chunk), 80 % outliers (all 2000 iterations: the replay does not depend on the
    chunk) and a set without a model (ESFM_ERR_NUMERIC)."""
    from easysfm_amd._lib import ESFM_ERR_NUMERIC, ESFM_ERR_UNSUPPORTED, EsfmError
    a, b, thr = _case(name)
    Hr, mr, itr, _ = R.find_homography(a, b, thr)
    if name == "no_model":
        assert Hr is None
        with pytest.raises(EsfmError) as e:
            M.find_homography(a, b, thr, 0.995, gpu_ctx)
        assert e.value.status == ESFM_ERR_NUMERIC
        return
    assert Hr is not None
    H, mask, it = M.find_homography(a, b, thr, 0.995, gpu_ctx)
    assert it == itr
    assert np.array_equal(mask, mr)
    assert np.array_equal(_bits(H), _bits(Hr))
    if name == "all_inliers":
        assert it < 64
    if name == "outliers_50":
        assert it > 64 and it % 64 != 0
    if name == "outliers_80":
        assert it == 2000
    if name == "4":
        assert it == 0 and mask.all()


def test_too_few_points_and_degenerate_sets(M, gpu_ctx):
    """n = 3 is ESFM_ERR_UNSUPPORTED; a set whose every 4-subset holds a collinear triple gives up in the sampler: ESFM_ERR_NUMERIC."""
    from easysfm_amd._lib import ESFM_ERR_NUMERIC, ESFM_ERR_UNSUPPORTED, EsfmError
    a, b = R.ransac_case(3, 0.0)
    with pytest.raises(EsfmError) as e:
        M.find_homography(a, b, 1.0, 0.995, gpu_ctx)
    assert e.value.status == ESFM_ERR_UNSUPPORTED
    x = np.arange(6, dtype=np.float32) * 10
    line = np.stack([x, 2 * x + 1], 1).astype(np.float32)
    with pytest.raises(EsfmError) as e:
        M.find_homography(line, line + np.float32(2.0), 1.0, 0.995, gpu_ctx)
    assert e.value.status == ESFM_ERR_NUMERIC


def test_pairs_equal_the_per_pair_calls(M, gpu_ctx):
    """esfm_find_homography_pairs on 7 pairs of ragged sizes (4, 0, 300, 21, 3, 257, 64), an empty and a too-small pair among them: H, mask
    and iterations equal the per-pair calls bit for bit; status is 0 exactly for the pairs without a model; n_inliers counts the
    correspondences within the threshold of the returned H."""
    sizes = [4, 0, 300, 21, 3, 257, 64]
    sets = [R.ransac_case(n, 0.0 if n <= 5 else 0.3, seed=k) for k, n in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    a = np.concatenate([s[0] for s in sets]); b = np.concatenate([s[1] for s in sets])
    H, mask, status, iters, n_inl = M.find_homography_pairs(off, a, b, 1.0, 0.995, gpu_ctx)
    assert status.tolist() == [True, False, True, True, False, True, True]
    for p, n in enumerate(sizes):
        m = mask[off[p]:off[p + 1]]
        if n < 4:
            assert not H[p].any() and not m.any() and iters[p] == 0 and n_inl[p] == 0
            continue
        H1, m1, it1 = M.find_homography(sets[p][0], sets[p][1], 1.0, 0.995, gpu_ctx)
        assert np.array_equal(_bits(H[p]), _bits(H1)) and np.array_equal(m, m1) and iters[p] == it1, p
        assert n_inl[p] == int(np.count_nonzero(R.inlier_mask(H1.reshape(9), sets[p][0], sets[p][1], 1.0))), p


@pytest.fixture(scope="module")
def scene():
    return R.scene_pairs()


def test_classification_on_synthetic_pairs(M, gpu_ctx, scene):
    """Pairs from synth.sfm_scene()'s cameras and K, 0.2 px noise, threshold 1: h_inlier_ratio = homography inliers / essential-matrix
    RANSAC inliers is at most 0.2 on the scene as it is and at least 0.8 with the points on the plane z = 0.3 x + 0.1 y and for camera 0
    against itself rotated by 0.1 rad."""
    pairs, K = scene
    kinds, sets = [], []
    for kind, lst in pairs.items():
        for a, b, _, _, _ in lst:
            kinds.append(kind); sets.append((a, b))
    off = np.concatenate([[0], np.cumsum([len(s[0]) for s in sets])]).astype(np.int32)
    a = np.concatenate([s[0] for s in sets]); b = np.concatenate([s[1] for s in sets])
    K4 = np.tile(np.array([K[0, 0], K[0, 2], K[1, 1], K[1, 2]], np.float32), (len(sets), 1))
    _, e_mask, e_status, _ = M.find_essential_pairs(off, a, b, K4, 0.99, 1.0, gpu_ctx)
    _, _, h_status, _, h_inl = M.find_homography_pairs(off, a, b, 1.0, 0.995, gpu_ctx)
    assert e_status.all()
    for p, kind in enumerate(kinds):
        e_inl = int(np.count_nonzero(e_mask[off[p]:off[p + 1]]))
        ratio = float(h_inl[p]) / e_inl
        print(f"{kind}: {off[p + 1] - off[p]} correspondences, E inliers {e_inl}, H inliers {int(h_inl[p])}, ratio {ratio:.3f}")
        assert e_inl > 0.5 * (off[p + 1] - off[p])
        if kind == "general":
            assert ratio <= 0.2
        else:
            assert h_status[p] and ratio >= 0.8


def test_refit_is_closer_to_the_plane_homography(M, gpu_ctx, scene):
    """On the planar pair the re-fitted H transfers the noise-free points with a smaller mean error than the minimal-sample winner it
    started from, and both are close to the ground-truth plane homography."""
    a, b, exact_a, exact_b, H_true = scene[0]["planar"][0]
    H, mask, it = M.find_homography(a, b, 1.0, 0.995, gpu_ctx)
    Hr, mr, itr, H_winner = R.find_homography(a, b, 1.0)
    assert np.array_equal(_bits(H), _bits(Hr)) and it == itr                  # the same run: H_winner is the model this re-fit started from

    def mean_transfer(Hm):
        h = np.c_[exact_a, np.ones(len(exact_a))] @ Hm.T
        return float(np.mean(np.linalg.norm(h[:, :2] / h[:, 2:] - exact_b, axis=1)))
    e_true, e_refit, e_winner = mean_transfer(H_true), mean_transfer(H), mean_transfer(H_winner)
    print(f"mean transfer error of noise-free points: truth {e_true:.2e}, re-fit {e_refit:.3f} px, minimal-sample winner {e_winner:.3f} px")
    assert e_true < 1e-6
    assert e_refit < e_winner
    assert e_refit < 0.2                                                       # 0.2 px noise averaged over some hundred inliers
