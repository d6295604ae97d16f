"""The fundamental-matrix RANSAC and the focal-length cost on the GPU (esfm.h "Fundamental-matrix RANSAC") against the host build and
the Python restatement (tests/fundamental_ref.py), bit for bit."""
import numpy as np
import pytest

import easysfm_amd as E

import fundamental_cases as Cs
import fundamental_ref as R

pytestmark = pytest.mark.gpu

THRESHOLD, CONFIDENCE = 1.0, 0.99


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_against_restatement(ctx, a, b, threshold=THRESHOLD):
    Fr, mr, itr, nr = R.find_fundamental(a, b, threshold, CONFIDENCE)
    off = np.array([0, len(a)], np.int32)
    F, mask, status, it, ninl = E.find_fundamental_pairs(off, a, b, threshold, CONFIDENCE, ctx)
    if Fr is None:
        assert not status[0] and not F.any() and not mask.any() and ninl[0] == 0 and it[0] == itr
        with pytest.raises(E.EsfmError) as ei:
            E.find_fundamental(a, b, threshold, CONFIDENCE, ctx)
        assert ei.value.status == -6                                   # ESFM_ERR_NUMERIC
        return None
    assert status[0]
    assert np.array_equal(_bits(F[0]), _bits(Fr)), (F[0], Fr)
    assert np.array_equal(mask, mr) and it[0] == itr and ninl[0] == nr
    F1, m1, it1 = E.find_fundamental(a, b, threshold, CONFIDENCE, ctx)
    assert np.array_equal(_bits(F1), _bits(Fr)) and np.array_equal(m1, mr) and it1 == itr
    return F[0], mask, itr, nr


def test_models_equal_the_host_build(gpu_ctx):
    """esfm_fundamental_models == esfm_fundamental_models_host on the 4096 samples: every model and the model count"""
    q1, q2 = Cs.solver_samples()
    Fh, nh = E.fundamental_models(q1, q2, host=True)
    Fg, ng = E.fundamental_models(q1, q2, gpu_ctx)
    assert np.array_equal(ng, nh) and np.array_equal(_bits(Fg), _bits(Fh))
    assert np.count_nonzero(ng == 1) >= 256 and np.count_nonzero(ng == 3) >= 256


@pytest.mark.parametrize("n", [7, 8, 9, 63, 64, 65, 255, 256, 257, 513])
def test_find_fundamental_equals_the_restatement(gpu_ctx, n):
    """F, mask, iterations and n_inliers at the sizes where the kernels change their path: the exact case, fewer than 8 inliers possible,
    one wave, 256 lanes and beyond.  20 % outliers."""
    a, b = Cs.ransac_case(n, 0.2)
    got = _check_against_restatement(gpu_ctx, a, b)
    assert got is not None
    F, mask, it, ninl = got
    if n == 7:
        assert mask.all() and it == 0
    else:
        assert it >= 1
    if n >= 63:
        assert ninl >= 0.4 * n                          # (80 % are true correspondences; half of them is a sanity floor, not a bar)


@pytest.mark.parametrize("name,frac", [("all_inliers", 0.0), ("outliers_50", 0.5), ("outliers_80", 0.8)])
def test_find_fundamental_outlier_rates(gpu_ctx, name, frac):
    a, b = Cs.ransac_case(300, frac, seed=1)
    got = _check_against_restatement(gpu_ctx, a, b)
    assert got is not None
    F, mask, it, ninl = got
    print(f"\n[fundamental] {name}: {it} iterations, {int(mask.sum())} in the mask, {ninl} under the returned F")
    if frac <= 0.5:                                     # (at 80 % outliers a clean seven is drawn once in 78 000 samples: the winner is chance)
        assert ninl >= 0.5 * (1.0 - frac) * 300
    else:
        assert it == 1000


def test_no_model_and_documented_statuses(gpu_ctx):
    """a set without a model (threshold 0), n < 7 and seven (or forty) identical points"""
    a, b = Cs.no_model_case()
    _check_against_restatement(gpu_ctx, a, b, threshold=0.0)
    with pytest.raises(E.EsfmError) as ei:
        E.find_fundamental(a[:6], b[:6], THRESHOLD, CONFIDENCE, gpu_ctx)
    assert ei.value.status == -5                                       # ESFM_ERR_UNSUPPORTED
    for n in (7, 40):
        same = np.tile(np.array([[100.5, 200.25]], np.float32), (n, 1))
        assert R.find_fundamental(same, same, THRESHOLD, CONFIDENCE)[0] is None
        with pytest.raises(E.EsfmError) as ei:
            E.find_fundamental(same, same, THRESHOLD, CONFIDENCE, gpu_ctx)
        assert ei.value.status == -6                                   # ESFM_ERR_NUMERIC


def test_pairs_batch_equals_the_per_pair_calls(gpu_ctx):
    """pairs of 0, 6, 7, 8 and 300 points in one batch (and a second 300 with other outliers): each pair's F, mask, iterations and
    n_inliers are those of its own call; pairs with fewer than 7 points have status 0 and zeros, without an error"""
    sizes = [0, 6, 7, 8, 300, 300]
    sets = [Cs.ransac_case(max(n, 1), 0.2, seed=10 + k) for k, n in enumerate(sizes)]
    sets = [(a[:n], b[:n]) for (a, b), n in zip(sets, sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    p1 = np.concatenate([s[0] for s in sets]); p2 = np.concatenate([s[1] for s in sets])
    F, mask, status, it, ninl = E.find_fundamental_pairs(off, p1, p2, THRESHOLD, CONFIDENCE, gpu_ctx)
    assert list(status) == [False, False, True, True, True, True]
    for k, n in enumerate(sizes):
        m = mask[off[k]:off[k + 1]]
        if n < 7:
            assert not F[k].any() and not m.any() and it[k] == 0 and ninl[k] == 0
            continue
        F1, m1, s1, it1, n1 = E.find_fundamental_pairs([0, n], sets[k][0], sets[k][1], THRESHOLD, CONFIDENCE, gpu_ctx)
        assert s1[0] and np.array_equal(_bits(F[k]), _bits(F1[0])) and np.array_equal(m, m1) and it[k] == it1[0] and ninl[k] == n1[0]
    Fr, mr, itr, nr = R.find_fundamental(sets[4][0], sets[4][1], THRESHOLD, CONFIDENCE)
    assert np.array_equal(_bits(F[4]), _bits(Fr)) and it[4] == itr and ninl[4] == nr
    # no pairs, and pairs that are all empty
    assert len(E.find_fundamental_pairs([0], np.zeros((0, 2)), np.zeros((0, 2)), THRESHOLD, CONFIDENCE, gpu_ctx)[0]) == 0
    assert not E.find_fundamental_pairs([0, 0, 0], np.zeros((0, 2)), np.zeros((0, 2)), THRESHOLD, CONFIDENCE, gpu_ctx)[2].any()


def test_focal_cost_equals_the_host_twin(gpu_ctx):
    """esfm_focal_cost == esfm_focal_cost_host on a whole estimate (both sweeps), on one pair and on more pairs than lanes"""
    Fs, w = Cs.scene_fundamentals(Cs.freehand_scene(0)[0])
    g = E.focal_from_fundamentals(Fs, w, Cs.WIDTH, Cs.HEIGHT, None, gpu_ctx)
    h = E.focal_from_fundamentals(Fs, w, Cs.WIDTH, Cs.HEIGHT, host=True)
    assert g["f"] == h["f"] and g["depth"] == h["depth"] and g["confident"]
    for key in ("coarse", "fine"):
        assert np.array_equal(_bits(g[key][1]), _bits(h[key][1]))
    cand = E.focal_candidates(230.4, 2304.0)
    assert np.array_equal(_bits(E.focal_cost(Fs[:1], w[:1], 384.0, 256.0, cand, gpu_ctx)), _bits(E.focal_cost(Fs[:1], w[:1], 384.0, 256.0, cand, host=True)))
    many = np.tile(Fs, (10, 1)); wm = np.tile(w, 10) + np.arange(10 * len(w))
    assert len(many) > 256
    assert np.array_equal(_bits(E.focal_cost(many, wm, 380.0, 250.0, cand[::8], gpu_ctx)), _bits(E.focal_cost(many, wm, 380.0, 250.0, cand[::8], host=True)))


def test_two_runs_agree_in_every_bit(gpu_ctx):
    a, b = Cs.ransac_case(513, 0.5, seed=4)
    off = np.array([0, 200, 513], np.int32)
    r1 = E.find_fundamental_pairs(off, a, b, THRESHOLD, CONFIDENCE, gpu_ctx)
    r2 = E.find_fundamental_pairs(off, a, b, THRESHOLD, CONFIDENCE, gpu_ctx)
    assert np.array_equal(_bits(r1[0]), _bits(r2[0])) and all(np.array_equal(x, y) for x, y in zip(r1[1:], r2[1:]))


def test_motion_estimator_member(gpu_ctx):
    """MotionEstimator.estimate2D2D_F7P_RANSAC reads no K_cam and returns the batch call's F and count"""
    frames, K, poses, pts = Cs.freehand_scene(0)
    f1 = E.Frame(frame_id=0, keypoints=frames[3]["keypoints"], descriptors=frames[3]["descriptors"])
    f2 = E.Frame(frame_id=1, keypoints=frames[2]["keypoints"], descriptors=frames[2]["descriptors"])
    ia = {int(p): k for k, p in enumerate(frames[3]["point_id"]) if p >= 0}
    ib = {int(p): k for k, p in enumerate(frames[2]["point_id"]) if p >= 0}
    matches = [E.DMatch(ia[p], ib[p], 0.0) for p in sorted(set(ia) & set(ib))]
    kept = []
    found, F, n_inl = E.MotionEstimator(gpu_ctx).estimate2D2D_F7P_RANSAC(f1, f2, matches, kept, 1.0, 0.99)
    assert found and n_inl > 0.8 * len(matches) and len(kept) > 0.6 * len(matches) and abs(np.linalg.norm(F) - 1.0) < 1e-12
    assert E.MotionEstimator(gpu_ctx).estimate2D2D_F7P_RANSAC(f1, f2, matches[:5], [], 1.0, 0.99)[0] is False
