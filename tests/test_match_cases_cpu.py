"""The shared matcher cases and references of match_cases.py, without a GPU: the two independent references equal the oracle on their
cases, every case has the property its name claims, and every builder is deterministic."""
import numpy as np
import pytest

import match_cases as MC


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dim", [64, 128])
def test_int_l2_reference_equals_the_oracle(oracle_lib, dim):
    q, t = MC.integer_sift(dim)
    idx, dist = MC.int_l2_knn2(q, t)
    ridx, rdist = oracle_lib.knn2_l2(q, t)
    assert np.array_equal(idx, ridx) and np.array_equal(MC.bits(dist), MC.bits(rdist))
    for ratio in MC.RATIOS:
        assert all(np.array_equal(a, b) for a, b in zip(MC.ratio_lists(idx, dist, ratio), oracle_lib.ratio_filter(ridx, rdist, ratio)))
    # a single train row: no second neighbour
    idx, dist = MC.int_l2_knn2(q[:5], t[:1]); ridx, rdist = oracle_lib.knn2_l2(q[:5], t[:1])
    assert np.array_equal(idx, ridx) and np.array_equal(MC.bits(dist), MC.bits(rdist))


@pytest.mark.parametrize("nbytes", [16, 32, 64])
def test_bit_hamming_reference_equals_the_oracle(oracle_lib, nbytes):
    probs = [MC.hamming_case(c, nbytes) for c in MC.HAMMING_CASES] + [MC.forced_ties(nbytes)]
    sets, pairs = MC.hamming_ragged_batch(nbytes)
    probs += [(sets[i], sets[j]) for i, j in pairs]
    for q, t in probs:
        idx, dist = MC.bit_hamming_knn2(q, t)
        ridx, rdist = oracle_lib.knn2_hamming(q, t)
        assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist)


@pytest.mark.parametrize("dim", [20, 37, 64, 128])
def test_integer_sift_ties(dim):
    q, t = MC.integer_sift(dim)
    assert q.dtype == np.float32 and q.min() >= 0 and q.max() <= 255 and np.array_equal(q, np.round(q)) and np.array_equal(t, np.round(t))
    idx, dist = MC.int_l2_knn2(q, t)
    tied = int((dist[:, 0] == dist[:, 1]).sum())
    assert 2 * tied >= len(q), tied
    assert (dist[:, 0] > 0).any() and (idx[:, 0] < idx[:, 1])[dist[:, 0] == dist[:, 1]].all()


@pytest.mark.parametrize("dim", [64, 128])
def test_negative_scores_are_negative(dim):
    q, t = MC.negative_scores(dim)
    qd, td = q.astype(np.float64), t.astype(np.float64)
    score = (td * td).sum(1)[None, :] - 2.0 * qd @ td.T
    assert (score < 0).mean() > 0.5, (score < 0).mean()
    ratio = np.linalg.norm(qd, axis=1).min() / np.linalg.norm(td, axis=1).max()
    assert ratio >= 4.9
    assert len(np.unique(t, axis=0)) <= len(t) - 29                 # the exact copies are there


@pytest.mark.parametrize("dim", [64, 128])
def test_top3_overflow_has_four_equal_minima_in_a_segment(dim):
    q, t, groups = MC.top3_overflow(dim)
    d = ((q[:40].astype(np.float64)[:, None, :] - t.astype(np.float64)[None, :, :]) ** 2).sum(2)      # (the groups' queries)
    for g, rows in enumerate(groups):
        assert len(rows) >= 4 and all(r % 8 == 0 for r in rows)
        for k in range(10 * g, 10 * g + 10):
            mins = np.nonzero(d[k] == d[k].min())[0]
            assert mins.tolist() == rows, (g, k)
            assert (d[k].min() == 0) == (k < 10 * g + 5)
    for g in (0, 1):                                                # all copies inside ONE 512-row segment
        assert len({r // 512 for r in groups[g]}) == 1
    for g in (2, 3):                                                # ... and spread over three
        assert len({r // 512 for r in groups[g]}) == 3


@pytest.mark.parametrize("dim,positions", [(128, [0, 31, 32, 63, 64, 127, 128, 511, 512, 513, 1023, 1024, 1099]),
                                           (64, [0, 3, 4, 31, 32, 127, 128, 255, 256, 1023, 1024, 1099])])
def test_seams_plants_the_nearest_rows(oracle_lib, dim, positions):
    nt = 1100
    q, t, pos = MC.seams(dim, positions, nt)
    assert pos == positions and len(t) == nt
    idx, dist = oracle_lib.knn2_l2(q, t)
    for k, p in enumerate(positions):
        dup = p + 1 if p + 1 < nt else p - 1
        assert idx[k, 0] == p and dist[k, 0] == 0.0 and abs(int(idx[k, 1]) - p) == 1, (p, idx[k])
        if p - 1 not in positions:
            assert idx[k, 1] == dup, (p, idx[k])
        near = set(range(max(p - 1, 0), min(p + 4, nt)))            # (chains of adjacent positions: up to three rows later)
        assert set(idx[32 + k].tolist()) <= near and dist[32 + k, 1] < 1e-2 * np.linalg.norm(t[p]), (p, idx[32 + k])


@pytest.mark.parametrize("dim", [64, 128])
def test_truncation_window_sits_between_the_two_allowances(oracle_lib, dim):
    q, t = MC.truncation_window(dim)
    qd, td = q.astype(np.float64), t.astype(np.float64)
    score = (td * td).sum(1) - 2.0 * td @ qd[0]
    rows = [r for r, _ in MC.WINDOW_ROWS]
    others = np.setdiff1d(np.arange(len(t)), rows)
    assert all(4.0 <= score[r] < 4.0 + 2.0 ** -13 for r in rows) and score[others].min() > 4.09
    assert all(r // 512 == 1 and r % 8 < 4 for r in rows)
    assert np.argsort(score, kind="stable")[:4].tolist() == [512, 1011, 513, 1010]
    idx, dist = oracle_lib.knn2_l2(q, t)
    assert (idx == [512, 1011]).all()
    # keys order by position code inside the bucket: rows 512, 513, 1010 (codes 0, 1, 250) are kept, 1011 (code 251) is not, and the
    # third key is 4 + 250 ulp.  Without the truncation allowance the certificate would accept (512, 513); with it, it cannot.
    qn, tmax = float((qd[0] ** 2).sum()), float((td * td).sum(1).max())
    tau, d2_second_kept = 4.0 + 250 * 2.0 ** -21, qn + score[513]
    assert qn + tau - (qn + tmax) / 65536.0 > d2_second_kept * (1 + 2.0 ** -20)
    assert qn + tau - (qn + tmax) / 65536.0 - tau / 16384.0 < d2_second_kept


def test_builders_are_deterministic():
    calls = [(lambda c=c: MC.adversarial(c, 128)) for c in MC.ADVERSARIAL + ["segment_edges"]]
    calls += [lambda: MC.seams(128, [0, 31, 32, 1099])[:2], lambda: MC.duplicates_and_ties(128), lambda: MC.near_ties(37), lambda: MC.nonfinite(20),
              lambda: MC.top3_overflow(64)[:2], lambda: MC.negative_scores(128), lambda: MC.truncation_window(64), lambda: MC.integer_sift(128), lambda: MC.forced_ties(16),
              lambda: MC.hamming_ragged_batch(64)[0], lambda: MC.l2_ragged(128)[0]]
    calls += [(lambda c=c: MC.hamming_case(c, 64)) for c in MC.HAMMING_CASES]
    for f in calls:
        a, b = f(), f()
        assert len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    assert len(MC.l2_battery(128, [0, 31, -1])) == 17
