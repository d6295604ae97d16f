"""Epipolar-guided matching (esfm_match_guided_*, esfm_knn2_guided_pairs_dev) on the MI355X, bit for bit against the numpy
restatement of tests/guided_ref.py: the guided 2-NN tables (idx, dist, n_adm) and the match lists of the three filters."""
import ctypes as C

import numpy as np
import pytest

import guided_ref as G

pytestmark = pytest.mark.gpu

K4 = np.array([689.87, 380.17, 691.04, 251.70], np.float32)
FILTERS = [(0.7, False), (None, True), (0.7, True)]             # ratio, cross, ratio+cross


def essential(seed):
    """E = [t]x R of a small random motion."""
    rng = np.random.default_rng(seed)
    w = 0.1 * rng.standard_normal(3)
    th = np.linalg.norm(w); k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    t = rng.standard_normal(3); t /= np.linalg.norm(t)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R


def keypoints(rng, n):
    return np.stack([rng.uniform(0, 768, n), rng.uniform(0, 512, n)], 1).astype(np.float32)


def l2_sets(rng, sizes, dim, pool=400):
    """Rows drawn from a small pool plus noise: near twins in every set, so that the ratio test has something to decide."""
    base = rng.standard_normal((pool, dim))
    out = []
    for n in sizes:
        d = base[rng.integers(0, pool, n)] + 0.05 * rng.standard_normal((n, dim))
        out.append(np.ascontiguousarray(d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9), np.float32))
    return out


def hamming_sets(rng, sizes, nbytes, pool=400):
    base = rng.integers(0, 2, (pool, nbytes * 8), dtype=np.uint8)
    out = []
    for n in sizes:
        bits = base[rng.integers(0, pool, n)] ^ (rng.random((n, nbytes * 8)) < 0.05).astype(np.uint8)
        out.append(np.ascontiguousarray(np.packbits(bits, axis=1), np.uint8))
    return out


def _same(got, want, what):
    for a, b, name in zip(got, want, ("queryIdx", "trainIdx", "distance")):
        a = np.asarray(a); b = np.asarray(b)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        assert a.tobytes() == b.astype(a.dtype).tobytes(), (what, name)


def check_against_restatement(E_mod, gpu_ctx, metric, sets, kps, pairs, Es, px, what):
    """Tables and the three filters' lists of a batched call against the restatement, pair by pair."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    bank = E_mod.DescriptorBank(sets, metric, keypoints=kps)
    pm = E_mod.PairMatcher(bank, pairs, gpu_ctx)
    sel = np.arange(len(pairs))
    K4s = np.tile(K4, (len(pairs), 1))
    idx, dist, n_adm, off = pm.knn2_guided(sel, Es, K4s, px)
    gpu_ctx.synchronize()
    idx = idx.cpu().numpy(); dist = dist.cpu().numpy(); n_adm = n_adm.cpu().numpy()
    ref_metric = G.L2 if metric == E_mod.ESFM_L2_F32 else G.HAMMING
    refs = []
    for p, (i, j) in enumerate(pairs):
        r = G.knn2_guided(ref_metric, sets[i], kps[i], sets[j], kps[j], Es[p], K4, px)
        refs.append(r)
        o, n = int(off[p]), len(sets[i])
        assert off[p + 1] - off[p] == n
        assert np.array_equal(n_adm[o:o + n], r[2]), (what, p, "n_adm")
        assert np.array_equal(idx[o:o + n], r[0]), (what, p, "idx")
        assert dist[o:o + n].tobytes() == r[1].tobytes(), (what, p, "dist")
    for ratio, cross in FILTERS:
        got = pm.match_guided(sel, Es, K4s, px, ratio, cross).to_host()
        host = E_mod.match_guided_pairs_host(sets, kps, pairs, Es, K4s, px, ratio, cross, metric, gpu_ctx)
        for p in range(len(pairs)):
            want = G.filter_lists(refs[p][0], refs[p][1], refs[p][3], refs[p][4], ratio, cross)
            _same(got[p], want, (what, p, ratio, cross))
            _same(host[p], want, (what, "host", p, ratio, cross))
    pm.close()
    return refs


@pytest.mark.parametrize("dim", [64, 128, 20])
def test_l2_tables_and_lists(gpu_ctx, dim):
    import easysfm_amd as E
    rng = np.random.default_rng(100 + dim)
    sizes = [700, 900, 333]
    sets = l2_sets(rng, sizes, dim); kps = [keypoints(rng, n) for n in sizes]
    pairs = [(0, 1), (1, 0), (2, 1), (0, 2)]
    Es = np.stack([essential(10 + p) for p in range(len(pairs))])
    refs = check_against_restatement(E, gpu_ctx, E.ESFM_L2_F32, sets, kps, pairs, Es, 3.0, ("l2", dim))
    assert sum(int(r[2].sum()) for r in refs) > 1000              # the predicate admits something to compare
    # the one-pair host form
    for ratio, cross in FILTERS:
        got = E.match_guided_l2(sets[0], kps[0], sets[1], kps[1], Es[0], K4, 3.0, ratio, cross, gpu_ctx)
        _same(got, G.filter_lists(refs[0][0], refs[0][1], refs[0][3], refs[0][4], ratio, cross), ("single", dim, ratio, cross))


def test_hamming_tables_and_lists(gpu_ctx):
    import easysfm_amd as E
    rng = np.random.default_rng(7)
    sizes = [650, 800]
    sets = hamming_sets(rng, sizes, 32); kps = [keypoints(rng, n) for n in sizes]
    pairs = [(0, 1), (1, 0)]
    Es = np.stack([essential(20), essential(21)])
    refs = check_against_restatement(E, gpu_ctx, E.ESFM_HAMMING, sets, kps, pairs, Es, 3.0, "hamming")
    assert sum(int(r[2].sum()) for r in refs) > 500
    for ratio, cross in FILTERS:
        got = E.match_guided_hamming(sets[1], kps[1], sets[0], kps[0], Es[1], K4, 3.0, ratio, cross, gpu_ctx)
        _same(got, G.filter_lists(refs[1][0], refs[1][1], refs[1][3], refs[1][4], ratio, cross), ("single", ratio, cross))


def test_batched_call_with_the_awkward_sets(gpu_ctx):
    """Sets of 0, 1 and 2 rows on either side, a pair without a single admissible row, a train set far larger than one LDS tile
    of 256 rows, duplicated descriptor rows (ties go to the lower index) and keypoints with a NaN coordinate."""
    import easysfm_amd as E
    rng = np.random.default_rng(11)
    sizes = [300, 20000, 0, 1, 2, 257, 500]
    sets = l2_sets(rng, sizes, 64, pool=150); kps = [keypoints(rng, n) for n in sizes]
    kps[5][:, 1] += 4000.0                                       # set 5 lies far below every other set's rows
    sets[6][:250] = sets[0][:250]; sets[6][250:] = sets[0][:250]  # every row of set 0's first 250 twice, bit for bit
    kps[6][250:] = kps[6][:250] + np.float32(0.25)                # ... at nearly the same place: admissible together
    sets[1][5000:5300] = sets[1][100:400]
    kps[0][17, 0] = np.nan; kps[1][123, 1] = np.nan; kps[6][3] = np.nan
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (0, 3), (3, 0), (4, 0), (0, 4), (0, 5), (5, 0), (0, 6), (6, 0), (3, 4), (4, 3), (3, 3), (6, 6)]
    Es = np.stack([essential(30 + p) for p in range(len(pairs))])
    sideways = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)          # epipolar lines = image rows
    for p, pr in enumerate(pairs):
        if 5 in pr or pr == (6, 6):
            Es[p] = sideways
    refs = check_against_restatement(E, gpu_ctx, E.ESFM_L2_F32, sets, kps, pairs, Es, 2.0, "awkward")
    assert int(refs[8][2].sum()) == 0 and int(refs[9][2].sum()) == 0              # the pairs with set 5: nothing admissible
    assert int(refs[0][2].sum()) > 5000                                            # 300 x 20000 rows
    tie = refs[15]                                                                 # (6, 6): a row, itself, and its twin
    both = (tie[0][:, 0] >= 0) & (tie[0][:, 1] >= 0) & (tie[1][:, 0] == tie[1][:, 1])
    assert both.sum() > 100 and np.all(tie[0][both, 0] < tie[0][both, 1])
    assert tie[2][3] == 0 and refs[0][2][17] == 0                                  # the NaN keypoints admit nothing


@pytest.mark.parametrize("metric_name", ["l2", "hamming"])
def test_property_a_infinite_threshold_is_the_plain_matcher(gpu_ctx, metric_name):
    import easysfm_amd as E
    rng = np.random.default_rng(3)
    sizes = [600, 1500, 257, 2, 1]
    if metric_name == "l2":
        sets, metric, ratio = l2_sets(rng, sizes, 64, pool=4000), E.ESFM_L2_F32, 0.7      # (few twins inside a set: the ratio test passes often)
    else:
        sets, metric, ratio = hamming_sets(rng, sizes, 32, pool=4000), E.ESFM_HAMMING, 0.8
    kps = [keypoints(rng, n) for n in sizes]
    pairs = np.array([(0, 1), (1, 0), (2, 1), (1, 2), (3, 0), (0, 3), (4, 0), (0, 4), (3, 4)], np.int32)
    Es = np.stack([essential(40 + p) for p in range(len(pairs))])
    K4s = np.tile(K4, (len(pairs), 1))
    pm = E.PairMatcher(E.DescriptorBank(sets, metric, keypoints=kps), pairs, gpu_ctx)
    sel = np.arange(len(pairs))
    plain = {(ratio, False): pm.match(ratio).to_host(), (None, True): pm.match_cross(None).to_host(), (ratio, True): pm.match_cross(ratio).to_host()}
    for (r, cross), want in plain.items():
        got = pm.match_guided(sel, Es, K4s, np.inf, r, cross).to_host()
        assert sum(len(w[0]) for w in want) > 50
        for p in range(len(pairs)):
            _same(got[p], want[p], (metric_name, p, r, cross))
    pm.close()


def test_invalid_arguments(gpu_ctx):
    import easysfm_amd as E
    L = E.lib()
    rng = np.random.default_rng(1)
    q = l2_sets(rng, [8], 64)[0]; kq = keypoints(rng, 8)
    Em = np.ascontiguousarray(essential(1)); k4 = K4.copy()
    qi = np.zeros(8, np.int32); ti = np.zeros(8, np.int32); d = np.zeros(8, np.float32); n = C.c_int32(0)
    vp = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731

    def call(px, use_ratio, ratio, cross):
        return L.esfm_match_guided_l2_f32(gpu_ctx.handle, vp(q), vp(kq), 8, vp(q), vp(kq), 8, 64, vp(Em), vp(k4), px, use_ratio, ratio, cross,
                                          vp(qi), vp(ti), vp(d), C.byref(n))
    assert call(1.0, 1, 0.5, 0) == 0 and call(1.0, 0, 0.0, 1) == 0 and call(1.0, 1, 0.5, 1) == 0
    assert call(float("inf"), 1, 0.5, 0) == 0
    assert call(1.0, 0, float("nan"), 1) == 0                     # the ratio is ignored without use_ratio
    for bad in ((1.0, 0, 0.5, 0), (1.0, 2, 0.5, 0), (1.0, -1, 0.5, 1), (1.0, 1, 0.5, 2), (1.0, 1, float("nan"), 0), (1.0, 1, float("nan"), 1),
                (float("nan"), 1, 0.5, 0), (0.0, 1, 0.5, 0), (-1.0, 1, 0.5, 0), (float("-inf"), 1, 0.5, 1)):
        assert call(*bad) == -1, bad                              # ESFM_ERR_INVALID_ARG
    with pytest.raises(E.EsfmError) as ei:                        # Hamming rows of a width the matcher does not serve
        E.match_guided_hamming(np.zeros((3, 24), np.uint8), kq[:3], np.zeros((3, 24), np.uint8), kq[:3], Em, K4, 1.0, 0.8, False, gpu_ctx)
    assert ei.value.status == -5


def test_two_runs_are_byte_identical(gpu_ctx):
    import easysfm_amd as E
    rng = np.random.default_rng(9)
    sizes = [3000, 4000]
    sets = l2_sets(rng, sizes, 64, pool=100); kps = [keypoints(rng, n) for n in sizes]
    pairs = np.array([(0, 1), (1, 0)], np.int32)
    Es = np.stack([essential(50), essential(51)]); K4s = np.tile(K4, (2, 1))
    pm = E.PairMatcher(E.DescriptorBank(sets, E.ESFM_L2_F32, keypoints=kps), pairs, gpu_ctx)
    runs = []
    for _ in range(2):
        idx, dist, n_adm, _ = pm.knn2_guided([0, 1], Es, K4s, 20.0)
        lists = pm.match_guided([0, 1], Es, K4s, 20.0, 0.8, True).to_host()
        gpu_ctx.synchronize()
        runs.append((idx.cpu().numpy().tobytes(), dist.cpu().numpy().tobytes(), n_adm.cpu().numpy().tobytes(),
                     b"".join(a.tobytes() for lst in lists for a in lst)))
    assert runs[0] == runs[1]
    assert np.frombuffer(runs[0][2], np.int32).sum() > 100000     # enough admissible rows for the queue to fill and drain many times
    pm.close()


def test_guided_call_leaves_the_prepared_buffer_and_plain_results_alone(gpu_ctx):
    import easysfm_amd as E
    rng = np.random.default_rng(13)
    sizes = [1200, 1000, 900]
    sets = l2_sets(rng, sizes, 64); kps = [keypoints(rng, n) for n in sizes]
    pairs = np.array([(1, 0), (2, 0), (2, 1)], np.int32)
    bank = E.DescriptorBank(sets, E.ESFM_L2_F32, keypoints=kps)
    pm = E.PairMatcher(bank, pairs, gpu_ctx)

    def prepared():
        p = C.c_void_p()
        E._lib.check(E.lib().esfm_match_prepared_buffer(gpu_ctx.handle, C.byref(p)))
        return p.value
    assert prepared() == bank.data.data_ptr()
    before = pm.match(0.7).to_host()
    Es = np.stack([essential(60 + p) for p in range(3)]); K4s = np.tile(K4, (3, 1))
    guided = pm.match_guided([0, 1, 2], Es, K4s, 2.0, 0.7, True).to_host()
    assert prepared() == bank.data.data_ptr()
    after = pm.match(0.7).to_host()
    for p in range(3):
        _same(after[p], before[p], p)
        want = G.match_guided(G.L2, sets[pairs[p][0]], kps[pairs[p][0]], sets[pairs[p][1]], kps[pairs[p][1]], Es[p], K4, 2.0, 0.7, True)
        _same(guided[p], want, ("guided", p))
    pm.close()
