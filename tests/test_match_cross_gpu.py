"""Cross-check matching (esfm_match_cross_*) on the MI355X against the rule of include/esfm.h, built here from the oracle's 2-NN
tables in both directions.  Bit-exact on indices and distance bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth
from test_match_cross_cpu import cross_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tables(oracle, q, t, hamming):
    knn = oracle.knn2_hamming if hamming else oracle.knn2_l2
    return knn(q, t) + knn(t, q)


def _expected(oracle, q, t, ratio, hamming):
    return cross_rule(*_tables(oracle, q, t, hamming), ratio)


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "query", len(got[0]), len(want[0]))
    assert np.array_equal(got[1], want[1]), (what, "train")
    assert np.array_equal(_bits(got[2]), _bits(want[2])), (what, "distance bits")


def _l2_sets(rng, nq, nt, dim):
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    t = rng.standard_normal((nt, dim)).astype(np.float32)
    # half of the queries re-observe train rows (true matches), the rest are clutter
    k = min(nq // 2, nt)
    if k:
        q[:k] = t[rng.choice(nt, k, replace=False)] + 0.05 * rng.standard_normal((k, dim)).astype(np.float32)
    return q, t


@pytest.mark.parametrize("dim", [64, 128, 32])
@pytest.mark.parametrize("nq,nt", [(0, 5), (5, 0), (1, 1), (1, 2), (2, 1), (2, 2), (37, 300), (700, 513)])
def test_l2_single_pair(gpu_ctx, oracle_lib, dim, nq, nt):
    rng = np.random.default_rng(dim * 7919 + nq * 31 + nt)
    q, t = _l2_sets(rng, nq, nt, dim)
    for ratio in (None, 0.5, 0.8):
        _same(E.match_cross_l2(q, t, ratio, gpu_ctx), _expected(oracle_lib, q, t, ratio, False), (dim, nq, nt, ratio))


@pytest.mark.parametrize("nbytes", [32, 16, 64])
@pytest.mark.parametrize("nq,nt", [(0, 3), (3, 0), (1, 1), (1, 2), (2, 2), (300, 41), (900, 1100)])
def test_hamming_single_pair(gpu_ctx, oracle_lib, nbytes, nq, nt):
    rng = np.random.default_rng(nbytes * 104729 + nq * 17 + nt)
    t = rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, nbytes), dtype=np.uint8)
    k = min(nq // 2, nt)
    if k:
        flips = np.packbits(rng.random((k, nbytes * 8)) < 0.06, axis=1)
        q[:k] = t[rng.choice(nt, k, replace=False)] ^ flips
    for ratio in (None, 0.5, 0.8):
        _same(E.match_cross_hamming(q, t, ratio, gpu_ctx), _expected(oracle_lib, q, t, ratio, True), (nbytes, nq, nt, ratio))


def test_ties_nan_inf_self_and_both_orders(gpu_ctx, oracle_lib):
    """Duplicated train AND query rows (equal distances in both directions: the lower index wins on both sides), rows of NaN and
    Inf, a self pair (i, i), and a list holding (i, j) and (j, i)."""
    rng = np.random.default_rng(77)
    base = rng.standard_normal((60, 64)).astype(np.float32)
    t = np.concatenate([base, base[:20], base[:10]])[rng.permutation(90)]
    q = np.concatenate([base[:40], base[:15], base[30:50] + 1e-3 * rng.standard_normal((20, 64)).astype(np.float32)])
    q[5] = np.nan; q[6] = np.inf; t[7] = np.nan; t[8] = -np.inf
    c = rng.standard_normal((200, 64)).astype(np.float32)
    sets = [q, t, c]
    pairs = np.array([(0, 1), (1, 0), (2, 2), (0, 2), (2, 0), (1, 1)], np.int32)
    bank = E.DescriptorBank(sets, E.ESFM_L2_F32)
    pm = E.PairMatcher(bank, pairs)
    for ratio in (None, 0.5, 0.8):
        got = pm.match_cross(ratio).to_host()
        for p, (i, j) in enumerate(pairs):
            _same(got[p], _expected(oracle_lib, sets[i], sets[j], ratio, False), (i, j, ratio))
    hb = [np.packbits(rng.random((n, 256)) < 0.5, axis=1) for n in (50, 70)]
    hb[1][:25] = hb[0][:25]; hb[1][25:35] = hb[0][:10]          # exact duplicates: Hamming distance 0, ties in both directions
    hb[0] = np.concatenate([hb[0], hb[0][:5]])
    hpairs = np.array([(0, 1), (1, 0), (0, 0)], np.int32)
    got = E.match_cross_pairs_host(hb, hpairs, 0.8, E.ESFM_HAMMING, gpu_ctx)
    for p, (i, j) in enumerate(hpairs):
        _same(got[p], _expected(oracle_lib, hb[i], hb[j], 0.8, True), (i, j))


def test_large_query_set_takes_the_fallback(gpu_ctx, oracle_lib):
    """70 000 query rows: the mirrored pass makes them a train set beyond the one-product pass's position code."""
    rng = np.random.default_rng(5)
    q, t = _l2_sets(rng, 70000, 512, 64)
    oracle_lib.set_num_threads(min(16, os.cpu_count() or 1))
    for ratio in (None, 0.8):
        _same(E.match_cross_l2(q, t, ratio, gpu_ctx), _expected(oracle_lib, q, t, ratio, False), ratio)


def _all_tables(oracle, sets, hamming):
    knn = oracle.knn2_hamming if hamming else oracle.knn2_l2
    n = len(sets)
    return {(i, j): knn(sets[i], sets[j]) for i in range(n) for j in range(n) if i != j}


def test_msurf4k_every_pair_both_filters(oracle_lib):
    sets = synth.surf_like_sets(25, 4096, pool=16384, seed_base=1000)
    pairs = synth.all_pairs(25)
    assert len(pairs) == 300
    oracle_lib.set_num_threads(min(16, os.cpu_count() or 1))
    tab = _all_tables(oracle_lib, sets, False)
    bank = E.DescriptorBank(sets, E.ESFM_L2_F32)
    pm = E.PairMatcher(bank, pairs)
    ratio_lists = pm.match(0.5).to_host()
    for ratio in (None, 0.5):
        got = pm.match_cross(ratio).to_host()
        n = 0
        for p, (i, j) in enumerate(pairs):
            want = cross_rule(*tab[(i, j)], *tab[(j, i)], ratio)
            _same(got[p], want, (i, j, ratio))
            n += len(want[0])
            if ratio is not None:        # ratio+cross is a subset of today's ratio list
                sel = np.isin(ratio_lists[p][0], got[p][0])
                assert sel.sum() == len(got[p][0])
                assert np.array_equal(ratio_lists[p][1][sel], got[p][1]) and np.array_equal(_bits(ratio_lists[p][2][sel]), _bits(got[p][2]))
        assert n > 0


def test_morb4k_ratio_cross(oracle_lib):
    sets = synth.orb_like_sets(25, 4096, pool=16384, seed_base=3000)
    pairs = synth.all_pairs(25)
    oracle_lib.set_num_threads(min(16, os.cpu_count() or 1))
    tab = _all_tables(oracle_lib, sets, True)
    bank = E.DescriptorBank(sets, E.ESFM_HAMMING)
    got = E.PairMatcher(bank, pairs).match_cross(0.8).to_host()
    for p, (i, j) in enumerate(pairs):
        _same(got[p], cross_rule(*tab[(i, j)], *tab[(j, i)], 0.8), (i, j))


def test_transpose_symmetry_and_entry_points_agree(gpu_ctx, oracle_lib):
    """ratio+cross of (i, j) is the transpose of (j, i), distance bits included; the four entry points, PairMatcher.match_cross and
    FeatureMatching(cross_check=True) return the same lists."""
    sets = synth.surf_like_sets(4, 900, pool=2048, seed_base=44)
    pairs = np.array([(i, j) for i in range(4) for j in range(4) if i != j], np.int32)
    bank = E.DescriptorBank(sets, E.ESFM_L2_F32)
    dev = E.PairMatcher(bank, pairs).match_cross(0.8).to_host()
    host = E.match_cross_pairs_host(sets, pairs, 0.8, E.ESFM_L2_F32, gpu_ctx)
    index = {tuple(pr): p for p, pr in enumerate(pairs.tolist())}
    fm = E.FeatureMatching(gpu_ctx)
    for p, (i, j) in enumerate(pairs):
        _same(dev[p], host[p], ("host", i, j))
        _same(dev[p], E.match_cross_l2(sets[i], sets[j], 0.8, gpu_ctx), ("single", i, j))
        fi, fj = E.Frame(), E.Frame()
        fi.descriptors, fj.descriptors = sets[i], sets[j]
        ms = []
        assert fm.matchFeaturesSURF(fi, fj, ms, 0.8, cross_check=True)
        _same((np.array([m.queryIdx for m in ms], np.int32), np.array([m.trainIdx for m in ms], np.int32),
               np.array([m.distance for m in ms], np.float32)), dev[p], ("FeatureMatching", i, j))
        r = dev[index[(j, i)]]
        order = np.argsort(r[1], kind="stable")
        _same((r[1][order], r[0][order], r[2][order]), dev[p], ("transpose", i, j))
    o = synth.orb_like_sets(3, 600, pool=1024, seed_base=9)
    hp = np.array([(1, 0), (0, 1), (2, 1)], np.int32)
    hdev = E.PairMatcher(E.DescriptorBank(o, E.ESFM_HAMMING), hp).match_cross(0.8).to_host()
    hhost = E.match_cross_pairs_host(o, hp, 0.8, E.ESFM_HAMMING, gpu_ctx)
    for p, (i, j) in enumerate(hp):
        _same(hdev[p], hhost[p]); _same(hdev[p], E.match_cross_hamming(o[i], o[j], 0.8, gpu_ctx))
        fi, fj = E.Frame(), E.Frame()
        fi.descriptors, fj.descriptors = o[i], o[j]
        ms = []
        assert fm.matchFeaturesORB(fi, fj, ms, 0.8, cross_check=True)
        assert [(m.queryIdx, m.trainIdx) for m in ms] == list(zip(hdev[p][0].tolist(), hdev[p][1].tolist()))


def test_bad_arguments(gpu_ctx):
    import ctypes as C
    L = E.lib()
    q = np.zeros((3, 64), np.float32)
    qi = np.zeros(3, np.int32); ti = np.zeros(3, np.int32); d = np.zeros(3, np.float32); n = C.c_int32(0)
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    for use_ratio, ratio in ((2, 0.5), (-1, 0.5), (1, float("nan"))):
        rc = L.esfm_match_cross_l2_f32(gpu_ctx.handle, vp(q), 3, vp(q), 3, 64, use_ratio, ratio, vp(qi), vp(ti), vp(d), C.byref(n))
        assert rc == -1, (use_ratio, ratio)
    assert L.esfm_match_cross_l2_f32(gpu_ctx.handle, vp(q), 3, vp(q), 3, 64, 0, float("nan"), vp(qi), vp(ti), vp(d), C.byref(n)) == 0


def test_drivers_ratio_cross_agree_stage_by_stage(tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    exe = os.path.join(ROOT, "bin", "sfm_native")
    if not os.path.exists(exe):
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "easysfm_amd", "csrc"), "../../bin/sfm_native"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
    z = np.load(os.path.join(ROOT, "tests", "golden", "fountain11_half_gray.npz"))
    img_dir = tmp_path / "images"; img_dir.mkdir()
    names = []
    for i, img in enumerate(z["images"][:6]):
        names.append(f"{i:04d}.png")
        PIL.fromarray(np.stack([img, np.roll(img, 1, 1), img // 2 + 60], axis=2)).save(str(img_dir / names[-1]))
    (tmp_path / "image_list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "K.txt").write_text(f"{689.87 / 2} 0 {380.17 / 2}\n0 {691.04 / 2} {251.70 / 2}\n0 0 1\n")
    args = [str(img_dir), str(tmp_path / "image_list.txt"), str(tmp_path / "K.txt"), "none"]
    tail = ["S", "100", "1.0", "1", "0", "4", "1", "0", "ratio+cross"]
    rc = subprocess.run([exe] + args + [str(tmp_path / "c.ply")] + tail, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert rc.returncode == 1, rc.stdout[-3000:]
    assert "Filtered by Lowe ratio test + cross-check" in rc.stdout
    rp = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "sfm")] + args + [str(tmp_path / "p.ply")] + tail, stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT, text=True, timeout=600)
    assert rp.returncode == 1, rp.stdout[-3000:]

    def stages(text):
        keys = ("verified matches", "total unique feature point number", "Initialization frames", "Triangulate [")
        return [l.strip() for l in text.splitlines() if any(k in l for k in keys)]
    assert len(stages(rc.stdout)) > 10 and stages(rc.stdout) == stages(rp.stdout)
