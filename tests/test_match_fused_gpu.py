"""The fused L2 launch (l2_fused_kernel: the distance pass's blocks and the finish stages' workgroups in one grid, handed over pair by
pair through pass_done) against the CPU oracle, bit for bit -- query index, train index, distance bits, lists in order -- at the
smallest shapes at which each piece of it can go wrong, and each case a second time as two launches (esfm_ctx_set_l2_two_launch),
which must give the same arrays.  No test makes the hand-over's wait run out."""
import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import _lib, synth

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _unit(rng, n):
    x = rng.standard_normal((n, 64)).astype(np.float32)
    return np.ascontiguousarray(x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), np.float32(1e-30)))


def _same(a, b, what):
    assert len(a) == len(b), what
    for p, ((q, t, d), (rq, rt, rd)) in enumerate(zip(a, b)):
        assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(_bits(d), _bits(rd)), (what, p, len(q), len(rq))


def _launches(pm, ratio):
    """(launches timed as the pass, launches timed as the finish kernel) of one match() call"""
    ctx = pm.ctx
    ctx.synchronize()
    ctx.set_kernel_timing(True)
    ctx.kernel_time(_lib.K_L2_KNN); ctx.kernel_time(_lib.K_L2_SECOND)
    pm.match(ratio)
    ctx.synchronize()
    n = (ctx.kernel_time(_lib.K_L2_KNN)[1], ctx.kernel_time(_lib.K_L2_SECOND)[1])
    ctx.set_kernel_timing(False)
    return n


def _both_arms(pm, ratio, ref, what):
    """One call per arm; either must equal the oracle's lists (hence each other).  Leaves the context on the fused arm."""
    try:
        pm.set_l2_two_launch(False)
        fused = pm.match(ratio).to_host()
        counters = (pm.second_pass(), pm.stats()[1])
        _same(fused, ref, what + ": fused launch against the oracle")
        pm.set_l2_two_launch(True)
        two = pm.match(ratio).to_host()
        _same(two, fused, what + ": two launches against the fused launch")
    finally:
        pm.set_l2_two_launch(False)
    return counters


def _case(gpu_ctx, oracle_lib, sets, pairs, ratio, what):
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    pm = E.PairMatcher(E.DescriptorBank(sets, E.ESFM_L2_F32), pairs, gpu_ctx)
    counters = _both_arms(pm, ratio, oracle_lib.match_pairs_l2(sets, pairs, ratio), what)
    return pm, counters


def test_one_query_two_train_rows(gpu_ctx, oracle_lib):
    """One pass block, and more finish slices (8 x 4 waves) than the pair has survivors."""
    rng = np.random.default_rng(1)
    t = _unit(rng, 2)
    q = np.ascontiguousarray(t[1:2] + np.float32(1e-3) * rng.standard_normal((1, 64)).astype(np.float32))
    pm, _ = _case(gpu_ctx, oracle_lib, [t, q], [(1, 0)], 0.5, "1 x 2")
    assert len(pm.match(0.5).to_host()[0][0]) == 1            # (the query has a match: the finish role's every stage saw it)
    # the switch selects what it says: one launch, timed as the pass, on the fused arm; two on the other
    assert _launches(pm, 0.5) == (1, 0)
    pm.set_l2_two_launch(True)
    try:
        assert _launches(pm, 0.5) == (1, 1)
    finally:
        pm.set_l2_two_launch(False)


def test_ragged_blocks_and_padding(gpu_ctx, oracle_lib):
    """513 queries: two pass blocks per pair, the second with one query; train sets of 300 and 200 rows: no full 256-row tile, a
    ring shorter than its depth.  Four pass blocks in all, so four padding workgroups run in front of the finish role."""
    rng = np.random.default_rng(2)
    a, b, c = _unit(rng, 513), _unit(rng, 300), _unit(rng, 200)
    a[:150] = b[rng.integers(0, 300, 150)] + np.float32(0.01) * rng.standard_normal((150, 64)).astype(np.float32)
    a[512] = c[7] + np.float32(0.01) * rng.standard_normal(64).astype(np.float32)       # the lone query of the second block matches
    pm, _ = _case(gpu_ctx, oracle_lib, [a, b, c], [(0, 1), (0, 2)], 0.7, "513 x 300 / 200")
    res = pm.match(0.7).to_host()
    assert len(res[0][0]) > 100 and 512 in res[1][0]


def test_pair_without_queries_and_pair_without_train_rows(gpu_ctx, oracle_lib):
    """A pair with zero queries has no pass block: its finish workgroups must not wait.  A pair with an empty train set has pass
    blocks that run no tile, and they must still be counted."""
    rng = np.random.default_rng(3)
    e, a, b = np.zeros((0, 64), np.float32), _unit(rng, 100), _unit(rng, 70)
    a[:30] = b[:30] + np.float32(0.01) * rng.standard_normal((30, 64)).astype(np.float32)
    pairs = [(0, 1), (1, 0), (1, 2), (0, 0), (2, 1)]
    pm, _ = _case(gpu_ctx, oracle_lib, [e, a, b], pairs, 0.6, "empty sets")
    res = pm.match(0.6).to_host()
    assert [len(r[0]) for r in res[:2]] == [0, 0] and len(res[3][0]) == 0 and len(res[2][0]) >= 25


@pytest.mark.parametrize("n_small", [600, 2400])
def test_finish_workgroups_outnumber_the_slots_and_wait(gpu_ctx, oracle_lib, n_small):
    """n_small pairs of 64 x 64 and then, last in plan order, one pair of 2048 x 2048 whose train set is the bank's FIRST set.  The
    fused launch gives lists of this length one finish workgroup per pair: 601 of them are more than the 512 resident slots, 2401
    several times as many; they start while pass blocks still run, and the large pair's -- first in the finish role's order, which
    is sorted by train set -- starts long before the pair's four pass blocks, the launch's last, are through: it really waits."""
    rng = np.random.default_rng(4)
    n_sets = 36 if n_small == 600 else 70
    big_t, big_q = _unit(rng, 2048), _unit(rng, 2048)
    big_q[:700] = big_t[rng.permutation(2048)[:700]] + np.float32(0.01) * rng.standard_normal((700, 64)).astype(np.float32)
    small = [_unit(rng, 64) for _ in range(n_sets)]
    for k in range(1, n_sets):
        small[k][:8] = small[k - 1][8:16] + np.float32(0.01) * rng.standard_normal((8, 64)).astype(np.float32)
    sets = [big_t, big_q] + small
    pairs = [(2 + i, 2 + j) for i, j in synth.all_pairs(n_sets)][:n_small] + [(1, 0)]
    assert len(pairs) == n_small + 1
    pm, _ = _case(gpu_ctx, oracle_lib, sets, pairs, 0.5, f"{n_small} small pairs + one large")
    assert len(pm.match(0.5).to_host()[-1][0]) >= 600


def test_threshold_filter_and_brute_force_in_the_fused_role(gpu_ctx, oracle_lib):
    """Ratio 0.8 on planted near-duplicates and exact duplicate rows, so that the finish role's later stages run too.
    Pair A: 100 exact copies of one row scattered through the train set, 12 copies among the queries -- more ties than the pass keeps
    groups for, so the 12 stay uncertified (more than the 8 a pair may brute-force straight away) and the threshold filter settles
    them: 1 200 hits, under the 2 048 a sweep holds, no brute force.  Pair B: 2 400 copies of three rows in the train set and 64
    copies among the queries: every sweep overflows and the exact brute force decides."""
    rng = np.random.default_rng(5)
    ratio = 0.8

    def near(x):
        return x + np.float32(2e-3) * rng.standard_normal(x.shape).astype(np.float32)

    base = _unit(rng, 4)
    ta, qa = _unit(rng, 500), _unit(rng, 212)
    ta[rng.permutation(500)[:100]] = base[0]
    qa[rng.permutation(212)[:12]] = base[0]
    free = np.flatnonzero(~(qa == base[0]).all(axis=1))[:60]
    qa[free] = near(ta[np.flatnonzero(~(ta == base[0]).all(axis=1))[:60]])             # true matches: near-duplicates of train rows
    pm, (second, brute) = _case(gpu_ctx, oracle_lib, [ta, qa], [(1, 0)], ratio, "pair A")
    assert second >= 12 and brute == 0, (second, brute)
    assert len(pm.match(ratio).to_host()[0][0]) >= 55

    tb, qb = _unit(rng, 3000), _unit(rng, 300)
    tb[rng.permutation(3000)[:2400]] = base[1 + rng.integers(0, 3, 2400)]
    qb[rng.permutation(300)[:64]] = base[1 + rng.integers(0, 3, 64)]
    freeb = np.flatnonzero(~np.isin(_bits(qb[:, 0]), _bits(base[:, 0])))[:40]
    qb[freeb] = near(tb[np.flatnonzero(~np.isin(_bits(tb[:, 0]), _bits(base[:, 0])))[:40]])
    pm, (second, brute) = _case(gpu_ctx, oracle_lib, [tb, qb], [(1, 0)], ratio, "pair B")
    assert second >= 64 and brute >= 64, (second, brute)


def test_alternating_pair_lists_on_one_matcher(gpu_ctx, oracle_lib):
    """Three calls on one matcher, alternating between two pair lists whose pairs differ in their block counts: the per-pair counters'
    two phases and the hand-over counters (reset by each pair's last finish workgroup) must be clean for every call."""
    rng = np.random.default_rng(6)
    sizes = [1100, 40, 513, 700, 5]
    sets = [_unit(rng, n) for n in sizes]
    for k in range(1, 5):
        n = min(sizes[k], sizes[k - 1], 30)
        sets[k][:n] = sets[k - 1][:n] + np.float32(0.01) * rng.standard_normal((n, 64)).astype(np.float32)
    list_a = np.array([(0, 1), (2, 0), (3, 2), (0, 3), (1, 4), (4, 0), (3, 0)], np.int32)      # blocks per pair: 3 1 2 3 1 1 2
    list_b = np.array([(1, 0), (0, 2), (4, 3)], np.int32)                                     #                 1 3 1
    pm = E.PairMatcher(E.DescriptorBank(sets, E.ESFM_L2_F32), list_a, gpu_ctx)                # (list A is the longer one: its buffers serve both)
    refs = {0: oracle_lib.match_pairs_l2(sets, list_a, 0.6), 1: oracle_lib.match_pairs_l2(sets, list_b, 0.6)}
    for two in (False, True):
        pm.set_l2_two_launch(two)
        try:
            for call, which in enumerate((0, 1, 0)):
                pm.pairs = (list_a, list_b)[which]
                pm.offset = np.zeros(len(pm.pairs) + 1, np.int64)
                _same(pm.match(0.6).to_host(), refs[which], f"call {call} (two launches: {two})")
        finally:
            pm.set_l2_two_launch(False)


def test_same_call_twice(gpu_ctx, oracle_lib):
    """The same call twice: every output array identical, the unused tails of the slices included."""
    rng = np.random.default_rng(7)
    sets = [_unit(rng, n) for n in (600, 513, 90)]
    sets[1][:200] = sets[0][:200] + np.float32(0.01) * rng.standard_normal((200, 64)).astype(np.float32)
    sets[2][:50] = sets[1][300:350] + np.float32(0.01) * rng.standard_normal((50, 64)).astype(np.float32)
    pairs = synth.all_pairs(3)
    pm, _ = _case(gpu_ctx, oracle_lib, sets, pairs, 0.7, "three sets")
    for buf in (pm.query_idx, pm.train_idx, pm.distance, pm.n_out):
        buf.zero_()
    pm.torch.cuda.synchronize(pm.bank.device)
    outs = []
    for _ in range(2):
        pm.match(0.7)
        pm.ctx.synchronize()
        outs.append([b.cpu().numpy().copy() for b in (pm.n_out, pm.query_idx, pm.train_idx, pm.distance)])
    for x, y in zip(*outs):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
