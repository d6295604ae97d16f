"""The one-product L2 pass on its 16x16x32 main loop (eight sets of 16 queries per wave, a fold group per lane quarter, the two
quarters of a lane half merged at the end of the block) against the CPU oracle: every (queryIdx, trainIdx, distance bits), lists in
order, and the 2-NN tables -- no tolerance, every query.  The cases sit on the seams of the layout: 4, 8, 16 and 32 train rows, the
256-row tile, the 512-row ring, the 16- and 32-query sets, the 128-query wave, the 512-query block, the last position code.  Each
case runs as the fused launch, as two launches and through the 2-NN table entry."""
import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth

import match_cases as MC

pytestmark = pytest.mark.gpu
_bits = MC.bits


def _unit(x):
    x = np.asarray(x, np.float64)
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), dtype=np.float32)


def _same_lists(a, b, what):
    assert len(a) == len(b), what
    for p, ((q, t, d), (rq, rt, rd)) in enumerate(zip(a, b)):
        assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(_bits(d), _bits(rd)), (what, "pair", p, len(q), len(rq))


def _check(gpu_ctx, oracle_lib, sets, pairs, ratio, what):
    """Fused lists, two-launch lists and the 2-NN tables of one PairMatcher against the oracle.  Returns the open matcher and the
    oracle's tables per pair."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    pm = E.PairMatcher(E.DescriptorBank(sets, E.ESFM_L2_F32), pairs, gpu_ctx)
    ref = oracle_lib.match_pairs_l2(sets, pairs, ratio)
    try:
        pm.set_l2_two_launch(False)
        _same_lists(pm.match(ratio).to_host(), ref, what + ": fused launch")
        pm.set_l2_two_launch(True)
        _same_lists(pm.match(ratio).to_host(), ref, what + ": two launches")
    finally:
        pm.set_l2_two_launch(False)
    idx, dist = MC.tables(pm)
    off = np.asarray(pm.offset, np.int64)
    refs = []
    for p, (i, j) in enumerate(pairs):
        ridx, rdist = oracle_lib.knn2_l2(sets[i], sets[j])
        refs.append((ridx, rdist))
        sl = slice(int(off[p]), int(off[p + 1]))
        assert np.array_equal(idx[sl], ridx) and np.array_equal(_bits(dist[sl]), _bits(rdist)), (what, "2-NN table, pair", p, int(i), int(j))
    return pm, refs


def _audits(pm, label, ratio=0.5):
    """Audit modes 3 (the one-product pass alone against the brute force: certified_but_wrong == 0, inside MC.audit) and 4 (the ratio
    screen: rejected_but_would_pass == 0).  Returns the number of queries the one-product pass left uncertified."""
    info = {}
    MC.audit(pm, label, front=True, info=info)
    pm.set_l2_audit(2)
    e_idx, e_dist = MC.tables(pm)
    pm.set_l2_audit(4)
    pm.match(ratio); pm.ctx.synchronize()
    rej = pm.flagged()
    pm.set_l2_audit(0)
    off = np.asarray(pm.offset, np.int64)
    would_pass = (e_idx[:, 0] >= 0) & (e_idx[:, 1] >= 0) & (e_dist[:, 0].astype(np.float64) < ratio * e_dist[:, 1].astype(np.float64))
    rows = (off[rej[:, 0]] + rej[:, 1]) if len(rej) else np.zeros(0, np.int64)
    assert len(set(rows.tolist())) == len(rows), f"{label}: a query was rejected twice"
    rejected_but_would_pass = int(would_pass[rows].sum())
    print(f"{label}: ratio screen at {ratio} dropped {len(rows)} queries, rejected-but-would-pass {rejected_but_would_pass}")
    assert rejected_but_would_pass == 0, (label, rows[would_pass[rows]][:10])
    return info["front_flagged"]


# ------------------------------------------------------------------------------------------------ ragged sizes
TRAIN_SIZES = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1100]
QUERY_SIZES = [1, 15, 16, 17, 31, 33, 127, 129, 511, 513]


def test_ragged_sizes(gpu_ctx, oracle_lib):
    """Every train size against every query size in ONE PairMatcher call: partial fold groups, steps, tiles and rings; partial
    query sets, waves and blocks.  A train set of n rows is the first n rows of one pool, so a query's planted neighbour is in
    some sets and missing from others."""
    rng = np.random.default_rng(101)
    pool = _unit(rng.standard_normal((1100, 64)))
    sets = [np.ascontiguousarray(pool[:n]) for n in TRAIN_SIZES]
    for k, n in enumerate(QUERY_SIZES):
        src = np.concatenate([rng.integers(0, 40, n // 2 + 1), rng.integers(0, 1100, n)])[:n]      # half of them near the first 40 rows
        sets.append(_unit(pool[src] + 0.03 * rng.standard_normal((n, 64)) * (rng.random((n, 1)) < 0.7)))
    nt_, nq_ = len(TRAIN_SIZES), len(QUERY_SIZES)
    pairs = [(nt_ + a, b) for a in range(nq_) for b in range(nt_)]
    pm, _ = _check(gpu_ctx, oracle_lib, sets, pairs, 0.7, "ragged sizes")
    try:
        res = pm.match(0.7).to_host()
        assert sum(len(r[0]) for r in res) > 100           # the lists are not empty: the planted neighbours are found
    finally:
        pm.close()


# ------------------------------------------------------------------------------------------------ planted neighbours
PLANTED_Q = [0, 15, 16, 31, 32, 47, 127, 128, 255, 256, 511]      # both queries of a lane, first and last set of a wave, every wave
NT = 1100


def _planted_specs():
    """[(kind, r1, r2)] for four scenes of eleven planted queries: (a) one 8-row group, r and r + 8; (b) one quarter, two steps, r and
    r + 32; (c) the two quarters merged at block end, r and r + 16; (d) the two halves, r and r + 4; (e) the tile seam and the ring
    wrap, 255 / 256, 511 / 512, 767 / 768; (f) the last, partial step, nt - 1 and nt - 2.  r1 mod 32 takes all 32 values."""
    allowed = {"a": lambda r: r % 16 < 8, "b": lambda r: True, "c": lambda r: r % 32 < 16, "d": lambda r: r % 8 < 4}
    delta = {"a": 8, "b": 32, "c": 16, "d": 4}
    steps = [1, 7, 8, 15, 16, 23, 24, 31, 9, 17, 30, 2]              # first, last and middle steps of both ring buffers, several tiles
    specs = [("e", 255, 256), ("e", 511, 512), ("e", 767, 768), ("f", NT - 1, NT - 2)]
    k = 0
    for rho in list(range(32)) + [0, 1, 2, 3, 16, 17, 18, 19]:     # every residue once, then more of (a) .. (d) in other steps
        kinds = [x for x in "abcd" if allowed[x](rho)]
        kind = kinds[k % len(kinds)]
        r1 = 32 * steps[k % len(steps)] + rho
        specs.append((kind, r1, r1 + delta[kind]))
        k += 1
    assert len(specs) == 4 * len(PLANTED_Q) and {s[1] % 32 for s in specs} == set(range(32)) and {s[0] for s in specs} == set("abcdef")
    return specs


def _planted_scenes():
    """(sets, pairs, expected): four train sets of 1100 unit rows and four query sets of 512; the planted queries' nearest row at
    distance ~0.05 and second nearest at ~0.2, everything else at ~1.4."""
    rng = np.random.default_rng(202)
    specs = _planted_specs()
    # deal the specs so that no two of a scene touch the same train row
    scenes = [[] for _ in range(4)]
    used = [set() for _ in range(4)]
    for spec in specs:
        for s in sorted(range(4), key=lambda s: len(scenes[s])):
            if len(scenes[s]) < len(PLANTED_Q) and not ({spec[1], spec[2]} & used[s]):
                scenes[s].append(spec); used[s] |= {spec[1], spec[2]}
                break
        else:
            raise AssertionError("could not place a planted pair")
    trains, queries, expected = [], [], []
    for s in range(4):
        t = _unit(np.abs(rng.standard_normal((NT, 64))))
        q = _unit(np.abs(rng.standard_normal((512, 64))))
        exp = {}
        for qi, (kind, r1, r2) in zip(PLANTED_Q, scenes[s]):
            d1, d2 = _unit(rng.standard_normal((2, 64)))
            t[r1] = q[qi] + np.float32(0.05) * d1
            t[r2] = q[qi] + np.float32(0.2) * d2
            exp[qi] = (kind, r1, r2)
        trains.append(t); queries.append(q); expected.append(exp)
    return trains + queries, [(4 + s, s) for s in range(4)], expected


def test_planted_neighbours(gpu_ctx, oracle_lib):
    sets, pairs, expected = _planted_scenes()
    pm, refs = _check(gpu_ctx, oracle_lib, sets, pairs, 0.5, "planted neighbours")
    try:
        res = pm.match(0.5).to_host()
        for s, exp in enumerate(expected):
            ridx, rdist = refs[s]
            for qi, (kind, r1, r2) in exp.items():
                assert tuple(ridx[qi]) == (r1, r2), ("the construction", s, qi, kind, ridx[qi])
                assert 0.04 < rdist[qi, 0] < 0.06 and 0.18 < rdist[qi, 1] < 0.22
                assert qi in res[s][0] and res[s][1][list(res[s][0]).index(qi)] == r1, (s, qi, kind)       # the ratio test at 0.5 passes
        _audits(pm, "planted neighbours")
    finally:
        pm.close()


# ------------------------------------------------------------------------------------------------ more copies than a quarter keeps keys
ONE_QUARTER = [32 * s for s in (1, 5, 9, 17, 20, 33)]                             # quarter (h 0, G 0), six steps, three tiles
TWO_QUARTERS = [32 * s for s in (2, 9, 33)] + [32 * s + 16 for s in (1, 9, 30)]   # quarters G 0 and G 1 of half 0
QUARTER_ROWS = [2, 0, 1, 3, 8, 9]                                                 # rows of quarter (h 0, G 0) inside a step: one per query


@pytest.mark.parametrize("rows", [ONE_QUARTER, TWO_QUARTERS], ids=["one_quarter", "two_quarters_of_a_half"])
def test_more_copies_than_keys(gpu_ctx, oracle_lib, rows):
    """Six exact copies of the nearest row where a quarter keeps four keys: the lowest two indices must win (the oracle's answer),
    for exact copies (distance 0) and for a query a little off (six equal distances above 0)."""
    rng = np.random.default_rng(303)
    t = _unit(np.abs(rng.standard_normal((NT, 64))))
    q = _unit(np.abs(rng.standard_normal((64, 64))))
    for k, qi in enumerate([0, 15, 16, 31, 32, 63]):
        b = _unit(np.abs(rng.standard_normal((1, 64))))[0]
        t[[r + QUARTER_ROWS[k] for r in rows]] = b
        q[qi] = b if k % 2 == 0 else _unit((b + np.float32(1e-3) * rng.standard_normal(64))[None, :])[0]
    pm, refs = _check(gpu_ctx, oracle_lib, [t, q], [(1, 0)], 0.5, "six copies")
    try:
        ridx, rdist = refs[0]
        for k, qi in enumerate([0, 15, 16, 31, 32, 63]):
            assert tuple(ridx[qi]) == tuple(sorted(r + QUARTER_ROWS[k] for r in rows)[:2]), ("the construction", qi, ridx[qi])
        assert rdist[0, 0] == 0 and rdist[0, 1] == 0
        _audits(pm, "six copies")
    finally:
        pm.close()


@pytest.mark.parametrize("case", ["duplicates_and_ties", "top3_overflow"])
def test_duplicate_cases(gpu_ctx, oracle_lib, case):
    q, t = MC.duplicates_and_ties(64) if case == "duplicates_and_ties" else MC.top3_overflow(64)[:2]
    pm, _ = _check(gpu_ctx, oracle_lib, [t, q], [(1, 0)], 0.5, case)
    try:
        _audits(pm, case)
    finally:
        pm.close()


# ------------------------------------------------------------------------------------------------ the position code's limit
def test_position_code_limit(gpu_ctx, oracle_lib):
    """65 536 train rows, 16 queries, two train sets: the nearest and second nearest rows at 65 535 and 65 504 -- the last step's
    codes 2047 << 1 | G, both quarters of a half -- and at 0 and 65 535: the first code and the last in one answer."""
    rng = np.random.default_rng(404)
    nt = 65536
    t = _unit(np.abs(rng.standard_normal((nt, 64))))
    base = _unit(np.abs(rng.standard_normal((1, 64))))[0]
    d = _unit(rng.standard_normal((2, 64)))
    t_last, t_both = t.copy(), t.copy()
    t_last[65535] = base + np.float32(0.05) * d[0]
    t_last[65504] = base + np.float32(0.2) * d[1]
    t_both[0] = base + np.float32(0.05) * d[0]
    t_both[65535] = base + np.float32(0.2) * d[1]
    q = _unit(base[None, :] + np.float32(0.01) * _unit(rng.standard_normal((16, 64))))          # 0.01 off the planted direction
    q[0] = base
    pm, refs = _check(gpu_ctx, oracle_lib, [t_last, t_both, q], [(2, 0), (2, 1)], 0.5, "65 536 train rows")
    try:
        assert all(tuple(r) == (65535, 65504) for r in refs[0][0]) and all(tuple(r) == (0, 65535) for r in refs[1][0])
        res = pm.match(0.5).to_host()
        assert len(res[0][0]) == 16 and len(res[1][0]) == 16
    finally:
        pm.close()


# ------------------------------------------------------------------------------------------------ the metric's pair, audited
PARENT_UNCERTIFIED_4096 = 19        # the 32x32 main loop's count on the same pair (printed beside this build's; not asserted)


def test_audit_surf_4096(gpu_ctx):
    """One 4096 x 4096 pair of the metric's workload: certified_but_wrong == 0, rejected_but_would_pass == 0.  The number of
    queries the one-product pass leaves uncertified is printed beside the 32x32 main loop's (the keys name the same groups; only
    the scores' low bits moved), for information."""
    sets = synth.surf_like_sets(2, 4096, seed_base=1000)
    pm = E.PairMatcher(E.DescriptorBank(sets, E.ESFM_L2_F32), np.array([[1, 0]], np.int32), gpu_ctx)
    try:
        n = _audits(pm, "M-SURF-4k pair")
        print(f"M-SURF-4k pair: {n} of 4096 queries uncertified by the one-product pass; the 32x32 main loop left {PARENT_UNCERTIFIED_4096}")
    finally:
        pm.close()
