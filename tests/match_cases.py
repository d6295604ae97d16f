"""Shared inputs, references and the certificate audit of the matcher tests (test_match_gpu.py, test_certificate_audit_gpu.py,
test_match_families_gpu.py, test_match_cases_cpu.py).

Every builder is a pure function of its arguments (seeded numpy generators): two calls return identical bytes.  The L2 builders take
the descriptor width, the Hamming builders the row bytes; at 64 floats / 32 bytes they return what the tests they were moved out of
built in line.  Two references share nothing with the oracle: int_l2_knn2 (integer-valued rows: int64 distances, every summation
order exact) and bit_hamming_knn2 (np.unpackbits and integer counts), both with a stable sort, so the lower index wins a tie.
`audit` is the certificate audit (esfm_ctx_set_l2_audit modes 1 and 2, mode 3 on the one-product path), `run_l2_battery` /
`run_hamming_battery` send every case through one kernel path and compare tables and ratio lists with the oracle, bit for bit."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ L2 inputs
ADVERSARIAL = ["cluster", "dynamic_range", "tiny", "denormal", "denormal_mixed", "huge_norms", "equal_rows", "sparse"]
_SEEDS = {"cluster": 1, "dynamic_range": 2, "tiny": 3, "huge_norms": 4, "equal_rows": 5, "sparse": 6, "denormal": 8, "denormal_mixed": 9, "segment_edges": 7}
SEGMENT_EDGES_64 = [0, 31, 32, 127, 128, 511, 512, 1023, 1024, 2047, 2048, 2099]


def adversarial(case, dim=64, spread=1e-5):
    """(q [300, dim], t [1500, dim]) built to sit inside an approximate distance pass's error (near-equal distances, cancellation,
    extreme magnitudes); `spread`: the relative width of `cluster`."""
    rng = np.random.default_rng(_SEEDS[case])
    nq, nt = 300, 1500
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    t = rng.standard_normal((nt, dim)).astype(np.float32)
    if case == "cluster":                   # every train within `spread` relative of one centre: all distances nearly equal
        c = rng.standard_normal(dim).astype(np.float32)
        t = (c[None, :] * (1 + spread * rng.standard_normal((nt, dim)))).astype(np.float32)
        q[:150] = (c[None, :] * (1 + spread * rng.standard_normal((150, dim)))).astype(np.float32)
    elif case == "dynamic_range":           # components spread over 12 decades inside a row
        q = (q * np.exp(rng.uniform(-14, 14, q.shape))).astype(np.float32)
        t = (t * np.exp(rng.uniform(-14, 14, t.shape))).astype(np.float32)
    elif case == "tiny":                    # magnitudes near the bottom of the normal range
        q = (q * 1e-18).astype(np.float32); t = (t * 1e-18).astype(np.float32)
    elif case == "denormal":                # |row|^2 and the bf16 residuals' squares are denormal or zero in f32
        q = (q * 1e-20).astype(np.float32); t = (t * 1e-20).astype(np.float32)
    elif case == "denormal_mixed":          # rows from 1e-23 (squares flush to zero) to 1e-17 (normal) in one train set
        q = (q * np.float32(10.0) ** rng.integers(-23, -16, (nq, 1))).astype(np.float32)
        t = (t * np.float32(10.0) ** rng.integers(-23, -16, (nt, 1))).astype(np.float32)
    elif case == "huge_norms":              # large common offset: d^2 << |q|^2 + |t|^2 (catastrophic cancellation in the GEMM form)
        q = (q + 300.0).astype(np.float32); t = (t + 300.0).astype(np.float32)
    elif case == "equal_rows":              # many identical trains and queries equal to trains
        t[100:400] = t[7]; t[900:] = t[13]; q[:50] = t[7]; q[50:100] = t[13]
    elif case == "sparse":
        q[rng.random(q.shape) < 0.9] = 0; t[rng.random(t.shape) < 0.9] = 0
    elif case == "segment_edges":           # the two nearest trains at the seams of the one-product pass (2100 train rows)
        nt = 2100
        t = rng.standard_normal((nt, dim)).astype(np.float32)
        for k, pos in enumerate(SEGMENT_EDGES_64):
            q[k] = t[pos] * np.float32(1 + 1e-4)
            q[k + 20] = t[pos]; t[(pos + 1) % nt] = t[pos] * np.float32(1 + 3e-7)
    else:
        raise KeyError(case)
    return q, t


def seams(dim, positions, nt=1100):
    """(q, t, positions): for every listed position p, train row p is the nearest row of two queries -- row k, an exact copy
    (distance 0), and row 32 + k, the copy scaled by 1 + 1e-4 -- and a near-duplicate of row p (3e-7 relative) sits one row later
    (one row earlier for the last row of the set).  Adjacent positions chain: the pair of nearest rows then straddles the seam
    between them.  nt is no multiple of a tile."""
    positions = [int(p) for p in positions]
    assert len(positions) <= 32 and all(0 <= p < nt for p in positions) and nt >= 4
    rng = np.random.default_rng(7)
    q = rng.standard_normal((300, dim)).astype(np.float32)
    t = rng.standard_normal((nt, dim)).astype(np.float32)
    for pos in sorted(positions):
        t[pos + 1 if pos + 1 < nt else pos - 1] = t[pos] * np.float32(1 + 3e-7)
    for k, pos in enumerate(positions):
        q[k] = t[pos]
        q[32 + k] = t[pos] * np.float32(1 + 1e-4)
    return q, t, positions


def duplicates_and_ties(dim=64):
    """Exact duplicates in the train set (distance-0 ties and equal-distance ties), more of them than a kernel keeps candidates."""
    rng = np.random.default_rng(7)
    base = rng.standard_normal((50, dim)).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    t = np.concatenate([base, base[:20], base[:20], base[:10], base[:10], base[:10], base[:10], base[:10]], axis=0)
    perm = rng.permutation(len(t)); t = t[perm]
    q = np.concatenate([base[:30], base[:30] + 1e-4 * rng.standard_normal((30, dim)).astype(np.float32)], axis=0)
    return q, t


def near_ties(dim=64):
    """Train rows that differ from each other by a few ulps."""
    rng = np.random.default_rng(9)
    q = rng.standard_normal((200, dim)).astype(np.float32); q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.repeat(q[:100], 6, axis=0)
    t = t * (1.0 + rng.integers(-3, 4, size=t.shape) * np.float32(6e-8))
    t = np.concatenate([t, rng.standard_normal((300, dim)).astype(np.float32) * 0.1], axis=0).astype(np.float32)
    return q, t[rng.permutation(len(t))]


def nonfinite(dim=64, rng=None):
    """(q, t, huge): 1e25-scaled train rows (their distances overflow), a NaN train row, a NaN query row; `huge` is a train set made
    of nothing but overflowing rows (no neighbours at all: indices -1)."""
    rng = np.random.default_rng(21) if rng is None else rng
    q = rng.standard_normal((300, dim)).astype(np.float32); t = rng.standard_normal((700, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True); t /= np.linalg.norm(t, axis=1, keepdims=True)
    t[[3, 77, 500]] *= np.float32(1e25)
    t[123, 5] = np.nan
    q[17, 40 % dim] = np.nan
    with np.errstate(over="ignore", invalid="ignore"):
        huge = (t[:50] * np.float32(1e25)).astype(np.float32)         # some entries overflow to inf themselves
    return q, t, huge


# rows of top3_overflow's copies; all are multiples of 8, so inside a 32-row sub-tile they fall to the same half of the f32 kernel's
# lanes (row & 4 == 0) -- one lane sees them all
TOP3_GROUPS = [[520, 600, 712, 1000],                       # four copies inside the 512-row segment 512 .. 1023
               [8, 40, 72, 104, 136, 200, 264],             # seven inside segment 0 .. 511
               [16, 528, 536, 1040],                        # four over three segments
               [24, 304, 544, 704, 1048, 1200, 1496]]       # seven over three segments


def top3_overflow(dim):
    """(q, t, groups): exact copies of a query's best train row, more than a lane's top-3 keeps -- the certificate must send the
    query to the exact scan, and the two lowest indices must win.  Group g's queries are rows 10 g .. 10 g + 9: five exact copies of
    the row (ties at distance 0) and five perturbed ones (ties at a distance above 0)."""
    rng = np.random.default_rng(31)
    q = rng.standard_normal((300, dim)).astype(np.float32)
    t = rng.standard_normal((1500, dim)).astype(np.float32)
    for g, rows in enumerate(TOP3_GROUPS):
        b = rng.standard_normal(dim).astype(np.float32)
        t[rows] = b
        q[10 * g:10 * g + 5] = b
        q[10 * g + 5:10 * g + 10] = b + np.float32(1e-3) * rng.standard_normal((5, dim)).astype(np.float32)
    return q, t, TOP3_GROUPS


def negative_scores(dim):
    """Non-negative rows (like real descriptors), queries of 5 to 50 times the train rows' norm: the score |t|^2 - 2 q.t the
    distance passes rank is negative for most pairs.  Thirty exact copies of one train row, sixty rows a few ulps from ten others,
    and queries that are scaled copies of those rows."""
    rng = np.random.default_rng(41)
    q = np.abs(rng.standard_normal((300, dim))); t = np.abs(rng.standard_normal((1300, dim)))
    q /= np.linalg.norm(q, axis=1, keepdims=True); t /= np.linalg.norm(t, axis=1, keepdims=True)
    t = (t * rng.uniform(0.5, 1.0, (1300, 1))).astype(np.float32)
    t[100:130] = t[5]
    near = np.repeat(t[10:20], 6, axis=0)
    t[200:260] = (near * (1.0 + rng.integers(-3, 4, size=near.shape) * np.float32(6e-8))).astype(np.float32)
    scale = rng.uniform(5.0, 50.0, (300, 1))
    q = (q * scale).astype(np.float32)
    q[:10] = (t[10:20] * scale[:10]).astype(np.float32)
    q[10:20] = (t[5][None, :] * scale[10:20]).astype(np.float32)
    return q, t[rng.permutation(len(t))]


# the planted rows of truncation_window: (row, |t|^2 - 2 q.t minus 4); row & 4 == 0 for all (one half of the f32 kernel's lanes), all in
# the 512-row segment 512 .. 1023, position codes 0, 1, 250 and 251
WINDOW_ROWS = [(512, 0.5e-5), (513, 3e-5), (1010, 1e-4), (1011, 1.5e-5)]


def truncation_window(dim):
    """Built against the f32 kernel's keys (the low 8 mantissa bits of a score replaced by a position code, top-3 per lane and
    segment): 40 queries (1.5, 0, ..., 0) and train rows (-1, r) have the score 4 + |r|^2 with no rounding to speak of.  Four rows
    have scores inside ONE key bucket [4, 4 + 2^-13): their keys order by position code alone, the lane keeps rows 512, 513 and 1010,
    and row 1011 -- the true second neighbour -- is left out.  The bound 2^-16 (|q|^2 + max|t|^2) alone does not cover the 250 code
    steps between the third key and the bucket's base; only the truncation allowance sends these queries to the exact scan."""
    rng = np.random.default_rng(91)
    nt = 1100
    r = rng.standard_normal((nt, dim - 1))
    r *= np.sqrt(rng.uniform(0.1, 0.5, (nt, 1))) / np.linalg.norm(r, axis=1, keepdims=True)
    t = np.concatenate([-np.ones((nt, 1)), r], axis=1).astype(np.float32)
    for row, delta in WINDOW_ROWS:
        t[row, 1:] = 0
        t[row, 1] = np.sqrt(delta)
    q = np.zeros((40, dim), np.float32); q[:, 0] = 1.5
    return q, t


def integer_sift(dim, nq=300, nt=1300, seed=51):
    """Rows of integers 0 .. 255 (as float32) drawn from a pool of 40, a few entries of half the rows changed by one: exactly equal
    distances everywhere (d0 == d1 for most queries).  Every squared distance is an integer below 2^24."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (40, dim))

    def draw(n):
        x = pool[rng.integers(0, len(pool), n)].copy()
        for r in np.nonzero(rng.random(n) < 0.5)[0]:
            cols = rng.integers(0, dim, 3)
            x[r, cols] = np.clip(x[r, cols] + rng.choice([-1, 1], 3), 0, 255)
        return x.astype(np.float32)
    t = draw(nt)
    return draw(nq), t


# ------------------------------------------------------------------------------------------------ Hamming inputs
HAMMING_CASES = ["dups_everywhere", "dups_late", "all_ones", "one_bit_apart"]


def hamming_case(case, nbytes=32, nt=3000):
    """(q [607, nbytes], t [nt, nbytes]): exact scores, so what a kernel can get wrong is WHICH rows win -- hundreds of copies of one
    row, copies whose lowest indices sit late in the set, all-ones rows (the largest scores), neighbours one bit apart."""
    rng = np.random.default_rng(21)
    t = rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)
    base = rng.integers(0, 256, (1, nbytes), dtype=np.uint8)
    if case == "dups_everywhere":
        t[rng.choice(nt, 400, replace=False)] = base
    elif case == "dups_late":
        t[[2990, 2995, 1501, 2047, 2048]] = base
    elif case == "all_ones":
        t[::7] = 0xFF
    elif case == "one_bit_apart":
        for k in range(0, nt, 5):
            t[k] = base; t[k, (k // 5) % nbytes] ^= np.uint8(1 << (k % 8))
    else:
        raise KeyError(case)
    q = np.concatenate([base, base ^ np.uint8(1), rng.integers(0, 256, (600, nbytes), dtype=np.uint8), np.full((3, nbytes), 0xFF, np.uint8),
                        np.zeros((2, nbytes), np.uint8)])
    return q, t


def hamming_ragged_batch(nbytes=32):
    """(sets, pairs): train sets of 1, 7, 300, 513, 2300 and 40 rows (fewer rows than a tile, partial last tiles), exact copies and
    one-bit neighbours across sets, all (i, j < i) pairs."""
    rng = np.random.default_rng(21)
    sizes = [1, 7, 300, 513, 2300, 40]
    sets = [rng.integers(0, 256, (n, nbytes), dtype=np.uint8) for n in sizes]
    sets[4][:200] = sets[2][:200]; sets[4][200:260, 3] ^= 1
    pairs = np.array([(i, j) for i in range(len(sizes)) for j in range(i)], np.int32)
    return sets, pairs


def forced_ties(nbytes=32):
    """(q, t): all-equal rows and three distinct distances -- ties for first AND second place everywhere."""
    t = np.zeros((300, nbytes), np.uint8)
    t[::3, 0] = 1; t[1::3, 1] = 3
    q = np.zeros((100, nbytes), np.uint8); q[50:, 5] = 0xFF
    return q, t


# ------------------------------------------------------------------------------------------------ references
def _two_smallest(d):
    """Stable 2-NN of a [nq, nt] integer distance table: (idx [nq, 2] int32, d [nq, 2] int64), -1 where there is no such row."""
    nq, nt = d.shape
    idx = np.full((nq, 2), -1, np.int32); val = np.zeros((nq, 2), np.int64)
    if nt and nq:
        order = np.argsort(d, axis=1, kind="stable")[:, :2]
        k = order.shape[1]
        idx[:, :k] = order
        val[:, :k] = np.take_along_axis(d, order, axis=1)
    return idx, val


def int_l2_knn2(q, t):
    """2-NN of integer-valued rows: squared distances in int64, stable sort (the lower index wins a tie), distance = sqrt of the
    float32 of the integer (exact below 2^24, where every summation order gives the same float)."""
    qi, ti = np.asarray(q).astype(np.int64), np.asarray(t).astype(np.int64)
    assert np.array_equal(qi, np.asarray(q)) and np.array_equal(ti, np.asarray(t)), "integer-valued rows only"
    d2 = (qi * qi).sum(1)[:, None] + (ti * ti).sum(1)[None, :] - 2 * (qi @ ti.T)
    assert d2.size == 0 or d2.max() < 1 << 24
    idx, val = _two_smallest(d2)
    dist = np.sqrt(val.astype(np.float32))
    dist[idx < 0] = FLT_MAX
    return idx, dist


def bit_hamming_knn2(q, t):
    """2-NN under the Hamming distance from np.unpackbits and integer counts, stable sort."""
    qb = np.unpackbits(np.ascontiguousarray(q, np.uint8), axis=1)
    tb = np.unpackbits(np.ascontiguousarray(t, np.uint8), axis=1)
    both = np.rint(qb.astype(np.float32) @ tb.astype(np.float32).T).astype(np.int64)      # counts of at most 512 ones: exact in float32
    d = qb.sum(1, dtype=np.int64)[:, None] + tb.sum(1, dtype=np.int64)[None, :] - 2 * both
    idx, val = _two_smallest(d)
    dist = val.astype(np.float32)
    dist[idx < 0] = FLT_MAX
    return idx, dist


def ratio_lists(idx, dist, ratio):
    """The reference's ratio test (d0 < ratio d1, in double) on a 2-NN table, in plain numpy: (query, train, distance)."""
    keep = np.nonzero((idx[:, 0] >= 0) & (idx[:, 1] >= 0) & (dist[:, 0].astype(np.float64) < ratio * dist[:, 1].astype(np.float64)))[0]
    return keep.astype(np.int32), idx[keep, 0].astype(np.int32), dist[keep, 0].astype(np.float32)


# ------------------------------------------------------------------------------------------------ the audit
def tables(pm):
    i_, d_ = pm.knn2(); pm.ctx.synchronize()
    return i_.cpu().numpy().copy(), d_.cpu().numpy().copy()


def audit(pm, label, front=False, info=None):
    """The certificate audit of one PairMatcher (L2).  A distance pass answers a query from a handful of candidates and CERTIFIES the
    answer, or flags the query for an exact re-scan.  Mode 1: the pass's own answers, the re-scan switched off; mode 2: a brute force
    of every query in the oracle's summation order; front (the one-product path only): mode 3 as well, the front pass alone with its
    own list of failures.  Asserts that the brute force equals the product path bit for bit, that the flagged list has the size the
    product path reports, and that every query whose pass-only answer differs from the brute force is on the flagged list
    (certified_but_wrong == []).  Returns (n_queries, n_flagged, n_pass_only_wrong); info (a dict) receives the front pass's count of
    uncertified queries."""
    idx, dist = tables(pm)
    n_q, n_rescan = pm.stats()
    pm.set_l2_audit(1)
    a_idx, a_dist = tables(pm)
    flagged = pm.flagged()
    if front:
        pm.set_l2_audit(3)           # the one-product bf16 pass alone: its answers, its own list of failures
        f_idx, f_dist = tables(pm)
        front_flagged = pm.flagged()
    pm.set_l2_audit(2)
    e_idx, e_dist = tables(pm)
    pm.set_l2_audit(0)
    assert np.array_equal(e_idx, idx) and np.array_equal(bits(e_dist), bits(dist)), f"{label}: brute force != product path"
    assert len(flagged) == n_rescan, (label, len(flagged), n_rescan)
    off = np.asarray(pm.offset, np.int64)
    wrong = np.nonzero(np.any(a_idx != e_idx, axis=1) | np.any(bits(a_dist) != bits(e_dist), axis=1))[0]
    flagged_rows = set((off[flagged[:, 0]] + flagged[:, 1]).tolist()) if len(flagged) else set()
    certified_but_wrong = [int(r) for r in wrong if int(r) not in flagged_rows]
    print(f"\n{label}: {n_q} queries, {len(flagged)} flagged ({100.0 * len(flagged) / max(n_q, 1):.3f} %), {len(wrong)} pass-only answers differ "
          f"from brute force, certified-but-wrong {len(certified_but_wrong)}")
    assert certified_but_wrong == [], (label, certified_but_wrong[:10])
    if front:
        # the same for the front pass on its own (its certificate carries the bf16 rounding of the operands)
        f_wrong = np.nonzero(np.any(f_idx != e_idx, axis=1) | np.any(bits(f_dist) != bits(e_dist), axis=1))[0]
        f_rows = set((off[front_flagged[:, 0]] + front_flagged[:, 1]).tolist()) if len(front_flagged) else set()
        f_cbw = [int(r) for r in f_wrong if int(r) not in f_rows]
        print(f"{label}: one-product pass alone: {len(front_flagged)} uncertified ({100.0 * len(front_flagged) / max(n_q, 1):.3f} %), {len(f_wrong)} of its answers "
              f"differ from brute force, certified-but-wrong {len(f_cbw)}")
        assert f_cbw == [], (label, f_cbw[:10])
        assert len(front_flagged) >= len(flagged)           # the second pass only sees what the first one left
        if info is not None:
            info["front_flagged"] = len(front_flagged)
    return n_q, len(flagged), len(wrong)


# ------------------------------------------------------------------------------------------------ batteries (GPU)
RATIOS = (0.6, 1.0)
RAGGED_QUERIES = [1, 127, 128, 129, 255, 256, 257]


def check_pairs(E, oracle, sets, pairs, metric, label, ctx=None, extra_ref=None, audit_totals=None):
    """One PairMatcher over `pairs`: the 2-NN table and the ratio lists at 0.6 and 1.0 against the oracle (and against
    extra_ref(q, t) -> (idx, dist) where given), indices and distance bit patterns; audit_totals (L2): a list that receives the
    audit's (queries, flagged, pass-only-wrong)."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    pm = E.PairMatcher(E.DescriptorBank(sets, metric), pairs, ctx) if ctx is not None else E.PairMatcher(E.DescriptorBank(sets, metric), pairs)
    knn = oracle.knn2_l2 if metric == E.ESFM_L2_F32 else oracle.knn2_hamming
    try:
        idx, dist = tables(pm)
        off = np.asarray(pm.offset, np.int64)
        refs = []
        for p, (i, j) in enumerate(pairs):
            ridx, rdist = knn(sets[i], sets[j])
            refs.append((ridx, rdist))
            sl = slice(int(off[p]), int(off[p + 1]))
            assert np.array_equal(idx[sl], ridx) and np.array_equal(bits(dist[sl]), bits(rdist)), (label, "2-NN table", int(i), int(j))
            if extra_ref is not None:
                xidx, xdist = extra_ref(sets[i], sets[j])
                assert np.array_equal(idx[sl], xidx) and np.array_equal(bits(dist[sl]), bits(xdist)), (label, "2-NN table, second reference", int(i), int(j))
        for ratio in RATIOS:
            res = pm.match(ratio).to_host()
            for p, (i, j) in enumerate(pairs):
                rq, rt, rd = oracle.ratio_filter(*refs[p], ratio) if len(sets[j]) >= 2 and len(sets[i]) else (np.zeros(0, np.int32),) * 3
                q_, t_, d_ = res[p]
                assert np.array_equal(q_, rq) and np.array_equal(t_, rt) and np.array_equal(bits(d_), bits(rd)), (label, "ratio list", ratio, int(i), int(j))
                if extra_ref is not None and len(sets[j]) >= 2 and len(sets[i]):
                    xq, xt, xd = ratio_lists(*extra_ref(sets[i], sets[j]), ratio)
                    assert np.array_equal(q_, xq) and np.array_equal(t_, xt) and np.array_equal(bits(d_), bits(xd)), (label, "ratio list, second reference", ratio)
        if audit_totals is not None:
            audit_totals.append((label,) + audit(pm, label))
    finally:
        pm.close()


def l2_battery(dim, seam_positions, spread=1e-5):
    """[(label, q, t, second reference or None)]: every L2 case at this width."""
    out = [(c, *adversarial(c, dim, spread), None) for c in ADVERSARIAL]
    q, t, _ = seams(dim, [p if p >= 0 else 1100 + p for p in seam_positions], 1100)
    out.append(("seams", q, t, None))
    out.append(("duplicates_and_ties", *duplicates_and_ties(dim), None))
    out.append(("near_ties", *near_ties(dim), None))
    q, t, huge = nonfinite(dim)
    out += [("nonfinite", q, t, None), ("nonfinite_all_overflow", q, huge, None)]
    q, t, _ = top3_overflow(dim)
    out.append(("top3_overflow", q, t, None))
    out.append(("negative_scores", *negative_scores(dim), None))
    out.append(("truncation_window", *truncation_window(dim), None))
    out.append(("integer_sift", *integer_sift(dim), int_l2_knn2))
    return out


def l2_ragged(dim):
    """(sets, pairs): query sets of 1, 127, 128, 129, 255, 256 and 257 rows against one train set of 1100 rows and against each
    other -- the edges of the 128- and 256-query blocks, several blocks per pair (find_pair_by_block)."""
    rng = np.random.default_rng(61)
    train = rng.standard_normal((1100, dim)).astype(np.float32)
    sets = [train]
    for n in RAGGED_QUERIES:
        x = train[rng.integers(0, len(train), n)] + np.float32(0.05) * rng.standard_normal((n, dim)).astype(np.float32)
        sets.append(np.ascontiguousarray(x, np.float32))
    k = len(RAGGED_QUERIES)
    pairs = [(s, 0) for s in range(1, k + 1)] + [(k, s) for s in range(1, k)] + [(s, k) for s in range(1, k)] + [(0, k)]
    return sets, np.array(pairs, np.int32)


def run_l2_battery(E, oracle, dim, seam_positions, path, ctx=None, spread=1e-5, with_audit=True):
    """Every L2 case and the ragged batch through whichever path the process takes at this width; with_audit: the certificate audit
    on every case, which must not be vacuous over the battery (some pass-only answer wrong, some query flagged).  Returns the
    audit's rows [(label, queries, flagged, pass-only-wrong)]."""
    totals = [] if with_audit else None
    for label, q, t, ref in l2_battery(dim, seam_positions, spread):
        check_pairs(E, oracle, [t, q], [[1, 0]], E.ESFM_L2_F32, f"{path} {dim} floats '{label}'", ctx, ref, totals)
    sets, pairs = l2_ragged(dim)
    check_pairs(E, oracle, sets, pairs, E.ESFM_L2_F32, f"{path} {dim} floats ragged batch", ctx, None, totals)
    if with_audit:
        n_q, n_f, n_w = (sum(r[k] for r in totals) for k in (1, 2, 3))
        print(f"\n{path} {dim} floats, whole battery: {n_q} queries, {n_f} flagged, {n_w} pass-only answers wrong, certified-but-wrong 0")
        assert n_f > 0 and n_w > 0, (path, "the audit is vacuous on this path", n_q, n_f, n_w)
    return totals


HAMMING_SIZES = [(1, 1), (3, 2), (64, 65), (257, 300), (1000, 999)]


def run_hamming_battery(E, oracle, nbytes, path, ctx=None):
    """knn_match_hamming, match_hamming and ragged PairMatcher batches at this row width: random rows at the sizes of
    test_hamming_knn_bitexact, every Hamming case, against the oracle and bit_hamming_knn2."""
    probs = []
    for nq, nt in HAMMING_SIZES:
        rng = np.random.default_rng(nq + 31 * nt + nbytes)
        probs.append((f"random {nq} x {nt}", rng.integers(0, 256, (nq, nbytes), dtype=np.uint8), rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)))
    probs += [(c, *hamming_case(c, nbytes)) for c in HAMMING_CASES]
    probs.append(("forced_ties", *forced_ties(nbytes)))
    for label, q, t in probs:
        label = f"{path} {nbytes} bytes '{label}'"
        ridx, rdist = oracle.knn2_hamming(q, t)
        xidx, xdist = bit_hamming_knn2(q, t)
        assert np.array_equal(ridx, xidx) and np.array_equal(rdist, xdist), (label, "the two references disagree")
        idx, dist = E.knn_match_hamming(q, t, ctx)
        assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist), (label, "knn_match_hamming")
        for ratio in RATIOS + ((0.5, 0.8, 2.0) if "forced_ties" in label else ()):     # d0 == ratio d1 must be rejected (strict <)
            a = E.match_hamming(q, t, ratio, ctx)
            b = oracle.ratio_filter(ridx, rdist, ratio) if len(t) >= 2 else (np.zeros(0, np.int32),) * 3
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (label, "match_hamming", ratio)
            assert all(np.array_equal(x, y) for x, y in zip(a, ratio_lists(xidx, xdist, ratio))), (label, "match_hamming, second reference", ratio)
    sets, pairs = hamming_ragged_batch(nbytes)
    check_pairs(E, oracle, sets, pairs, E.ESFM_HAMMING, f"{path} {nbytes} bytes ragged_batch", ctx, bit_hamming_knn2)
    rng = np.random.default_rng(71 + nbytes)
    train = rng.integers(0, 256, (1100, nbytes), dtype=np.uint8)
    sets = [train]
    for n in RAGGED_QUERIES:
        x = train[rng.integers(0, len(train), n)].copy()
        x[:, rng.integers(0, nbytes)] ^= np.uint8(1 << int(rng.integers(0, 8)))
        sets.append(x)
    check_pairs(E, oracle, sets, [(s, 0) for s in range(1, len(sets))] + [(7, 6), (6, 7), (0, 7)], E.ESFM_HAMMING,
                f"{path} {nbytes} bytes ragged query counts", ctx, bit_hamming_knn2)
