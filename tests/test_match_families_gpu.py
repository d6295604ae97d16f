"""Every kernel family of the matcher (select_path, match_api.cpp) on the adversarial inputs of match_cases.py, with the certificate
audit where the path has a certificate.  All comparisons are on indices and distance bit patterns: 2-NN tables and the ratio lists
at 0.6 and 1.0 against the oracle, and against the integer references where the rows are integer-valued / binary.

In process: L2_F32_MFMA at 128 floats (the default of every 128-float descriptor), L2_THREE_PRODUCT reached by size (65 537 train
rows) and its hand-over from / to the one-product path on one context, HM_VALU (16- and 64-byte rows), L2_EXACT (20 and 37 floats).
In a child process per switch value (the switches are read once per process): ESFM_L2_PASS=bf16x3, ESFM_L2_PASS=f32 and
ESFM_HM_PASS=i8, each with the whole battery of its path.  Each audited path must show, over its battery, at least one pass-only
answer that differs from brute force and a non-empty flagged list -- an audit that never sees the certificate at work proves nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import _lib

import match_cases as MC

pytestmark = pytest.mark.gpu

# the seams of the f32 kernel: its 32-row sub-tiles, 64- and 128-row tiles and 512-row segments (-1: the last row)
F32_SEAMS = [0, 31, 32, 63, 64, 127, 128, 511, 512, 513, 1023, 1024, -1]
# ... and of the three-product kernel: 4-row fold groups, 32-row steps, 128-row tiles
BF16X3_SEAMS = [0, 3, 4, 31, 32, 127, 128, 255, 256, 1023, 1024, -1]
# the width of `cluster` per path: narrow enough that the pass's own answers (audit mode 1) are wrong for some query
CLUSTER_SPREAD = {"f32": 1e-5, "bf16x3": 1e-5}


def _launches(ctx, fn):
    """(K_L2_RESCAN launches, K_L2_SECOND launches) of fn(): the finish kernel's timer records launches only on the one-product
    path, the re-scan's only off it."""
    ctx.synchronize(); ctx.set_kernel_timing(True); ctx.kernel_time(_lib.K_L2_RESCAN); ctx.kernel_time(_lib.K_L2_SECOND)
    try:
        out = fn(); ctx.synchronize()
        return out, ctx.kernel_time(_lib.K_L2_RESCAN)[1], ctx.kernel_time(_lib.K_L2_SECOND)[1]
    finally:
        ctx.set_kernel_timing(False)


def test_l2_f32_mfma_128_floats(oracle_lib):
    """l2_knn_mfma_kernel<128> + the exact scan of its failures: the whole L2 battery (integer-valued SIFT-like rows, negative
    scores, more copies than a lane's top-3, non-finite rows, the seams of its tiles and segments, a ragged batch) and the audit."""
    MC.run_l2_battery(E, oracle_lib, 128, F32_SEAMS, "L2_F32_MFMA", spread=CLUSTER_SPREAD["f32"])


def _large_set(nt):
    """(q [256, 64], t [nt, 64]): three exact copies of query 0 in the last two rows and in row 3 (rows 3 and nt - 2 win),
    neighbours of queries 1 and 2 in the last 32-row step and mid-set, queries 3 .. 39 a hair away from rows spread over the set."""
    rng = np.random.default_rng(nt)
    t = rng.standard_normal((nt, 64)).astype(np.float32); t /= np.linalg.norm(t, axis=1, keepdims=True)
    q = rng.standard_normal((256, 64)).astype(np.float32); q /= np.linalg.norm(q, axis=1, keepdims=True)
    t[[nt - 1, nt - 2, 3]] = q[0]
    t[nt - 21] = q[1] + 0.01 * rng.standard_normal(64).astype(np.float32)
    t[40000] = q[2] + 0.02 * rng.standard_normal(64).astype(np.float32)
    rows = np.linspace(5, nt - 40, 37).astype(np.int64)
    q[3:40] = t[rows] * np.float32(1 + 1e-4)
    t[rows + 1] = t[rows] * np.float32(1 + 3e-7)
    return q, t


@pytest.mark.parametrize("nt", [65535, 65536, 65537])
def test_l2_three_product_reached_by_size(gpu_ctx, oracle_lib, nt):
    """65 536 train rows is the last size the one-product pass numbers; at 65 537 the call takes l2_knn_bf16_kernel +
    l2_rescan64_pairs, the way a user reaches them.  Which path ran is read off the kernel timers; the audit runs on both sides."""
    q, t = _large_set(nt)
    oracle_lib.set_num_threads(os.cpu_count() or 1)
    ridx, rdist = oracle_lib.knn2_l2(q, t)
    assert ridx[0].tolist() == [3, nt - 2] and rdist[0].tolist() == [0.0, 0.0]
    pm = E.PairMatcher(E.DescriptorBank([t, q], E.ESFM_L2_F32), np.array([[1, 0]], np.int32), gpu_ctx)
    (idx, dist), rescans, finishes = _launches(gpu_ctx, lambda: MC.tables(pm))
    assert (rescans > 0 and finishes == 0) if nt > 65536 else (rescans == 0 and finishes > 0), (nt, rescans, finishes)
    assert np.array_equal(idx, ridx) and np.array_equal(MC.bits(dist), MC.bits(rdist))
    for ratio in MC.RATIOS:
        a = pm.match(ratio).to_host()[0]; b = oracle_lib.ratio_filter(ridx, rdist, ratio)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(MC.bits(a[2]), MC.bits(b[2])), (nt, ratio)
    MC.audit(pm, f"{nt} train rows", front=nt <= 65536)
    pm.close()


def test_l2_paths_alternate_on_one_context(gpu_ctx, oracle_lib):
    """One bank with a 65 537-row set and three small ones.  A pair list that includes the large set takes the three-product path as
    a whole and ends the prepared state; a list of the small sets alone takes the one-product path and re-derives its operand images;
    then the first list again.  The alternation moves l2_phase, the phase counters and prep_desc: every result equals the oracle's,
    and the first and third are identical bytes."""
    rng = np.random.default_rng(81)
    q, big = _large_set(65537)
    sets = [big]
    for n in (300, 513, 257):
        x = big[rng.integers(0, len(big), n)] + np.float32(0.02) * rng.standard_normal((n, 64)).astype(np.float32)
        sets.append(np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), np.float32))
    sets[1][:40] = q[:40]
    sets[3][:100] = sets[2][:100] * np.float32(1 + 1e-4)
    with_large = np.array([(1, 0), (2, 1), (3, 0), (3, 2)], np.int32)
    small_only = np.array([(1, 2), (2, 3), (3, 1), (1, 3)], np.int32)
    bank = E.DescriptorBank(sets, E.ESFM_L2_F32)
    pm_large = E.PairMatcher(bank, with_large, gpu_ctx)
    pm_small = E.PairMatcher(bank, small_only, gpu_ctx)
    oracle_lib.set_num_threads(os.cpu_count() or 1)
    ref = {(int(i), int(j)): oracle_lib.knn2_l2(sets[i], sets[j]) for i, j in np.concatenate([with_large, small_only])}

    def run(pm):
        idx, dist = MC.tables(pm)
        lists = pm.match(0.6).to_host()
        off = np.asarray(pm.offset, np.int64)
        for p, (i, j) in enumerate(pm.pairs):
            ridx, rdist = ref[int(i), int(j)]
            sl = slice(int(off[p]), int(off[p + 1]))
            assert np.array_equal(idx[sl], ridx) and np.array_equal(MC.bits(dist[sl]), MC.bits(rdist)), (int(i), int(j))
            rq, rt, rd = oracle_lib.ratio_filter(ridx, rdist, 0.6)
            assert np.array_equal(lists[p][0], rq) and np.array_equal(lists[p][1], rt) and np.array_equal(MC.bits(lists[p][2]), MC.bits(rd)), (int(i), int(j))
        return idx.tobytes() + dist.tobytes() + b"".join(a.tobytes() for l in lists for a in l)

    pm_large.prepare()                                   # operand images of the one-product pass, for the whole bank
    first, rescans, finishes = _launches(gpu_ctx, lambda: run(pm_large))
    assert rescans > 0 and finishes == 0, (rescans, finishes)
    _, rescans, finishes = _launches(gpu_ctx, lambda: run(pm_small))
    assert rescans == 0 and finishes > 0, (rescans, finishes)
    third, rescans, finishes = _launches(gpu_ctx, lambda: run(pm_large))
    assert rescans > 0 and finishes == 0, (rescans, finishes)
    assert first == third
    run(pm_small)
    pm_large.close(); pm_small.close()


@pytest.mark.parametrize("nbytes", [16, 64])
def test_hm_valu_128_and_512_bit_rows(gpu_ctx, oracle_lib, nbytes):
    """hamming_knn_kernel<4> / <16>: the plain 2-NN table, the ratio lists and ragged PairMatcher batches, with ties."""
    MC.run_hamming_battery(E, oracle_lib, nbytes, "HM_VALU", gpu_ctx)


@pytest.mark.parametrize("dim", [20, 37])
def test_l2_exact_widths_without_an_mfma_build(gpu_ctx, oracle_lib, dim):
    """l2_exact_scan_kernel<true> (20 floats) and <false> (37: the scalar tail of the canonical sum) on ties, near-ties, non-finite
    rows, integer-valued rows and a ragged batch."""
    q, t, huge = MC.nonfinite(dim)
    probs = [("duplicates_and_ties", *MC.duplicates_and_ties(dim), None), ("near_ties", *MC.near_ties(dim), None), ("nonfinite", q, t, None),
             ("nonfinite_all_overflow", q, huge, None), ("integer_sift", *MC.integer_sift(dim), MC.int_l2_knn2)]
    for label, q, t, ref in probs:
        MC.check_pairs(E, oracle_lib, [t, q], [[1, 0]], E.ESFM_L2_F32, f"L2_EXACT {dim} floats '{label}'", gpu_ctx, ref)
    sets, pairs = MC.l2_ragged(dim)
    MC.check_pairs(E, oracle_lib, sets, pairs, E.ESFM_L2_F32, f"L2_EXACT {dim} floats ragged batch", gpu_ctx)


_CHILD = r'''
import sys; sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, easysfm_amd as E, oracle, match_cases as MC
from easysfm_amd import _lib
which, spread = sys.argv[1], float(sys.argv[2])
seams = [int(s) for s in sys.argv[3].split(",")]
oracle.build()
rng = np.random.default_rng(17)
if which == "i8":
    MC.run_hamming_battery(E, oracle, 32, "HM_I8")
    sets = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (700, 300)]
    sets[1][:200] = sets[0][:200]; sets[1][:200, 3] ^= 1
    pm = E.PairMatcher(E.DescriptorBank(sets, E.ESFM_HAMMING), np.array([[1, 0]], np.int32))
    # the switch took: the FP4 kernel's ratio screen marks the queries it drops with train index -2, the i8 kernel leaves every
    # query its exact 2-NN
    idx, _ = pm.knn2_screened(0.6); pm.ctx.synchronize()
    assert not (idx.cpu().numpy() == -2).any(), "the FP4 kernel ran"
else:
    MC.run_l2_battery(E, oracle, 64, seams, {"bf16x3": "L2_THREE_PRODUCT", "f32": "L2_F32_MFMA"}[which], spread=spread)
    sets = [rng.standard_normal((n, 64)).astype(np.float32) for n in (700, 300)]
    pm = E.PairMatcher(E.DescriptorBank(sets, E.ESFM_L2_F32), np.array([[1, 0]], np.int32))
    # the switch took: l2_finish_kernel's timer (K_L2_SECOND) records launches only on the one-product path, the fallbacks time
    # their re-scan as K_L2_RESCAN
    ctx = pm.ctx
    ctx.synchronize(); ctx.set_kernel_timing(True); ctx.kernel_time(_lib.K_L2_RESCAN); ctx.kernel_time(_lib.K_L2_SECOND)
    pm.match(0.6); pm.knn2(); ctx.synchronize()
    rescans, finishes = ctx.kernel_time(_lib.K_L2_RESCAN)[1], ctx.kernel_time(_lib.K_L2_SECOND)[1]
    ctx.set_kernel_timing(False)
    assert rescans > 0 and finishes == 0, (rescans, finishes)
print("ok")
'''


@pytest.mark.parametrize("switch,value", [("ESFM_L2_PASS", "bf16x3"), ("ESFM_L2_PASS", "f32"), ("ESFM_HM_PASS", "i8")])
def test_switched_kernel_families_whole_battery(gpu_ctx, switch, value):
    """The families behind a switch, each in a fresh child process with the switch set: ESFM_L2_PASS=bf16x3 (l2_knn_bf16_kernel +
    l2_rescan64_pairs: the whole L2 battery at 64 floats with the audit, seams at its fold groups, steps and tiles), ESFM_L2_PASS=f32
    (the 64-float form of the f32 MFMA kernel + l2_rescan64_kernel: the same) and ESFM_HM_PASS=i8 (the byte-per-bit kernel: the
    Hamming battery at 32 bytes).  A child that ends on a signal or at its timeout fails the test with its output."""
    env = dict(os.environ, **{switch: value})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spread = CLUSTER_SPREAD.get(value, 1e-5)
    seams = {"bf16x3": BF16X3_SEAMS, "f32": F32_SEAMS}.get(value, [0])
    out = subprocess.run([sys.executable, "-c", _CHILD, value, repr(spread), ",".join(str(s) for s in seams)], cwd=root, env=env,
                         capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
