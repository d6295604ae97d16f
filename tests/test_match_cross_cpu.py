"""Cross-check matching (esfm_match_cross_*, include/esfm.h "Cross-check matching") without a GPU: the ABI surface, no CPU
fallback, the rule itself on hand-built 2-NN tables, and the drivers' refusal of an unknown match filter.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROSS_SYMBOLS = ("esfm_match_cross_l2_f32", "esfm_match_cross_hamming", "esfm_match_cross_pairs_dev", "esfm_match_cross_pairs")


def ratio_ok(idx, dist, ratio):
    """The predicate of ratio_compact_pair on a 2-NN table (-3 in slot 1: proved to pass), in double."""
    idx = np.asarray(idx, np.int32).reshape(-1, 2); dist = np.asarray(dist, np.float32).reshape(-1, 2)
    i0, i1 = idx[:, 0], idx[:, 1]
    return (i0 >= 0) & ((i1 == -3) | ((i1 >= 0) & (dist[:, 0].astype(np.float64) < ratio * dist[:, 1].astype(np.float64))))


def cross_rule(fidx, fdist, ridx, rdist, ratio=None):
    """The strict rule: query q emits (q, F(q), d0) iff F(q) >= 0 and R(F(q)) == q (ratio: and ratio_ok on the forward row q and
    the reverse row F(q)).  fidx / fdist: the forward 2-NN table [nq, 2], ridx / rdist the reverse one [nt, 2]."""
    fidx = np.asarray(fidx, np.int32).reshape(-1, 2); fdist = np.asarray(fdist, np.float32).reshape(-1, 2)
    ridx = np.asarray(ridx, np.int32).reshape(-1, 2); rdist = np.asarray(rdist, np.float32).reshape(-1, 2)
    nq, nt = len(fidx), len(ridx)
    f = fidx[:, 0]
    ok = (f >= 0) & (f < nt)
    fc = np.where(ok, f, 0)
    if nt:
        ok &= ridx[fc, 0] == np.arange(nq)
        if ratio is not None:
            ok &= ratio_ok(fidx, fdist, ratio) & ratio_ok(ridx, rdist, ratio)[fc]
    q = np.nonzero(ok)[0]
    return q.astype(np.int32), f[q].astype(np.int32), fdist[q, 0].astype(np.float32)


def opencv_style_cross(fidx, ridx):
    """What a 'keep, for each train row, the query whose nearest it is' cross-check returns: q -> t for every t with R(t) = q,
    the closest such t (not always a mutual pair).  Only used to show where the strict rule differs."""
    out = {}
    for t, (q, _) in enumerate(np.asarray(ridx).reshape(-1, 2)):
        if q >= 0:
            out.setdefault(int(q), []).append(t)
    return out


def test_cross_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "esfm.h")).read()
    from easysfm_amd._lib import EXPORTED_SYMBOLS
    for s in CROSS_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in EXPORTED_SYMBOLS, s
    for cite in ("feature_match.py:24-27", "SURVEY.md:196"):
        assert cite in hdr, cite
    import easysfm_amd as E
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = E.lib()
    for s in CROSS_SYMBOLS:
        assert hasattr(L, s), s
    from easysfm_amd import _lib
    assert _lib.K_CROSS_CHECK == 14


def test_cross_entry_points_have_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import easysfm_amd as E
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    q = np.zeros((3, 64), np.float32); t = np.zeros((4, 64), np.float32)
    for call in (lambda: E.match_cross_l2(q, t), lambda: E.match_cross_l2(q, t, 0.8),
                 lambda: E.match_cross_hamming(np.zeros((3, 32), np.uint8), np.zeros((4, 32), np.uint8)),
                 lambda: E.match_cross_pairs_host([q, t], [(0, 1)], 0.5)):
        with pytest.raises(E.EsfmError) as ei:
            call()
        assert ei.value.status == -2, ei.value          # ESFM_ERR_NO_DEVICE: the context cannot be created


def test_rule_on_hand_built_tables():
    # forward: 4 queries over 3 train rows; reverse: 3 train rows over 4 queries
    fidx = [[1, 0], [1, 2], [-1, -1], [2, 1]]
    fdist = [[1.0, 3.0], [2.0, 2.5], [np.finfo(np.float32).max] * 2, [0.5, 4.0]]
    ridx = [[1, 0], [0, 1], [3, 0]]
    rdist = [[1.5, 2.0], [1.0, 2.0], [0.5, 3.0]]
    q, t, d = cross_rule(fidx, fdist, ridx, rdist)
    assert q.tolist() == [0, 3] and t.tolist() == [1, 2] and d.tolist() == [1.0, 0.5]
    # ratio+cross at 0.5: q0 passes its own test (1.0 < 1.5) but t1 fails the reverse one (1.0 < 0.5 * 2.0 is false)
    q, t, d = cross_rule(fidx, fdist, ridx, rdist, 0.5)
    assert q.tolist() == [3]
    # -3 (proved) passes whatever slot 1's distance says; -2 (screened) never passes
    q, _, _ = cross_rule([[0, -3]], [[5.0, 1.0]], [[0, -3]], [[5.0, 1.0]], 0.5)
    assert q.tolist() == [0]
    q, _, _ = cross_rule([[-2, -2]], [[1.0, 1.0]], [[0, 1]], [[1.0, 9.0]])
    assert q.tolist() == []
    # one train row / one query row: cross alone still emits
    q, t, _ = cross_rule([[0, -1]], [[1.0, np.finfo(np.float32).max]], [[0, -1]], [[1.0, np.finfo(np.float32).max]])
    assert q.tolist() == [0] and t.tolist() == [0]
    q, _, _ = cross_rule([[0, -1]], [[1.0, np.finfo(np.float32).max]], [[0, -1]], [[1.0, np.finfo(np.float32).max]], 0.8)
    assert q.tolist() == []                    # no second neighbour in either direction: the ratio test cannot pass
    # empty sides
    assert len(cross_rule(np.zeros((0, 2)), np.zeros((0, 2)), [[-1, -1]], [[0, 0]])[0]) == 0
    assert len(cross_rule([[-1, -1]], [[0, 0]], np.zeros((0, 2)), np.zeros((0, 2)))[0]) == 0


def test_strict_rule_differs_from_opencv_style():
    """F(q) = t1, R(t1) = q' != q, R(t2) = q: the one-sided 'closest train row whose nearest query is q' would pair q with t2;
    the strict rule emits nothing for q."""
    q_, q2 = 0, 1
    fidx = [[1, 2], [1, 0]]                 # F(0) = t1, F(1) = t1
    fdist = [[1.0, 1.2], [0.5, 3.0]]
    ridx = [[1, 0], [1, 0], [0, 1]]         # R(t0) = 1, R(t1) = 1 (= q'), R(t2) = 0 (= q)
    rdist = [[2.0, 3.0], [0.5, 1.0], [1.2, 4.0]]
    q, t, _ = cross_rule(fidx, fdist, ridx, rdist)
    assert q.tolist() == [q2] and t.tolist() == [1]
    assert q_ not in q.tolist()
    assert opencv_style_cross(fidx, ridx)[q_] == [2]          # what the one-sided rule would have kept for q


@pytest.mark.parametrize("driver", ["python", "native"])
def test_drivers_reject_an_unknown_match_filter(tmp_path, driver):
    args = ["imgs", "list.txt", "K.txt", "none", str(tmp_path / "out.ply"), "S", "100", "1.0", "1", "0", "4", "1", "0", "mutual"]
    if driver == "python":
        cmd = [sys.executable, os.path.join(ROOT, "bin", "sfm")] + args
    else:
        exe = os.path.join(ROOT, "bin", "sfm_native")
        if not os.path.exists(exe):
            import easysfm_amd as E
            if not os.path.exists(E.LIB_PATH):
                import __graft_entry__ as g
                g.build()
            exe = str(tmp_path / "sfm_native")
            cmd = ["g++", "-O2", "-std=c++17", os.path.join(ROOT, "easysfm_amd", "host", "sfm_main.cpp"), "-o", exe,
                   os.path.join(ROOT, "easysfm_amd", "libesfm_hip.so"), "-lz", "-Wl,-rpath," + os.path.join(ROOT, "easysfm_amd"),
                   "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 0, r.stdout
        cmd = [exe] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2, r.stdout[-2000:]
    assert "match_filter" in r.stdout
    assert not (tmp_path / "out.ply").exists()
