"""Image retrieval without a GPU (esfm.h "Image retrieval"): what the rule list retrieves, on the restatement (tests/retrieval_ref.py);
the host-only pair list against the restatement; option defaults and argument checks; the stand-alone program over
easysfm_amd/csrc/retrieval_host.hpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import retrieval_cases as cases
import retrieval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E():
    import easysfm_amd
    return easysfm_amd


@pytest.mark.parametrize("n_centres", [8, 16, 64])
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_corridor_retrieval(seed, n_centres):
    """kmeans_iterations 10, top_k 4: no selected neighbour shares zero scene points with its query, and image 23's table holds
    image 1.  The margin is printed: the lowest score of a pair sharing >= 90 points minus the highest of a pair sharing none."""
    sets, ids = cases.corridor(seed)
    out = R.chain(sets, R.L2, R.Options(n_centres=n_centres, kmeans_iterations=10, top_k=4))
    n_chosen, n_none = cases.check_corridor(out["nearest"], out["scores"], ids)
    shared = cases.shared_points(ids)
    off = ~np.eye(len(ids), dtype=bool)
    margin = out["scores"][(shared >= 90) & off].min() - out["scores"][(shared == 0) & off].max()
    print(f"seed {seed}, {n_centres} centres: {n_none} of {n_chosen} neighbours share nothing, margin {margin:.3f}")


def table(rows, top_k):
    t = np.full((len(rows), top_k), -1, np.int32)
    for i, r in enumerate(rows):
        t[i, :len(r)] = r
    return t


PAIR_LIST_CASES = {
    "window_alone": (5, None, 2),
    "padding": (4, table([[1], [], [0, 1], [2]], 2), 0),
    "both_directions": (4, table([[1, 2], [0, 3], [0, 1], [1, 0]], 2), 1),
    "window_beyond_n": (4, table([[3], [], [], []], 1), 9),
    "one_set": (1, table([[]], 3), 2),
    "capacity_reached": (3, table([[1, 2], [0, 2], [0, 1]], 2), 0),
}


@pytest.mark.parametrize("name", sorted(PAIR_LIST_CASES))
def test_pair_list(E, name):
    n, nearest, window = PAIR_LIST_CASES[name]
    want = R.pair_list(nearest, n, window)
    got = E.retrieval_pair_list(nearest, n, window)
    assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)
    assert np.all(got[:, 0] > got[:, 1]) if len(got) else True
    if name == "window_alone":
        assert [tuple(p) for p in got] == [(1, 0), (2, 0), (2, 1), (3, 1), (3, 2), (4, 2), (4, 3)]
    if name == "one_set":
        assert len(got) == 0
    if name == "window_beyond_n":
        assert len(got) == 6                                  # every pair of four images


def test_pair_list_exact_capacity(E):
    """a cycle 0 -> 1 -> 2 -> 0 names three different pairs with top_k = 1: the list fills its capacity of n_sets * (top_k + window)
    exactly, and nothing is written behind it"""
    L = E.lib()
    n, top_k, window = 3, 1, 0
    nearest = table([[1], [2], [0]], 1)
    cap = n * (top_k + window)
    buf = np.full((cap + 1, 2), -7, np.int32)
    cnt = C.c_int32(-1)
    assert L.esfm_retrieval_pair_list(n, top_k, C.c_void_p(nearest.ctypes.data), window, C.c_void_p(buf.ctypes.data), C.byref(cnt)) == 0
    want = R.pair_list(nearest, n, window)
    assert cnt.value == len(want) == cap and np.array_equal(buf[:cap], want) and np.all(buf[cap:] == -7)
    full = table([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], 3)   # all 6 pairs, each named twice
    assert np.array_equal(E.retrieval_pair_list(full, 4, 0), R.pair_list(full, 4, 0))


def test_pair_list_rejects_bad_tables(E):
    for bad in (table([[1], [2]], 1), table([[0], [0]], 1), table([[-2], [0]], 1)):   # out of range; names its own row; below -1
        with pytest.raises(E.EsfmError) as ei:
            E.retrieval_pair_list(bad, 2, 0)
        assert ei.value.status == -1
    with pytest.raises(E.EsfmError):
        E.retrieval_pair_list(None, 3, -1)


def test_default_options(E):
    s = E._lib.RetrievalOptionsStruct(-1, -1, -1, -1, -1, -1)
    E.lib().esfm_retrieval_options_default(s)
    assert (s.n_centres, s.kmeans_iterations, s.max_train, s.top_k, s.window, s.reserved) == (64, 10, 65536, 10, 0, 0)
    d, r = E.RetrievalOptions(), R.Options()
    assert (d.n_centres, d.kmeans_iterations, d.max_train, d.top_k, d.window) == (64, 10, 65536, 10, 0)
    assert d.struct().n_centres == r.n_centres and d.struct().top_k == r.top_k and d.struct().max_train == r.max_train
    hdr = open(os.path.join(ROOT, "include", "esfm.h")).read()
    assert "NOT been tuned on this project's data" in hdr


def test_invalid_arguments_write_nothing(E):
    """arguments are judged before the context is looked at: each case is ESFM_ERR_INVALID_ARG with its own message and untouched
    outputs, also here, where no context can exist"""
    L = E.lib()
    rows = np.ones((6, 4), np.float32)
    off = np.array([0, 2, 6], np.int32)
    down = np.array([0, 4, 2], np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731

    def opt(**kw):
        return E.RetrievalOptions(**kw).struct()

    bad = [(None, off, "options are NULL"), (opt(n_centres=0), off, "n_centres"), (opt(n_centres=257), off, "n_centres"),
           (opt(top_k=-1), off, "top_k"), (opt(), down, "decreases")]
    for o, offsets, word in bad:
        centres = np.full((257, 4), 7.0, np.float32); pairs = np.full((64, 2), -7, np.int32); n = C.c_int32(-7)
        o_arg = C.byref(o) if o is not None else None
        rc = L.esfm_retrieval_train(None, R.L2, ptr(rows), ptr(offsets), 2, 4, o_arg, ptr(centres))
        assert rc == -1 and word in L.esfm_last_error().decode(), (word, L.esfm_last_error())
        for fn in (L.esfm_retrieval_pairs, L.esfm_retrieval_pairs_dev):
            rc = fn(None, R.L2, ptr(rows), ptr(offsets), 2, 4, o_arg, ptr(pairs), C.byref(n))
            assert rc == -1 and word in L.esfm_last_error().decode(), (word, L.esfm_last_error())
        assert np.all(centres == 7.0) and np.all(pairs == -7) and n.value == -7
    # the stage calls' own arguments
    vlad = np.full((2, 8), 7, np.int8); norm2 = np.full(2, -7, np.int32)
    cen = np.zeros((2, 4), np.float32)
    assert L.esfm_retrieval_vlad(None, R.L2, ptr(rows), ptr(down), 2, 4, 2, ptr(cen), ptr(vlad), ptr(norm2), None, None) == -1
    assert L.esfm_retrieval_vlad(None, R.L2, ptr(rows), ptr(off), 2, 4, 0, ptr(cen), ptr(vlad), ptr(norm2), None, None) == -1
    assert L.esfm_retrieval_vlad(None, R.L2, ptr(rows), ptr(off), 2, 4, 2, None, ptr(vlad), ptr(norm2), None, None) == -1
    nearest = np.full((2, 1), -7, np.int32)
    assert L.esfm_retrieval_rank(None, 2, 8, ptr(vlad), -1, ptr(nearest), None, None) == -1
    assert L.esfm_retrieval_rank(None, 2, 8, None, 1, ptr(nearest), None, None) == -1
    assert np.all(vlad == 7) and np.all(norm2 == -7) and np.all(nearest == -7)
    # a value the fixed point cannot hold, and the limits
    huge = rows.copy(); huge[3, 1] = 20000.0
    nan = rows.copy(); nan[0, 0] = np.nan
    for r in (huge, nan):
        assert L.esfm_retrieval_train(None, R.L2, ptr(r), ptr(off), 2, 4, C.byref(opt()), ptr(centres)) == -1
        assert "16384" in L.esfm_last_error().decode()
    assert L.esfm_retrieval_train(None, R.L2, ptr(rows), ptr(np.zeros(3, np.int32)), 2, 4, C.byref(opt()), ptr(centres)) == -1   # total == 0
    assert L.esfm_retrieval_train(None, R.L2, ptr(rows), ptr(off), 2, 257, C.byref(opt()), ptr(centres)) == -1
    assert L.esfm_retrieval_train(None, R.HAMMING, ptr(rows), ptr(off), 2, 65, C.byref(opt()), ptr(centres)) == -1
    assert L.esfm_retrieval_train(None, R.L2, ptr(rows), ptr(off), 2, 256, C.byref(opt(n_centres=256)), ptr(centres)) == -5   # D = 65536
    # valid arguments reach the context check
    assert L.esfm_retrieval_train(None, R.L2, ptr(rows), ptr(off), 2, 4, C.byref(opt(n_centres=2)), ptr(centres)) == -1
    assert "ctx is NULL" in L.esfm_last_error().decode()


def test_without_a_device(E):
    """the device entry points need a context, and creating one still reports ESFM_ERR_NO_DEVICE: no CPU fallback (a gpu-marked test
    cannot check this)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    sets = cases.float_sets(3, 4, 1)
    calls = (lambda: E.retrieval_train(sets, R.L2, E.RetrievalOptions(n_centres=2)), lambda: E.select_pairs(sets, R.L2, E.RetrievalOptions(n_centres=2)),
             lambda: E.retrieval_vlad(sets, np.zeros((2, 4), np.float32)), lambda: E.retrieval_rank(np.zeros((3, 8), np.int8), 1))
    for call in calls:
        with pytest.raises(E.EsfmError) as ei:
            call()
        assert ei.value.status == -2, ei.value


def test_restatement_edges():
    """properties of the rule list that the GPU tests rely on, on the restatement alone"""
    assert list(R.sample_rows(10, 4)) == [0, 3, 6, 9] and list(R.sample_rows(10, 10)) == list(range(10)) and list(R.sample_rows(7, 100)) == list(range(7))
    # more centres than sample rows: duplicates, and the tie rule sends every row to the lower index; the empty centres keep their value
    sets = [np.array([[0.0], [1.0]], np.float32), np.array([[5.0]], np.float32)]
    m = R.train(sets, R.L2, R.Options(n_centres=6, kmeans_iterations=3))
    assert np.array_equal(m.reshape(-1), np.array([0, 0, 1, 1, 5, 5], np.float32))
    assert list(R.assign(R.working(np.concatenate(sets), R.L2), m)) == [0, 2, 4]
    # Hamming components are the bits, least significant first
    assert list(R.working(np.array([[0x05, 0x80]], np.uint8), R.HAMMING)[0]) == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    # rint is half-to-even and the largest entry maps to 127
    V, norm2, _, S = R.vlad([np.array([[4.0], [0.0]], np.float32)], R.L2, np.array([[1.0]], np.float32))
    assert S[0, 0] == 2 * 65536 and V[0, 0] == 127 and norm2[0] == 127 * 127
    # equal scores rank by index; a zero image is never selected and selects nothing
    nearest, dots, scores = R.rank(np.array([[1, 0], [0, 0], [2, 0], [1, 0]], np.int8), 3)
    assert [list(r) for r in nearest] == [[2, 3, -1], [-1, -1, -1], [0, 3, -1], [0, 2, -1]]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_host_code_stand_alone(tmp_path, flags):
    """tests/cpp/retrieval_check_main.cpp: retrieval_host.hpp compiled into a stand-alone program with g++ on the pair-list cases"""
    exe = str(tmp_path / "retrieval_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", *flags, os.path.join(ROOT, "tests", "cpp", "retrieval_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "retrieval check ok" in r.stdout, r.stdout[-4000:]
