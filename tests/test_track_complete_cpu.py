"""Track completion without a GPU (esfm.h "Track completion"): the host build of easysfm_amd/csrc/complete_core.hpp
(esfm_track_complete_host) against the brute-force restatement (tests/complete_ref.py), bit for bit, on the shared cases of
tests/complete_cases.py; the properties the contract promises; the argument rules; and what the operation is for, on the purpose
scene."""
import ctypes as C

import numpy as np
import pytest

import complete_cases as cases
import complete_ref as R

FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def E():
    import easysfm_amd
    return easysfm_amd


def host(E, case):
    return E.track_complete(*case["args"], E.TrackCompleteOptions(**case["opts"]), host=True)


@pytest.fixture(scope="module")
def purpose():
    """the purpose scene and the restatement's answer to it, computed once"""
    case = cases.purpose_scene()
    return case, R.run_case(case)


def test_default_options(E):
    s = E._lib.TrackCompleteOptionsStruct()
    E.lib().esfm_track_complete_options_default(s)
    d = E.TrackCompleteOptions()
    assert (s.search_radius_px, s.max_distance, s.ratio, s.max_refs) == (4.0, np.inf, 0.8, 8)
    assert (d.search_radius_px, d.max_distance, d.ratio, d.max_refs) == (4.0, np.inf, 0.8, 8)


@pytest.mark.parametrize("case", cases.exact_cases(), ids=lambda c: c["name"])
def test_host_equals_restatement(E, case):
    R.assert_same(host(E, case), R.run_case(case), case["name"])


def test_many_jobs(E):
    case = cases.many_jobs()
    ref = R.run_case(case)
    assert ref.stats[0] == case["n_jobs"] > 65536
    R.assert_same(host(E, case), ref)


def test_what_the_cases_are_for():
    """the restatement's answers to the hand-made cases say what the case is named for"""
    five_below = float(np.nextafter(np.float64(5.0), 0.0))
    run = R.run_case
    assert run(cases.radius_edge(5.0)).kp_point.tolist() == [-1, 0] and run(cases.radius_edge(five_below)).kp_point.tolist() == [-1, -1]
    cb = run(cases.cell_borders(4.0))
    assert cb.kp_point[7 + 3] == 0 and cb.kp_point[7 + 6] == 1 and cb.kp_point[7 + 7] == 2 and cb.kp_point[7 + 5] == 3 and cb.kp_point[7 + 8] == 5
    assert cb.kp_point[7 + 10] == 6 and cb.kp_point[7 + 14] == -1 and not np.any(cb.kp_point == 4)
    nj = run(cases.no_jobs())
    assert nj.kp_point.tolist() == [-1] * 5 + [-1, -1, -1, -1, -1, 4] and nj.stats.tolist() == [1, 1, 0, 1]
    assert run(cases.non_free_ignored()).kp_point.tolist() == [-1, -1, 0]
    assert run(cases.tie(0.5)).stats.tolist() == [1, 0, 0, 0] and run(cases.tie(1.0)).stats.tolist() == [1, 0, 0, 0]
    t = run(cases.tie(1.5))
    assert t.kp_point.tolist() == [-1, -1, 0, -1] and t.kp_dist[2] == 5.0
    for hamming in (False, True):
        assert run(cases.gate(5.0, hamming)).kp_point[1] == 0 and run(cases.gate(five_below, hamming)).kp_point[1] == -1
    for n in (2, 3):
        d = run(cases.conflict(n, False)); e = run(cases.conflict(n, True))
        assert d.kp_point[n] == n - 1 and e.kp_point[n] == 0                       # the nearest; of equals the lowest index
        assert d.stats.tolist() == e.stats.tolist() == [n, n, n - 1, 1] and np.all(d.kp_point[n + 1:] == -1) and np.all(e.kp_point[n + 1:] == -1)
    assert [int(run(cases.references(n)).stats[3]) for n in (1, 2, 8, 9)] == [1, 1, 1, 0]
    assert run(cases.references(2, 1)).stats[3] == 0 and run(cases.references(9, 1)).stats[3] == 0
    for n in (1, 63, 64, 65, 300):
        assert run(cases.crowded(n)).stats[0] == 1
    for c in (cases.job_count(3, 2, in_all=True), cases.job_count(1, 1), cases.job_count(128, 2), cases.job_count(257, 1)):
        assert run(c).stats[0] == c["n_jobs"]
    assert run(cases.none_free()).stats.tolist() == [0, 0, 0, 0] and run(cases.no_points()).stats.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("what", ["point", "Rt", "keypoint", "descriptor"])
def test_nan_takes_no_part(E, what):
    """the affected rows and points take no part; everything else is as in the clean scene -- in the host form's answers"""
    clean, dirty = cases.small(), cases.with_nan(what)
    a, b = host(E, clean), host(E, dirty)
    R.assert_same(a, R.run_case(clean)); R.assert_same(b, R.run_case(dirty))
    off = clean["args"][3]
    if what == "point":
        hit = np.isin(a.kp_point, (3, 11))
        assert not np.any(np.isin(b.kp_point, (3, 11)))
    elif what == "Rt":
        hit = np.zeros(len(a.kp_point), bool); hit[off[2]:off[3]] = True
        assert np.all(b.kp_point[hit] == -1)
    elif what == "keypoint":
        hit = ~np.isfinite(dirty["args"][1]).all(axis=1)
        assert hit.any() and np.all(b.kp_point[hit] == -1)
    else:
        hit = np.isnan(dirty["args"][0]).any(axis=1) | np.isin(a.kp_point, (0, 7))
        assert np.all(b.kp_point[np.isnan(dirty["args"][0]).any(axis=1)] == -1) and not np.any(b.kp_point == 0)
    assert np.count_nonzero(a.kp_point >= 0) > 20
    assert np.array_equal(a.kp_point[~hit], b.kp_point[~hit]) and np.array_equal(a.kp_dist[~hit], b.kp_dist[~hit])


def check_properties(E, case, res, evaluate_host=True):
    """no keypoint twice (one entry per row), no point twice in a camera, every assignment on a free row and a track_evaluate inlier
    at the search radius, and nothing more after the assignments are applied"""
    desc, kp, free, off, K4, Rt, X, cam, pt, ok = case["args"]
    rows = np.nonzero(res.kp_point >= 0)[0]
    cams = np.searchsorted(off, rows, side="right") - 1
    pairs = np.stack([cams, res.kp_point[rows]], 1)
    assert len(np.unique(pairs, axis=0)) == len(pairs)
    assert np.all(np.asarray(free)[rows] != 0)
    have = set(zip(cam.tolist(), pt.tolist()))
    assert not any((int(c), int(p)) in have for c, p in pairs)
    # judged with the track they join (a track of one observation has no verdict): the new observations go behind the old ones
    old_rows = np.asarray(off)[cam] + ok
    ev = E.track_evaluate(np.concatenate([cam, cams]).astype(np.int32), np.concatenate([pt, res.kp_point[rows]]).astype(np.int32),
                          np.asarray(kp)[np.concatenate([old_rows, rows])], K4, Rt, X,
                          E.TrackOptions(max_reproj_error_px=case["opts"]["search_radius_px"]), host=evaluate_host)
    assert np.all(ev.obs_inlier[len(cam):])
    return R.apply(case, res)


def test_purpose_scene(E, purpose):
    """Conditions, not measurements: every assignment is a withheld true observation, every withheld observation is recovered
    (720 of them for the committed seed), every assignment is an inlier at 4 px, and a second call after applying returns nothing."""
    case, ref = purpose
    got = host(E, case)
    R.assert_same(got, ref)
    rows = np.nonzero(got.kp_point >= 0)[0]
    print(f"purpose scene: {len(case['withheld'])} withheld, {len(rows)} assigned, stats {got.stats.tolist()}")
    assert np.array_equal(got.kp_point[rows], case["truth"][rows])                      # no wrong one (clutter has truth -1)
    assert np.array_equal(rows, np.sort(case["withheld"])) and len(rows) > 600         # all of them, and nothing else
    again = check_properties(E, case, got)
    second = host(E, again)
    assert np.all(second.kp_point == -1) and np.all(second.kp_dist == FLT_MAX) and second.stats[1:].tolist() == [0, 0, 0]


def test_properties_on_small_scenes(E):
    for case in [cases.small()] + cases.widths()[:2] + [cases.crowded(65), cases.conflict(3, False)]:
        got = host(E, case)
        again = check_properties(E, case, got)
        assert np.all(host(E, again).kp_point == -1), case["name"]


def _raw(E, case, entry=None, **change):
    """esfm_track_complete_host (or `entry`, a form with the same arguments) through ctypes with one argument replaced: (status,
    whether the outputs are untouched)"""
    desc, kp, free, off, K4, Rt, X, cam, pt, ok = [np.ascontiguousarray(a) for a in case["args"]]
    X = np.ascontiguousarray(X, np.float64); Rt = np.ascontiguousarray(Rt, np.float64)
    opt = E.TrackCompleteOptions(**case["opts"]).struct()
    for k in ("search_radius_px", "max_distance", "ratio", "max_refs"):
        if k in change:
            setattr(opt, k, change.pop(k))
    kp_point = np.full(len(kp), 77, np.int32); kp_dist = np.full(len(kp), 7.0, np.float32); stats = np.full(4, 7, np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    args = dict(metric=1 if desc.dtype == np.uint8 else 0, desc=ptr(desc), kp=ptr(kp), kp_free=ptr(free), off=ptr(off), n_cam=len(K4),
                width=desc.shape[1], K4=ptr(K4), Rt=ptr(Rt), n_pt=len(X), xyz=ptr(X), n_obs=len(cam), cam=ptr(cam), pt=ptr(pt), ok=ptr(ok),
                opt=C.byref(opt), kp_point=ptr(kp_point), kp_dist=ptr(kp_dist), stats=ptr(stats))
    keep = []
    for k, v in change.items():
        if isinstance(v, np.ndarray):
            keep.append(np.ascontiguousarray(v)); v = ptr(keep[-1])
        args[k] = v
    rc = (entry or E.lib().esfm_track_complete_host)(*args.values())
    untouched = np.all(kp_point == 77) and np.all(kp_dist == 7.0) and np.all(stats == 7)
    return rc, untouched


def invalid_changes(case):
    """one change of _raw's arguments per argument rule of the contract"""
    desc, kp, free, off, K4, Rt, X, cam, pt, ok = case["args"]
    bad_cam = cam.copy(); bad_cam[5] = len(K4)
    bad_pt = pt.copy(); bad_pt[2] = -1
    bad_kp = ok.copy(); bad_kp[0] = off[cam[0] + 1] - off[cam[0]]
    bad_off = off.copy(); bad_off[2] = off[1] - 1
    return [dict(opt=None), dict(desc=None), dict(kp=None), dict(kp_free=None), dict(off=None), dict(K4=None), dict(Rt=None), dict(xyz=None),
            dict(cam=None), dict(pt=None), dict(ok=None), dict(kp_point=None), dict(kp_dist=None),
            dict(search_radius_px=0.0), dict(search_radius_px=-1.0), dict(search_radius_px=np.inf), dict(search_radius_px=np.nan),
            dict(ratio=np.nan), dict(max_distance=np.nan), dict(max_refs=0), dict(max_refs=9),
            dict(cam=bad_cam), dict(pt=bad_pt), dict(ok=bad_kp), dict(off=bad_off), dict(width=0), dict(metric=2), dict(n_pt=-1)]


def test_invalid_arguments(E):
    case = cases.small()
    assert _raw(E, case) == (0, False)
    for ch in invalid_changes(case):
        assert _raw(E, case, **ch) == (-1, True), ch
    ham = cases.widths()[-1]
    for w in (8, 24, 63):
        assert _raw(E, ham, width=w) == (-1, True), w
    assert _raw(E, case, stats=None)[0] == 0                                     # stats may be NULL
