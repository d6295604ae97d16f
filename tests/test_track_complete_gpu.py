"""Track completion on the MI355X (esfm.h "Track completion"): esfm_track_complete and esfm_track_complete_dev against the
brute-force restatement (tests/complete_ref.py), bit for bit (kp_point, kp_dist, stats), on the shared cases of
tests/complete_cases.py; two runs identical; the promised properties and the purpose scene; the kernel timers."""
import ctypes as C

import numpy as np
import pytest

import complete_cases as cases
import complete_ref as R
from test_track_complete_cpu import _raw as raw, check_properties, invalid_changes

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def E():
    import easysfm_amd
    return easysfm_amd


def device(E, ctx, case):
    return E.track_complete(*case["args"], E.TrackCompleteOptions(**case["opts"]), ctx)


def device_resident(E, ctx, case):
    """esfm_track_complete_dev: descriptors, keypoints and the three outputs in device memory"""
    import torch
    desc, kp, free, off, K4, Rt, X, cam, pt, ok = [np.ascontiguousarray(a) for a in case["args"]]
    free = free.astype(np.uint8); X = np.ascontiguousarray(X, np.float64); Rt = np.ascontiguousarray(Rt, np.float64)
    rows = len(kp)
    if rows == 0:
        desc = np.zeros((1, desc.shape[1]), desc.dtype); kp = np.zeros((1, 2), np.float32)        # (no empty device tensors)
    d_desc = torch.from_numpy(desc).cuda(); d_kp = torch.from_numpy(kp).cuda()
    d_point = torch.full((max(rows, 1),), 77, dtype=torch.int32, device="cuda"); d_dist = torch.full((max(rows, 1),), 7.0, dtype=torch.float32, device="cuda")
    d_stats = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    opt = E.TrackCompleteOptions(**case["opts"]).struct()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    dev = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    E._lib.check(E.lib().esfm_track_complete_dev(ctx.handle, 1 if desc.dtype == np.uint8 else 0, dev(d_desc), dev(d_kp), ptr(free), ptr(off), len(K4),
                                                 desc.shape[1], ptr(K4), ptr(Rt), len(X), ptr(X), len(cam), ptr(cam), ptr(pt), ptr(ok), C.byref(opt),
                                                 dev(d_point), dev(d_dist), dev(d_stats)))
    ctx.synchronize()
    return E.TrackCompleteResult(d_point.cpu().numpy()[:rows], d_dist.cpu().numpy()[:rows], d_stats.cpu().numpy())


@pytest.fixture(scope="module")
def purpose():
    case = cases.purpose_scene()
    return case, R.run_case(case)


@pytest.mark.parametrize("case", cases.exact_cases(), ids=lambda c: c["name"])
def test_device_equals_restatement(E, gpu_ctx, case):
    ref = R.run_case(case)
    first = device(E, gpu_ctx, case)
    R.assert_same(first, ref, case["name"])
    R.assert_same(device(E, gpu_ctx, case), first, case["name"] + " (second run)")
    R.assert_same(device_resident(E, gpu_ctx, case), ref, case["name"] + " (_dev)")


def test_many_jobs(E, gpu_ctx):
    case = cases.many_jobs()
    ref = R.run_case(case)
    assert ref.stats[0] == case["n_jobs"] > 65536
    R.assert_same(device(E, gpu_ctx, case), ref)
    R.assert_same(device_resident(E, gpu_ctx, case), ref)


def test_purpose_scene(E, gpu_ctx, purpose):
    """as the CPU test's: every assignment a withheld true observation, every withheld observation recovered, every assignment a
    track_evaluate inlier at 4 px (judged on the device), nothing more on a second call after applying"""
    case, ref = purpose
    got = device(E, gpu_ctx, case)
    R.assert_same(got, ref)
    R.assert_same(device(E, gpu_ctx, case), got, "second run")
    R.assert_same(device_resident(E, gpu_ctx, case), ref, "_dev")
    rows = np.nonzero(got.kp_point >= 0)[0]
    assert np.array_equal(got.kp_point[rows], case["truth"][rows])
    assert np.array_equal(rows, np.sort(case["withheld"])) and len(rows) > 600
    again = check_properties(E, case, got, evaluate_host=False)
    second = device(E, gpu_ctx, again)
    assert np.all(second.kp_point == -1) and np.all(second.kp_dist == FLT_MAX) and second.stats[1:].tolist() == [0, 0, 0]


def test_kernel_timers(E, gpu_ctx, purpose):
    case, ref = purpose
    ids = (E._lib.K_COMPLETE_GRID, E._lib.K_COMPLETE_JOBS, E._lib.K_COMPLETE_SEARCH)
    gpu_ctx.set_kernel_timing(True)
    try:
        for k in ids:
            gpu_ctx.kernel_time(k)
        R.assert_same(device(E, gpu_ctx, case), ref)
        times = [gpu_ctx.kernel_time(k) for k in ids]
    finally:
        gpu_ctx.set_kernel_timing(False)
    print("track completion, purpose scene: grid %.3f ms, jobs %.3f ms, search %.3f ms" % tuple(t[0] for t in times))
    assert [t[1] for t in times] == [1, 2, 1] and all(t[0] > 0 for t in times)


def test_invalid_arguments_leave_outputs(E, gpu_ctx):
    """every argument rule of the contract (the CPU test's list), through esfm_track_complete and through esfm_track_complete_dev:
    ESFM_ERR_INVALID_ARG, and the outputs -- the caller's arrays, the device arrays of the _dev form -- are as they were"""
    import torch
    case = cases.small()
    ham = cases.widths()[-1]

    def host_pointers(*a):
        return E.lib().esfm_track_complete(gpu_ctx.handle, *a)

    def resident(case, kept):
        """esfm_track_complete_dev behind _raw's arguments: device copies stand in for the descriptors, keypoints and outputs that
        are not NULL; kept[-1] says whether the device outputs still hold what they were filled with"""
        rows = len(case["args"][1])
        d_desc = torch.from_numpy(np.ascontiguousarray(case["args"][0])).cuda(); d_kp = torch.from_numpy(np.ascontiguousarray(case["args"][1])).cuda()
        d_point = torch.full((rows,), 77, dtype=torch.int32, device="cuda"); d_dist = torch.full((rows,), 7.0, dtype=torch.float32, device="cuda")
        d_stats = torch.full((4,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        dev = lambda given, t: C.c_void_p(t.data_ptr()) if given else None   # noqa: E731

        def entry(metric, desc, kp, *rest):
            *mid, kp_point, kp_dist, stats = rest
            rc = E.lib().esfm_track_complete_dev(gpu_ctx.handle, metric, dev(desc, d_desc), dev(kp, d_kp), *mid, dev(kp_point, d_point),
                                                 dev(kp_dist, d_dist), dev(stats, d_stats))
            gpu_ctx.synchronize()
            kept.append(bool(torch.all(d_point == 77)) and bool(torch.all(d_dist == 7.0)) and bool(torch.all(d_stats == 7)))
            return rc
        return entry

    assert raw(E, case, entry=host_pointers) == (0, False)
    for ch in invalid_changes(case):
        assert raw(E, case, entry=host_pointers, **ch) == (-1, True), ch
    for w in (8, 24, 63):
        assert raw(E, ham, entry=host_pointers, width=w) == (-1, True), w
    kept = []
    assert raw(E, case, entry=resident(case, kept))[0] == 0 and kept == [False]
    for ch in invalid_changes(case):
        kept = []
        assert raw(E, case, entry=resident(case, kept), **ch)[0] == -1 and kept == [True], ch
    for w in (8, 24, 63):
        kept = []
        assert raw(E, ham, entry=resident(ham, kept), width=w)[0] == -1 and kept == [True], w
