"""The bundle-adjustment problems with free radial distortion that tests/test_ba_radial_gpu.py solves on the GPU, and the numpy
reference's solve of each (tests/ba_radial_ref.py), computed once per process and shared: tests/test_ba_radial_cpu.py checks on the
CPU that every accept / reject and every Armijo decision of these traces is far from a tie, the GPU tests compare against them.

Scenes are synth.ba_scene shapes whose cameras project with the TRUE pinhole intrinsics of their group; the observations are then
passed through the group's TRUE radial model (ba_radial_ref.distort_observations).  The solve starts every group a few percent off
its true pinhole model and at k1 = k2 = 0."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from easysfm_amd import synth

import ba_groups_cases as gcases
import ba_radial_ref as ref

K0 = gcases.K0
MODELS, STARTS = gcases.MODELS, gcases.STARTS
# true k1, k2 of group g
RADIAL_TRUE = np.array([[-0.12, 0.03], [0.05, 0.0], [-0.05, 0.01], [0.08, -0.02], [-0.02, 0.0], [0.03, 0.01]])

# name; scene shape and seed; camera -> group; number of groups; half widths of the pinhole and of the radial box per group; LM
# iterations; Cauchy scale (<= 0: squared loss); reference camera; what else is done to the scene
Case = namedtuple("Case", "name n_real n_pt per seed grp G tol rtol iters cauchy_a ref_cam edit")


def _alt(n):
    return tuple(c % 2 for c in range(n))


def _two(name, n_real, n_pt, per, seed):
    return Case(name, n_real, n_pt, per, seed, _alt(n_real), 2, (100.0, 100.0), (1.0, 1.0), 3, 0.5, -1, None)


CASES = [
    # the smallest problem: one group (the grouped kernels all the same), 3 cameras, tracks of length 2
    Case("one3", 3, 60, 2, 41, (0, 0, 0), 1, (100.0,), (1.0,), 4, 0.5, -1, None),
    # every point seen by both groups: the 6 x 6 group-by-group cross blocks
    Case("two6", 6, 200, 4, 43, _alt(6), 2, (100.0, 100.0), (1.0, 1.0), 4, 0.5, -1, None),
    Case("own5", 5, 300, 4, 5, tuple(range(5)), 5, (100.0,) * 5, (1.0,) * 5, 4, 0.5, -1, None),
    # G = 3 with no camera in group 2
    Case("unobserved", 6, 200, 4, 46, _alt(6), 3, (100.0,) * 3, (1.0,) * 3, 4, 0.5, -1, None),
    # a radial box of 1e-3 in group 0 only (true k1 = -0.12): a bound of that group becomes active, the Armijo search contracts and
    # two steps are rejected.  (Seeds 427 and 403, not the 402 and 465 of the grouped cases: with those the reference's search runs
    # 12 and 13 contractions, to where the Armijo test is decided by 1e-11 of the cost -- a coin flip between two correct
    # implementations; test_ba_radial_cpu.py::test_no_decision_is_near_a_tie holds every case to 1e-9.)
    Case("tight", 4, 120, 3, 427, _alt(4), 2, (100.0, 100.0), (1e-3, 1.0), 8, 0.5, -1, None),
    Case("ref_squared", 5, 80, 4, 403, _alt(5), 2, (10.0, 10.0), (1.0, 1.0), 8, -1.0, 0, "reference_frame"),
    # point 0 on the optical axis of the held reference camera: x = y = 0 exactly, both k columns of that observation are zero
    Case("axis", 5, 80, 4, 466, _alt(5), 2, (100.0, 100.0), (1.0, 1.0), 4, 0.5, 0, "on_axis"),
    # the boundaries of the size-dependent kernel forms with two groups (n_cam = n_real + 2), 3 iterations each
    _two("r27", 27, 1500, 5, 327), _two("r28", 28, 1500, 5, 328), _two("r30", 30, 1500, 5, 330), _two("r31", 31, 1500, 5, 331),
    _two("r111", 111, 4000, 6, 111), _two("r112", 112, 4000, 6, 112),
    _two("r538", 538, 6000, 6, 538), _two("r539", 539, 6000, 6, 539),
    _two("r27_obs_2p20", 27, 131072, 8, 27),
]
CASE_BY_NAME = {c.name: c for c in CASES}

Built = namedtuple("Built", "sc grp calib_true calib0 tol radial_true radial0 rtol")


@lru_cache(maxsize=2)          # (the big scenes are 1M observations: two at a time)
def build(name):
    case = CASE_BY_NAME[name]
    grp = np.array(case.grp, np.int32)
    calib_true = K0[None, :] * MODELS[np.arange(case.G) % len(MODELS)]
    radial_true = RADIAL_TRUE[np.arange(case.G) % len(RADIAL_TRUE)]
    big = case.n_real > 100
    kw = dict(outlier_frac=0.0) if case.edit in ("reference_frame", "on_axis") else {}
    sc = synth.ba_scene(case.n_real, case.n_pt, case.per, radius=20.0 if big else 5.0, extent=8.0 if big else 2.0, seed=case.seed,
                        K4_per_cam=calib_true[grp], **kw)
    uv = ref.distort_observations(sc.uv, sc.K4.astype(np.float64)[sc.cam_idx], radial_true[grp[sc.cam_idx]])
    calib0 = calib_true * STARTS[np.arange(case.G) % 2]
    cams0, pts0, cams_gt, pts_gt = sc.cams0, sc.pts0, sc.cams_gt, sc.pts_gt
    if case.edit in ("reference_frame", "on_axis"):
        moved = synth.in_reference_frame(sc, case.ref_cam)
        cams0, pts0, cams_gt, pts_gt = moved.cams0, moved.pts0, moved.cams_gt, moved.pts_gt
    if case.edit == "on_axis":
        k = int(np.nonzero(sc.cam_idx == case.ref_cam)[0][0])         # an observation of the reference camera: its point goes on the axis
        pts0 = pts0.copy(); pts0[sc.pt_idx[k]] = [0.0, 0.0, float(pts0[sc.pt_idx[k], 2])]
    sc = synth.BAScene(cam_idx=sc.cam_idx, pt_idx=sc.pt_idx, uv=uv, K4=sc.K4, cams0=cams0, pts0=pts0, cams_gt=cams_gt, pts_gt=pts_gt)
    return Built(sc, grp, calib_true, calib0, np.array(case.tol, np.float64), radial_true, np.zeros((case.G, 2)), np.array(case.rtol, np.float64))


def problem(name, radial=True):
    case, b = CASE_BY_NAME[name], build(name)
    return ref.Problem(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, b.grp, b.sc.cams0, b.sc.pts0, b.calib0, b.tol, b.radial0, b.rtol, case.ref_cam, 1e-10,
                       case.cauchy_a, radial=radial)


@lru_cache(maxsize=None)
def reference(name):
    """(cams, pts, block [G, 6], log) of the numpy reference's solve; read-only for every test that shares it"""
    P = problem(name)
    x, log = ref.solve(P, CASE_BY_NAME[name].iters, "schur")
    cams, pts, blk = P.split(x)
    for a in (cams, pts, blk):
        a.setflags(write=False)
    return cams, pts, blk, log
