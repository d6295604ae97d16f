"""Bundle adjustment with free radial distortion (k1, k2 per camera group), the parts that need no GPU.

tests/ba_radial_ref.py -- the numpy statement of the bounded LM loop with 6-wide blocks that judges the GPU in
tests/test_ba_radial_gpu.py -- is pinned here first: with its two radial columns switched off it IS tests/ba_groups_ref.py, to the
bit, on that module's cases; its analytic Jacobian agrees with central differences; on a noise-free scene it recovers fx, fy, k1, k2.
Every GPU case's reference trace is then checked to be far from a tie in each accept / reject and each Armijo decision.  Then the
host logic: the LDS rule of the grouped block-row kernel for radial problems, argument validation of the new C entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth
from easysfm_amd._lib import ESFM_ERR_INVALID_ARG, ESFM_ERR_NUMERIC

import ba_groups_cases as gcases
import ba_radial_cases as cases
import ba_radial_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")
K0 = np.array(synth.FOUNTAIN_K4, np.float64)


# ---- (a) radial columns off: the grouped reference, exactly ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "split", "own", "unobserved", "tight", "ref_squared", "g27"])
def test_radial_columns_off_is_the_grouped_reference_exactly(name):
    """k1 = k2 = 0 held out of the unknowns: every number of the iteration log and the final vector equal ba_groups_ref's, bit for bit,
    on that module's own cases (the small ones and the first of its form boundaries)."""
    case, b = gcases.CASE_BY_NAME[name], gcases.build(name)
    G = len(b.calib0)
    P = ref.Problem(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, b.grp, b.sc.cams0, b.sc.pts0, b.calib0, b.tol, np.zeros((G, 2)), 1.0, case.ref_cam, 1e-10,
                    case.cauchy_a, radial=False)
    x, log = ref.solve(P, case.iters, "schur")
    gc, gp, gk, glog = gcases.reference(name)
    assert x.tobytes() == np.concatenate([gc.ravel(), gp.ravel(), gk.ravel()]).tobytes()
    assert len(log) == len(glog)
    for e, g in zip(log, glog):
        assert e.keys() == g.keys()
        for key in e:
            assert e[key] == g[key], (key, e[key], g[key])


# ---- (b) the Jacobian against central differences ---------------------------------------------------------------------------------
def _jacobian_scene():
    """200 observations: random cameras (one on the small-angle branch), points in front of them, k of a few percent; observation 0
    sits on the optical axis of its camera (identity pose, point (0, 0, d)): r2 = 0"""
    rng = np.random.default_rng(77)
    n = 200
    cams = np.concatenate([0.3 * rng.standard_normal((n, 3)), 0.2 * rng.standard_normal((n, 3))], 1)
    pts = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), rng.uniform(3.0, 6.0, (n, 1))], 1)
    cams[0] = 0.0; pts[0] = [0.0, 0.0, 4.0]
    cams[1, :3] = [3e-9, -2e-9, 1e-9]
    calib6 = np.concatenate([K0[None, :] * np.array([[1.0, 1.0, 1.0, 1.0], [0.8, 1.01, 0.8, 0.99]]), [[-0.12, 0.03], [0.05, -0.01]]], 1)
    grp = (np.arange(n) % 2).astype(np.int64)
    idx = np.arange(n)
    uv = rng.uniform(0, 3000, (n, 2)).astype(np.float32)
    return cams, pts, calib6, grp, idx, uv


def test_jacobian_agrees_with_central_differences():
    """Analytic Jc, Jp, Jk against central differences of the residual in f64, 200 random observations, every one of the 6 + 3 + 6
    columns; steps 1e-6 x max(1, |parameter|).  Differences are taken relative to the column's largest entry over the observations.
    Measured (numpy f64, x86-64): largest relative difference 1.24e-9 (truncation of the central difference,
    h^2 f''' / 6, and cancellation at |r| ~ 3000 px: 3e3 x 2.2e-16 / 1e-6 ~ 7e-7 px against columns of ~ 700 px); the bar is
    10 x that, 1.24e-8.  The on-axis observation: both k columns are exactly zero in both rows."""
    cams, pts, calib6, grp, idx, uv = _jacobian_scene()
    r, Jc, Jp, Jk = ref.residual_jac(cams, pts, calib6, grp, idx, idx, uv)
    assert np.all(Jk[0, :, 4:] == 0.0) and np.all(Jk[1:, :, 4:] != 0.0)
    worst = 0.0

    def column(analytic, perturb, size):
        nonlocal worst
        for j in range(size):
            def at(sign):
                c, p, k = cams.copy(), pts.copy(), calib6.copy()
                h = perturb(c, p, k, j, sign)
                return ref.residual_jac(c, p, k, grp, idx, idx, uv, jac=False), h
            (rp, h), (rm, _) = at(+1.0), at(-1.0)
            num = (rp - rm) / (2.0 * h)[:, None]
            worst = max(worst, np.abs(num - analytic[:, :, j]).max() / max(np.abs(analytic[:, :, j]).max(), 1e-300))

    def step(v):
        return 1e-6 * np.maximum(1.0, np.abs(v))

    def pc(c, p, k, j, s):
        h = step(c[:, j]); c[:, j] += s * h; return h

    def pp(c, p, k, j, s):
        h = step(p[:, j]); p[:, j] += s * h; return h

    column(Jc, pc, 6); column(Jp, pp, 3)
    # a block is shared by the observations of its group: perturb one group at a time
    for g in range(2):
        sel = grp == g
        for j in range(6):
            h = float(step(calib6[g, j]))
            kp, km = calib6.copy(), calib6.copy()
            kp[g, j] += h; km[g, j] -= h
            num = (ref.residual_jac(cams, pts, kp, grp, idx, idx, uv, jac=False) - ref.residual_jac(cams, pts, km, grp, idx, idx, uv, jac=False)) / (2.0 * h)
            worst = max(worst, np.abs(num[sel] - Jk[sel, :, j]).max() / np.abs(Jk[sel, :, j]).max())
            assert np.all(num[~sel] == 0.0)
    print(f"\n[ba radial] Jacobian against central differences: largest relative difference {worst:.3e}")
    assert worst <= 1.24e-8


# ---- (c) recovery ---------------------------------------------------------------------------------------------------------------------
def _angle_axis(R):
    """rotation matrix -> angle-axis, also at an angle of pi (cameras 0 and 3 of a ring of 6 face each other, where the quotient
    by sin(theta) of synth's converter loses everything): the axis is the eigenvector of the symmetric part to the eigenvalue 1"""
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])            # 2 sin(theta) k
    c = (np.trace(R) - 1.0) / 2.0
    if np.linalg.norm(v) < 1e-12 and c > 0:
        return np.zeros(3)
    k = np.linalg.eigh((R + R.T) / 2.0)[1][:, -1]
    return k * np.arctan2(0.5 * (v @ k), c)


def _in_frame_of_camera0(cams, pts):
    R0, t0 = synth.aa_to_R(cams[0, :3]), cams[0, 3:]
    out = np.zeros_like(cams)
    for c in range(1, len(cams)):
        Rc = synth.aa_to_R(cams[c, :3]) @ R0.T
        out[c, :3] = _angle_axis(Rc); out[c, 3:] = cams[c, 3:] - Rc @ t0
    return out, pts @ R0.T + t0


def _recovery_problem():
    """6 cameras in 2 groups, truth k = (-0.12, 0.03) and (0.05, 0), no pixel noise and no outliers; start k = 0, fx and fy 2 % off
    (one up, one down, per group the other way round), poses and points at the truth; everything in the frame of camera 0, which is
    held.  Squared loss.  (With synth's start noise on poses and points the loop, whose steps are projected onto the held camera's
    box, is still descending after 50 iterations -- cost 16 from 1.5e5, fx 9e-4 off -- and says nothing about where it ends.)"""
    grp = np.array([0, 1, 0, 1, 0, 1], np.int32)
    calib_true = np.tile(K0, (2, 1))
    radial_true = np.array([[-0.12, 0.03], [0.05, 0.0]])
    sc = synth.ba_scene(6, 300, 4, radius=5.0, seed=52, uv_noise=0.0, outlier_frac=0.0, start_noise=(0.0, 0.0, 0.0))
    uv = ref.distort_observations(sc.uv, calib_true[grp[sc.cam_idx]], radial_true[grp[sc.cam_idx]])
    calib0 = calib_true * np.array([[1.02, 1.0, 0.98, 1.0], [0.98, 1.0, 1.02, 1.0]])
    cams0, pts0 = _in_frame_of_camera0(sc.cams0, sc.pts0)
    P = ref.Problem(sc.cam_idx, sc.pt_idx, uv, grp, cams0, pts0, calib0, 100.0, np.zeros((2, 2)), 1.0, ref_cam=0, ref_thr=1e-10, cauchy_a=-1.0)
    truth = np.concatenate([np.concatenate(_in_frame_of_camera0(sc.cams_gt, sc.pts_gt), None), np.concatenate([calib_true, radial_true], 1).ravel()])
    return P, calib_true, radial_true, truth


def test_reference_recovers_focal_lengths_and_radial_coefficients():
    """Up to 50 iterations from k = 0 and fx, fy 2 % off.  fx, fy, k1, k2 are gauge-free.  The observations are f32 pixels (a
    rounding of up to 3e-5 px at u ~ 700), so the truth is reached to that, not to f64.  Measured (numpy f64, x86-64): the
    loop ends after 17 iterations at cost 3.4e-5 (from 1.5e5); largest relative error of fx, fy 3.3e-8; largest absolute error of
    k1, k2 3.2e-7.  Bars: 10 x those, 3.3e-7 and 3.2e-6."""
    P, calib_true, radial_true, truth = _recovery_problem()
    assert P.cost(truth) < 1e-6                                   # the scene is what it claims: (nearly) zero residual at the truth
    x, log = ref.solve(P, 50, "schur")
    blk = P.split(x)[2]
    f_err = np.abs(blk[:, [0, 2]] / calib_true[:, [0, 2]] - 1.0).max()
    k_err = np.abs(blk[:, 4:] - radial_true).max()
    print(f"\n[ba radial] recovery: cost {log[0]['cost']:.6g} -> {log[-1]['cost']:.6g} in {len(log) - 1} iterations; "
          f"fx, fy relative error {f_err:.3e}; k1, k2 absolute error {k_err:.3e}")
    assert np.all(np.abs(P.split(x)[0][0]) <= 1e-10)           # the reference camera is held
    assert f_err <= 3.3e-7 and k_err <= 3.2e-6


# ---- the GPU cases' traces --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_no_decision_is_near_a_tie(name):
    """As tests/test_ba_groups_cpu.py: in the reference's trace of every GPU case the gain ratio stays 1e-4 away from the acceptance
    threshold 1e-3 and every Armijo test is decided by at least 1e-9 of the cost."""
    log = cases.reference(name)[3]
    rho_gap, armijo_gap = ref.stability(log)
    print(f"\n[ba radial] {name}: smallest |rho - 1e-3| {rho_gap:.3e}, smallest Armijo margin {armijo_gap:.3e} of the cost; "
          f"accepted {[e['ok'] for e in log]}, line search {[e['ls'] for e in log]}")
    assert len(log) == cases.CASE_BY_NAME[name].iters + 1
    assert rho_gap >= 1e-4 and armijo_gap >= 1e-9


def test_the_cases_are_what_they_claim():
    b = cases.build("tight")
    blk, log = cases.reference("tight")[2:]
    assert sum(e["ls"] for e in log) > 0 and 0 in [e["ok"] for e in log]
    assert np.any(np.abs(np.abs(blk[0, 4:] - b.radial0[0]) - 1e-3) < 1e-12) and np.all(np.abs(blk[1, 4:] - b.radial0[1]) < 0.5)
    assert sum(e["ls"] for e in cases.reference("ref_squared")[3]) > 0
    b = cases.build("two6")                # every track mixes the groups
    for p in range(b.sc.n_pt):
        assert len(set(b.grp[b.sc.cam_idx[b.sc.pt_idx == p]])) == 2
    b = cases.build("one3")                # tracks of length 2
    assert np.all(np.bincount(b.sc.pt_idx) == 2) and b.sc.n_cam == 3
    b = cases.build("unobserved")
    assert not np.any(b.grp == 2) and len(b.calib0) == 3
    assert np.all(cases.reference("unobserved")[2][2] == np.concatenate([b.calib0[2], b.radial0[2]]))
    # the point on the optical axis: x = y = 0 exactly at the start point, both k columns of that observation zero
    b = cases.build("axis")
    k = int(np.nonzero(b.sc.cam_idx == 0)[0][0])
    blk0 = np.concatenate([b.calib0, b.radial0], 1)
    Jk = ref.residual_jac(b.sc.cams0, b.sc.pts0, blk0, b.grp.astype(np.int64), b.sc.cam_idx, b.sc.pt_idx, b.sc.uv)[3]
    assert np.all(b.sc.cams0[0] == 0.0) and np.all(Jk[k, :, 4:] == 0.0) and Jk[k, 0, 0] == 0.0 and Jk[k, 1, 2] == 0.0
    # the radial model is worth something in every case: the distortion moves the observations by pixels
    for name in ("one3", "two6"):
        b = cases.build(name)
        P = cases.problem(name)
        assert cases.reference(name)[3][-1]["cost"] < 0.2 * P.cost(P.plus(P.x0, 0.0))


# ---- host logic -------------------------------------------------------------------------------------------------------------------------
def test_ba_forms_radial_lds_rule_at_its_boundary(tmp_path):
    exe = str(tmp_path / "ba_forms_radial_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ba_forms_radial_check.cpp"),
                        os.path.join(CSRC, "ba_forms.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ba forms (radial) ok" in r.stdout, r.stdout


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_radial_entry_points_validate_before_the_device_is_looked_at():
    """The group and radial arguments are checked first, with no context at all: error code, message, nothing written."""
    L = E.lib()
    cams = np.zeros((3, 6)); pts = np.zeros((2, 3))
    cam_idx = np.array([0, 1, 2, 0], np.int32); pt_idx = np.array([0, 0, 1, 1], np.int32); uv = np.zeros((4, 2), np.float32)
    good = dict(n_groups=2, grp=np.array([0, 1, 0], np.int32), cal=np.tile(K0, (2, 1)), tol=np.array([5.0, 5.0]), rad=np.zeros((2, 2)),
                rtol=np.array([1.0, 1.0]))

    def create(**kw):
        a = dict(good, **kw)
        out = C.c_void_p(0xdead)
        rc = L.esfm_ba_problem_create_radial_groups(None, 3, 2, 4, _p(cam_idx), _p(pt_idx), _p(uv), a["n_groups"], _p(a["grp"]), _p(a["cal"]), _p(a["tol"]),
                                                    _p(a["rad"]) if a["rad"] is not None else None, _p(a["rtol"]), _p(cams), _p(pts), C.byref(out))
        assert out.value is None                       # *out = NULL, nothing else written
        return rc, L.esfm_last_error().decode()

    def solve(**kw):
        a = dict(good, **kw)
        c, p, k, rd = cams.copy(), pts.copy(), a["cal"].copy(), (a["rad"].copy() if a["rad"] is not None else None)
        rc = L.esfm_ba_solve_radial_groups(None, 3, 2, 4, _p(cam_idx), _p(pt_idx), _p(uv), _p(c), _p(p), a["n_groups"], _p(a["grp"]), _p(k), _p(a["tol"]),
                                           _p(rd) if rd is not None else None, _p(a["rtol"]), -1, 0.0, None, C.cast(None, E._lib.ALLREDUCE_FN), None, None)
        assert np.array_equal(c, cams) and np.array_equal(p, pts) and np.array_equal(k, a["cal"], equal_nan=True)
        assert rd is None or np.array_equal(rd, a["rad"], equal_nan=True)
        return rc, L.esfm_last_error().decode()

    nan_rad = good["rad"].copy(); nan_rad[1, 0] = np.nan
    for call in (create, solve):
        assert call(rtol=np.array([1.0, 0.0])) == (ESFM_ERR_INVALID_ARG, "checked_radial: radial tolerance must be positive")
        assert call(rtol=np.array([-1.0, 1.0]))[0] == ESFM_ERR_INVALID_ARG
        assert call(rtol=np.array([1.0, np.nan])) == (ESFM_ERR_NUMERIC, "non-finite radial tolerance")
        assert call(rtol=np.array([np.inf, 1.0]))[0] == ESFM_ERR_NUMERIC
        assert call(rad=nan_rad) == (ESFM_ERR_NUMERIC, "non-finite radial coefficient")
        assert call(rad=None)[0] == ESFM_ERR_INVALID_ARG
        # the group arguments come first, with the grouped entry points' codes
        assert call(n_groups=0) == (ESFM_ERR_INVALID_ARG, "checked_groups: n_groups must be at least 1")
        assert call(tol=np.array([5.0, 0.0]), rtol=np.array([np.nan, 1.0])) == (ESFM_ERR_INVALID_ARG, "checked_groups: intrinsics tolerance must be positive")
    # valid arguments: the next thing looked at is the context
    rc, msg = create()
    assert rc == ESFM_ERR_INVALID_ARG and "ctx" in msg
    assert L.esfm_ba_problem_radial_groups(None) == 0
    assert L.esfm_ba_problem_set_radial_groups(None, _p(good["rad"]), _p(good["rtol"])) == ESFM_ERR_INVALID_ARG
    assert L.esfm_ba_problem_get_radial_groups(None, _p(good["rad"])) == ESFM_ERR_INVALID_ARG
