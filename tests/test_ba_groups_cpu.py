"""Multiple-camera bundle adjustment, the parts that need no GPU.

tests/ba_groups_ref.py -- the numpy statement of Ceres' bounded LM loop with G intrinsics blocks that judges the GPU in
tests/test_ba_groups_gpu.py -- is pinned here to the project's existing yardsticks first: with one group it reproduces the committed
golden traces and the CPU oracle at the bars the GPU is held to (cost 1e-8 accepted / 1e-6 rejected, radius 1e-6, step norm 1e-3,
accept pattern and line-search counts exact, final parameters rtol 1e-4 / atol 1e-5); its Jacobian agrees with the oracle's row by
row; its point-eliminated and its dense solve agree.  Every GPU case's reference trace is then checked to be far from a tie in each
accept / reject and each Armijo decision.  Then the host logic: the form rule with groups, argument validation of the new C entry
points, the packing of the BundleAdjustment mirror, synth's per-camera intrinsics."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth
from easysfm_amd._lib import ESFM_ERR_INVALID_ARG, ESFM_ERR_NUMERIC

import ba_groups_cases as cases
import ba_groups_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")
K0 = np.array(synth.FOUNTAIN_K4, np.float64)


# ---- the reference against the golden traces and the oracle (one group) ---------------------------------------------------------
def _at_the_gpu_bars(log, ok, ls, cost, radius, step_norm):
    assert len(log) == len(cost)
    assert [e["ok"] for e in log] == list(ok)
    assert [e["ls"] for e in log] == list(ls)
    for i, (e, c, rad, sn) in enumerate(zip(log, cost, radius, step_norm)):
        assert abs(e["cost"] - c) <= (1e-8 if e["ok"] else 1e-6) * abs(c), (i, e["cost"], c)
        assert abs(e["radius"] - rad) <= 1e-6 * rad, i
        assert abs(e["step_norm"] - sn) <= 1e-3 * max(sn, 1e-6), (i, e["step_norm"], sn)


@pytest.mark.parametrize("method", ["schur", "dense"])
@pytest.mark.parametrize("tag", ["calib_loose", "calib_tight", "both_squared"])
def test_one_group_reproduces_the_golden_traces(tag, method):
    z = np.load(os.path.join(GOLD, "ba_lm_constrained.npz"))
    n = len(z[f"{tag}.cost"]) - 1
    cams0 = z[f"{tag}.cams0"]
    P = ref.Problem(z[f"{tag}.cam_idx"], z[f"{tag}.pt_idx"], z[f"{tag}.uv"], np.zeros(len(cams0), int), cams0, z[f"{tag}.pts0"], z[f"{tag}.calib0"],
                    float(z[f"{tag}.calib_tol"]), int(z[f"{tag}.ref_cam"]), 1e-10, float(z[f"{tag}.cauchy_a"]))
    x, log = ref.solve(P, n, method)
    _at_the_gpu_bars(log, z[f"{tag}.ok"], z[f"{tag}.ls"], z[f"{tag}.cost"], z[f"{tag}.radius"], z[f"{tag}.step_norm"])
    assert np.allclose(x, z[f"{tag}.x_final"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("n_cam,n_pt,k,seed,tol", [(4, 60, 3, 41, 100.0), (25, 2000, 8, 3, 15.0)])
def test_one_group_agrees_with_the_oracle(oracle_lib, n_cam, n_pt, k, seed, tol):
    sc = synth.ba_scene(n_cam, n_pt, k, seed=seed)
    calib0 = K0 * np.array([1.02, 0.99, 0.98, 1.01])
    ropt = oracle_lib.ba_default_options(); ropt.max_num_iterations = 6
    rc, rp, rk, rs = oracle_lib.ba_solve_ex(sc.cam_idx, sc.pt_idx, sc.uv, None, sc.cams0, sc.pts0, calib=calib0, calib_tol=tol, options=ropt)
    its = oracle_lib.iterations(rs)
    P = ref.Problem(sc.cam_idx, sc.pt_idx, sc.uv, np.zeros(n_cam, int), sc.cams0, sc.pts0, calib0, tol)
    x, log = ref.solve(P, 6, "schur")
    _at_the_gpu_bars(log, [it.step_is_successful for it in its], [it.line_search_steps for it in its], [it.cost for it in its],
                     [it.trust_region_radius for it in its], [it.step_norm for it in its])
    assert np.allclose(x, np.concatenate([rc.ravel(), rp.ravel(), rk.ravel()]), rtol=1e-4, atol=1e-5)
    assert abs(P.cost(x) - oracle_lib.ba_cost_calib(sc.cam_idx, sc.pt_idx, sc.uv, rk, rc, rp)) <= 1e-8 * rs.final_cost


def test_schur_and_dense_variants_agree_with_two_groups():
    P = cases.problem("mixed")
    xs, ls = ref.solve(P, 4, "schur")
    xd, ld = ref.solve(P, 4, "dense")
    assert [e["ok"] for e in ls] == [e["ok"] for e in ld] and [e["ls"] for e in ls] == [e["ls"] for e in ld]
    for a, b in zip(ls, ld):
        assert abs(a["cost"] - b["cost"]) <= 1e-10 * abs(b["cost"])
    # the step itself, from one linearisation: Jacobi-scaled blocks at the start point, LM diagonal at the initial radius
    x = P.plus(P.x0, 0.0)
    _, r, F, E_, K = P.evaluate(x)
    scale = 1.0 / (1.0 + np.sqrt(P.colsq(F, E_, K)))
    F, E_, K = P.scaled(F, E_, K, scale)
    D = np.clip(P.colsq(F, E_, K), 1e-6, 1e32) / 1e4
    a, b = P.step_schur(F, E_, K, r, D), P.step_dense(F, E_, K, r, D)
    assert np.linalg.norm(a - b) <= 1e-10 * np.linalg.norm(b)


def test_jacobian_agrees_with_the_oracle_row_by_row(oracle_lib):
    b = cases.build("mixed")
    cams = b.sc.cams0.copy()
    cams[2, :3] = [3e-9, -2e-9, 1e-9]             # the small-angle branch of the rotation (theta^2 <= epsilon)
    r, Jc, Jp, Jk = ref.residual_jac(cams, b.sc.pts0, b.calib0, b.grp.astype(np.int64), b.sc.cam_idx, b.sc.pt_idx, b.sc.uv)
    assert np.any(b.sc.cam_idx == 2)
    for k in range(b.sc.n_obs):
        c, p = b.sc.cam_idx[k], b.sc.pt_idx[k]
        orr, oJc, oJp, oJk = oracle_lib.ba_residual_jac_calib(cams[c], b.sc.pts0[p], b.calib0[b.grp[c]], b.sc.uv[k])
        for mine, theirs in ((r[k], orr), (Jc[k], oJc), (Jp[k], oJp), (Jk[k], oJk)):
            assert np.allclose(mine, theirs, rtol=1e-11, atol=1e-9 * max(1.0, np.abs(theirs).max())), (k, mine, theirs)


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_no_decision_is_near_a_tie(name):
    """An exact accept-pattern / line-search-count assertion must not hang on a coin flip: in the reference's trace of every GPU
    case the gain ratio stays 1e-4 away from the acceptance threshold 1e-3 and every Armijo test is decided by at least 1e-9 of the cost."""
    log = cases.reference(name)[3]
    rho_gap, armijo_gap = ref.stability(log)
    print(f"\n[ba groups] {name}: smallest |rho - 1e-3| {rho_gap:.3e}, smallest Armijo margin {armijo_gap:.3e} of the cost; "
          f"accepted {[e['ok'] for e in log]}, line search {[e['ls'] for e in log]}")
    assert len(log) == cases.CASE_BY_NAME[name].iters + 1
    assert rho_gap >= 1e-4 and armijo_gap >= 1e-9


def test_the_cases_are_what_they_claim():
    b = cases.build("tight")
    cal, log = cases.reference("tight")[2:]
    assert sum(e["ls"] for e in log) > 0 and np.any(np.abs(np.abs(cal[0] - b.calib0[0]) - 6.0) < 1e-12)
    log = cases.reference("ref_squared")[3]
    assert sum(e["ls"] for e in log) > 0 and 0 in [e["ok"] for e in log]
    b = cases.build("mixed")               # every track mixes the groups
    for p in range(b.sc.n_pt):
        assert len(set(b.grp[b.sc.cam_idx[b.sc.pt_idx == p]])) == 2


# ---- host logic -----------------------------------------------------------------------------------------------------------------
def test_ba_forms_with_groups_at_every_boundary(tmp_path):
    exe = str(tmp_path / "ba_forms_groups_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ba_forms_groups_check.cpp"),
                        os.path.join(CSRC, "ba_forms.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ba forms (groups) ok" in r.stdout, r.stdout


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_grouped_entry_points_validate_before_the_device_is_looked_at():
    """The group arguments are checked first, with no context at all: error code, message, nothing written."""
    L = E.lib()
    cams = np.zeros((3, 6)); pts = np.zeros((2, 3))
    cam_idx = np.array([0, 1, 2, 0], np.int32); pt_idx = np.array([0, 0, 1, 1], np.int32); uv = np.zeros((4, 2), np.float32)
    good = dict(n_groups=2, grp=np.array([0, 1, 0], np.int32), cal=np.tile(K0, (2, 1)), tol=np.array([5.0, 5.0]))

    def create(**kw):
        a = dict(good, **kw)
        out = C.c_void_p(0xdead)
        rc = L.esfm_ba_problem_create_calib_groups(None, 3, 2, 4, _p(cam_idx), _p(pt_idx), _p(uv), a["n_groups"], _p(a["grp"]) if a["grp"] is not None else None,
                                                   _p(a["cal"]), _p(a["tol"]), _p(cams), _p(pts), C.byref(out))
        assert out.value is None                       # *out = NULL, nothing else written
        return rc, L.esfm_last_error().decode()

    def solve(**kw):
        a = dict(good, **kw)
        c, p, k = cams.copy(), pts.copy(), a["cal"].copy()
        rc = L.esfm_ba_solve_groups(None, 3, 2, 4, _p(cam_idx), _p(pt_idx), _p(uv), _p(c), _p(p), a["n_groups"], _p(a["grp"]), _p(k), _p(a["tol"]), -1, 0.0,
                                    None, C.cast(None, E._lib.ALLREDUCE_FN), None, None)
        assert np.array_equal(c, cams) and np.array_equal(p, pts) and np.array_equal(k, a["cal"], equal_nan=True)
        return rc, L.esfm_last_error().decode()

    nan_cal = good["cal"].copy(); nan_cal[1, 2] = np.nan
    for call in (create, solve):
        assert call(n_groups=0) == (ESFM_ERR_INVALID_ARG, "checked_groups: n_groups must be at least 1")
        assert call(n_groups=-3)[0] == ESFM_ERR_INVALID_ARG
        assert call(grp=np.array([0, 2, 0], np.int32)) == (ESFM_ERR_INVALID_ARG, "checked_groups: camera group index out of range")
        assert call(grp=np.array([0, -1, 0], np.int32))[0] == ESFM_ERR_INVALID_ARG
        assert call(tol=np.array([5.0, 0.0])) == (ESFM_ERR_INVALID_ARG, "checked_groups: intrinsics tolerance must be positive")
        assert call(tol=np.array([-1.0, 5.0]))[0] == ESFM_ERR_INVALID_ARG
        assert call(tol=np.array([5.0, np.nan])) == (ESFM_ERR_NUMERIC, "non-finite intrinsics tolerance")
        assert call(tol=np.array([np.inf, 5.0]))[0] == ESFM_ERR_NUMERIC
        assert call(cal=nan_cal) == (ESFM_ERR_NUMERIC, "non-finite intrinsics")
        # 6 (n_cam + n_groups) must stay below the library's limit of 46 000
        big = 45999 // 6 - 3 + 1
        rc, msg = call(n_groups=big, cal=np.ones((big, 4)), tol=np.ones(big))
        assert rc == ESFM_ERR_INVALID_ARG and "reduced system too large" in msg
    assert create(grp=None)[0] == ESFM_ERR_INVALID_ARG
    # valid groups: the next thing looked at is the context
    rc, msg = create()
    assert rc == ESFM_ERR_INVALID_ARG and "ctx" in msg
    assert L.esfm_ba_problem_calib_groups(None) == 0


def _frames(camera_ids, process):
    sc = synth.ba_scene(len(camera_ids), 120, 3, seed=9)
    frames = []
    for c, cid in enumerate(camera_ids):
        sel = np.nonzero(sc.cam_idx == c)[0]
        fr = E.Frame(frame_id=c, keypoints=sc.uv[sel])
        fr.unique_pixel_ids = sc.pt_idx[sel].astype(np.int64)
        fr.unique_pixel_has_match = np.ones(len(sel), bool)
        fr.K_cam = np.array([[2000.0 + c, 0, 700 + c], [0, 2100.0 + c, 500 + c], [0, 0, 1]], np.float32)
        fr.camera_id = cid
        frames.append(fr)
    cloud = E.SparsePointCloud(xyz=sc.pts0.astype(np.float32), unique_point_ids=np.arange(sc.n_pt))
    ba = E.BundleAdjustment.__new__(E.BundleAdjustment); ba._ctx = None; ba.options = None; ba.initBA()
    return ba, frames, cloud, sc


def test_setBAProblem_packs_one_block_per_camera_id():
    assert E.Frame().camera_id == 0
    ids, process = [7, 3, 7, 3, 5, 7], [False, True, False, False, False, False]       # frame 1 is not processed
    ba, frames, cloud, sc = _frames(ids, process)
    ba.setBAProblem(frames, process, cloud, 25.0, 0)
    # groups: the distinct ids of the PROCESSED frames in order of first appearance; each starts from its first processed frame's K
    assert ba.group_camera_ids_ == [7, 3, 5]
    assert ba.camera_group_.tolist() == [0, 0, 1, 2, 0]
    assert ba.num_cameras_ == 5 and ba.num_parameters_ == 6 * 5 + 3 * sc.n_pt + 4 * 3
    first = {7: 0, 3: 3, 5: 4}
    for g, cid in enumerate(ba.group_camera_ids_):
        K = frames[first[cid]].K_cam
        assert ba.parameters_[6 * 5 + 3 * sc.n_pt + 4 * g:][:4].tolist() == [K[0, 0], K[0, 2], K[1, 1], K[1, 2]]
    # fixed intrinsics: camera ids play no part
    ba.initBA(); ba.setBAProblem(frames, process, cloud, 0.0, 0)
    assert ba.group_camera_ids_ == [] and ba.num_parameters_ == 6 * 5 + 3 * sc.n_pt
    # one distinct id among the processed frames: the shared block of calibs_[0], exactly as before
    ba2, frames2, cloud2, _ = _frames([4, 9, 4, 4, 4, 4], process)
    ba2.setBAProblem(frames2, process, cloud2, 25.0, 0)
    ba3, frames3, cloud3, _ = _frames([0] * 6, process)
    ba3.setBAProblem(frames3, process, cloud3, 25.0, 0)
    assert ba2.group_camera_ids_ == [] and ba2.camera_group_.size == 0 and ba2.num_parameters_ == 6 * 5 + 3 * sc.n_pt + 4
    assert ba2.parameters_.tobytes() == ba3.parameters_.tobytes()
    K = frames2[0].K_cam
    assert ba2.parameters_[-4:].tolist() == [K[0, 0], K[0, 2], K[1, 1], K[1, 2]]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_cpp_mirror_packs_one_block_per_camera_id(tmp_path, flags):
    """tests/cpp/ba_groups_host_check.cpp: setBAProblem of the esfm_host.hpp mirror, the assertions of the Python test above; a
    stand-alone host program, g++."""
    exe = str(tmp_path / "ba_groups_host_check")
    lib_dir = os.path.join(ROOT, "easysfm_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "ba_groups_host_check.cpp"), "-o", exe, os.path.join(lib_dir, "libesfm_hip.so"), "-lz",
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ba groups host check ok" in r.stdout, r.stdout[-4000:]


def test_synth_per_camera_intrinsics_default_is_bit_identical():
    a, b = synth.ba_scene(6, 100, 4, seed=5), synth.ba_scene(6, 100, 4, seed=5, K4_per_cam=None)
    for f in ("cam_idx", "pt_idx", "uv", "K4", "cams0", "pts0"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()
    # the same K for every camera, given explicitly: the same scene
    c = synth.ba_scene(6, 100, 4, seed=5, K4_per_cam=np.tile(np.array(synth.FOUNTAIN_K4, np.float32), (6, 1)))
    assert np.array_equal(c.K4, a.K4) and np.allclose(c.uv, a.uv, rtol=0, atol=1e-3) and c.cams0.tobytes() == a.cams0.tobytes()
    # two models: the observations of camera 1 are those of a camera with 0.8 x the focal lengths about the same principal point
    K4 = np.tile(np.array(synth.FOUNTAIN_K4, np.float32), (6, 1)); K4[1::2, 0] *= 0.8; K4[1::2, 2] *= 0.8
    d = synth.ba_scene(6, 100, 4, seed=5, K4_per_cam=K4, uv_noise=0.0, outlier_frac=0.0)
    e = synth.ba_scene(6, 100, 4, seed=5, uv_noise=0.0, outlier_frac=0.0)
    odd = d.cam_idx % 2 == 1
    pp = np.array([synth.FOUNTAIN_K4[1], synth.FOUNTAIN_K4[3]])
    assert np.allclose(d.uv[~odd], e.uv[~odd], atol=1e-3) and np.allclose(d.uv[odd] - pp, 0.8 * (e.uv[odd] - pp), atol=2e-3)
    assert np.array_equal(d.K4, K4)
