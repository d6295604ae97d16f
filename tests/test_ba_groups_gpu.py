"""Bundle adjustment in multiple-camera mode on the GPU: G free intrinsics blocks, one per camera group (esfm_ba_solve_groups,
esfm_ba_problem_create_calib_groups).

With one group the grouped entry points must be today's free-intrinsics path to the bit.  With several, the reference is the numpy
restatement of Ceres' bounded LM loop in tests/ba_groups_ref.py (pinned to the golden traces and the oracle by
tests/test_ba_groups_cpu.py, which also checks that no decision of the traces used here is near a tie), at the bars
test_constrained_golden_traces applies: cost 1e-8 on accepted and 1e-6 on rejected iterations, radius 1e-6, step norm 1e-3, the
accept pattern and the line-search counts exactly, the final parameters at rtol 1e-4 / atol 1e-5.  The cases and the reference's
solve of each are shared through tests/ba_groups_cases.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth

import ba_groups_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")
K0 = np.array(synth.FOUNTAIN_K4, np.float64)
LDS_SLABS, TABLES = "SCHUR_LDS_SLABS", "SCHUR_TABLES"
SMALL, LDS, TILED = "SOLVE_SMALL_ONE_WG", "SOLVE_LDS", "SOLVE_TILED"

# the forms each boundary case is meant to take: schur, solve, sweep_sums_in_lds, large, block rows of the grouped kernel in LDS
FORMS = {
    "g27": (LDS_SLABS, SMALL, 0, 0, 1), "g28": (LDS_SLABS, LDS, 0, 0, 1),
    "g30": (LDS_SLABS, LDS, 0, 0, 1), "g31": (TABLES, TILED, 0, 0, 1),
    "g168": (TABLES, TILED, 0, 0, 1), "g169": (TABLES, TILED, 0, 0, 0),
    "g539": (TABLES, TILED, 0, 0, 0), "g27_obs_2p20": (LDS_SLABS, SMALL, 0, 1, 1),
}


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _log_fields(summ):
    """every field of the iteration log and of the summary except the wall time, as raw bytes"""
    n = min(summ.num_iterations + 1, len(summ.iterations))
    its = bytes(ctypes.string_at(ctypes.addressof(summ.iterations), ctypes.sizeof(summ.iterations[0]) * n))
    head = (summ.termination, summ.num_iterations, summ.num_successful_steps, summ.num_unsuccessful_steps, summ.num_active_cameras,
            summ.num_active_points, np.float64(summ.initial_cost).tobytes(), np.float64(summ.final_cost).tobytes())
    return head, its


def _gpu(name, ctx):
    case, b = cases.CASE_BY_NAME[name], cases.build(name)
    opt = E.default_options(); opt.max_num_iterations = case.iters; opt.cauchy_a = case.cauchy_a
    return E.ba_solve_groups(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, b.sc.cams0, b.sc.pts0, b.grp, b.calib0, b.tol, ref_cam=case.ref_cam,
                             options=opt, ctx=ctx)


def _against_reference(name, out):
    cams, pts, cal, summ = out
    rc, rp, rk, rlog = cases.reference(name)
    b = cases.build(name)
    log = summ.log()
    print(f"\n[ba groups] {name}: cost {summ.initial_cost:.6f} -> {summ.final_cost:.6f}; accepted {[it.step_is_successful for it in log]}; "
          f"line search {[it.line_search_steps for it in log]}; reference cost {[e['cost'] for e in rlog]}", flush=True)
    assert len(log) == len(rlog)
    assert [it.step_is_successful for it in log] == [e["ok"] for e in rlog]
    assert [it.line_search_steps for it in log] == [e["ls"] for e in rlog]
    for it, e in zip(log, rlog):
        assert abs(it.cost - e["cost"]) <= (1e-8 if it.step_is_successful else 1e-6) * abs(e["cost"]), (it.iteration, it.cost, e["cost"])
        assert abs(it.trust_region_radius - e["radius"]) <= 1e-6 * e["radius"], it.iteration
        assert abs(it.step_norm - e["step_norm"]) <= 1e-3 * max(e["step_norm"], 1e-6), (it.iteration, it.step_norm, e["step_norm"])
    x = np.concatenate([cams.ravel(), pts.ravel(), cal.ravel()]); rx = np.concatenate([rc.ravel(), rp.ravel(), rk.ravel()])
    assert np.allclose(x, rx, rtol=1e-4, atol=1e-5), np.abs(x - rx).max()
    # inside the boxes; and the returned parameters are the ones the final cost was evaluated with
    assert np.all(cal >= b.calib0 - b.tol[:, None]) and np.all(cal <= b.calib0 + b.tol[:, None])
    c = cases.problem(name).cost(x)
    assert abs(c - summ.final_cost) <= 1e-10 * summ.final_cost, (c, summ.final_cost)
    assert summ.final_cost < summ.initial_cost


# ---- 1. one group is today's path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cam,n_pt,k,seed,tol", [(4, 60, 3, 41, 100.0), (25, 2000, 8, 3, 15.0), (64, 3000, 5, 21, 30.0)])
def test_one_group_is_bit_identical_to_the_shared_block(gpu_ctx, n_cam, n_pt, k, seed, tol):
    sc = synth.ba_scene(n_cam, n_pt, k, seed=seed)
    calib0 = K0 * np.array([1.02, 0.99, 0.98, 1.01])
    opt = E.default_options(); opt.max_num_iterations = 4
    c1, p1, k1, s1 = E.ba_solve_ex(sc.cam_idx, sc.pt_idx, sc.uv, None, sc.cams0, sc.pts0, calib=calib0, calib_tol=tol, options=opt, ctx=gpu_ctx)
    c2, p2, k2, s2 = E.ba_solve_groups(sc.cam_idx, sc.pt_idx, sc.uv, sc.cams0, sc.pts0, np.zeros(n_cam, np.int32), calib0[None, :], [tol],
                                       options=opt, ctx=gpu_ctx)
    assert k2.shape == (1, 4)
    assert _bytes(c1) == _bytes(c2) and _bytes(p1) == _bytes(p2) and _bytes(k1) == _bytes(k2[0])
    assert _log_fields(s1) == _log_fields(s2)
    assert s1.num_iterations == 4 and s1.final_cost < s1.initial_cost
    # ... and through the resident problem: created with groups, read with the one-block accessor
    prob = E.BAProblem(sc.cam_idx, sc.pt_idx, sc.uv, None, sc.cams0, sc.pts0, gpu_ctx, calib_groups=(np.zeros(n_cam, np.int32), calib0[None, :], tol))
    try:
        assert E.lib().esfm_ba_problem_calib_groups(prob._h) == 1
        s3 = prob.solve(opt)
        c3, p3 = prob.get_params()
        assert _bytes(c3) == _bytes(c1) and _bytes(p3) == _bytes(p1) and _bytes(prob.get_calib()) == _bytes(k1) and _bytes(prob.get_calib_groups()[0]) == _bytes(k1)
        assert _log_fields(s3) == _log_fields(s1)
    finally:
        prob.close()


# ---- 2 - 6. several groups against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "split", "own", "ref_squared"])
def test_groups_match_reference(gpu_ctx, name):
    out = _gpu(name, gpu_ctx)
    _against_reference(name, out)
    if name == "ref_squared":
        assert np.all(np.abs(out[0][0]) <= 1e-10)             # the reference camera is held


def test_group_nobody_observes_and_camera_without_observations(gpu_ctx):
    """G = 3 with no camera in group 2; camera 5 (group 1) has no observation: both come back bit for bit, the rest follows the
    reference."""
    b = cases.build("unobserved")
    assert not np.any(b.sc.cam_idx == 5) and not np.any(b.grp == 2) and len(b.calib0) == 3
    cams, pts, cal, summ = out = _gpu("unobserved", gpu_ctx)
    assert _bytes(cal[2]) == _bytes(b.calib0[2])
    assert _bytes(cams[5]) == _bytes(b.sc.cams0[5])
    assert summ.num_active_cameras == 5
    _against_reference("unobserved", out)


def test_tight_box_in_one_group_only(gpu_ctx):
    b = cases.build("tight")
    cams, pts, cal, summ = out = _gpu("tight", gpu_ctx)
    _against_reference("tight", out)
    assert sum(it.line_search_steps for it in summ.log()) > 0
    assert np.any(np.abs(np.abs(cal[0] - b.calib0[0]) - b.tol[0]) < 1e-12)         # a bound of group 0 is active, exactly
    assert np.all(np.abs(cal[1] - b.calib0[1]) < b.tol[1] - 1.0)                   # group 1's box is loose


def test_several_groups_reject_the_one_block_accessors(gpu_ctx):
    b = cases.build("mixed")
    prob = E.BAProblem(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, None, b.sc.cams0, b.sc.pts0, gpu_ctx, calib_groups=(b.grp, b.calib0, b.tol))
    try:
        assert E.lib().esfm_ba_problem_calib_groups(prob._h) == 2
        with pytest.raises(RuntimeError, match="several intrinsics blocks"):
            prob.get_calib()
        with pytest.raises(RuntimeError, match="several intrinsics blocks"):
            prob.set_calib(b.calib0[0], 5.0)
        assert _bytes(prob.get_calib_groups()) == _bytes(b.calib0)
        # new start values and boxes, then the solve of case "mixed"
        prob.set_calib_groups(b.calib0 * 1.5, [1.0, 2.0])
        assert _bytes(prob.get_calib_groups()) == _bytes(b.calib0 * 1.5)
        prob.set_calib_groups(b.calib0, b.tol)
        opt = E.default_options(); opt.max_num_iterations = cases.CASE_BY_NAME["mixed"].iters
        summ = prob.solve(opt)
        cams, pts = prob.get_params()
        _against_reference("mixed", (cams, pts, prob.get_calib_groups(), summ))
    finally:
        prob.close()


# ---- 7. the size-dependent kernel forms -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forms_of(tmp_path_factory):
    """The host rule's answer for every boundary case: {name: (schur, solve, sweep_sums_in_lds, large, group_rows_in_lds)}."""
    exe = str(tmp_path_factory.mktemp("ba_forms_groups") / "ba_forms_groups_print")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ba_forms_groups_print.cpp"),
                        os.path.join(CSRC, "ba_forms.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    args = []
    for name in FORMS:
        c = cases.CASE_BY_NAME[name]
        args += [str(c.n_real), str(c.G), str(c.n_pt * min(c.per, c.n_real))]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(FORMS), r.stdout
    out = {}
    for name, line in zip(FORMS, lines):
        schur, solve, sums, large, rows = line.split()
        out[name] = (schur, solve, int(sums), int(large), int(rows))
    return out


def _takes_its_forms(name, forms_of):
    c = cases.CASE_BY_NAME[name]
    assert forms_of[name] == FORMS[name], (f"{name}: this size ({c.n_real} cameras, {c.G} groups, {c.n_pt * min(c.per, c.n_real)} observations) no longer "
                                           f"takes forms {FORMS[name]}: ba_forms says {forms_of[name]}")


@pytest.mark.parametrize("name", list(FORMS))
def test_form_boundaries_with_two_groups(gpu_ctx, forms_of, name):
    _takes_its_forms(name, forms_of)
    assert cases.build(name).sc.n_obs == cases.CASE_BY_NAME[name].n_pt * cases.CASE_BY_NAME[name].per
    _against_reference(name, _gpu(name, gpu_ctx))


def test_cases_reach_every_grouped_row_of_the_form_table(forms_of):
    """DESIGN.md section 5.1a, the rows for several intrinsics blocks."""
    for name in FORMS:
        _takes_its_forms(name, forms_of)
    at = {cases.CASE_BY_NAME[n].n_real: f for n, f in forms_of.items() if not f[3]}
    rows = {
        "one-workgroup solve at its limit (n_cam = 29: n_real = 27 | 28)": at[27][1] == SMALL and at[28][1] == LDS,
        "LDS solve and LDS-slab Schur at their limit (n_cam = 32: n_real = 30 | 31)": at[30][:2] == (LDS_SLABS, LDS) and at[31][:2] == (TABLES, TILED),
        "the grouped block rows in LDS at their limit (two groups: n_real = 168 | 169)": at[168][4] == 1 and at[169][4] == 0,
        "camera-chunk sums at every size": all(f[2] == 0 for f in forms_of.values()),
        "beyond the one-block sweep's LDS limit (n_real = 539)": at[539][:2] == (TABLES, TILED) and at[539][4] == 0,
        "large (2^20 observations)": forms_of["g27_obs_2p20"][3] == 1 and cases.CASE_BY_NAME["g27_obs_2p20"].n_pt * 8 == 1 << 20,
    }
    missed = [k for k, hit in rows.items() if not hit]
    assert not missed, missed


# ---- 8. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "g31"])
def test_two_solves_agree_in_every_bit(gpu_ctx, name):
    a, b = _gpu(name, gpu_ctx), _gpu(name, gpu_ctx)
    for x, y in zip(a[:3], b[:3]):
        assert _bytes(x) == _bytes(y)
    assert _log_fields(a[3]) == _log_fields(b[3])


# ---- 10. the BundleAdjustment mirror ----------------------------------------------------------------------------------------------
def _mirror_frames(sc, K_of_frame, camera_ids):
    frames = []
    for c in range(sc.n_cam):
        sel = np.nonzero(sc.cam_idx == c)[0]
        fr = E.Frame(frame_id=c, keypoints=sc.uv[sel])
        fr.unique_pixel_ids = sc.pt_idx[sel].astype(np.int64)
        fr.unique_pixel_has_match = np.ones(len(sel), bool)
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = synth.aa_to_R(sc.cams0[c, :3]).astype(np.float32); pose[:3, 3] = sc.cams0[c, 3:].astype(np.float32)
        fr.pose_cam = pose; fr.K_cam = K_of_frame[c].copy(); fr.camera_id = camera_ids[c]
        frames.append(fr)
    return frames, E.SparsePointCloud(xyz=sc.pts0.astype(np.float32), unique_point_ids=np.arange(sc.n_pt))


def _K3(k4):
    return np.array([[k4[0], 0, k4[1]], [0, k4[2], k4[3]], [0, 0, 1]], np.float32)


MIRROR_TRUE = K0[None, :] * np.array([[1.0, 1.0, 1.0, 1.0], [0.8, 1.0, 0.8, 1.0]])
MIRROR_START = MIRROR_TRUE * np.array([1.02, 1.0, 0.98, 1.0])
MIRROR_IDS = [c % 2 for c in range(6)]


def _mirror_scene():
    """(6, 300, 4) seen by two camera models (camera_id = c % 2), in the reference frame of camera 0"""
    return synth.in_reference_frame(synth.ba_scene(6, 300, 4, seed=52, K4_per_cam=MIRROR_TRUE[MIRROR_IDS]), 0)


def test_mirror_doSFMBA_writes_each_group_its_own_intrinsics(gpu_ctx):
    """doSFMBA over frames of two cameras (camera_id = c % 2), free intrinsics within +-25, fx of both started 2 % off: each group's
    frames receive that group's K and only it, each fx error falls below 0.2 x its initial error (the bar of
    test_mirror_doSFMBA_free_calib_and_reference_frame), the reference frame's pose stays."""
    true, start, ids = MIRROR_TRUE, MIRROR_START, MIRROR_IDS
    sc = _mirror_scene()
    frames, cloud = _mirror_frames(sc, [_K3(start[g]) for g in ids], ids)
    pose0 = frames[0].pose_cam.copy()
    ba = E.BundleAdjustment(gpu_ctx)
    ba.doSFMBA(frames, [False] * 6, cloud, 25.0, 0)
    assert ba.group_camera_ids_ == [0, 1] and ba.num_parameters_ == 6 * 6 + 3 * sc.n_pt + 8
    assert ba.ref_process_camera_id_ == 0 and np.allclose(frames[0].pose_cam, pose0, atol=1e-6)
    assert ba.summary.final_cost < ba.summary.initial_cost
    for g in (0, 1):
        mine = [fr.K_cam for fr, i in zip(frames, ids) if i == g]
        assert all(np.array_equal(K, mine[0]) for K in mine)
        got = np.array([mine[0][0, 0], mine[0][0, 2], mine[0][1, 1], mine[0][1, 2]], np.float64)
        assert np.array_equal(got, ba.parameters_[6 * 6 + 3 * sc.n_pt + 4 * g:][:4].astype(np.float32).astype(np.float64))
        assert abs(got[0] - true[g, 0]) < 0.2 * abs(start[g, 0] - true[g, 0]), (g, got, true[g])
        assert np.all(np.abs(got - start[g].astype(np.float32)) <= 25.0 + 1e-3)
    assert not np.array_equal(frames[0].K_cam, frames[1].K_cam)


def test_mirror_doSFMBA_with_one_camera_id_is_the_shared_block(gpu_ctx):
    """The scene and the frames of the grouped mirror test -- data from two camera models, two start K's -- with every camera_id 0,
    or any one id: the existing path, to the bit, whatever the id is called."""
    sc = _mirror_scene()
    Ks = [_K3(MIRROR_START[g]) for g in MIRROR_IDS]
    n = sc.n_cam
    results = []
    for cid in (0, 5):
        frames, cloud = _mirror_frames(sc, Ks, [cid] * n)
        ba = E.BundleAdjustment(gpu_ctx)
        ba.doSFMBA(frames, [False] * n, cloud, 25.0, 0)
        assert ba.group_camera_ids_ == [] and ba.num_parameters_ == 6 * n + 3 * sc.n_pt + 4
        assert all(np.array_equal(fr.K_cam, frames[0].K_cam) for fr in frames)                # one K for every frame afterwards
        results.append((ba.parameters_.tobytes(), _log_fields(ba.summary), [fr.K_cam.tobytes() for fr in frames], [fr.pose_cam.tobytes() for fr in frames]))
    assert results[0] == results[1]
    # ... and it is esfm_ba_solve_ex's result from the same packing
    frames, cloud = _mirror_frames(sc, Ks, [0] * n)
    ba = E.BundleAdjustment(gpu_ctx); ba.initBA(); ba.setBAProblem(frames, [False] * n, cloud, 25.0, 0)
    assert ba.parameters_[-4:].tolist() == [Ks[0][0, 0], Ks[0][0, 2], Ks[0][1, 1], Ks[0][1, 2]]       # calibs_[0]
    nc, npt = n, sc.n_pt
    c, p, k, summ = E.ba_solve_ex(ba.camera_index_, ba.point_index_, ba.points_2d_, None, ba.parameters_[:6 * nc].reshape(nc, 6),
                                  ba.parameters_[6 * nc:6 * nc + 3 * npt].reshape(npt, 3), calib=ba.parameters_[-4:].copy(), calib_tol=25.0, ref_cam=0,
                                  ref_threshold=1e-10, ctx=gpu_ctx)
    assert np.concatenate([c.ravel(), p.ravel(), k]).tobytes() == results[0][0] and _log_fields(summ) == results[0][1]


def test_cpp_mirror_doSFMBA_with_two_cameras(tmp_path):
    """tests/cpp/ba_groups_host_gpu.cpp: the esfm_host.hpp mirror's grouped solveBA / doSFMBA -- the esfm_ba_solve_groups call, the
    per-group write-back of K_cam -- on the scene of the Python mirror test, with its assertions; a stand-alone program, g++."""
    sc = _mirror_scene()
    lines = [f"{sc.n_cam} {sc.n_pt}"]
    for c in range(sc.n_cam):
        g = MIRROR_IDS[c]
        sel = np.nonzero(sc.cam_idx == c)[0]
        pose = np.concatenate([synth.aa_to_R(sc.cams0[c, :3]), sc.cams0[c, 3:, None]], 1)
        lines.append(f"{g} " + " ".join(repr(float(v)) for v in MIRROR_START[g]) + f" {float(MIRROR_TRUE[g, 0])!r}")
        lines.append(" ".join(repr(float(v)) for v in pose.ravel()))
        lines.append(str(len(sel)))
        lines += [f"{int(sc.pt_idx[k])} {float(sc.uv[k, 0])!r} {float(sc.uv[k, 1])!r}" for k in sel]
    lines += [" ".join(repr(float(v)) for v in p) for p in sc.pts0]
    scene = tmp_path / "scene.txt"
    scene.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "ba_groups_host_gpu")
    lib_dir = os.path.join(ROOT, "easysfm_amd")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "cpp", "ba_groups_host_gpu.cpp"), "-o", exe, os.path.join(lib_dir, "libesfm_hip.so"), "-lz",
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, str(scene)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ba groups host gpu ok" in r.stdout, r.stdout[-4000:]
