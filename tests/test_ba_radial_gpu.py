"""Bundle adjustment with free radial distortion on the GPU: blocks fx, cx, fy, cy, k1, k2, one per camera group
(esfm_ba_solve_radial_groups, esfm_ba_problem_create_radial_groups).

The reference is the numpy restatement of the bounded LM loop with 6-wide blocks in tests/ba_radial_ref.py (pinned by
tests/test_ba_radial_cpu.py, which also checks that no decision of the traces used here is near a tie), at the bars
tests/test_ba_groups_gpu.py applies: cost 1e-8 on accepted and 1e-6 on rejected iterations, radius 1e-6, step norm 1e-3, the accept
pattern and the line-search counts exactly, the final parameters at rtol 1e-4 / atol 1e-5.  The cases and the reference's solve of
each are shared through tests/ba_radial_cases.py.  Every non-radial problem must give the bits it gave before the radial entry
points existed: tests/golden/ba_nonradial_parent.npz (tests/ba_nonradial_record.py)."""
import os
import subprocess

import numpy as np
import pytest

import easysfm_amd as E

import ba_groups_cases as gcases
import ba_nonradial_record as record
import ba_radial_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")
LDS_SLABS, TABLES = "SCHUR_LDS_SLABS", "SCHUR_TABLES"
SMALL, LDS, TILED = "SOLVE_SMALL_ONE_WG", "SOLVE_LDS", "SOLVE_TILED"

# the forms each boundary case is meant to take: schur, solve, sweep_sums_in_lds, large, the 6 G block rows of the grouped kernel in LDS
FORMS = {
    "r27": (LDS_SLABS, SMALL, 0, 0, 1), "r28": (LDS_SLABS, LDS, 0, 0, 1),
    "r30": (LDS_SLABS, LDS, 0, 0, 1), "r31": (TABLES, TILED, 0, 0, 1),
    "r111": (TABLES, TILED, 0, 0, 1), "r112": (TABLES, TILED, 0, 0, 0),
    "r538": (TABLES, TILED, 0, 0, 0), "r539": (TABLES, TILED, 0, 0, 0),
    "r27_obs_2p20": (LDS_SLABS, SMALL, 0, 1, 1),
}


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _gpu(name, ctx):
    case, b = cases.CASE_BY_NAME[name], cases.build(name)
    opt = E.default_options(); opt.max_num_iterations = case.iters; opt.cauchy_a = case.cauchy_a
    return E.ba_solve_radial(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, b.sc.cams0, b.sc.pts0, b.grp, b.calib0, b.tol, b.radial0, b.rtol, ref_cam=case.ref_cam,
                             options=opt, ctx=ctx)


def _against_reference(name, out):
    cams, pts, cal, rad, summ = out
    rc, rp, rblk, rlog = cases.reference(name)
    b = cases.build(name)
    log = summ.log()
    print(f"\n[ba radial] {name}: cost {summ.initial_cost:.6f} -> {summ.final_cost:.6f}; accepted {[it.step_is_successful for it in log]}; "
          f"line search {[it.line_search_steps for it in log]}; reference cost {[e['cost'] for e in rlog]}; k {rad.tolist()}", flush=True)
    blk = np.concatenate([cal, rad], 1)
    x = np.concatenate([cams.ravel(), pts.ravel(), blk.ravel()]); rx = np.concatenate([rc.ravel(), rp.ravel(), rblk.ravel()])
    for it, e in zip(log, rlog):
        print(f"    {it.iteration}: cost {it.cost:.12g} / {e['cost']:.12g} ({abs(it.cost - e['cost']) / abs(e['cost']):.1e}), radius "
              f"{abs(it.trust_region_radius - e['radius']) / e['radius']:.1e}, step norm {abs(it.step_norm - e['step_norm']) / max(e['step_norm'], 1e-6):.1e}")
    print(f"    parameters: largest |difference| {np.abs(x - rx).max():.3e}, largest excess over atol + rtol |ref| {(np.abs(x - rx) - 1e-5 - 1e-4 * np.abs(rx)).max():.3e}", flush=True)
    assert len(log) == len(rlog)
    assert [it.step_is_successful for it in log] == [e["ok"] for e in rlog]
    assert [it.line_search_steps for it in log] == [e["ls"] for e in rlog]
    for it, e in zip(log, rlog):
        assert abs(it.cost - e["cost"]) <= (1e-8 if it.step_is_successful else 1e-6) * abs(e["cost"]), (it.iteration, it.cost, e["cost"])
        assert abs(it.trust_region_radius - e["radius"]) <= 1e-6 * e["radius"], it.iteration
        assert abs(it.step_norm - e["step_norm"]) <= 1e-3 * max(e["step_norm"], 1e-6), (it.iteration, it.step_norm, e["step_norm"])
    assert np.allclose(x, rx, rtol=1e-4, atol=1e-5), np.abs(x - rx).max()
    # inside the boxes; and the returned parameters are the ones the final cost was evaluated with
    assert np.all(cal >= b.calib0 - b.tol[:, None]) and np.all(cal <= b.calib0 + b.tol[:, None])
    assert np.all(rad >= b.radial0 - b.rtol[:, None]) and np.all(rad <= b.radial0 + b.rtol[:, None])
    c = cases.problem(name).cost(x)
    assert abs(c - summ.final_cost) <= 1e-10 * summ.final_cost, (c, summ.final_cost)
    assert summ.final_cost < summ.initial_cost


# ---- 1. against the reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one3", "two6", "own5", "ref_squared", "axis"])
def test_radial_matches_reference(gpu_ctx, name):
    out = _gpu(name, gpu_ctx)
    _against_reference(name, out)
    if name in ("ref_squared", "axis"):
        assert np.all(np.abs(out[0][0]) <= 1e-10)             # the reference camera is held
    assert out[2].shape == (cases.CASE_BY_NAME[name].G, 4) and out[3].shape == (cases.CASE_BY_NAME[name].G, 2)


def test_group_nobody_observes_keeps_its_six_values(gpu_ctx):
    """G = 3 with no camera in group 2: its block comes back bit for bit -- from a start that is not zero, so that a write of zeros would
    show -- and the rest follows the reference."""
    b = cases.build("unobserved")
    case = cases.CASE_BY_NAME["unobserved"]
    assert not np.any(b.grp == 2) and len(b.calib0) == 3
    out = _gpu("unobserved", gpu_ctx)
    assert _bytes(out[2][2]) == _bytes(b.calib0[2]) and _bytes(out[3][2]) == _bytes(b.radial0[2])
    _against_reference("unobserved", out)
    rad0 = b.radial0.copy(); rad0[2] = [0.0625, -0.03125]
    opt = E.default_options(); opt.max_num_iterations = case.iters
    cams, pts, cal, rad, summ = E.ba_solve_radial(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, b.sc.cams0, b.sc.pts0, b.grp, b.calib0, b.tol, rad0, b.rtol, options=opt,
                                                  ctx=gpu_ctx)
    assert _bytes(cal[2]) == _bytes(b.calib0[2]) and _bytes(rad[2]) == _bytes(rad0[2])
    assert _bytes(cams) == _bytes(out[0]) and _bytes(rad[:2]) == _bytes(out[3][:2])


def test_tight_radial_box_in_one_group_only(gpu_ctx):
    b = cases.build("tight")
    cams, pts, cal, rad, summ = out = _gpu("tight", gpu_ctx)
    _against_reference("tight", out)
    assert sum(it.line_search_steps for it in summ.log()) > 0
    assert np.any(np.abs(np.abs(rad[0] - b.radial0[0]) - b.rtol[0]) < 1e-12)       # a bound of group 0 is active, exactly
    assert np.all(np.abs(rad[1] - b.radial0[1]) < b.rtol[1] - 0.5)                 # group 1's box is loose


def test_resident_problem_and_accessors(gpu_ctx):
    b = cases.build("two6")
    prob = E.BAProblem(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, None, b.sc.cams0, b.sc.pts0, gpu_ctx, calib_groups=(b.grp, b.calib0, b.tol),
                       radial=b.radial0 + 0.25, radial_tol=b.rtol)
    try:
        assert E.lib().esfm_ba_problem_radial_groups(prob._h) == 2 and E.lib().esfm_ba_problem_calib_groups(prob._h) == 2
        assert _bytes(prob.get_radial_groups()) == _bytes(b.radial0 + 0.25) and _bytes(prob.get_calib_groups()) == _bytes(b.calib0)
        # the pinhole accessors serve a radial problem and leave k1, k2 alone; the radial ones leave the pinhole values alone
        prob.set_calib_groups(b.calib0 * 1.5, [1.0, 2.0])
        assert _bytes(prob.get_calib_groups()) == _bytes(b.calib0 * 1.5) and _bytes(prob.get_radial_groups()) == _bytes(b.radial0 + 0.25)
        prob.set_radial_groups(b.radial0, b.rtol)
        assert _bytes(prob.get_calib_groups()) == _bytes(b.calib0 * 1.5) and _bytes(prob.get_radial_groups()) == _bytes(b.radial0)
        prob.set_calib_groups(b.calib0, b.tol)
        with pytest.raises(RuntimeError, match="radial tolerance must be positive"):
            prob.set_radial_groups(b.radial0, [1.0, 0.0])
        with pytest.raises(RuntimeError, match="or a radial one"):
            prob.get_calib()
        # ... then the solve of case "two6"
        opt = E.default_options(); opt.max_num_iterations = cases.CASE_BY_NAME["two6"].iters
        summ = prob.solve(opt)
        cams, pts = prob.get_params()
        _against_reference("two6", (cams, pts, prob.get_calib_groups(), prob.get_radial_groups(), summ))
    finally:
        prob.close()


def test_radial_accessors_on_a_non_radial_problem_and_the_reverse(gpu_ctx):
    b = gcases.build("mixed")
    for kw in (dict(calib_groups=(b.grp, b.calib0, b.tol)), dict(calib=b.calib0[0], calib_tol=5.0), dict()):
        prob = E.BAProblem(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, b.sc.K4, b.sc.cams0, b.sc.pts0, gpu_ctx, **kw)
        try:
            assert E.lib().esfm_ba_problem_radial_groups(prob._h) == 0
            with pytest.raises(RuntimeError, match="without free radial distortion"):
                prob.get_radial_groups()
            with pytest.raises(RuntimeError, match="without free radial distortion"):
                prob.set_radial_groups(np.zeros((max(prob.n_groups, 1), 2)), 1.0)
        finally:
            prob.close()
    with pytest.raises(ValueError):
        E.BAProblem(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, b.sc.K4, b.sc.cams0, b.sc.pts0, gpu_ctx, radial=np.zeros((1, 2)), radial_tol=1.0)
    # a radial problem with ONE group is not the one-block problem: its one-block accessors are refused
    b = cases.build("one3")
    prob = E.BAProblem(b.sc.cam_idx, b.sc.pt_idx, b.sc.uv, None, b.sc.cams0, b.sc.pts0, gpu_ctx, calib_groups=(b.grp, b.calib0, b.tol), radial=b.radial0,
                       radial_tol=b.rtol)
    try:
        assert E.lib().esfm_ba_problem_radial_groups(prob._h) == 1
        with pytest.raises(RuntimeError, match="or a radial one"):
            prob.set_calib(b.calib0[0], 5.0)
    finally:
        prob.close()


# ---- 2. the size-dependent kernel forms -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forms_of(tmp_path_factory):
    """The host rule's answer for every boundary case: {name: (schur, solve, sweep_sums_in_lds, large, group_rows_in_lds)}."""
    exe = str(tmp_path_factory.mktemp("ba_forms_radial") / "ba_forms_radial_print")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ba_forms_radial_print.cpp"),
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
def test_form_boundaries_with_two_radial_groups(gpu_ctx, forms_of, name):
    """(the 2^20-observation case: its numpy reference takes 17 s on the CPU, under the 20 s from which a stored trace would be used)"""
    _takes_its_forms(name, forms_of)
    assert cases.build(name).sc.n_obs == cases.CASE_BY_NAME[name].n_pt * cases.CASE_BY_NAME[name].per
    _against_reference(name, _gpu(name, gpu_ctx))


def test_cases_reach_every_radial_row_of_the_form_table(forms_of):
    """DESIGN.md section 5.1a, the rows for radial problems."""
    for name in FORMS:
        _takes_its_forms(name, forms_of)
    at = {cases.CASE_BY_NAME[n].n_real: f for n, f in forms_of.items() if not f[3]}
    rows = {
        "one-workgroup solve at its limit (n_cam = 29: n_real = 27 | 28)": at[27][1] == SMALL and at[28][1] == LDS,
        "LDS solve and LDS-slab Schur at their limit (n_cam = 32: n_real = 30 | 31)": at[30][:2] == (LDS_SLABS, LDS) and at[31][:2] == (TABLES, TILED),
        "the 6 G block rows in LDS at their limit (two groups: n_real = 111 | 112)": at[111][4] == 1 and at[112][4] == 0,
        "camera-chunk sums at every size": all(f[2] == 0 for f in forms_of.values()),
        "either side of the one-block sweep's LDS limit (n_real = 538 | 539)": at[538][:2] == (TABLES, TILED) and at[539][:2] == (TABLES, TILED),
        "large (2^20 observations)": forms_of["r27_obs_2p20"][3] == 1 and cases.CASE_BY_NAME["r27_obs_2p20"].n_pt * 8 == 1 << 20,
    }
    missed = [k for k, hit in rows.items() if not hit]
    assert not missed, missed


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two6", "r31"])
def test_two_solves_agree_in_every_bit(gpu_ctx, name):
    a, b = _gpu(name, gpu_ctx), _gpu(name, gpu_ctx)
    for x, y in zip(a[:4], b[:4]):
        assert _bytes(x) == _bytes(y)
    assert _bytes(record._log_bytes(a[4])) == _bytes(record._log_bytes(b[4]))


# ---- 4. every non-radial problem gives the bits it gave -------------------------------------------------------------------------------
def test_non_radial_entry_points_unchanged(gpu_ctx):
    """The shared-block and the grouped solve of three existing-style problems (tests/ba_nonradial_record.py), byte for byte what
    the same calls returned on an MI355X with the library built from the commit before the radial entry points existed."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ba_nonradial_parent.npz"))
    now = record.solves(E, gpu_ctx)
    assert sorted(now) == sorted(gold.files) and len(now) == 8 * len(record.PROBLEMS)
    differ = [k for k in now if _bytes(now[k]) != _bytes(gold[k])]
    assert not differ, differ
