"""One bundle-adjustment solve per size-dependent kernel form, at the sizes where the forms change, against the CPU oracle.

`ba_forms` (easysfm_amd/csrc/ba_forms.cpp, table in DESIGN.md section 5.1a) decides from the camera count, free intrinsics and the
observation count which kernels a problem runs; tests/test_ba_forms.py pins that rule on the CPU.  Here every case names the forms
it is meant to take, asks the host rule itself (tests/cpp/ba_forms_print.cpp, built with g++ against ba_forms.cpp) whether its size
still takes them -- a moved threshold fails the case with "this size no longer takes ..." instead of quietly testing another kernel --
and then solves 3 LM iterations on the GPU and with the oracle.  The bars are the project's existing ones: `_compare` and
RTOL_PAR / ATOL_PAR of tests/test_ba_gpu.py without free intrinsics; `_compare` of tests/test_ba_constrained_gpu.py (line-search counts
included), intrinsics at rtol 1e-7 / atol 1e-5 and the oracle's cost at the returned parameters to 1e-10 with them.
`test_cases_cover_every_form` asserts that the cases together reach every row of the table.

Each case prints its oracle and GPU wall time (pytest -s shows them)."""
import os
import subprocess
import time
from collections import namedtuple

import numpy as np
import pytest

import easysfm_amd as E
from easysfm_amd import synth

import test_ba_constrained_gpu as constrained
from test_ba_gpu import ATOL_PAR, RTOL_PAR, _compare, _solve_both

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")
K0 = np.array(synth.FOUNTAIN_K4, np.float64)
ITERS = 3
KCAMCHUNK = 256                 # kCamChunk of ba_layout.hpp: observations per camera chunk

LDS_SLABS, TABLES = "SCHUR_LDS_SLABS", "SCHUR_TABLES"
SMALL, LDS, TILED = "SOLVE_SMALL_ONE_WG", "SOLVE_LDS", "SOLVE_TILED"

# name; scene: n_real, points, observations per point, seed; free intrinsics; ESFM_BA_SOLVE or None; the forms the size is meant to take:
# schur, solve, sweep_sums_in_lds, large, and with free intrinsics whether ba_schur_calib keeps its block row in LDS ("-" without)
Case = namedtuple("Case", "name n_real n_pt per seed calib mode schur solve sums_in_lds large row_in_lds")
CASES = [
    # fixed intrinsics
    Case("cams29", 29, 1500, 5, 129, 0, None, LDS_SLABS, SMALL, 1, 0, "-"),       # ba_chol_small_kernel at kSmallMaxNb: 174 unknowns, 11 tiles
    Case("cams30", 30, 1500, 5, 130, 0, None, LDS_SLABS, LDS, 1, 0, "-"),         # first ba_chol_solve_kernel size
    Case("cams32", 32, 1500, 5, 132, 0, None, LDS_SLABS, LDS, 1, 0, "-"),         # ba_chol_solve_kernel / ba_schur_lds_kernel at their largest LDS
    Case("cams33_dense", 33, 1500, 5, 133, 0, "dense", TABLES, TILED, 1, 0, "-"),   # first Schur tables, the shortest tiled chain
    Case("cams33_sparse", 33, 1500, 5, 133, 0, "sparse", TABLES, TILED, 1, 0, "-"),  # ... and the shortest structure-aware one
    Case("cams538", 538, 6000, 6, 538, 0, None, TABLES, TILED, 1, 0, "-"),        # the in-LDS sweep sums at 163 696 of 163 840 bytes
    Case("cams539_chunk_edges", 539, 27000, 6, 11, 0, None, TABLES, TILED, 0, 0, "-"),   # camera chunks: the scene of _chunk_edge_scene
    Case("obs_2p20", 29, 131072, 8, 29, 0, None, LDS_SLABS, SMALL, 1, 1, "-"),      # exactly 2^20 observations
    Case("obs_2p20_less_8", 29, 131071, 8, 29, 0, None, LDS_SLABS, SMALL, 1, 0, "-"),
    # free intrinsics: the shared block is camera block n_real, so every n_cam boundary sits one real camera lower
    Case("calib28", 28, 1500, 5, 228, 1, None, LDS_SLABS, SMALL, 1, 0, "1"),
    Case("calib29", 29, 1500, 5, 229, 1, None, LDS_SLABS, LDS, 1, 0, "1"),
    Case("calib31", 31, 1500, 5, 231, 1, None, LDS_SLABS, LDS, 1, 0, "1"),
    Case("calib32", 32, 1500, 5, 232, 1, None, TABLES, TILED, 1, 0, "1"),
    Case("calib341", 341, 6000, 6, 341, 1, None, TABLES, TILED, 1, 0, "1"),      # ba_schur_calib_kernel's block row: exactly 64 KiB of LDS
    Case("calib342", 342, 6000, 6, 342, 1, None, TABLES, TILED, 1, 0, "0"),      # ... and without it
    Case("calib539", 539, 6000, 6, 539, 1, None, TABLES, TILED, 0, 0, "0"),      # ba_camacc_chunk_kernel<true>, the intrinsics block of the final kernel
    Case("calib28_obs_2p20", 28, 131072, 8, 28, 1, None, LDS_SLABS, SMALL, 1, 1, "1"),
]
CASE_BY_NAME = {c.name: c for c in CASES}

# what camera c of the chunk-edge scene must have: none; one observation short of a chunk, a full chunk, a chunk and one; three chunks
# and five; two full chunks at the very last camera
CHUNK_EDGE_COUNTS = {7: 0, 102: KCAMCHUNK - 1, 100: KCAMCHUNK, 101: KCAMCHUNK + 1, 200: 3 * KCAMCHUNK + 5, 538: 2 * KCAMCHUNK}


def _n_obs(case):
    if case.name == "cams539_chunk_edges":
        return len(_scene(case).cam_idx)
    return case.n_pt * min(case.per, case.n_real)


@pytest.fixture(scope="module")
def forms_of(tmp_path_factory):
    """The host rule's answer for every case: {name: (schur, solve, sweep_sums_in_lds, large, calib_row_in_lds)}."""
    exe = str(tmp_path_factory.mktemp("ba_forms") / "ba_forms_print")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ba_forms_print.cpp"),
                        os.path.join(CSRC, "ba_forms.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    args = []
    for c in CASES:
        args += [str(c.n_real), str(c.calib), str(_n_obs(c))]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(CASES), r.stdout
    out = {}
    for c, line in zip(CASES, lines):
        schur, solve, sums, large, row = line.split()
        out[c.name] = (schur, solve, int(sums), int(large), row)
    return out


def _takes_its_forms(case, forms_of):
    got, want = forms_of[case.name], (case.schur, case.solve, case.sums_in_lds, case.large, case.row_in_lds)
    assert got == want, (f"{case.name}: this size ({case.n_real} cameras, free intrinsics {case.calib}, {_n_obs(case)} observations) no longer "
                         f"takes forms {want}: ba_forms says {got}")


def _chunk_edge_scene(case):
    """539 cameras x 27 000 points x 6, edited so that the per-camera observation counts sit on the edges of ba_camacc_chunk_kernel's
    chunks (CHUNK_EDGE_COUNTS): surplus observations of a camera are dropped (its last ones), missing ones are projections of further
    ground-truth points the camera does not see yet, with the scene's 0.5 px noise; then camera-major, point-minor again."""
    sc = synth.ba_scene(case.n_real, case.n_pt, case.per, radius=40.0, extent=8.0, seed=case.seed)
    rng = np.random.default_rng(case.seed)
    cam, pt, uv = sc.cam_idx.copy(), sc.pt_idx.copy(), sc.uv.copy()
    K = K0
    for c, want in CHUNK_EDGE_COUNTS.items():
        mine = np.nonzero(cam == c)[0]
        if len(mine) > want:
            keep = np.ones(len(cam), bool); keep[mine[want:]] = False
            cam, pt, uv = cam[keep], pt[keep], uv[keep]
        elif len(mine) < want:
            seen = np.zeros(sc.n_pt, bool); seen[pt[mine]] = True
            new = np.nonzero(~seen)[0][:want - len(mine)].astype(np.int32)
            P = sc.pts_gt[new] @ synth.aa_to_R(sc.cams_gt[c, :3]).T + sc.cams_gt[c, 3:]
            assert np.all(P[:, 2] > 1.0)                                # in front of the camera
            new_uv = np.stack([P[:, 0] / P[:, 2] * K[0] + K[1], P[:, 1] / P[:, 2] * K[2] + K[3]], 1) + 0.5 * rng.standard_normal((len(new), 2))
            cam = np.concatenate([cam, np.full(len(new), c, np.int32)]); pt = np.concatenate([pt, new]); uv = np.concatenate([uv, new_uv.astype(np.float32)])
    order = np.lexsort((pt, cam))
    return synth.BAScene(cam_idx=np.ascontiguousarray(cam[order], np.int32), pt_idx=np.ascontiguousarray(pt[order], np.int32),
                         uv=np.ascontiguousarray(uv[order], np.float32), K4=sc.K4, cams0=sc.cams0, pts0=sc.pts0, cams_gt=sc.cams_gt, pts_gt=sc.pts_gt)


_scenes, _edge_scene = {}, {}


def _scene(case):
    if case.name == "cams539_chunk_edges":
        if case.name not in _edge_scene:
            _edge_scene[case.name] = _chunk_edge_scene(case)
        return _edge_scene[case.name]
    key = (case.n_real, case.n_pt, case.per, case.seed)
    if key not in _scenes:
        _scenes.clear()                                                 # (one scene at a time: the big ones are 1M observations)
        big = case.n_real > 100
        _scenes[key] = synth.ba_scene(case.n_real, case.n_pt, case.per, radius=40.0 if big else 10.0, extent=8.0 if big else 2.0, seed=case.seed)
    return _scenes[key]


_oracle_runs = {}


def _oracle_fixed(oracle, case, sc):
    """The oracle's solve of a fixed-intrinsics scene: once per scene (the dense and the structure-aware case of 33 cameras share it)."""
    key = (case.n_real, case.n_pt, case.per, case.seed)
    if key not in _oracle_runs:
        _, ropt = _solve_both(oracle, sc, ITERS)
        t = time.perf_counter()
        res = oracle.ba_solve(sc.cam_idx, sc.pt_idx, sc.uv, sc.K4, sc.cams0, sc.pts0, ropt)
        _oracle_runs[key] = (res, time.perf_counter() - t)
    return _oracle_runs[key]


def _gpu_fixed(case, sc, ctx):
    opt = E.default_options(); opt.max_num_iterations = ITERS
    old = os.environ.get("ESFM_BA_SOLVE")
    try:
        if case.mode:
            os.environ["ESFM_BA_SOLVE"] = case.mode
        t = time.perf_counter()
        out = E.ba_solve(sc.cam_idx, sc.pt_idx, sc.uv, sc.K4, sc.cams0, sc.pts0, opt, ctx)
        return out, time.perf_counter() - t
    finally:
        os.environ.pop("ESFM_BA_SOLVE", None)
        if old is not None:
            os.environ["ESFM_BA_SOLVE"] = old


def _report(case, forms, t_oracle, t_gpu, summ):
    print(f"\n[ba forms] {case.name}: {case.n_real} cameras, free intrinsics {case.calib}, {_n_obs(case)} observations -> {' '.join(map(str, forms))}; "
          f"oracle {t_oracle:.2f} s, GPU {t_gpu:.3f} s; cost {summ.initial_cost:.3f} -> {summ.final_cost:.3f}, "
          f"steps accepted {[it.step_is_successful for it in summ.log()][1:]}", flush=True)


@pytest.mark.parametrize("name", [c.name for c in CASES if not c.calib and c.name != "cams539_chunk_edges"])
def test_fixed_intrinsics_form_matches_oracle(gpu_ctx, oracle_lib, forms_of, name):
    case = CASE_BY_NAME[name]
    _takes_its_forms(case, forms_of)
    sc = _scene(case)
    assert sc.n_obs == _n_obs(case)
    (cams, pts, summ), t_gpu = _gpu_fixed(case, sc, gpu_ctx)
    (rc, rp, rs), t_oracle = _oracle_fixed(oracle_lib, case, sc)
    _report(case, forms_of[name], t_oracle, t_gpu, summ)
    _compare(summ, rs, oracle_lib)
    assert np.allclose(cams, rc, rtol=RTOL_PAR, atol=ATOL_PAR) and np.allclose(pts, rp, rtol=RTOL_PAR, atol=ATOL_PAR)
    assert summ.final_cost < summ.initial_cost


def test_camera_chunk_edges_match_oracle(gpu_ctx, oracle_lib, forms_of):
    """The camera-chunk form of the per-camera sums (539 cameras: ba_linearize_kernel without its LDS sums, ba_camacc_chunk_kernel,
    ba_camacc_final_kernel) with cameras of 0, 255, 256, 257, 3 * 256 + 5 and -- the last camera -- 512 observations: an empty chunk
    list, a chunk one short of full, a full one, a chunk of ONE observation behind a full one, several chunks added in order.  The
    camera nobody observes must come back bit-identical."""
    case = CASE_BY_NAME["cams539_chunk_edges"]
    _takes_its_forms(case, forms_of)
    sc = _scene(case)
    counts = np.bincount(sc.cam_idx, minlength=sc.n_cam)
    assert {c: int(counts[c]) for c in CHUNK_EDGE_COUNTS} == CHUNK_EDGE_COUNTS
    assert np.all(np.diff(sc.cam_idx) >= 0)                             # camera-major
    assert np.bincount(sc.pt_idx, minlength=sc.n_pt).min() >= 2
    (cams, pts, summ), t_gpu = _gpu_fixed(case, sc, gpu_ctx)
    (rc, rp, rs), t_oracle = _oracle_fixed(oracle_lib, case, sc)
    _report(case, forms_of[case.name], t_oracle, t_gpu, summ)
    _compare(summ, rs, oracle_lib)
    assert np.allclose(cams, rc, rtol=RTOL_PAR, atol=ATOL_PAR) and np.allclose(pts, rp, rtol=RTOL_PAR, atol=ATOL_PAR)
    assert np.array_equal(cams[7], sc.cams0[7]) and np.array_equal(rc[7], sc.cams0[7])
    assert summ.num_active_cameras == rs.num_active_cameras == sc.n_cam - 1
    assert summ.final_cost < summ.initial_cost


@pytest.mark.parametrize("name", [c.name for c in CASES if c.calib])
def test_free_intrinsics_form_matches_oracle(gpu_ctx, oracle_lib, forms_of, name):
    case = CASE_BY_NAME[name]
    _takes_its_forms(case, forms_of)
    sc = _scene(case)
    assert sc.n_obs == _n_obs(case)
    calib0 = K0 * np.array([1.01, 1.0, 0.99, 1.0])
    opt, ropt = constrained._opts(oracle_lib, ITERS)
    t = time.perf_counter()
    cams, pts, cal, summ = E.ba_solve_ex(sc.cam_idx, sc.pt_idx, sc.uv, None, sc.cams0, sc.pts0, calib=calib0, calib_tol=30.0, options=opt, ctx=gpu_ctx)
    t_gpu = time.perf_counter() - t
    t = time.perf_counter()
    rc, rp, rk, rs = oracle_lib.ba_solve_ex(sc.cam_idx, sc.pt_idx, sc.uv, None, sc.cams0, sc.pts0, calib=calib0, calib_tol=30.0, options=ropt)
    t_oracle = time.perf_counter() - t
    _report(case, forms_of[name], t_oracle, t_gpu, summ)
    constrained._compare(summ, rs, oracle_lib)
    assert np.allclose(cal, rk, rtol=1e-7, atol=1e-5)
    c = oracle_lib.ba_cost_calib(sc.cam_idx, sc.pt_idx, sc.uv, cal, cams, pts)
    assert abs(c - summ.final_cost) <= 1e-10 * summ.final_cost
    assert summ.final_cost < summ.initial_cost


def test_cases_cover_every_form(forms_of):
    """The union of the cases above, as the host rule sees them: every value of schur, solve, sweep_sums_in_lds and large, without and
    with free intrinsics; both sides of ba_schur_calib's block-row threshold; and each boundary size of the table."""
    for c in CASES:
        _takes_its_forms(c, forms_of)
    for calib in (0, 1):
        seen = [forms_of[c.name] for c in CASES if c.calib == calib]
        assert {f[0] for f in seen} == {LDS_SLABS, TABLES}, calib
        assert {f[1] for f in seen} == {SMALL, LDS, TILED}, calib
        assert {f[2] for f in seen} == {0, 1}, calib
        assert {f[3] for f in seen} == {0, 1}, calib
    assert {forms_of[c.name][4] for c in CASES if c.calib} == {"0", "1"}
    assert {forms_of[c.name][4] for c in CASES if not c.calib} == {"-"}
    at = {(c.n_real, c.calib): forms_of[c.name] for c in CASES if not forms_of[c.name][3]}
    rows = {
        "camera chunks (n_real >= 539)": at[(539, 0)][2] == 0 and at[(539, 1)][2] == 0,
        "LDS sweep sums at their limit (n_real = 538)": at[(538, 0)][2] == 1 and at[(539, 0)][2] == 0,
        "one-workgroup solve at its limit (n_cam = 29)": at[(29, 0)][1] == SMALL and at[(30, 0)][1] == LDS,
        "LDS solve and LDS-slab Schur at their limits (n_cam = 32)": at[(32, 0)][:2] == (LDS_SLABS, LDS),
        "first Schur tables / tiled solve (n_cam = 33), dense and structure-aware":
            at[(33, 0)][:2] == (TABLES, TILED) and {c.mode for c in CASES if c.n_real == 33 and not c.calib} == {"dense", "sparse"},
        "the four boundaries with free intrinsics (n_real = 28, 29, 31, 32)":
            at[(28, 1)][:2] == (LDS_SLABS, SMALL) and at[(29, 1)][:2] == (LDS_SLABS, LDS) and at[(31, 1)][:2] == (LDS_SLABS, LDS)
            and at[(32, 1)][:2] == (TABLES, TILED),
        "ba_schur_calib without its LDS row (n_real >= 342)": at[(341, 1)][4] == "1" and at[(342, 1)][4] == "0",
        "large beside the LDS-slab Schur and the one-workgroup solve, without and with free intrinsics":
            all(any(c.calib == calib and forms_of[c.name][:4] == (LDS_SLABS, SMALL, 1, 1) for c in CASES) for calib in (0, 1))
            and forms_of["obs_2p20_less_8"][3] == 0 and _n_obs(CASE_BY_NAME["obs_2p20"]) == 1 << 20,
    }
    missed = [k for k, hit in rows.items() if not hit]
    assert not missed, missed
