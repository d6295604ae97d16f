"""The fundamental-matrix model and the focal-length cost without a GPU (esfm.h "Fundamental-matrix RANSAC"): the host builds of
easysfm_amd/csrc/fundamental_core.hpp against the Python restatement (tests/fundamental_ref.py route (a), bit for bit), the restatement
against an independent numpy.linalg.svd + numpy.roots route (route (b)), and the focal verdicts on the two synthetic scenes."""
import numpy as np
import pytest

import fundamental_cases as Cs
import fundamental_ref as R


@pytest.fixture(scope="module")
def M():
    from easysfm_amd import motion
    return motion


@pytest.fixture(scope="module")
def samples():
    return Cs.solver_samples()


@pytest.fixture(scope="module")
def ref_models(samples):
    q1, q2 = samples
    return [R.minimal_solve(q1[i], q2[i], detail=True) for i in range(len(q1))]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _packed(models):
    out = np.zeros((len(models), 27))
    for g, ms in enumerate(models):
        for k, F in enumerate(ms):
            out[g, 9 * k:9 * k + 9] = F
    return out.reshape(-1, 3, 3, 3)


def test_host_build_equals_the_restatement_bit_for_bit(M, samples, ref_models):
    """esfm_fundamental_models_host == route (a) on the 4096 samples (sampled sevens of two general pairs and a plane, noisy collinear
    sevens, repeated points, the hand-made degenerate ones): every model and the model count.  The restatement itself gives at least
    256 samples one model and at least 256 three."""
    q1, q2 = samples
    assert len(q1) == 4096
    F, nm = M.fundamental_models(q1, q2, host=True)
    na = np.array([len(r[0]) for r in ref_models])
    print(f"\n[fundamental] model counts of the restatement: {np.bincount(na, minlength=4)}")
    assert np.count_nonzero(na == 1) >= 256 and np.count_nonzero(na == 3) >= 256
    assert np.array_equal(nm, na)
    assert np.array_equal(_bits(F), _bits(_packed([r[0] for r in ref_models])))
    # the models are canonical: unit Frobenius norm, the entry of largest magnitude positive
    for g in np.nonzero(nm)[0][:500]:
        for k in range(nm[g]):
            f = F[g, k].reshape(9)
            assert abs(np.linalg.norm(f) - 1.0) < 1e-14 and f[np.argmax(np.abs(f))] > 0.0
    # seven identical points, a non-finite coordinate and a collapsed second image give no model
    assert nm[-8] == 0 and nm[-4] == 0 and nm[-1] == 0 and not F[-8].any() and not F[-4].any() and not F[-1].any()


def test_restatement_against_the_svd_and_roots_route(samples, ref_models):
    """Route (a) against route (b) on the same 4096 samples.  Excluded: samples whose normalised system route (b) finds rank-deficient
    (sigma_7 <= 1e-10 sigma_1 or not finite: the null space is then not unique and the two routes legitimately span different ones)
    and samples with a near-double root (two roots of route (b) closer than 1e-6, or a complex pair with an imaginary part below
    1e-6): together at most 1 % of the samples.  On the others the model count equals route (b)'s number of real roots, and every model's
    max |x2' F x1| over its seven points and |det F|, in the normalised frame at unit norm, stay below 16 x the largest value route
    (b)'s own models show on the same samples.
    Measured: 23 rank-deficient samples (0.56 %), none near-double; route (a) 4.3e-15 and 2.4e-16, route (b) 3.6e-15 and 7.0e-16."""
    q1, q2 = samples
    excluded = 0
    worst_a, worst_b = [0.0, 0.0], [0.0, 0.0]
    for g in range(len(q1)):
        b = R.svd_route(q1[g], q2[g])
        if b is None or not b["sv"][6] > 1e-10 * b["sv"][0]:
            excluded += 1
            continue
        r = b["roots"]
        sep = min(abs(r[i] - r[j]) for i in range(3) for j in range(i))
        imag = [abs(z.imag) for z in r if z.imag != 0.0]
        if sep < 1e-6 or (imag and min(imag) < 1e-6):
            excluded += 1
            continue
        normalised = ref_models[g][1]["normalised"]
        assert len(normalised) == len(b["real"]), (g, len(normalised), r)
        for fn in normalised:
            e, d = R.residuals_normalised(fn, b["A"])
            worst_a = [max(worst_a[0], e), max(worst_a[1], d)]
        for fn in b["models"]:
            e, d = R.residuals_normalised(fn, b["A"])
            worst_b = [max(worst_b[0], e), max(worst_b[1], d)]
    print(f"\n[fundamental] excluded {excluded} of {len(q1)}; route (a) {worst_a}, route (b) {worst_b}")
    assert excluded <= 0.01 * len(q1)
    assert worst_a[0] <= 16.0 * worst_b[0] and worst_a[1] <= 16.0 * worst_b[1]


def test_cubic_rule_on_hand_made_polynomials():
    """The written root rule where the sampled cubics do not reach: a vanishing leading coefficient (quadratic, linear, nothing), a
    double root met exactly, three well separated roots in ascending order."""
    assert R.cubic_roots([0.0, 0.0, 0.0, 0.0]) == []
    assert R.cubic_roots([1.0, 0.0, 0.0, 0.0]) == []
    assert R.cubic_roots([-2.0, 4.0, 0.0, 0.0]) == [0.5]
    assert R.cubic_roots([2.0, -3.0, 1.0, 0.0]) == [1.0, 2.0]                 # the root at infinity is dropped
    assert R.cubic_roots([1.0, -2.0, 1.0, 1e-13]) == [1.0]                    # disc == 0
    assert R.cubic_roots([1.0, 0.0, 1.0, 0.0]) == []
    got = R.cubic_roots([-6.0, 11.0, -6.0, 1.0])
    assert len(got) == 3 and np.allclose(got, [1.0, 2.0, 3.0], rtol=0, atol=1e-14)
    got = R.cubic_roots([1.0, 1.0, 1.0, 1.0])                                  # monotone: one root, -1
    assert got == [-1.0]
    assert R.cubic_roots([float("nan"), 1.0, 1.0, 1.0]) == []


def test_refit_host_equals_the_restatement(M):
    """esfm_fundamental_refit_host == the restatement, bit for bit: all points, a mask, more points than lanes, exactly 8; fewer than 8 is
    an error on both sides.  The result has rank 2."""
    sets = Cs.correspondence_sets()
    a, b = sets["general"]
    rng = np.random.default_rng(3)
    cases = [(a, b, None), (a, b, rng.random(len(a)) < 0.6), (a[:300], b[:300], None), (a[:8], b[:8], None), (sets["plane"][0][:257], sets["plane"][1][:257], None)]
    for p1, p2, mask in cases:
        Fr, ok = R.refit(p1, p2, mask)
        assert ok
        Fh = M.fundamental_refit_host(p1, p2, mask)
        assert np.array_equal(_bits(Fh.reshape(9)), _bits(Fr))
        assert np.linalg.svd(Fh, compute_uv=False)[2] < 1e-12
    from easysfm_amd import EsfmError
    assert R.refit(a[:7], b[:7])[1] is False
    with pytest.raises(EsfmError):
        M.fundamental_refit_host(a[:7], b[:7])
    # the re-fit of noisy true correspondences is the epipolar geometry: every point within a pixel of its line
    e1, e2 = R.epipolar_errors(M.fundamental_refit_host(a, b), a, b)
    assert np.max(e1) < 4.0 and np.max(e2) < 4.0 and np.median(e1) < 0.3


def test_sample_stream_equals_the_restatement(M):
    for count in (7, 8, 50, 1000):
        assert np.array_equal(M.fundamental_sample_stream(count, 200), R.sample_stream(count, 200))
    idx = M.fundamental_sample_stream(9, 500)
    assert all(len(set(r)) == 7 for r in idx.tolist()) and idx.min() == 0 and idx.max() == 8


@pytest.fixture(scope="module")
def freehand_fundamentals():
    return [Cs.scene_fundamentals(Cs.freehand_scene(seed)[0]) for seed in range(5)]


def test_focal_cost_host_equals_the_restatement(M, freehand_fundamentals):
    """esfm_focal_cost_host == the restatement on both sweeps' candidates, bit for bit, also with more pairs than lanes."""
    Fs, w = freehand_fundamentals[0]
    cand = M.focal_candidates(0.3 * 768, 3.0 * 768)[::4]
    assert np.array_equal(_bits(M.focal_cost(Fs, w, 384.0, 256.0, cand, host=True)), _bits(R.focal_cost(Fs, w, 384.0, 256.0, cand)))
    many = np.concatenate([f for f, _ in freehand_fundamentals] * 2); wm = np.concatenate([x for _, x in freehand_fundamentals] * 2)
    assert len(many) > 256
    cand = np.array([300.0, 620.0, 1500.0])
    assert np.array_equal(_bits(M.focal_cost(many, wm, 380.0, 250.0, cand, host=True)), _bits(R.focal_cost(many, wm, 380.0, 250.0, cand)))


def test_focal_term_vanishes_for_an_essential_matrix(M):
    """K' F K of an exact F = K^-T [t]x R K^-1 is an essential matrix: the cost at the true f is at rounding level, away from it not."""
    K = np.array([[620.0, 0, 384.0], [0, 620.0, 256.0], [0, 0, 1.0]])
    from easysfm_amd.synth import aa_to_R
    Rm = aa_to_R(np.array([0.1, -0.2, 0.05])); t = np.array([1.0, 0.2, -0.3])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(K).T @ tx @ Rm @ np.linalg.inv(K)
    c = M.focal_cost(F.reshape(1, 9), [1.0], 384.0, 256.0, [620.0, 400.0, 900.0], host=True)
    assert c[0] < 1e-12 and c[1] > 1e-3 and c[2] > 1e-3


def test_focal_verdicts_on_the_two_scenes(M, freehand_fundamentals):
    """The 8-point F of the true correspondences (0.3 px noise) of all pairs, eight cameras.  Free-hand scene, seeds 0 - 4: the coarse
    minimum is the grid candidate nearest 620 or a neighbour, and the estimate is confident (depth >= 0.01).  Arc scene (cameras
    equidistant from the point they fixate, the critical configuration): not confident.
    Measured: free-hand depth 0.082 .. 0.092, f 619.9 .. 621.4; arc depth 3.0e-4 with the minimum at the grid's end."""
    for seed, (Fs, w) in enumerate(freehand_fundamentals):
        est = M.focal_from_fundamentals(Fs, w, Cs.WIDTH, Cs.HEIGHT, host=True)
        near = int(np.argmin(np.abs(est["coarse"][0] - Cs.FREEHAND_F)))
        print(f"\n[focal] free-hand seed {seed}: {len(Fs)} pairs, f {est['f']:.2f}, coarse index {est['coarse_index']} (nearest {near}), depth {est['depth']:.4f}")
        assert abs(est["coarse_index"] - near) <= 1
        assert est["confident"] and est["depth"] >= 0.01
        assert len(est["coarse"][0]) == 129 and len(est["fine"][0]) == 129
        assert est["coarse"][0][0] == pytest.approx(0.3 * 768) and est["coarse"][0][-1] == pytest.approx(3.0 * 768)
    Fs, w = Cs.scene_fundamentals(Cs.arc_scene()[0])
    est = M.focal_from_fundamentals(Fs, w, Cs.WIDTH, Cs.HEIGHT, host=True)
    print(f"[focal] arc: {len(Fs)} pairs, f {est['f']:.2f}, depth {est['depth']:.2e}")
    assert not est["confident"]


def test_calibrate_hook_default_and_options():
    """match_and_verify_all_pairs takes `calibrate` (default None), run_sfm takes `auto_focal` (default None); a frame without an image
    needs AutoFocalOptions.image_size."""
    import inspect
    import easysfm_amd as E
    from easysfm_amd import pipeline
    assert inspect.signature(pipeline.match_and_verify_all_pairs).parameters["calibrate"].default is None
    assert inspect.signature(pipeline.run_sfm).parameters["auto_focal"].default is None
    fr = E.Frame(frame_id=0, keypoints=np.zeros((1, 2), np.float32), descriptors=np.zeros((1, 64), np.float32))
    with pytest.raises(ValueError, match="image size"):
        pipeline.auto_focal_calibration([fr], E.AutoFocalOptions(), 1.0, 20, ctx=object())
    pipeline.auto_focal_calibration([fr], E.AutoFocalOptions(image_size=(768, 512)), 1.0, 20, ctx=object())


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_host_header_on_degenerate_samples_under_sanitizers(tmp_path, flags):
    """tests/cpp/fundamental_degenerate_main.cpp: a stand-alone host program (its own main, g++, no GPU) that runs the host build of
    fundamental_core.hpp on the degenerate samples, the cubic rule's edges, the re-fit and the focal cost; plainly and with
    -fsanitize=address,undefined"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fundamental_degenerate")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(root, "tests", "cpp", "fundamental_degenerate_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "fundamental degenerate check ok" in r.stdout, r.stdout[-4000:]


def test_drivers_and_the_word_auto(tmp_path):
    """bin/sfm_native refuses `auto` as calib_K_file with a clear message (as it refuses +radial); bin/sfm refuses `auto` together with
    +cameras before any work"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    native = os.path.join(root, "bin", "sfm_native")
    if not os.path.exists(native):
        import __graft_entry__ as g
        g.build()
    args = [str(tmp_path), str(tmp_path / "list.txt"), "auto", "none", str(tmp_path / "out.ply"), "S", "300", "1.0", "1", "50", "4", "0", "0"]
    r = subprocess.run([native, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 2 and "auto" in r.stdout and "bin/sfm" in r.stdout, r.stdout
    (tmp_path / "list.txt").write_text("")
    r = subprocess.run([sys.executable, os.path.join(root, "bin", "sfm"), *args, "ratio+cameras"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 3 and "auto takes" in r.stdout, r.stdout
    # with ba_calib_change_tolerance 0 one line advises a non-zero tolerance (printed before any work; the empty image list ends the run)
    args[9] = "0"
    r = subprocess.run([sys.executable, os.path.join(root, "bin", "sfm"), *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 2 and r.stdout.count("Auto focal: ba_calib_change_tolerance is 0") == 1, r.stdout
