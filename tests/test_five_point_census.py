"""A census of the 5-point solver against an OUTSIDE reference.

tests/test_five_point_stages.py compares the product with oracle/ransac_ref.c, which restates the product's arithmetic to the letter: a
shared mistake passes it.  Here the judge is tests/five_point_ref.py -- numpy's SVD, the ten constraints expanded as polynomials,
the multiplication matrix of x and numpy's eigenvectors: no step in common -- on 2 048 samples drawn the way RANSAC draws them
(test_five_point_stages.samples: noise, gross outliers, planar scenes, tiny baselines, repeated and collinear correspondences).

What is measured, on the samples the reference does not call degenerate or grey:
  quality       r(E) = max(|x2'E x1| on the sample, |det E|, max |2 E E'E - tr(E E')E|) of every model; no matching of models needed
  completeness  does the product return the reference's models -- the same number, each within 1e-8 (1e-6)?  How far the reference
                agrees with ITSELF on another null-space basis (the oracle's) is measured first: that share is inherent in the sample.
The bounds are the reference's own shares plus a sampling allowance; nothing is taken from what the product returns.

Measured (2 048 samples, 89 left out: 86 degenerate, 3 grey; shares of the 1 959 kept):
                                               reference    product       product before refine_solution (parent commit)
  samples with a model of r > 1e-10            92  4.70 %     6  0.31 %   273  13.94 %      <- failed: bound 5.70 %
  largest r of any model                       1.16e-4      3.38e-4       7.33e-2           <- failed: bound 1.16e-2
  disagree in count or beyond 1e-8             60  3.06 %    65  3.32 %   197  10.06 %      <- failed: bound 4.06 %
  disagree in count or beyond 1e-6             12  0.61 %    20  1.02 %    95   4.85 %      <- failed: bound 1.11 %
  (reference column of the last two rows: the reference on its SVD basis against the reference on the oracle's basis)
What remains after the refinement is the completeness gap: root clusters of det B(z) that the root finder returns as complex pairs (a
missed pair of models: samples 417, 1215, 1550), complex pairs taken for real ones (spurious models of r 5e-6 .. 3e-4: samples 38, 930),
a near-double solution that the steps approach only linearly (two models left at r 1e-5: sample 1619) and two roots refined towards
the same solution (a near-duplicate and a missed model: samples 37, 233, 1824).  Nine samples of 1 959;
the other eleven of the twenty are samples where the REFERENCE is the inaccurate side (its r 1e-7, the product's 1e-16)."""
from types import SimpleNamespace

import numpy as np
import pytest

import easysfm_amd as E
import five_point_ref as ref
from test_five_point_stages import samples

SEEDS = ((303, 16), (404, 16))      # samples(seed, n_problems): 1 024 samples each; sample k of the census = sample k % 1024 of seed k // 1024
R_GOOD = 1e-10                      # a model with r above this has lost accuracy somewhere (eps x a condition number of 1e6)


def quality_count(Es, nm, q1, q2, keep):
    """the samples among `keep` whose worst model has r > R_GOOD, and the largest r of all"""
    worst = np.array([ref.worst_residual(Es[k, :nm[k]], q1[k], q2[k]) for k in keep])
    return int((worst > R_GOOD).sum()), float(worst.max())


def disagreements(A, B, keep, tol):
    """the samples among `keep` where two lists of model sets differ in count or by more than tol in some model"""
    return [int(k) for k in keep if len(A[k]) != len(B[k]) or ref.model_distance(A[k], B[k]) > tol]


@pytest.fixture(scope="module")
def census(oracle_lib):
    q1, q2 = (np.concatenate(x) for x in zip(*(samples(seed, n) for seed, n in SEEDS)))
    c = SimpleNamespace(q1=q1, q2=q2, n=len(q1))
    c.ref_svd = ref.solve_many(q1, q2)
    c.Es, c.nm, st = E.five_point_models(q1, q2, host=True, stages=True)              # the product: the host build of the kernels' routines
    c.ref_orc = ref.solve_many(q1, q2, basis=st[:, :36].reshape(-1, 4, 9))            # the reference again, on the product's basis
    c.degenerate = np.array([r["degenerate"] for r in c.ref_svd])
    c.grey = np.array([a["grey"] or b["grey"] for a, b in zip(c.ref_svd, c.ref_orc)]) & ~c.degenerate
    c.keep = np.nonzero(~c.degenerate & ~c.grey)[0]
    c.product = [c.Es[k, :c.nm[k]] for k in range(c.n)]
    c.A = [r["models"] for r in c.ref_svd]; c.B = [r["models"] for r in c.ref_orc]
    return c


def test_host_build_is_the_oracle_on_the_census(census, oracle_lib):
    """the product side of the census stands for the CPU oracle too: bit for bit"""
    for k in range(census.n):
        assert np.array_equal(oracle_lib.five_point(census.q1[k], census.q2[k]), census.product[k], equal_nan=True), k


def test_few_samples_are_left_out(census):
    """a condition of the census, not a measurement: 86 degenerate (4.2 %: the repeated and the collinear ones) + 3 grey of 2 048"""
    assert census.n >= 2000
    left = census.n - len(census.keep)
    print(f"left out {left} of {census.n}: {int(census.degenerate.sum())} degenerate, {int(census.grey.sum())} grey")
    assert left <= 0.08 * census.n


def test_reference_residual_measures_what_it_says():
    """r of an exact essential matrix through its own sample is rounding noise; r sees a broken constraint"""
    rng = np.random.default_rng(1)
    t = np.array([0.3, -1.0, 0.2]); Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0]; Rm *= np.sign(np.linalg.det(Rm))
    X = rng.uniform(-1, 1, (5, 3)) + [0, 0, 5.0]; Xc = X @ Rm.T + t
    q1 = X[:, :2] / X[:, 2:]; q2 = Xc[:, :2] / Xc[:, 2:]
    Et = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ Rm
    assert ref.residual(Et, q1, q2) < 1e-14
    assert ref.residual(Et + 1e-6 * np.eye(3), q1, q2) > 1e-7
    out = ref.solve(q1, q2)
    assert not out["degenerate"] and min(np.abs(M - ref.canonical(Et)).max() for M in out["models"]) < 1e-9


def test_model_quality(census):
    c = census
    bad_p, max_p = quality_count(c.Es, c.nm, c.q1, c.q2, c.keep)
    worst_ref = np.array([ref.worst_residual(c.A[k], c.q1[k], c.q2[k]) for k in c.keep])
    bad_r, max_r = int((worst_ref > R_GOOD).sum()), float(worst_ref.max())
    print(f"r > {R_GOOD:g}: product {bad_p} ({bad_p / len(c.keep):.2%}), reference {bad_r} ({bad_r / len(c.keep):.2%}) of {len(c.keep)}; "
          f"largest r: product {max_p:.3g}, reference {max_r:.3g}")
    # measured: product 6 (0.31 %), reference 92 (4.70 %) of 1 959; parent commit: product 273 (13.94 %) -> failed
    assert bad_p / len(c.keep) <= bad_r / len(c.keep) + 0.01                          # one point: the sampling allowance (20 of 2 000)
    # measured: product 3.38e-4 (a complex pair taken for a real root, sample 38), reference 1.16e-4; parent commit: 7.33e-2 -> failed.
    # 100 x: the gap between an ill-conditioned solution and a wrong one
    assert max_p <= 100.0 * max_r


def test_completeness(census):
    c = census
    n = len(c.keep)
    s8, s6 = (len(disagreements(c.A, c.B, c.keep, tol)) / n for tol in (1e-8, 1e-6))   # inherent: the reference against itself on another basis
    p8, p6 = (disagreements(c.product, c.A, c.keep, tol) for tol in (1e-8, 1e-6))
    print(f"beyond 1e-8: reference/reference {s8:.2%}, product/reference {len(p8) / n:.2%} ({len(p8)}); "
          f"beyond 1e-6: {s6:.2%}, {len(p6) / n:.2%} ({len(p6)}: {p6})")
    # measured: s = 3.06 % (60), product 3.32 % (65); parent commit: 10.06 % (197)
    assert len(p8) / n <= s8 + 0.01
    # measured: reference 0.61 % (12), product 1.02 % (20); parent commit: 4.85 % (95) -> failed
    assert len(p6) / n <= s6 + 0.005


# The two samples that showed the gap first, kept by name (index in the census = index in samples(303, 16)).
MISSED_CLUSTER = 417       # the reference finds 6 solutions, the product 2: four roots of det B(z) form a cluster that comes back complex
SPURIOUS_ROOTS = 38        # the reference finds 4, the product 6: two complex pairs close to the real axis pass the real-root gate


def test_known_case_missed_cluster(census):
    c, k = census, MISSED_CLUSTER
    for run in (c.A, c.B):                                   # the six solutions are real ones: on both bases, each to 1e-9
        assert len(run[k]) == 6 and ref.worst_residual(run[k], c.q1[k], c.q2[k]) < 1e-9
    assert ref.model_distance(c.A[k], c.B[k]) < 1e-8
    P = c.product[k].reshape(-1, 9)
    print(f"sample {k}: product {len(P)} models, reference 6")
    assert 2 <= len(P) <= 6                                  # (2 today: the cluster is missed, before and after the refinement)
    assert ref.worst_residual(c.product[k], c.q1[k], c.q2[k]) < R_GOOD
    for M in P:                                              # what the product returns is among the reference's solutions
        assert np.abs(c.A[k].reshape(-1, 9) - M).max(axis=1).min() < 1e-8


def test_known_case_spurious_roots(census):
    c, k = census, SPURIOUS_ROOTS
    assert len(c.A[k]) == 4 and len(c.B[k]) == 4
    P = c.product[k]
    r = np.array([ref.residual(M, c.q1[k], c.q2[k]) for M in P])
    print(f"sample {k}: product {len(P)} models, r = {r}")
    # parent commit: six models, three of them with r 2e-5 .. 7e-4 and two more above 1e-10; today: six, the two that belong to no
    # solution stay at r ~ 3e-4 (the refinement moves them nowhere better: they are kept as they were), the other four below 1e-15
    assert 4 <= len(P) <= 6 and (r > R_GOOD).sum() <= 2
    # the good ones are the reference's four, as far as the reference is good here (cond 8.5e6; its two runs differ by 7e-6)
    tol = 10.0 * ref.model_distance(c.A[k], c.B[k])
    assert (r <= R_GOOD).sum() == 4
    for M in P[r <= R_GOOD]:
        assert np.abs(c.A[k].reshape(-1, 9) - M.ravel()).max(axis=1).min() < tol


@pytest.mark.gpu
def test_kernels_give_the_census_models(census, gpu_ctx):
    """essential_roots_kernel on the census samples: the host build's models bit for bit, and so the same quality count"""
    c = census
    Es_g, nm_g = E.five_point_models(c.q1, c.q2, gpu_ctx)
    assert np.array_equal(nm_g, c.nm)
    for k in range(c.n):
        assert np.array_equal(Es_g[k, :nm_g[k]], c.product[k], equal_nan=True), k
    assert quality_count(Es_g, nm_g, c.q1, c.q2, c.keep) == quality_count(c.Es, c.nm, c.q1, c.q2, c.keep)
