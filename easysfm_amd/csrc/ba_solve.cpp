// esfm_ba_problem_solve: the Levenberg-Marquardt loop over a resident problem.
// The control flow restates Ceres' TrustRegionMinimizer + LevenbergMarquardtStrategy
// with DENSE_SCHUR, which is what BundleAdjustment::solveBA configures (reference
// cpp_code/src/ba.cpp:146-151, :201-206); the oracle (oracle/ba_ref.c) documents the upstream rules.
// All arithmetic on the observations runs in ba_linearize.hip, ba_schur.hip and ba_step.hip; this file only sequences kernels, reads
// back a handful of scalars per iteration and takes the accept/reject decision.
#include <chrono>
#include <thread>
#include <cstdlib>
#include <cmath>
#include <cfloat>
#include <vector>

#include "ba_problem.hpp"
#include "ba_linesearch.hpp"
#include "ba_sparse_plan.hpp"

using esfm::BADev;

namespace {

// upper bound (seconds) on the host's wait for one scalar read-back; see Solver::fetch_scal
long readback_timeout_s()
{
    static const long v = [] {
        const char *e = getenv("ESFM_BA_READBACK_TIMEOUT_S");
        const long t = e ? atol(e) : 0;
        return t > 0 ? t : 600L;
    }();
    return v;
}

int fill_ones(hipStream_t st, double *dst, size_t n)
{
    std::vector<double> ones(n, 1.0);
    if (n == 0) return ESFM_OK;
    ESFM_HIP_TRY(esfm::copy_h2d(dst, ones.data(), sizeof(double) * n, st));
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return ESFM_OK;
}

struct Solver {
    esfm_ba_problem *P;
    esfm_ba_options opt;
    esfm_allreduce_fn ar;
    void *ar_user;
    hipStream_t st;
    esfm_ba_summary *sum;
    double *h = nullptr;        // P->h_scal
    bool multi = false, constrained = false;
    // state of the trust-region loop
    double radius = 0.0, decrease_factor = 2.0;
    double x_cost = 0.0, x_norm = 0.0, gmax = 0.0;
    double prep_radius = 0.0;     // radius the per-point inverses were built with
    bool prep_singular = false;   // ... and whether one of them could not be inverted (any rank)
    int n_invalid = 0;
    bool terminated = false;
    int rc_final = ESFM_OK;
    // the deferred read-back of an accepted step's re-linearisation (see run)
    bool pending_lin = false;
    double pending_cost_bound = 0.0;

    int allreduce(double *buf, int64_t count, int op)
    {
        if (!ar || count <= 0) return ESFM_OK;
        if (ar(ar_user, buf, count, op, reinterpret_cast<void *>(st)) != 0) {
            esfm::set_error("all-reduce callback failed");
            return ESFM_ERR_COMM;
        }
        return ESFM_OK;
    }
    bool scal_zeroed = false;   // the read-back kernel (ba_publish_scalars) leaves d.scal zeroed: a reset right after a fetch needs no memset
    int zero_scal()
    {
        if (!scal_zeroed) ESFM_HIP_TRY(hipMemsetAsync(P->d.scal, 0, sizeof(double) * esfm::SC_COUNT, st));
        scal_zeroed = false;
        esfm::ba_scal_discard(P->d, 0, esfm::SC_SUM_COUNT);
        return ESFM_OK;
    }
    // SUM the partial-sum slots and MAX the gradient slot across ranks, then fetch all scalars.
    int fetch_scal()
    {
        if (ar) { if (int rc = esfm::ba_scal_reduce(st, P->d)) return rc; }   // this rank's partials -> d.scal before the exchange
        if (int rc = allreduce(P->d.scal, esfm::SC_SUM_COUNT, ESFM_REDUCE_SUM)) return rc;
        if (int rc = allreduce(P->d.scal + esfm::SC_GMAX, esfm::SC_MAX_COUNT, ESFM_REDUCE_MAX)) return rc;
        // The device publishes the slots into pinned memory and then a sequence number; the host spins on that instead of
        // paying a stream synchronisation (two read-backs per LM iteration of ~0.4 ms: the wake-up latency is a tenth of it).
        unsigned long long *flag = reinterpret_cast<unsigned long long *>(h + esfm::SC_COUNT);
        const unsigned long long seq = ++P->seq;
        if (int rc = esfm::ba_publish_scalars(st, P->d, h, flag, seq)) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        for (long spins = 0; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq; ++spins) {
            if ((spins & 0xFFF) == 0xFFF) {
                if (hipStreamQuery(st) != hipErrorNotReady) {           // finished (or failed) without the store being seen: settle by sync
                    ESFM_HIP_TRY(hipStreamSynchronize(st));
                    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) break;
                    esfm::set_error("BA scalar publication was not observed");
                    return ESFM_ERR_HIP;
                }
                // A large reduced system (6 n_cam up to 46 000) legitimately keeps the stream busy for seconds; hipStreamQuery above
                // is what detects completion and failure.  After a while stop burning a core -- and past a generous bound (10 min,
                // ESFM_BA_READBACK_TIMEOUT_S overrides) give up with an error instead of spinning forever behind a wedged stream
                // (a dataflow kernel that lost a flag, a stuck collective of a sharded solve).
                const auto waited = std::chrono::steady_clock::now() - t0;
                if (waited > std::chrono::seconds(2)) std::this_thread::sleep_for(std::chrono::microseconds(200));
                if (waited > std::chrono::seconds(readback_timeout_s())) {
                    esfm::set_error("BA scalar read-back timed out (stream never completed)");
                    return ESFM_ERR_HIP;
                }
            }
        }
        scal_zeroed = true;
        return ESFM_OK;
    }
    // residuals + Jacobian at x, per-camera sums, per-point blocks; leaves cost/gmax in h[].
    int linearize(bool use_scaling, double radius, double cost_bound = -1.0)
    {
        const BADev &d = P->d;
        int deferred = 0;      // one rank: the slab reduction of the sweep's per-camera sums rides in the per-point launch
        if (int rc = esfm::ba_linearize(st, d, P->ctx->num_cu, opt.cauchy_a, use_scaling, P->ctx, ar ? nullptr : &deferred, cost_bound)) return rc;
        if (int rc = allreduce(d.camacc, (int64_t)esfm::ba_camacc_doubles(d.n_cam), ESFM_REDUCE_SUM)) return rc;
        if (int rc = esfm::ba_point_prep(st, d, radius, opt.min_lm_diagonal, opt.max_lm_diagonal, true, deferred)) return rc;
        return ESFM_OK;
    }

    // ---- set-up, in the order the solve calls it ----
    int take_mailbox()
    {
        if (!P->h_scal && !P->ctx->ba_mailboxes.empty()) {
            P->h_scal = static_cast<double *>(P->ctx->ba_mailboxes.back());
            P->ctx->ba_mailboxes.pop_back();
            memset(P->h_scal, 0, sizeof(double) * (esfm::SC_COUNT + 2));
        }
        if (!P->h_scal) {
            hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&P->h_scal), sizeof(double) * (esfm::SC_COUNT + 2), hipHostMallocCoherent);   // explicit: the host spins on a device-written flag
            if (e == hipSuccess) memset(P->h_scal, 0, sizeof(double) * (esfm::SC_COUNT + 2));
            if (e != hipSuccess) { esfm::set_error("hipHostMalloc failed: %s", hipGetErrorString(e)); return ESFM_ERR_HIP; }
        }
        h = P->h_scal;
        return ESFM_OK;
    }
    // camera observation counts over all shards
    int reduce_observation_counts()
    {
        const BADev &d = P->d;
        if (d.n_cam) ESFM_HIP_TRY(esfm::copy_h2d(d.cam_nobs, P->cam_nobs_local.data(), sizeof(double) * (size_t)d.n_cam, st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
        return allreduce(d.cam_nobs, d.n_cam, ESFM_REDUCE_SUM);
    }
    // Jacobi scaling starts at 1; several ranks: the points at entry, for the merge at the end
    int reset_scaling()
    {
        const BADev &d = P->d;
        if (int rc = fill_ones(st, d.scale_c, (size_t)6 * d.n_cam)) return rc;
        if (int rc = fill_ones(st, d.scale_p, (size_t)3 * d.n_pt)) return rc;
        if (multi && d.n_pt) ESFM_HIP_TRY(hipMemcpyAsync(d.x0_p, d.x_p, sizeof(double) * 3 * (size_t)d.n_pt, hipMemcpyDeviceToDevice, st));
        return ESFM_OK;
    }
    // active cameras / points of the summary, and the box bounds -- only on blocks that take part in the problem (Ceres drops
    // unused blocks with their bounds)
    int count_active_and_set_bounds()
    {
        BADev &d = P->d;
        std::vector<double> cn((size_t)d.n_cam);
        if (d.n_cam) ESFM_HIP_TRY(esfm::copy_d2h(cn.data(), d.cam_nobs, sizeof(double) * (size_t)d.n_cam, st));
        std::vector<int32_t> ps((size_t)d.n_pt + 1);
        ESFM_HIP_TRY(esfm::copy_d2h(ps.data(), d.pt_start, sizeof(int32_t) * ((size_t)d.n_pt + 1), st));
        ESFM_HIP_TRY(hipStreamSynchronize(st));
        for (int c = 0; c < d.n_real_cam; ++c) sum->num_active_cameras += cn[(size_t)c] > 0.0;
        for (int p = 0; p < d.n_pt; ++p) sum->num_active_points += ps[(size_t)p + 1] > ps[(size_t)p];
        std::vector<double> lo((size_t)6 * d.n_cam, -INFINITY), up((size_t)6 * d.n_cam, INFINITY);
        d.constrained = 0;
        if (P->ref_cam >= 0 && cn[(size_t)P->ref_cam] > 0.0) {
            for (int i = 0; i < 6; ++i) { lo[6 * (size_t)P->ref_cam + i] = -P->ref_threshold; up[6 * (size_t)P->ref_cam + i] = P->ref_threshold; }
            d.constrained = 1;
        }
        // (a block's count is its group's, summed over all ranks: a rank that holds none of a group's observations still boxes it)
        for (int g = 0; g < d.has_calib; ++g) {
            const size_t blk = (size_t)d.n_real_cam + g;
            if (!(cn[blk] > 0.0)) continue;
            for (int i = 0; i < 4; ++i) {
                lo[6 * blk + i] = P->calib_center[4 * (size_t)g + i] - P->calib_tol[(size_t)g];
                up[6 * blk + i] = P->calib_center[4 * (size_t)g + i] + P->calib_tol[(size_t)g];
            }
            for (int i = 0; i < 2 && d.radial; ++i) {
                lo[6 * blk + 4 + i] = P->radial_center[2 * (size_t)g + i] - P->radial_tol[(size_t)g];
                up[6 * blk + 4 + i] = P->radial_center[2 * (size_t)g + i] + P->radial_tol[(size_t)g];
            }
            d.constrained = 1;
        }
        if (d.n_cam) {
            ESFM_HIP_TRY(esfm::copy_h2d(d.lo_c, lo.data(), sizeof(double) * lo.size(), st));
            ESFM_HIP_TRY(esfm::copy_h2d(d.up_c, up.data(), sizeof(double) * up.size(), st));
            ESFM_HIP_TRY(hipStreamSynchronize(st));
        }
        constrained = d.constrained != 0;
        return ESFM_OK;
    }

    // ---- the loop's pieces ----
    void log_iteration(int iter, const esfm_ba_iteration &cur)
    {
        if (iter < ESFM_BA_MAX_LOG) sum->iterations[iter] = cur;
        sum->num_iterations = iter;
    }
    // The scalars of the re-linearisation after an accepted step have been fetched: take the cost, gradient norm and validity at the
    // new point.  Used right after the step, or one read-back later when that read-back was deferred: the log entry `deferred_entry`
    // of the accepted iteration was then written without them.  false: the solve ends here.
    bool complete_accepted_step(int deferred_entry = -1)
    {
        pending_lin = false;
        if (h[esfm::SC_LIN_BAD] > 0.0) {
            esfm::set_error("non-finite residual or Jacobian after an accepted step");
            sum->termination = ESFM_BA_FAILURE; rc_final = ESFM_ERR_NUMERIC; terminated = true;
        }
        x_cost = h[esfm::SC_COST];
        prep_singular = h[esfm::SC_PT_SINGULAR] > 0.0;
        gmax = h[esfm::SC_GMAX];
        if (deferred_entry >= 0 && deferred_entry < ESFM_BA_MAX_LOG) { sum->iterations[deferred_entry].cost = x_cost; sum->iterations[deferred_entry].gradient_max_norm = gmax; }
        if (!terminated && gmax <= opt.gradient_tolerance) { sum->termination = ESFM_BA_CONVERGENCE; terminated = true; }
        return !terminated;
    }
    int iteration_zero();
    int line_search(esfm_ba_iteration &cur, double &step_norm, double &cand_norm);
    int run();
};

// Structure of the reduced camera system for this solve (see ba_sparse_plan.hpp).  Camera blocks (a, b) of S are non-zero only where
// a and b observe a common point; when that leaves at most half of the dense factorisation's tiles -- or half its dependency chain
// -- the tiled solve visits only the tiles of the symbolic fill (ba_chol_sparse.hip).  Several ranks: every rank holds the
// observations of ITS points, so the ranks' pair sets are united first (one small all-reduce per solve; four 13-bit counters per
// double, exact for up to 8191 ranks), every rank plans from the same union and the plans are identical.  ESFM_BA_SOLVE=dense keeps the
// dense path, =sparse takes the plan even where it does not pay (tests); ESFM_BA_LEAF_MAX: cameras per undissected leaf.
int plan_reduced_structure(esfm_ba_problem *P, Solver &S, bool multi)
{
    BADev &d = P->d;
    d.sparse = nullptr;
    const char *mode = getenv("ESFM_BA_SOLVE");
    const bool force_dense = mode && mode[0] == 'd', force_sparse = mode && mode[0] == 's';
    if (force_dense || d.has_calib || P->parts.forms.solve != esfm::BaForms::SOLVE_TILED || P->h_pt_start.empty()) return ESFM_OK;
    const char *lm = getenv("ESFM_BA_LEAF_MAX");
    const int leaf_max = lm && atoi(lm) > 0 ? atoi(lm) : 32;
    const int key = multi ? 1 : 0;
    if (P->sparse_key != key || P->sparse_leaf_max != leaf_max) {
        esfm::ba_sparse_destroy(P->sparse); P->sparse = nullptr;
        if (P->pair_flags.empty()) P->pair_flags = esfm::cam_pair_flags(d.n_real_cam, d.n_pt, P->h_pt_start.data(), P->h_obs_cam.data());
        std::vector<uint8_t> all;
        if (multi) {
            const size_t nf = P->pair_flags.size(), nd = (nf + 3) / 4;
            std::vector<double> pk(nd, 0.0);
            for (size_t k = 0; k < nf; ++k) if (P->pair_flags[k]) pk[k / 4] += (double)(1ull << (13 * (k % 4)));
            double *dev = nullptr;
            ESFM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dev), sizeof(double) * std::max<size_t>(nd, 1)));
            int rc = ESFM_OK;
            if (esfm::copy_h2d(dev, pk.data(), sizeof(double) * nd, S.st) != hipSuccess || hipStreamSynchronize(S.st) != hipSuccess) rc = ESFM_ERR_HIP;
            if (rc == ESFM_OK) rc = S.allreduce(dev, (int64_t)nd, ESFM_REDUCE_SUM);
            if (rc == ESFM_OK && (esfm::copy_d2h(pk.data(), dev, sizeof(double) * nd, S.st) != hipSuccess || hipStreamSynchronize(S.st) != hipSuccess)) rc = ESFM_ERR_HIP;
            (void)hipFree(dev);
            if (rc != ESFM_OK) { if (rc == ESFM_ERR_HIP) esfm::set_error("exchange of the camera co-visibility failed"); return rc; }
            all.assign(nf, 0);
            for (size_t k = 0; k < nf; ++k) all[k] = (((unsigned long long)pk[k / 4] >> (13 * (k % 4))) & 0x1FFFull) ? 1 : 0;
        }
        const esfm::CamGraph g = esfm::cam_graph_from_tracks(d.n_real_cam, d.n_pt, P->h_pt_start.data(), P->h_obs_cam.data(), multi ? &all : nullptr);
        const esfm::SparsePlan plan = esfm::make_sparse_plan(g, leaf_max);
        P->sparse_worthwhile = plan.worthwhile();
        if (int rc = esfm::ba_sparse_create(S.st, plan, g, &P->sparse)) return rc;
        P->sparse_key = key; P->sparse_leaf_max = leaf_max;
    }
    if (P->sparse && (P->sparse_worthwhile || force_sparse)) d.sparse = P->sparse;
    return ESFM_OK;
}

// ---- iteration 0 (TrustRegionMinimizer::IterationZero) ----
int Solver::iteration_zero()
{
    const BADev &d = P->d;
    radius = opt.initial_trust_region_radius; decrease_factor = 2.0;
    if (int rc = zero_scal()) return rc;
    if (constrained) { if (int rc = esfm::ba_project_cameras(st, d)) return rc; }   // x <- Plus(x, 0)
    if (int rc = esfm::ba_param_sqnorm(st, d)) return rc;
    if (int rc = linearize(false, radius)) return rc;
    if (opt.jacobi_scaling) {
        if (int rc = esfm::ba_jacobi_scaling(st, d)) return rc;
        // keep |x|^2, restart the other accumulators, and linearise again with scaled columns
        ESFM_HIP_TRY(hipMemsetAsync(d.scal, 0, sizeof(double) * esfm::SC_XNORM_SQ_PT, st));
        ESFM_HIP_TRY(hipMemsetAsync(d.scal + esfm::SC_LIN_BAD, 0, sizeof(double) * (esfm::SC_SUM_COUNT - esfm::SC_LIN_BAD), st));
        esfm::ba_scal_discard(d, 0, esfm::SC_XNORM_SQ_PT); esfm::ba_scal_discard(d, esfm::SC_LIN_BAD, esfm::SC_SUM_COUNT);
        ESFM_HIP_TRY(hipMemsetAsync(d.scal + esfm::SC_GMAX, 0, sizeof(double), st));
        if (int rc = linearize(true, radius)) return rc;
    }
    if (int rc = esfm::ba_camera_gradient(st, d)) return rc;
    if (int rc = fetch_scal()) return rc;
    if (h[esfm::SC_LIN_BAD] > 0.0) {
        esfm::set_error("non-finite residual or Jacobian at the initial point");
        sum->termination = ESFM_BA_FAILURE;
        return ESFM_ERR_NUMERIC;
    }
    x_cost = h[esfm::SC_COST];
    gmax = h[esfm::SC_GMAX];
    x_norm = std::sqrt(h[esfm::SC_XNORM_SQ_PT] + h[esfm::SC_XNORM_SQ_CAM]);
    prep_radius = radius;
    prep_singular = h[esfm::SC_PT_SINGULAR] > 0.0;
    n_invalid = 0;
    sum->initial_cost = x_cost;
    {
        esfm_ba_iteration &it = sum->iterations[0];
        it.iteration = 0; it.step_is_valid = 1; it.step_is_successful = 1; it.cost = x_cost;
        it.gradient_max_norm = gmax; it.trust_region_radius = radius;
    }
    sum->num_iterations = 0; sum->num_successful_steps = 1;
    if (opt.verbose)
        printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius\n%4d % .6e  % .2e  % .2e  % .2e  % .2e  % .2e\n",
               0, x_cost, 0.0, gmax, 0.0, 0.0, radius);
    if (gmax <= opt.gradient_tolerance) { sum->termination = ESFM_BA_CONVERGENCE; terminated = true; }
    return ESFM_OK;
}

// TrustRegionMinimizer::DoLineSearch (bounded problems; the scalars of the full step are in h): Armijo search from step size 1
// along delta; every trial is one take-step + cost-with-slope pass over the observations and one scalar read-back.
int Solver::line_search(esfm_ba_iteration &cur, double &step_norm, double &cand_norm)
{
    namespace ls = esfm::linesearch;
    const BADev &d = P->d;
    const double g0 = h[esfm::SC_GDOTD], dmax = h[esfm::SC_DMAX];
    auto sample_from_h = [&](double x) {
        ls::Sample s;
        s.x = x; s.f = h[esfm::SC_CAND_COST]; s.g = h[esfm::SC_LS_GRAD];
        s.valid = h[esfm::SC_CAND_BAD] == 0.0 && std::isfinite(s.f) && std::isfinite(s.g);
        return s;
    };
    auto evaluate_at = [&](double t, bool slope) -> int {
        if (int rc = zero_scal()) return rc;
        if (int rc = esfm::ba_take_step(st, d, t)) return rc;
        if (int rc = esfm::ba_cost(st, d, P->ctx->num_cu, d.cand_c, d.cand_p, opt.cauchy_a, esfm::SC_CAND_COST, esfm::SC_CAND_BAD, slope)) return rc;
        return fetch_scal();
    };
    ls::Sample initial, previous, current = sample_from_h(1.0);
    initial.x = 0.0; initial.f = x_cost; initial.g = g0; initial.valid = true;
    int ls_it = 0;
    bool ls_ok = true;
    while (!current.valid || current.f > x_cost + ls::kSufficientDecrease * g0 * current.x) {
        if (++ls_it >= ls::kMaxIterations) { ls_ok = false; break; }
        const double t = ls::next_step(initial, previous, current);
        if (t * dmax < ls::kMinStepSize) { ls_ok = false; break; }
        previous = current;
        if (int rc = evaluate_at(t, true)) return rc;
        current = sample_from_h(t);
    }
    cur.line_search_steps = ls_it;
    // a failed search leaves delta as it was: back to the full step
    if (!ls_ok && current.x != 1.0) { if (int rc = evaluate_at(1.0, false)) return rc; }
    step_norm = std::sqrt(h[esfm::SC_STEP_SQ_PT] + h[esfm::SC_STEP_SQ_CAM]);
    cand_norm = std::sqrt(h[esfm::SC_CAND_SQ_PT] + h[esfm::SC_CAND_SQ_CAM]);
    return ESFM_OK;
}

// ---- main loop (TrustRegionMinimizer::Minimize) ----
int Solver::run()
{
    BADev &d = P->d;
    int iter = 0;
    // No bounds: the read-back that follows the re-linearisation of an accepted step is DEFERRED to the next step's --
    // the next Schur complement and solve are enqueued straight behind the sweep (one host round trip and one read-back launch
    // less per accepted step).  What that read-back delivers -- the cost, gradient norm and validity at the accepted point --
    // is only needed after the next step has been computed: the right-hand side's fixed-point exponent takes its bound from the
    // candidate's cost (the same function value, computed by the back-substitution launch), the gradient-tolerance test and the
    // log entry of the accepted iteration are completed one read-back later (a step computed past convergence is discarded).
    const bool may_defer = !constrained && !opt.verbose;     // (sharded solves too: the deferred scalars are all-reduced like the others, every rank decides alike)
    while (!terminated) {
        if (iter >= opt.max_num_iterations) { sum->termination = ESFM_BA_NO_CONVERGENCE; break; }
        if (radius <= opt.min_trust_region_radius) {
            if (pending_lin) { if (int rc = fetch_scal()) return rc; if (!complete_accepted_step(iter)) break; }
            sum->termination = ESFM_BA_CONVERGENCE; break;
        }
        ++iter;
        esfm_ba_iteration cur;
        memset(&cur, 0, sizeof(cur));
        cur.iteration = iter; cur.gradient_max_norm = gmax;
        // LevenbergMarquardtStrategy::ComputeStep: D^2 = clamp(diag(J'J)) / radius, then the Schur solve.  (The LM diagonal is a
        // function of J only: a rejected or invalid step re-scales the per-point inverses below and nothing else is recomputed.)
        // (a deferred read-back: the slots were reset by the last read-back and hold the sweep's sums -- nothing to reset, nothing to forget)
        if (!pending_lin) { if (int rc = zero_scal()) return rc; }
        bool reprepped = false;
        if (prep_radius != radius) {
            if (int rc = esfm::ba_point_prep(st, d, radius, opt.min_lm_diagonal, opt.max_lm_diagonal, false)) return rc;
            prep_radius = radius; reprepped = true;
        }
        {
            esfm::KernelTimer tm(P->ctx, ESFM_K_BA_SCHUR);
            // |robustified residual vector| over all ranks (deferred read-back: the candidate's cost bounds the cost at the same point)
            const double rhs_bound = std::sqrt(2.0 * std::max(pending_lin ? pending_cost_bound : x_cost, 0.0));
            if (int rc = esfm::ba_schur(st, d, P->ctx->num_cu, rhs_bound)) return rc;
            if (int rc = esfm::ba_schur_calib(st, d, rhs_bound)) return rc;
        }
        if (multi && d.sparse) {
            // one exchange per LM iteration, of the co-visible camera blocks and the right-hand side only (BA-512: 1.4 MB instead of 37.8)
            if (int rc = esfm::ba_sparse_pack(st, d, d.sparse, d.red_packed)) return rc;
            if (int rc = allreduce(d.red_packed, (int64_t)esfm::ba_sparse_packed_doubles(d.sparse, d.n_cam), ESFM_REDUCE_SUM)) return rc;
        } else if (multi) {
            // one exchange per LM iteration: the block-lower-triangular S and the right-hand side, packed
            if (int rc = esfm::ba_red_pack(st, d, d.red_packed, false)) return rc;
            if (int rc = allreduce(d.red_packed, (int64_t)esfm::ba_red_packed_doubles(d.n_cam), ESFM_REDUCE_SUM)) return rc;
            if (int rc = esfm::ba_red_pack(st, d, d.red_packed, true)) return rc;
        }
        {
            esfm::KernelTimer tm(P->ctx, ESFM_K_BA_SOLVE);
            if (int rc = esfm::ba_solve_reduced(st, d, radius, opt.min_lm_diagonal, opt.max_lm_diagonal)) return rc;
        }
        if (int rc = esfm::ba_camera_step(st, d)) return rc;
        // back-substitution; the candidate's cost at full step comes out of the same launch -- bounded problems also need the slope
        // there for the line search, which is ba_cost's job
        // (fused only on small problems: it saves a launch gap, but the chunk kernel's occupancy is LDS-bound and the extra f64
        // work costs more than ba_cost's own pass from ~1M observations: BA-512 281 us fused against 140 + 42 us)
        const bool fuse_cost = !constrained && !P->parts.forms.large;
        if (int rc = esfm::ba_backsub(st, d, fuse_cost, opt.cauchy_a)) return rc;
        if (!fuse_cost) {
            if (int rc = esfm::ba_cost(st, d, P->ctx->num_cu, d.cand_c, d.cand_p, opt.cauchy_a, esfm::SC_CAND_COST, esfm::SC_CAND_BAD, constrained)) return rc;
        }
        if (int rc = fetch_scal()) return rc;
        if (pending_lin) {
            // the accepted iteration iter - 1 is completed first; past convergence (or on failure) the step just computed is dropped
            if (!complete_accepted_step(iter - 1)) { sum->num_iterations = iter - 1; break; }
            cur.gradient_max_norm = gmax;
        }
        const double model_cost_change = h[esfm::SC_MODEL_CHANGE];
        double step_norm = std::sqrt(h[esfm::SC_STEP_SQ_PT] + h[esfm::SC_STEP_SQ_CAM]);
        double cand_norm = std::sqrt(h[esfm::SC_CAND_SQ_PT] + h[esfm::SC_CAND_SQ_CAM]);
        if (reprepped) prep_singular = h[esfm::SC_PT_SINGULAR] > 0.0;
        const bool lin_ok = h[esfm::SC_CHOL_FAIL] == 0.0 && !prep_singular && std::isfinite(model_cost_change) &&
                            std::isfinite(step_norm);
        cur.model_cost_change = model_cost_change;
        cur.step_is_valid = lin_ok && (model_cost_change > 0.0);
        if (!cur.step_is_valid) {
            // HandleInvalidStep + StepIsInvalid
            if (++n_invalid >= opt.max_num_consecutive_invalid_steps) { sum->termination = ESFM_BA_FAILURE; terminated = true; }
            radius *= 0.5;
            cur.cost = x_cost; cur.trust_region_radius = radius;
            sum->num_unsuccessful_steps++;
            log_iteration(iter, cur);
            continue;
        }
        n_invalid = 0;
        if (constrained) { if (int rc = line_search(cur, step_norm, cand_norm)) return rc; }
        const double cand_cost = h[esfm::SC_CAND_BAD] > 0.0 ? DBL_MAX : h[esfm::SC_CAND_COST];
        cur.step_norm = step_norm;
        cur.cost_change = x_cost - cand_cost;
        // ParameterToleranceReached / FunctionToleranceReached: tested before acceptance, step not applied
        if (step_norm <= opt.parameter_tolerance * (x_norm + opt.parameter_tolerance) || std::fabs(cur.cost_change) <= opt.function_tolerance * x_cost) {
            sum->termination = ESFM_BA_CONVERGENCE; terminated = true;
            cur.cost = x_cost; cur.trust_region_radius = radius;
            log_iteration(iter, cur);
            break;
        }
        cur.relative_decrease = (x_cost - cand_cost) / model_cost_change;
        if (cur.relative_decrease > opt.min_relative_decrease) {
            // HandleSuccessfulStep: x <- candidate (pointer swap), re-linearise
            std::swap(d.x_c, d.cand_c); std::swap(d.x_p, d.cand_p);
            x_norm = cand_norm;
            const double q = 2.0 * cur.relative_decrease - 1.0;
            radius = radius / std::max(1.0 / 3.0, 1.0 - q * q * q);
            radius = std::min(opt.max_trust_region_radius, radius);
            decrease_factor = 2.0;
            if (int rc = zero_scal()) return rc;
            if (int rc = linearize(opt.jacobi_scaling != 0, radius, cand_cost < DBL_MAX ? cand_cost * (1.0 + 1e-9) : -1.0)) return rc;
            prep_radius = radius;
            if (int rc = esfm::ba_camera_gradient(st, d)) return rc;
            cur.step_is_successful = 1;
            sum->num_successful_steps++;
            if (may_defer && iter < opt.max_num_iterations && radius > opt.min_trust_region_radius) {
                // read-back deferred to the next step's (see may_defer); cost and gradient norm of this log entry follow then
                pending_lin = true;
                pending_cost_bound = cand_cost * (1.0 + 1e-9);
                cur.cost = cand_cost; cur.gradient_max_norm = gmax;
                cur.trust_region_radius = radius;
                log_iteration(iter, cur);
                continue;
            }
            if (int rc = fetch_scal()) return rc;
            complete_accepted_step();
            cur.cost = x_cost; cur.gradient_max_norm = gmax;
        } else {
            // HandleUnsuccessfulStep + StepRejected
            cur.step_is_successful = 0; cur.cost = cand_cost;
            radius = radius / decrease_factor; decrease_factor *= 2.0;
            sum->num_unsuccessful_steps++;
        }
        cur.trust_region_radius = radius;
        log_iteration(iter, cur);
        if (opt.verbose)
            printf("%4d % .6e  % .2e  % .2e  % .2e  % .2e  % .2e\n", iter, cur.cost, cur.cost_change, cur.gradient_max_norm, cur.step_norm,
                   cur.relative_decrease, radius);
    }
    sum->final_cost = x_cost;
    if (multi && d.n_pt) {
        // every rank ends with the full point set: sum the owners' deltas
        if (int rc = esfm::ba_points_delta(st, d, true)) return rc;
        if (int rc = allreduce(d.x_p, (int64_t)3 * d.n_pt, ESFM_REDUCE_SUM)) return rc;
        if (int rc = esfm::ba_points_delta(st, d, false)) return rc;
    }
    ESFM_HIP_TRY(hipStreamSynchronize(st));
    return rc_final;
}

}  // namespace

extern "C" int esfm_ba_problem_solve(esfm_ba_problem *P, const esfm_ba_options *options, esfm_allreduce_fn allreduce, void *allreduce_user,
                                     esfm_ba_summary *sum)
{
    if (!P) { esfm::set_error("problem is NULL"); return ESFM_ERR_INVALID_ARG; }
    if (int rc = esfm::set_device(P->ctx)) return rc;
    esfm_ba_summary local_sum;
    if (!sum) sum = &local_sum;
    memset(sum, 0, sizeof(*sum));
    Solver S;
    S.P = P; S.ar = allreduce; S.ar_user = allreduce_user; S.st = P->ctx->stream; S.sum = sum;
    S.multi = allreduce != nullptr;
    if (int rc = S.take_mailbox()) return rc;
    if (options) S.opt = *options; else esfm::ba_options_default(&S.opt);
    ESFM_REQUIRE(S.opt.initial_trust_region_radius > 0.0 && S.opt.max_num_iterations >= 0, "bad options");
    BADev &d = P->d;
    P->parts.single_rank = !S.multi; P->parts.grad_done = false;
    if (S.multi && !d.red_packed) { if (int rc = esfm::ba_dev_alloc(P, &d.red_packed, esfm::ba_red_packed_doubles(d.n_cam))) return rc; }
    if (int rc = S.reduce_observation_counts()) return rc;
    if (int rc = plan_reduced_structure(P, S, S.multi)) return rc;
    if (int rc = S.reset_scaling()) return rc;
    if (int rc = S.count_active_and_set_bounds()) return rc;

    const auto t0 = std::chrono::steady_clock::now();
    int rc = S.iteration_zero();
    if (rc == ESFM_OK) rc = S.run();
    sum->solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}
