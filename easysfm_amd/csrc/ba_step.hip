// Bundle adjustment, step stage: from the reduced camera system to the accepted or rejected candidate -- the solve, the step and the
// cost evaluations of ceres::Solve's LM iteration (reference cpp_code/src/ba.cpp:132-212).  Kernels and their launchers:
//
//   ba_chol_solve_kernel       dense Cholesky of the reduced camera system in one workgroup's LDS + both triangular solves
//   ba_camera_step_kernel      candidate cameras
//   ba_backsub_chunk_kernel    back-substitution per point chunk, candidate points, model cost change
//   ba_cost_kernel             robustified cost of a parameter vector (candidate evaluation), with the slope along the step
//   ba_take_step_kernel        line-search candidate; ba_project_cameras / ba_param_sqnorm / ba_points_delta: the small vector kernels
//   ba_scal_reduce_kernel, ba_publish_scalars_kernel   the scalar sums' read-back (scal_commit, ba_device.hpp)
//
// The LM control flow (accept/reject, radius) lives in ba_solve.cpp.  DESIGN.md "Bundle adjustment".
#include <array>

#include "ba_device.hpp"
#include "ba_chol_sparse.hpp"

namespace esfm {

// Dense solve of the reduced camera system (DENSE_SCHUR's Cholesky):
//   (F'F + D_c^2 + S_schur) y = F'r + rhs_corr
// One workgroup, right-looking blocked Cholesky on a packed lower matrix in LDS with the right-hand side carried
// as row n (so the forward substitution comes for free), then the backward substitution.
constexpr int kCholThreads = 1024;
constexpr int kCholNB = 8;  // panel width

// Per panel of kCholNB columns (3 barriers):
//   B1  wave 0 factors the nb x nb diagonal block in registers (lane r = block row r, __shfl)
//   B2  every row below (and the rhs row) solves against the block's transpose
//   C   all waves apply the rank-nb update to the trailing matrix in 4 x 4 register tiles: per panel column 8 LDS loads
//       feed 16 independent FMAs (the left-looking form this replaces issued 2 dependent loads per FMA and was
//       LDS-latency bound: 161 us at n = 150)
// The backward substitution is blocked the same way.
__global__ __launch_bounds__(kCholThreads) void ba_chol_solve_kernel(BADev d, double radius, double min_diag, double max_diag)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int n = 6 * d.n_cam;
    const size_t tot = (size_t)(n + 1) * (n + 2) / 2;
    double *L = smem;                                 // packed lower, (n+1) rows; row n = rhs
    double *rd = smem + tot;                          // [n] reciprocal diagonal of L
    // failure flag kept inside the dynamic region (a static __shared__ object in front of it would
    // shift the f64 array off its 8-byte alignment)
    volatile double *failp = rd + n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) *failp = 0.0;
    const double *S = d.red;
    const double *rc = d.red + (size_t)n * n;
    const double *FtF = d.camacc;
    const double *Ftr = d.camacc + 36 * (size_t)d.n_cam;
    // assemble: L = F'F + D_c^2 + S_schur (lower), row n = F'r + rhs_corr
    for (size_t e = tid; e < tot; e += kCholThreads) {
        int i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        while ((size_t)(i + 1) * (i + 2) / 2 <= e) ++i;
        while ((size_t)i * (i + 1) / 2 > e) --i;
        const int k = (int)(e - (size_t)i * (i + 1) / 2);
        double v;
        if (i < n) {
            v = S[(size_t)i * n + k];
            if (i / 6 == k / 6) {
                const int c = i / 6;
                v += FtF[36 * (size_t)c + 6 * (i % 6) + (k % 6)];
                if (i == k) v += fmin(fmax(FtF[36 * (size_t)c + 7 * (i % 6)], min_diag), max_diag) / radius;
            }
        } else {
            v = (k < n) ? (Ftr[k] + rc[k]) : 0.0;
        }
        L[e] = v;
    }
    __syncthreads();
    auto row = [&](int i) -> double * { return L + (size_t)i * (i + 1) / 2; };

    for (int j0 = 0; j0 < n; j0 += kCholNB) {
        const int nb = min(kCholNB, n - j0);
        // B1: wave 0 factors the nb x nb diagonal block in registers (lane r = block row r)
        if (wave == 0) {
            const int r = lane;
            double a[kCholNB];
#pragma unroll
            for (int c = 0; c < kCholNB; ++c) a[c] = (r < nb && c <= r) ? row(j0 + r)[j0 + c] : 0.0;
#pragma unroll
            for (int c = 0; c < kCholNB; ++c) {
                if (c < nb) {
                    const double piv = readlane_f64(a[c], c);
                    if (!(piv > 0.0) || !isfinite(piv)) { if (lane == 0) *failp = 1.0; }
                    const double rinv = rsqrt(piv > 0.0 ? piv : 1.0);
                    a[c] = (r == c) ? piv * rinv : a[c] * rinv;
                    if (lane == c) rd[j0 + c] = rinv;
#pragma unroll
                    for (int c2 = c + 1; c2 < kCholNB; ++c2) {
                        const double l2 = readlane_f64(a[c], c2);   // L[j0+c2][j0+c]
                        if (r >= c2) a[c2] -= a[c] * l2;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < kCholNB; ++c)
                if (r < nb && c <= r) row(j0 + r)[j0 + c] = a[c];
        }
        __syncthreads();
        // B2: every row below the block (and the rhs row) solves against the block's transpose
        for (int i = j0 + nb + tid; i <= n; i += kCholThreads) {
            double *Li = row(i);
            double x[kCholNB];
#pragma unroll
            for (int c = 0; c < kCholNB; ++c) x[c] = c < nb ? Li[j0 + c] : 0.0;
#pragma unroll
            for (int c = 0; c < kCholNB; ++c) {
                if (c < nb) {
                    const double *Lc = row(j0 + c) + j0;
                    double v = x[c];
#pragma unroll
                    for (int c1 = 0; c1 < c; ++c1) v -= x[c1] * Lc[c1];
                    x[c] = v * rd[j0 + c];
                    Li[j0 + c] = x[c];
                }
            }
        }
        __syncthreads();
        // C: trailing update A[i][j] -= sum_c L[i][j0+c] L[j][j0+c] over j0+nb <= j <= i <= n, j < n, in 4 x 4 tiles
        {
            const int base = j0 + nb;
            const int R = (n + 1 - base + 3) / 4;           // tile rows (the rhs row n included)
            const int ntile = R * (R + 1) / 2;
            for (int t = tid; t < ntile; t += kCholThreads) {
                int ta = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
                while ((ta + 1) * (ta + 2) / 2 <= t) ++ta;
                while (ta * (ta + 1) / 2 > t) --ta;
                const int tb = t - ta * (ta + 1) / 2;
                const int i0 = base + 4 * ta, c0 = base + 4 * tb;
                double acc[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = 0.0;
                const double *ri[4], *rj[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ri[r] = row(min(i0 + r, n)) + j0;        // clamped rows are masked at the store
                    rj[r] = row(min(c0 + r, n)) + j0;
                }
#pragma unroll
                for (int c = 0; c < kCholNB; ++c) {
                    if (c < nb) {
                        double li[4], lj[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) { li[r] = ri[r][c]; lj[r] = rj[r][c]; }
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int q = 0; q < 4; ++q) acc[4 * r + q] += li[r] * lj[q];
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = i0 + r;
                    if (i > n) continue;
                    double *Ai = row(i);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = c0 + q;
                        if (j <= i && j < n) Ai[j] -= acc[4 * r + q];
                    }
                }
            }
        }
        __syncthreads();
    }
    // backward substitution L' y = z (z = row n), panels from the bottom
    double *z = row(n);
    const int last = ((n - 1) / kCholNB) * kCholNB;
    for (int j0 = last; j0 >= 0; j0 -= kCholNB) {
        const int nb = min(kCholNB, n - j0);
        if (wave == 0) {
            // the nb x nb block in registers: lane k holds z[j0+k] and column k of the block (L[j0+i][j0+k], i > k)
            const int kk = lane;
            double zk = kk < nb ? z[j0 + kk] : 0.0;
            double col[kCholNB];
#pragma unroll
            for (int i = 0; i < kCholNB; ++i) col[i] = (i < nb && kk < i) ? row(j0 + i)[j0 + kk] : 0.0;
            const double rdk = kk < nb ? rd[j0 + kk] : 0.0;
#pragma unroll
            for (int i = kCholNB - 1; i >= 0; --i) {
                if (i < nb) {
                    const double yi = readlane_f64(zk * rdk, i);
                    zk = (kk == i) ? yi : zk - col[i] * yi;
                }
            }
            if (kk < nb) z[j0 + kk] = zk;
        }
        __syncthreads();
        for (int k = tid; k < j0; k += kCholThreads) {
            double s = 0.0;
            for (int i = j0; i < j0 + nb; ++i) s += row(i)[k] * z[i];
            z[k] -= s;
        }
        __syncthreads();
    }
    const bool fail = *failp != 0.0;
    for (int i = tid; i < n; i += kCholThreads) d.y_c[i] = fail ? 0.0 : z[i];
    if (tid == 0 && fail) d.scal[SC_CHOL_FAIL] = 1.0;
}

// ---------------------------------------------------------------------------------------------
// Candidate cameras: x + (-y) .* scaling for cameras that have observations; step/candidate norms (ba_camera_step_body in
// ba_kernels.hpp; the one-workgroup reduced solve calls it at its end instead of this launch).
__global__ __launch_bounds__(256) void ba_camera_step_kernel(BADev d)
{
    __shared__ double red[48];
    ba_camera_step_body(d, d.y_c, red);
}

// Back-substitution: y_p = M^-1 (E'r - sum_k E_k'F_k y_c), step = -y, candidate point, and the model cost change
// -sum (J s).(r + J s / 2)  (trust_region_minimizer.cc).  One workgroup per point chunk (pchunk_pt0: consecutive points whose
// observations -- contiguous in the point-sorted order -- number at most kPtChunkObs = 256, built once per problem):
//   1. thread = observation: one coalesced read of its Jacobian rows (kept in registers), f = F_k y_c, t_k = E_k' f -> LDS;
//   2. thread = point: adds its t_k in observation order, s_p = -M^-1 (E'r - sum t_k), candidate point, s_p -> LDS;
//   3. thread = observation again: J s = -f + E_k s_p  (-(a + b) == (-a) + (-b) exactly), its share of the scalars.
// No atomics, every sum in a fixed order.  (Round 1 had one thread per point walking its observations: 16 dependent memory round
// trips on an 8-observation track, 43 us on the 25-camera problem; and, from 2^20 observations, two observation-parallel passes
// joined by f64 atomics.)  A single point with more observations than a chunk holds gets a chunk of its own and loops.

// 1/2 rho(|r|^2) of observation k at the candidate (d.cand_c, point X): what ba_cost_kernel<false> evaluates, here inside the
// back-substitution that has just produced X (WITH_COST: unbounded problems, where no slope along the step is needed)
template <bool GROUPS>
__device__ __forceinline__ void candidate_cost(const BADev &d, int k, const double (&X)[3], double cauchy_a, double &cost, double &bad)
{
    const int c = d.obs_cam[k];
    const float2 uv = d.obs_uv[k];
    double in4[4];
    load_intrinsics<GROUPS>(d, d.cand_c, c, in4);
    double cam[6], pt[3];
#pragma unroll
    for (int q = 0; q < 6; ++q) cam[q] = d.cand_c[6 * (size_t)c + q];
    transform_point<false>(cam, X, pt, nullptr, nullptr);
    const double x = pt[0] / pt[2], y = pt[1] / pt[2];
    const double r0 = (double)uv.x - (x * in4[0] + in4[1]), r1 = (double)uv.y - (y * in4[2] + in4[3]);
    const double s2 = r0 * r0 + r1 * r1;
    if (!isfinite(s2)) { bad += 1.0; return; }
    double rho0, rho1;
    loss_eval(cauchy_a, s2, rho0, rho1);
    cost += 0.5 * rho0;
}

// (register budget: four workgroups per CU.  The WITH_COST form had been compiled to 198 registers -- two waves per SIMD for a kernel
// that streams; at 128 BA-25's iteration went 0.136 -> 0.133 ms.  The same audit found nothing else: the sweep at three / four
// workgroups per CU spills, 25.7 / 36 us against 22.5; the f64-MFMA Schur kernel at one / three: 462 / 640 us against 294.)
// GROUPS (several free intrinsics blocks): the intrinsics part of the step is that of the observation's camera's group, read per
// observation where the one block's is read once per workgroup.
// RADIAL (a GROUPS form; a radial problem is bounded, so its candidate cost is a pass of its own: never WITH_COST): six values of
// the block's step against the 8 stored scalars.
template <bool WITH_COST, bool GROUPS = false, bool RADIAL = false>
__global__ __launch_bounds__(kPtChunkObs, 4) void ba_backsub_chunk_kernel(BADev d, ScalBase sbase, double cauchy_a)
{
    static_assert(!RADIAL || (GROUPS && !WITH_COST), "the radial back-substitution is grouped and leaves the candidate cost to ba_cost");
    __shared__ double red[8];
    __shared__ double tE[kPtChunkObs][3];
    __shared__ double sps[kPtChunkObs][3];
    __shared__ double cnd[kPtChunkObs][3];      // WITH_COST: the candidate points of the chunk
    const int tid = threadIdx.x;
    const int4 ci4 = d.pchunk_info[blockIdx.x];          // (one load where p0 / p1, then pt_start[p0] / pt_start[p1], were two dependent ones)
    const int p0 = ci4.x, p1 = ci4.y, k0 = ci4.z, k1 = ci4.w;
    const int nobs = k1 - k0;
    const size_t n = d.n_obs;
    double mc = 0.0, ssq = 0.0, csq = 0.0, gd = 0.0, dmax = 0.0, ccost = 0.0, cbad = 0.0;
    double yk[RADIAL ? 6 : 4] = {0.0, 0.0, 0.0, 0.0};
    if (d.has_calib && !GROUPS) {
#pragma unroll
        for (int a = 0; a < 4; ++a) yk[a] = d.y_c[6 * d.n_real_cam + a];
    }
    auto group_step = [&](int c) {
        if (GROUPS) {
#pragma unroll
            for (int a = 0; a < (RADIAL ? 6 : 4); ++a) yk[a] = d.y_c[6 * calib_block_of<true>(d, c) + a];
        }
    };
    // the block's part of F_k y_c: rows 0 and 1
    auto block_f = [&](size_t k, double &f0, double &f1) {
        f0 = d.Jk[k] * yk[0] + d.Jk[n + k] * yk[1];
        f1 = d.Jk[2 * n + k] * yk[2] + d.Jk[3 * n + k] * yk[3];
        if constexpr (RADIAL) {
            f0 += d.Jk[4 * n + k] * yk[4] + d.Jk[5 * n + k] * yk[5];
            f1 += d.Jk[6 * n + k] * yk[4] + d.Jk[7 * n + k] * yk[5];
        }
    };
    auto point_step_pre = [&](int p, const double g[3], const double (&Mi)[6], const double (&xq)[3], const double (&scq)[3]) {   // the same from operands already in registers
        double sp[3] = {-(Mi[0] * g[0] + Mi[1] * g[1] + Mi[2] * g[2]), -(Mi[1] * g[0] + Mi[3] * g[1] + Mi[4] * g[2]),
                        -(Mi[2] * g[0] + Mi[4] * g[1] + Mi[5] * g[2])};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double xp = xq[a];
            const double dl = sp[a] * scq[a];
            const double cnd = xp + dl;
            const double df = xp - cnd;
            ssq += df * df; csq += cnd * cnd;
            d.cand_p[3 * (size_t)p + a] = cnd;
            if (d.constrained) { d.delta_p[3 * (size_t)p + a] = dl; dmax = fmax(dmax, fabs(dl)); }
        }
        return std::array<double, 3>{sp[0], sp[1], sp[2]};
    };
    auto point_step = [&](int p, const double g[3]) {       // s_p, candidate point, norms
        const double *Mi = d.Minv + 6 * (size_t)p;
        double sp[3] = {-(Mi[0] * g[0] + Mi[1] * g[1] + Mi[2] * g[2]), -(Mi[1] * g[0] + Mi[3] * g[1] + Mi[4] * g[2]),
                        -(Mi[2] * g[0] + Mi[4] * g[1] + Mi[5] * g[2])};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double xp = d.x_p[3 * (size_t)p + a];
            const double dl = sp[a] * d.scale_p[3 * (size_t)p + a];
            const double cnd = xp + dl;
            const double df = xp - cnd;
            ssq += df * df; csq += cnd * cnd;
            d.cand_p[3 * (size_t)p + a] = cnd;
            if (d.constrained) { d.delta_p[3 * (size_t)p + a] = dl; dmax = fmax(dmax, fabs(dl)); }
        }
        return std::array<double, 3>{sp[0], sp[1], sp[2]};
    };
    if (nobs <= kPtChunkObs) {
        const bool has = tid < nobs;
        const int k = k0 + (has ? tid : 0);
        double Jp[6], f0 = 0.0, f1 = 0.0, r0 = 0.0, r1 = 0.0;
        int pl = 0;
        // the point phase's operands are requested in front of the rows (see ba_point_prep_chunk_kernel)
        const bool is_pt = tid < p1 - p0;
        int pt_b = 0, pt_e = 0;
        double pt_g[3] = {0.0, 0.0, 0.0}, pt_M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, pt_x[3] = {0.0, 0.0, 0.0}, pt_sc[3] = {0.0, 0.0, 0.0};
        if (is_pt) {
            const size_t p = (size_t)(p0 + tid);
            pt_b = d.pt_start[p] - k0; pt_e = d.pt_start[p + 1] - k0;
#pragma unroll
            for (int a = 0; a < 3; ++a) { pt_g[a] = d.Etr[3 * p + a]; pt_x[a] = d.x_p[3 * p + a]; pt_sc[a] = d.scale_p[3 * p + a]; }
#pragma unroll
            for (int a = 0; a < 6; ++a) pt_M[a] = d.Minv[6 * p + a];
        }
        if (has) {
            const int c = d.obs_cam[k];
            pl = d.obs_pt[k] - p0;
            double Jc[12], yc[6];
#pragma unroll
            for (int a = 0; a < 12; ++a) Jc[a] = d.Jc[a * n + k];
#pragma unroll
            for (int a = 0; a < 6; ++a) { Jp[a] = d.Jp[a * n + k]; yc[a] = d.y_c[6 * c + a]; }
            r0 = d.res[k]; r1 = d.res[n + k];
#pragma unroll
            for (int a = 0; a < 6; ++a) { f0 += Jc[a] * yc[a]; f1 += Jc[6 + a] * yc[a]; }
            if (d.has_calib) {
                group_step(c);
                if constexpr (RADIAL) {
                    double b0, b1;
                    block_f(k, b0, b1);
                    f0 += b0; f1 += b1;
                } else {
                    f0 += d.Jk[k] * yk[0] + d.Jk[n + k] * yk[1];
                    f1 += d.Jk[2 * n + k] * yk[2] + d.Jk[3 * n + k] * yk[3];
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) tE[tid][a] = Jp[a] * f0 + Jp[3 + a] * f1;
        }
        __syncthreads();
        if (is_pt) {
            const int p = p0 + tid;
            const int b = pt_b, e = pt_e;
            if (e > b) {
                double g[3] = {pt_g[0], pt_g[1], pt_g[2]};
                for (int o = b; o < e; ++o) { g[0] -= tE[o][0]; g[1] -= tE[o][1]; g[2] -= tE[o][2]; }
                const auto sp = point_step_pre(p, g, pt_M, pt_x, pt_sc);
                sps[tid][0] = sp[0]; sps[tid][1] = sp[1]; sps[tid][2] = sp[2];
                if (WITH_COST) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) cnd[tid][a] = d.cand_p[3 * (size_t)p + a];      // (this thread's own stores)
                }
            } else {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    d.cand_p[3 * (size_t)p + a] = pt_x[a];
                    if (d.constrained) d.delta_p[3 * (size_t)p + a] = 0.0;
                }
            }
        }
        __syncthreads();
        if (has) {
            double m0 = -f0, m1 = -f1;
#pragma unroll
            for (int a = 0; a < 3; ++a) { m0 += Jp[a] * sps[pl][a]; m1 += Jp[3 + a] * sps[pl][a]; }
            mc = -(m0 * (r0 + m0 / 2.0) + m1 * (r1 + m1 / 2.0));
            gd = m0 * r0 + m1 * r1;
            if (WITH_COST) {
                const double X[3] = {cnd[pl][0], cnd[pl][1], cnd[pl][2]};
                candidate_cost<GROUPS>(d, k, X, cauchy_a, ccost, cbad);
            }
        }
    } else {
        // one point, more observations than threads: strided passes, block-wide sums in a fixed tree
        const int p = p0;
        double t[3] = {0.0, 0.0, 0.0};
        for (int k = k0 + tid; k < k1; k += kPtChunkObs) {
            const int c = d.obs_cam[k];
            double f0 = 0.0, f1 = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) { const double yc = d.y_c[6 * c + a]; f0 += d.Jc[a * n + k] * yc; f1 += d.Jc[(6 + a) * n + k] * yc; }
            if (d.has_calib) {
                group_step(c);
                if constexpr (RADIAL) {
                    double b0, b1;
                    block_f(k, b0, b1);
                    f0 += b0; f1 += b1;
                } else {
                    f0 += d.Jk[k] * yk[0] + d.Jk[n + k] * yk[1];
                    f1 += d.Jk[2 * n + k] * yk[2] + d.Jk[3 * n + k] * yk[3];
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) t[a] += d.Jp[a * n + k] * f0 + d.Jp[(3 + a) * n + k] * f1;
        }
        double g[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] = d.Etr[3 * (size_t)p + a] - block_sum(t[a], red);
        if (tid == 0) {
            const auto sp = point_step(p, g);
            sps[0][0] = sp[0]; sps[0][1] = sp[1]; sps[0][2] = sp[2];
#pragma unroll
            for (int a = 0; a < 3; ++a) cnd[0][a] = d.cand_p[3 * (size_t)p + a];
        }
        __syncthreads();
        for (int k = k0 + tid; k < k1; k += kPtChunkObs) {
            const int c = d.obs_cam[k];
            double m0 = 0.0, m1 = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) { const double sc = -d.y_c[6 * c + a]; m0 += d.Jc[a * n + k] * sc; m1 += d.Jc[(6 + a) * n + k] * sc; }
            if (d.has_calib) {
                group_step(c);
                if constexpr (RADIAL) {
                    double b0, b1;
                    block_f(k, b0, b1);
                    m0 -= b0; m1 -= b1;
                } else {
                    m0 -= d.Jk[k] * yk[0] + d.Jk[n + k] * yk[1];
                    m1 -= d.Jk[2 * n + k] * yk[2] + d.Jk[3 * n + k] * yk[3];
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) { m0 += d.Jp[a * n + k] * sps[0][a]; m1 += d.Jp[(3 + a) * n + k] * sps[0][a]; }
            const double r0 = d.res[k], r1 = d.res[n + k];
            mc -= m0 * (r0 + m0 / 2.0) + m1 * (r1 + m1 / 2.0);
            gd += m0 * r0 + m1 * r1;
            if (WITH_COST) {
                const double X[3] = {cnd[0][0], cnd[0][1], cnd[0][2]};
                candidate_cost<GROUPS>(d, k, X, cauchy_a, ccost, cbad);
            }
        }
    }
    if (WITH_COST) {
        const int slots[6] = {SC_MODEL_CHANGE, SC_STEP_SQ_PT, SC_CAND_SQ_PT, SC_GDOTD, SC_CAND_COST, SC_CAND_BAD};
        const double vals[6] = {mc, ssq, csq, d.constrained ? gd : 0.0, ccost, cbad};
        scal_commit<6>(d, sbase, slots, vals, red);
    } else {
        const int slots[4] = {SC_MODEL_CHANGE, SC_STEP_SQ_PT, SC_CAND_SQ_PT, SC_GDOTD};
        const double vals[4] = {mc, ssq, csq, d.constrained ? gd : 0.0};
        scal_commit<4>(d, sbase, slots, vals, red);
    }
    if (d.constrained) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, o));
        if ((threadIdx.x & 63) == 0 && dmax > 0.0) atomic_max_nonneg(&d.scal[SC_DMAX], dmax);
    }
}

// Robustified cost 1/2 sum rho(|r|^2) of (cams, pts) over this rank's observations.
// SLOPE: also d/dt cost(Plus(x, t delta)) at this point = gradient . delta = sum rho' r.(J delta), the derivative
// the Armijo search's cubic interpolation uses [upstream line_search.cc LineSearchFunction::Evaluate].
// RADIAL (a GROUPS form): the radial model and six values of the block and of its step.
template <bool SLOPE, bool GROUPS = false, bool RADIAL = false>
__global__ __launch_bounds__(256) void ba_cost_kernel(BADev d, const double *__restrict__ cams, const double *__restrict__ pts,
                                                      double cauchy_a, int slot, int bad_slot, ScalBase sbase)
{
    __shared__ double red[8];
    double cost = 0.0, bad = 0.0, slope = 0.0;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < d.n_obs; k += gridDim.x * 256) {
        const int c = d.obs_cam[k], p = d.obs_pt[k];
        const float2 uv = d.obs_uv[k];
        double in4[RADIAL ? 6 : 4];
        if constexpr (RADIAL) load_intrinsics_radial(d, cams, c, in4);
        else load_intrinsics<GROUPS>(d, cams, c, in4);
        double cam[6], X[3];
#pragma unroll
        for (int i = 0; i < 6; ++i) cam[i] = cams[6 * (size_t)c + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) X[i] = pts[3 * (size_t)p + i];
        double r0, r1, m0 = 0.0, m1 = 0.0;
        if (SLOPE) {
            double Jc[12], Jp[6], xn, yn;
            double Jk[8];
            if constexpr (RADIAL) reproject_jac_radial(cam, X, in4, uv, r0, r1, Jc, Jp, Jk);
            else reproject_jac(cam, X, in4, uv, r0, r1, Jc, Jp, xn, yn);
#pragma unroll
            for (int a = 0; a < 6; ++a) { const double dl = d.delta_c[6 * (size_t)c + a]; m0 += Jc[a] * dl; m1 += Jc[6 + a] * dl; }
#pragma unroll
            for (int a = 0; a < 3; ++a) { const double dl = d.delta_p[3 * (size_t)p + a]; m0 += Jp[a] * dl; m1 += Jp[3 + a] * dl; }
            if constexpr (RADIAL) {
                const double *dk = d.delta_c + 6 * (size_t)calib_block_of<true>(d, c);
                m0 += Jk[0] * dk[0] + Jk[1] * dk[1] + Jk[4] * dk[4] + Jk[5] * dk[5];
                m1 += Jk[2] * dk[2] + Jk[3] * dk[3] + Jk[6] * dk[4] + Jk[7] * dk[5];
            } else if (d.has_calib) {
                const double *dk = d.delta_c + 6 * (size_t)calib_block_of<GROUPS>(d, c);
                m0 -= xn * dk[0] + dk[1];
                m1 -= yn * dk[2] + dk[3];
            }
        } else {
            double pt[3];
            transform_point<false>(cam, X, pt, nullptr, nullptr);
            if constexpr (RADIAL) {
                reproject_radial(pt, in4, uv, r0, r1);
            } else {
                const double x = pt[0] / pt[2], y = pt[1] / pt[2];
                r0 = (double)uv.x - (x * in4[0] + in4[1]);
                r1 = (double)uv.y - (y * in4[2] + in4[3]);
            }
        }
        const double s = r0 * r0 + r1 * r1;
        if (!isfinite(s)) { bad += 1.0; continue; }
        double rho0, rho1;
        loss_eval(cauchy_a, s, rho0, rho1);
        cost += 0.5 * rho0;
        if (SLOPE) slope += rho1 * (r0 * m0 + r1 * m1);
    }
    if (SLOPE) {
        const int slots[3] = {slot, bad_slot, SC_LS_GRAD};
        const double vals[3] = {cost, bad, slope};
        scal_commit<3>(d, sbase, slots, vals, red);
    } else {
        const int slots[2] = {slot, bad_slot};
        const double vals[2] = {cost, bad};
        scal_commit<2>(d, sbase, slots, vals, red);
    }
}

// candidate = Plus(x, t delta): cameras (projected onto the box) by workgroup 0, points by all; step / candidate norms.
__global__ __launch_bounds__(256) void ba_take_step_kernel(BADev d, double t, ScalBase sbase)
{
    __shared__ double red[8];
    double ssq = 0.0, csq = 0.0, ssc = 0.0, csc = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 3 * d.n_pt; i += gridDim.x * 256) {
        const int p = i / 3;
        const double x = d.x_p[i];
        if (d.pt_start[p + 1] > d.pt_start[p]) {
            const double cnd = x + t * d.delta_p[i];
            const double df = x - cnd;
            ssq += df * df; csq += cnd * cnd;
            d.cand_p[i] = cnd;
        } else d.cand_p[i] = x;
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 6 * d.n_cam; i += 256) {
            const double x = d.x_c[i];
            if (d.cam_nobs[i / 6] > 0.0) {
                const double cnd = fmin(fmax(x + t * d.delta_c[i], d.lo_c[i]), d.up_c[i]);
                const double df = x - cnd;
                ssc += df * df; csc += cnd * cnd;
                d.cand_c[i] = cnd;
            } else d.cand_c[i] = x;
        }
    const double c = block_sum(ssc, red);
    const double e = block_sum(csc, red);
    if (threadIdx.x == 0 && blockIdx.x == 0) { d.scal[SC_STEP_SQ_CAM] = c; d.scal[SC_CAND_SQ_CAM] = e; }
    const int slots[2] = {SC_STEP_SQ_PT, SC_CAND_SQ_PT};
    const double vals[2] = {ssq, csq};
    scal_commit<2>(d, sbase, slots, vals, red);
}

// x_c <- projection onto the box (TrustRegionMinimizer::IterationZero: Plus(x, 0))
__global__ void ba_project_cameras_kernel(BADev d)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 6 * d.n_cam && d.cam_nobs[i / 6] > 0.0) d.x_c[i] = fmin(fmax(d.x_c[i], d.lo_c[i]), d.up_c[i]);
}

// |x|^2 over the parameter blocks that take part in the problem (Ceres drops unused blocks).
__global__ __launch_bounds__(256) void ba_param_sqnorm_kernel(BADev d, ScalBase sbase)
{
    __shared__ double red[8];
    double sp = 0.0, sc = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 3 * d.n_pt; i += gridDim.x * 256) {
        const int p = i / 3;
        if (d.pt_start[p + 1] > d.pt_start[p]) sp += d.x_p[i] * d.x_p[i];
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 6 * d.n_cam; i += 256)
            if (d.cam_nobs[i / 6] > 0.0) sc += d.x_c[i] * d.x_c[i];
    const double b = block_sum(sc, red);
    if (threadIdx.x == 0 && blockIdx.x == 0) d.scal[SC_XNORM_SQ_CAM] = b;
    const int slots[1] = {SC_XNORM_SQ_PT};
    const double vals[1] = {sp};
    scal_commit<1>(d, sbase, slots, vals, red);
}

// Multi-GPU merge of the point blocks: each rank owns the points it has observations for.
//   to_delta: x_p <- (owned ? x_p - x0_p : 0)   (then SUM all-reduce)
//   else    : x_p <- x0_p + x_p
__global__ void ba_points_delta_kernel(BADev d, int to_delta)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * d.n_pt) return;
    const int p = i / 3;
    if (to_delta) d.x_p[i] = (d.pt_start[p + 1] > d.pt_start[p]) ? d.x_p[i] - d.x0_p[i] : 0.0;
    else d.x_p[i] = d.x0_p[i] + d.x_p[i];
}

__global__ __launch_bounds__(1024) void ba_scal_reduce_kernel(const double *__restrict__ scal_part, int scal_cap, double *scal, ScalCounts c)
{
    scal_reduce_pending(scal_part, scal_cap, scal, c);
}

// Scalar read-back without a stream synchronisation: one workgroup adds the pending per-workgroup partials to the sum slots (see
// scal_commit), copies the scalar slots into pinned host memory, fences to system scope and then stores the sequence number the
// host is spinning on.
__global__ __launch_bounds__(1024) void ba_publish_scalars_kernel(const double *__restrict__ scal_part, int scal_cap, double *scal, ScalCounts c,
                                                                  double *host, unsigned long long *flag, unsigned long long seq)
{
    scal_reduce_pending(scal_part, scal_cap, scal, c);
    __syncthreads();
    const int i = threadIdx.x;
    // system-scope stores (write-through to the pinned host page) ordered against the flag by a workgroup-scope fence (s_waitcnt) and
    // a barrier: a system-scope release fence here is a write-back of the whole L2 on this part (see ba_chol_large.hip, st_coh)
    if (i < SC_COUNT) {
        __hip_atomic_store(&host[i], scal[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        scal[i] = 0.0;       // every read-back is followed by a reset before the next scalar-producing launch: done here, not by a memset launch
    }
    // (the workgroup-scope fence emits no s_waitcnt vmcnt(0) on gfx950: the explicit one is what keeps the flag behind the slots)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (i == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------------------------
int ba_solve_reduced(hipStream_t st, const BADev &d, double radius, double min_diag, double max_diag)
{
    if (d.n_cam <= 0) return ESFM_OK;
    switch (d.parts->forms.solve) {
    case BaForms::SOLVE_SMALL_ONE_WG: return ba_solve_reduced_small(st, d, radius, min_diag, max_diag);
    case BaForms::SOLVE_TILED:
        if (d.sparse) return ba_solve_reduced_sparse(st, d, d.sparse, radius, min_diag, max_diag);
        return ba_solve_reduced_large(st, d, radius, min_diag, max_diag);
    case BaForms::SOLVE_LDS: break;
    }
    const size_t bytes = chol_lds_bytes(d.n_cam);
    ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&ba_chol_solve_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(ba_chol_solve_kernel, dim3(1), dim3(kCholThreads), bytes, st, d, radius, min_diag, max_diag);
    LAUNCH_CHECK();
    return ESFM_OK;
}

static ScalCounts take_counts(const BADev &d)
{
    ScalCounts c;
    for (int q = 0; q < SC_SUM_COUNT; ++q) { c.n[q] = d.parts->n[q]; d.parts->n[q] = 0; }
    return c;
}

int ba_publish_scalars(hipStream_t st, const BADev &d, double *host, unsigned long long *flag, unsigned long long seq)
{
    hipLaunchKernelGGL(ba_publish_scalars_kernel, dim3(1), dim3(1024), 0, st, d.scal_part, d.scal_cap, d.scal, take_counts(d), host, flag, seq);
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_scal_reduce(hipStream_t st, const BADev &d)
{
    bool any = false;
    for (int q = 0; q < SC_SUM_COUNT; ++q) any = any || d.parts->n[q] > 0;
    if (!any) return ESFM_OK;
    hipLaunchKernelGGL(ba_scal_reduce_kernel, dim3(1), dim3(1024), 0, st, d.scal_part, d.scal_cap, d.scal, take_counts(d));
    LAUNCH_CHECK();
    return ESFM_OK;
}

void ba_scal_discard(const BADev &d, int first_slot, int end_slot)
{
    for (int q = std::max(0, first_slot); q < std::min<int>(SC_SUM_COUNT, end_slot); ++q) d.parts->n[q] = 0;
}

int ba_camera_step(hipStream_t st, const BADev &d)
{
    if (d.parts->forms.solve == BaForms::SOLVE_SMALL_ONE_WG) return ESFM_OK;     // the one-workgroup reduced solve has done it
    hipLaunchKernelGGL(ba_camera_step_kernel, dim3(1), dim3(256), 0, st, d);
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_backsub(hipStream_t st, const BADev &d, bool with_cost, double cauchy_a)
{
    if (d.n_pt <= 0 || d.n_pchunks <= 0) return ESFM_OK;
    ScalBase sbase;
    if (with_cost) {
        // the candidate's cost comes out of the same launch (SC_CAND_COST / SC_CAND_BAD): no ba_cost pass over the observations
        const int slots[6] = {SC_MODEL_CHANGE, SC_STEP_SQ_PT, SC_CAND_SQ_PT, SC_GDOTD, SC_CAND_COST, SC_CAND_BAD};
        if (int rc = scal_reserve<6>(st, d, slots, d.n_pchunks, sbase)) return rc;
        if (d.radial) { set_error("BA back-substitution: a radial problem is bounded and takes the candidate cost in its own pass"); return ESFM_ERR_INVALID_ARG; }
        auto kern = d.has_calib > 1 ? &ba_backsub_chunk_kernel<true, true> : &ba_backsub_chunk_kernel<true>;
        hipLaunchKernelGGL(kern, dim3(d.n_pchunks), dim3(kPtChunkObs), 0, st, d,
                           sbase, cauchy_a);
    } else {
        const int slots[4] = {SC_MODEL_CHANGE, SC_STEP_SQ_PT, SC_CAND_SQ_PT, SC_GDOTD};
        if (int rc = scal_reserve<4>(st, d, slots, d.n_pchunks, sbase)) return rc;
        auto kern = d.radial ? &ba_backsub_chunk_kernel<false, true, true> : d.has_calib > 1 ? &ba_backsub_chunk_kernel<false, true> : &ba_backsub_chunk_kernel<false>;
        hipLaunchKernelGGL(kern, dim3(d.n_pchunks), dim3(kPtChunkObs), 0, st, d,
                           sbase, cauchy_a);
    }
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_cost(hipStream_t st, const BADev &d, int num_cu, const double *cams, const double *pts, double cauchy_a, int slot, int bad_slot,
            bool with_slope)
{
    if (d.n_obs <= 0) return ESFM_OK;
    const int grid = std::min(div_up(d.n_obs, 256), std::max(1, num_cu) * 8);
    ScalBase sbase;
    if (with_slope) {
        const int slots[3] = {slot, bad_slot, SC_LS_GRAD};
        if (int rc = scal_reserve<3>(st, d, slots, grid, sbase)) return rc;
        auto kern = d.radial ? &ba_cost_kernel<true, true, true> : d.has_calib > 1 ? &ba_cost_kernel<true, true> : &ba_cost_kernel<true>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, d, cams, pts, cauchy_a, slot, bad_slot,
                           sbase);
    } else {
        const int slots[2] = {slot, bad_slot};
        if (int rc = scal_reserve<2>(st, d, slots, grid, sbase)) return rc;
        auto kern = d.radial ? &ba_cost_kernel<false, true, true> : d.has_calib > 1 ? &ba_cost_kernel<false, true> : &ba_cost_kernel<false>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, d, cams, pts, cauchy_a, slot, bad_slot,
                           sbase);
    }
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_take_step(hipStream_t st, const BADev &d, double t)
{
    const int grid = std::max(1, std::min(div_up(3LL * d.n_pt, 256), 1024));
    ScalBase sbase;
    { const int slots[2] = {SC_STEP_SQ_PT, SC_CAND_SQ_PT}; if (int rc = scal_reserve<2>(st, d, slots, grid, sbase)) return rc; }
    hipLaunchKernelGGL(ba_take_step_kernel, dim3(grid), dim3(256), 0, st, d, t, sbase);
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_project_cameras(hipStream_t st, const BADev &d)
{
    if (d.n_cam <= 0) return ESFM_OK;
    hipLaunchKernelGGL(ba_project_cameras_kernel, dim3(div_up(6 * d.n_cam, 256)), dim3(256), 0, st, d);
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_param_sqnorm(hipStream_t st, const BADev &d)
{
    const int grid = std::max(1, std::min(div_up(3LL * d.n_pt, 256), 1024));
    ScalBase sbase;
    { const int slots[1] = {SC_XNORM_SQ_PT}; if (int rc = scal_reserve<1>(st, d, slots, grid, sbase)) return rc; }
    hipLaunchKernelGGL(ba_param_sqnorm_kernel, dim3(grid), dim3(256), 0, st, d, sbase);
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_points_delta(hipStream_t st, const BADev &d, bool to_delta)
{
    if (d.n_pt <= 0) return ESFM_OK;
    hipLaunchKernelGGL(ba_points_delta_kernel, dim3(div_up(3LL * d.n_pt, 256)), dim3(256), 0, st, d, to_delta ? 1 : 0);
    LAUNCH_CHECK();
    return ESFM_OK;
}

}  // namespace esfm
