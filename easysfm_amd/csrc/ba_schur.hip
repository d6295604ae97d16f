// Bundle adjustment, elimination stage: the point-block Schur complement of DENSE_SCHUR (reference cpp_code/src/ba.cpp:201, Ceres'
// schur_eliminator_impl.h [upstream]) into the reduced camera system, accumulated in 64-bit fixed point (BADev::qexp).  Kernels
// and their launchers:
//
//   ba_schur_kernel            per observation into global memory (the wide tracks of large problems)
//   ba_schur_lds_kernel        all camera blocks in every workgroup's LDS + ba_schur_reduce_kernel over the slabs (n_cam <= 32)
//   ba_schur_window_kernel     an LDS window of consecutive cameras per chunk of points
//   ba_schur_mfma_kernel       the narrow tracks as dense products on the f64 matrix cores
//   ba_schur_calib_kernel      the block row of the free intrinsics
//   ba_schur_to_double_kernel  fixed point -> f64; ba_red_pack_kernel: the exchange buffer between GPUs
//
// Which form runs when: BaForms (ba_forms.hpp).  DESIGN.md "Bundle adjustment".
#include "ba_device.hpp"

namespace esfm {

// Point-block Schur complement (schur_eliminator_impl.h [upstream]).  Thread i owns observation i of
// point p: W_i = F_i'E_i, Y_i = W_i M^-1; rhs_corr[c_i] -= W_i M^-1 E'r; and for every observation j of
// the same point with camera(j) <= camera(i):  S[c_i][c_j] -= Y_i W_j'.  Only blocks on or below the
// block diagonal are produced (the factorisation reads the lower triangle).
// One pair of observations (i, j) of a point: block (c_i, c_j) of the Schur complement gets -Y_i W_j' (Y_i = W_i M^-1, rows scaled
// by 2^(60 - qexp[row]); W_j's columns by 2^-qexp[col] here), as fixed-point adds.  Entry (a, c2) goes to Sb[a * ra + c2 * rc]:
// (ra, rc) = (6, 1) normally, (1, 6) when the pair was met with c_j > c_i and the contribution belongs to the stored block
// (c_j, c_i) as its transpose -- run-time strides, so that a wave whose lanes disagree does not execute the loop twice.
// BOTH: a camera that sees the point twice -- the diagonal block is stored in full and takes the product and its transpose.
template <bool BOTH>
__device__ __forceinline__ void schur_pair(double *Sb, int ra, int rc, const double (&Y)[18], const double (&Wj)[18], const int *qe_j)
{
#pragma unroll
    for (int c2 = 0; c2 < 6; ++c2) {
        const int ej = -qe_j[c2];
        const double w0 = ldexp(Wj[3 * c2], ej), w1 = ldexp(Wj[3 * c2 + 1], ej), w2 = ldexp(Wj[3 * c2 + 2], ej);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const unsigned long long v = fx64_scaled(-fma(Y[3 * a + 2], w2, fma(Y[3 * a + 1], w1, Y[3 * a] * w0)));   // (explicit fma: the file is built with -ffp-contract=off)
            atomicAdd(reinterpret_cast<unsigned long long *>(&Sb[a * ra + c2 * rc]), v);
            if (BOTH) atomicAdd(reinterpret_cast<unsigned long long *>(&Sb[a * rc + c2 * ra]), v);
        }
    }
}

// list != NULL: the observations list[0 .. n_list) only (the wide tracks the windowed kernel leaves out)
__global__ __launch_bounds__(256) void ba_schur_kernel(BADev d, int rhs_exp, const int32_t *__restrict__ list, int n_list)
{
    const int li = blockIdx.x * 256 + threadIdx.x;
    if (li >= (list ? n_list : d.n_obs)) return;
    const int i = list ? list[li] : li;
    const size_t n_obs = d.n_obs;
    const int n = 6 * d.n_cam;
    const int p = d.obs_pt[i], ci = d.obs_cam[i];
    double W[18];
    load_W(d, n_obs, i, W);
    const double *Mi = d.Minv + 6 * (size_t)p;
    const double M[9] = {Mi[0], Mi[1], Mi[2], Mi[1], Mi[3], Mi[4], Mi[2], Mi[4], Mi[5]};
    const double ag0 = d.Aig[3 * (size_t)p], ag1 = d.Aig[3 * (size_t)p + 1], ag2 = d.Aig[3 * (size_t)p + 2];
    const int b = d.pt_start[p], T = d.pt_start[p + 1] - b, t = i - b;
    double Y[18];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const double w0 = W[3 * a], w1 = W[3 * a + 1], w2 = W[3 * a + 2];
        const int ei = kFxBits - d.qexp[6 * ci + a];
        fx_add(&d.red[(size_t)n * n + 6 * ci + a], -(w0 * ag0 + w1 * ag1 + w2 * ag2), ei - rhs_exp);
        Y[3 * a + 0] = ldexp(w0 * M[0] + w1 * M[3] + w2 * M[6], ei);
        Y[3 * a + 1] = ldexp(w0 * M[1] + w1 * M[4] + w2 * M[7], ei);
        Y[3 * a + 2] = ldexp(w0 * M[2] + w1 * M[5] + w2 * M[8], ei);
    }
    schur_pair<false>(d.red + (size_t)(6 * ci) * n + 6 * ci, n, 1, Y, W, d.qexp + 6 * ci);
    for (int s2 = 1; 2 * s2 <= T; ++s2) {
        if (2 * s2 == T && t < s2) continue;
        int q = t - s2; if (q < 0) q += T;
        const int j = b + q;
        const int cj = d.obs_cam[j];
        double Wj[18];
        load_W(d, n_obs, j, Wj);
        const int hi = cj > ci ? cj : ci, lo = cj > ci ? ci : cj;
        double *Sb = d.red + (size_t)(6 * hi) * n + 6 * lo;
        if (cj != ci) schur_pair<false>(Sb, cj > ci ? 1 : n, cj > ci ? n : 1, Y, Wj, d.qexp + 6 * cj);
        else schur_pair<true>(Sb, n, 1, Y, Wj, d.qexp + 6 * cj);
    }
}

__global__ __launch_bounds__(1024) void ba_schur_lds_kernel(BADev d, double *__restrict__ slabs, int slab_doubles, int rhs_exp)
{
    extern __shared__ __attribute__((aligned(16))) double sl[];   // [nblk * kSchurPitch] blocks, [n] rhs_corr, then [n] ints: qexp
    const int tid = threadIdx.x;
    const int n = 6 * d.n_cam;
    const int nblk = d.n_cam * (d.n_cam + 1) / 2;
    const int lds_doubles = nblk * kSchurPitch + n;
    for (int e = tid; e < lds_doubles; e += blockDim.x) sl[e] = 0.0;
    double *srhs = sl + (size_t)nblk * kSchurPitch;
    int *qe = reinterpret_cast<int *>(sl + lds_doubles);
    for (int e = tid; e < n; e += blockDim.x) qe[e] = d.qexp[e];
    __syncthreads();
    const size_t n_obs = d.n_obs;
    for (int i = blockIdx.x * blockDim.x + tid; i < d.n_obs; i += gridDim.x * blockDim.x) {
        const int p = d.obs_pt[i], ci = d.obs_cam[i];
        double W[18];
        load_W(d, n_obs, i, W);
        const double *Mi = d.Minv + 6 * (size_t)p;
        const double M[9] = {Mi[0], Mi[1], Mi[2], Mi[1], Mi[3], Mi[4], Mi[2], Mi[4], Mi[5]};
        const double ag0 = d.Aig[3 * (size_t)p], ag1 = d.Aig[3 * (size_t)p + 1], ag2 = d.Aig[3 * (size_t)p + 2];
        const int b = d.pt_start[p], T = d.pt_start[p + 1] - b, t = i - b;
        double Y[18];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double w0 = W[3 * a], w1 = W[3 * a + 1], w2 = W[3 * a + 2];
            const int ei = kFxBits - qe[6 * ci + a];
            fx_add(&srhs[6 * ci + a], -(w0 * ag0 + w1 * ag1 + w2 * ag2), ei - rhs_exp);
            Y[3 * a + 0] = ldexp(w0 * M[0] + w1 * M[3] + w2 * M[6], ei);
            Y[3 * a + 1] = ldexp(w0 * M[1] + w1 * M[4] + w2 * M[7], ei);
            Y[3 * a + 2] = ldexp(w0 * M[2] + w1 * M[5] + w2 * M[8], ei);
        }
        // its own block, then the partners at distance s = 1 .. T/2 around the track (cyclically): every unordered pair of the
        // point's observations is met exactly once and every observation does the same number of pairs (walking j over the
        // whole track and keeping c_j <= c_i did 8 iterations for 4.5 pairs on an 8-observation track)
        schur_pair<false>(sl + (size_t)(ci * (ci + 1) / 2 + ci) * kSchurPitch, 6, 1, Y, W, qe + 6 * ci);
        for (int s2 = 1; 2 * s2 <= T; ++s2) {
            if (2 * s2 == T && t < s2) continue;              // the half-way partners meet once
            int q = t - s2; if (q < 0) q += T;
            const int j = b + q;
            const int cj = d.obs_cam[j];
            double Wj[18];
            load_W(d, n_obs, j, Wj);
            const int hi = cj > ci ? cj : ci, lo = cj > ci ? ci : cj;
            double *Sb = sl + (size_t)(hi * (hi + 1) / 2 + lo) * kSchurPitch;
            if (cj != ci) schur_pair<false>(Sb, cj > ci ? 1 : 6, cj > ci ? 6 : 1, Y, Wj, qe + 6 * cj);
            else schur_pair<true>(Sb, 6, 1, Y, Wj, qe + 6 * cj);
        }
    }
    __syncthreads();
    double *out = slabs + (size_t)blockIdx.x * slab_doubles;
    for (int e = tid; e < slab_doubles; e += blockDim.x) out[e] = e < nblk * 36 ? sl[(e / 36) * kSchurPitch + e % 36] : sl[e + nblk * (kSchurPitch - 36)];
}

// Large camera counts: the Schur matrix does not fit LDS, but a workgroup that walks points ordered by their
// lowest camera only touches a narrow band of it.  Each workgroup owns one chunk of that point order and an
// LDS window of kWinCams consecutive cameras starting at the chunk's lowest one: contributions whose two
// cameras fall inside the window are accumulated with LDS f64 atomics, the few that do not (wide baselines,
// ring wrap-around) go straight to global f64 atomics; the window is flushed once at the end.
constexpr int kWinCams = kSchurWinCams;
constexpr int kWinBlocks = kWinCams * (kWinCams + 1) / 2;

// rot: camera indices are rotated by rot (mod n_real_cam) before the window test -- the second pass, rot = n_real_cam / 2, takes
// the tracks that straddle the seam of a closed camera loop (cameras 508 .. 511, 0 .. 5 of a ring of 512): in true indices they
// are 500 cameras wide and would all go to same-address global atomics (measured: 2.1 ms for 2 % of BA-512's observations).
__global__ __launch_bounds__(1024) void ba_schur_window_kernel(BADev d, int rhs_exp, const int32_t *__restrict__ slot_obs,
                                                               const int32_t *__restrict__ chunk_slot, const int32_t *__restrict__ chunk_cam0, int rot)
{
    extern __shared__ __attribute__((aligned(16))) double sl[];   // [kWinBlocks * kSchurPitch] blocks, then [6*kWinCams] rhs_corr
    const int tid = threadIdx.x;
    const int n = 6 * d.n_cam, nrc = d.n_real_cam;
    const int chunk = blockIdx.x;
    const int s0 = chunk_slot[chunk], s1 = chunk_slot[chunk + 1];
    const int cw = chunk_cam0[chunk];                               // window base, in ROTATED camera indices
    auto rotated = [&](int c) { const int r = c + rot; return r >= nrc ? r - nrc : r; };
    constexpr int kWinDoubles = kWinBlocks * kSchurPitch + 6 * kWinCams;
    for (int e = tid; e < kWinDoubles; e += 1024) sl[e] = 0.0;
    __syncthreads();
    double *srhs = sl + kWinBlocks * kSchurPitch;
    const size_t n_obs = d.n_obs;
    for (int s = s0 + tid; s < s1; s += 1024) {
        const int i = slot_obs[s];
        const int p = d.obs_pt[i], ci = d.obs_cam[i];
        double W[18];
        load_W(d, n_obs, i, W);
        const double *Mi = d.Minv + 6 * (size_t)p;
        const double M[9] = {Mi[0], Mi[1], Mi[2], Mi[1], Mi[3], Mi[4], Mi[2], Mi[4], Mi[5]};
        const double ag0 = d.Aig[3 * (size_t)p], ag1 = d.Aig[3 * (size_t)p + 1], ag2 = d.Aig[3 * (size_t)p + 2];
        const int b = d.pt_start[p], T = d.pt_start[p + 1] - b, t = i - b;
        const int wi = rotated(ci) - cw;
        const bool in_i = wi >= 0 && wi < kWinCams;
        double Y[18];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double w0 = W[3 * a], w1 = W[3 * a + 1], w2 = W[3 * a + 2];
            const int ei = kFxBits - d.qexp[6 * ci + a];
            const unsigned long long rv = fx64(-(w0 * ag0 + w1 * ag1 + w2 * ag2), ei - rhs_exp);
            atomicAdd(reinterpret_cast<unsigned long long *>(in_i ? &srhs[6 * wi + a] : &d.red[(size_t)n * n + 6 * ci + a]), rv);
            Y[3 * a + 0] = ldexp(w0 * M[0] + w1 * M[3] + w2 * M[6], ei);
            Y[3 * a + 1] = ldexp(w0 * M[1] + w1 * M[4] + w2 * M[7], ei);
            Y[3 * a + 2] = ldexp(w0 * M[2] + w1 * M[5] + w2 * M[8], ei);
        }
        // its own block, then the partners at distance 1 .. T/2 around the track (see ba_schur_lds_kernel).  A pair's block sits
        // in the LDS window when both cameras do; there it is oriented by the ROTATED indices (row = the larger one) and turned
        // the right way round when the window is flushed.
        if (in_i) schur_pair<false>(sl + (size_t)(wi * (wi + 1) / 2 + wi) * kSchurPitch, 6, 1, Y, W, d.qexp + 6 * ci);
        else schur_pair<false>(d.red + (size_t)(6 * ci) * n + 6 * ci, n, 1, Y, W, d.qexp + 6 * ci);
        for (int s2 = 1; 2 * s2 <= T; ++s2) {
            if (2 * s2 == T && t < s2) continue;              // the half-way partners meet once
            int q = t - s2; if (q < 0) q += T;
            const int j = b + q;
            const int cj = d.obs_cam[j];
            double Wj[18];
            load_W(d, n_obs, j, Wj);
            const int wj = rotated(cj) - cw;
            const bool in_w = in_i && wj >= 0 && wj < kWinCams;
            // (two call sites on purpose: with the address space known the window gets ds_add_u64; one merged pointer made every
            // add a flat atomic)
            if (in_w) {
                const int wh = wj > wi ? wj : wi, wl = wj > wi ? wi : wj;
                double *Sb = sl + (size_t)(wh * (wh + 1) / 2 + wl) * kSchurPitch;
                if (wj != wi) schur_pair<false>(Sb, wj > wi ? 1 : 6, wj > wi ? 6 : 1, Y, Wj, d.qexp + 6 * cj);
                else schur_pair<true>(Sb, 6, 1, Y, Wj, d.qexp + 6 * cj);
            } else {
                const int hi = cj > ci ? cj : ci, lo = cj > ci ? ci : cj;
                double *Sb = d.red + (size_t)(6 * hi) * n + 6 * lo;
                if (cj != ci) schur_pair<false>(Sb, cj > ci ? 1 : n, cj > ci ? n : 1, Y, Wj, d.qexp + 6 * cj);
                else schur_pair<true>(Sb, n, 1, Y, Wj, d.qexp + 6 * cj);
            }
        }
    }
    __syncthreads();
    // flush the window: rotated-local (wi >= wj) -> true cameras; the stored triangle wants row camera >= column camera
    const unsigned long long *sq = reinterpret_cast<const unsigned long long *>(sl);   // same grid per entry as d.red: integer adds
    auto true_cam = [&](int w) { int c = cw + w - rot; if (c < 0) c += nrc; return c; };
    for (int e = tid; e < kWinBlocks * 36; e += 1024) {
        const int blk = e / 36, r = e % 36;
        const unsigned long long v = sq[blk * kSchurPitch + r];
        if (v == 0ull) continue;
        int wi = 0, wj = blk;
        while (wj > wi) { wj -= wi + 1; ++wi; }
        const int ci = true_cam(wi), cj = true_cam(wj);
        if (ci >= nrc || cj >= nrc) continue;
        const size_t at = ci >= cj ? (size_t)(6 * ci + r / 6) * n + 6 * cj + r % 6 : (size_t)(6 * cj + r % 6) * n + 6 * ci + r / 6;
        atomicAdd(reinterpret_cast<unsigned long long *>(&d.red[at]), v);
    }
    for (int e = tid; e < 6 * kWinCams; e += 1024) {
        const unsigned long long v = sq[kWinBlocks * kSchurPitch + e];
        if (v == 0ull) continue;
        const int c = true_cam(e / 6);
        if (c < nrc) atomicAdd(reinterpret_cast<unsigned long long *>(&d.red[(size_t)n * n + 6 * c + e % 6]), v);
    }
}

// ---------------------------------------------------------------------------------------------
// Point-block Schur complement on the f64 matrix cores (round 3).  For one point p with observations i = 1..T,
//     sum over the pairs (i, j) of p of  -Y_i W_j'  =  -(Yhat_p)(What_p)',      Yhat_p = [Y_i]_i (6 T x 3),  Y_i = W_i M_p^-1,
// a rank-3 update of the rows / columns of p's cameras -- and the sum over the points of a chunk whose cameras lie in one window of
// kSchurMfCams indices is a dense product  G = sum_p Yw_p Ww_p'  (80 x 80, rows = 6 (camera - window base) + a), symmetric because
// M^-1 is.  ba_schur_window_kernel adds the 36 entries of every pair with 64-bit LDS atomics, and consecutive points see the same
// cameras: up to 64 lanes on one address, 0.93 ms per pass over BA-512 (25 x what conflict-free LDS adds would take).  Here a wave
// takes a batch of whole points (<= 64 observations, one per lane): the lanes form W_i and Y_i of their observation (the same loads
// and arithmetic as the atomic kernels) and park them in a wave-private LDS table; then point by point the 16-row operand
// fragments are gathered from that table (a lane's row belongs to one camera slot: looked up in the point's slot -> lane table,
// zero if the point does not see it) and the lower block triangle of G is accumulated with v_mfma_f64_16x16x4_f64 -- K = 4 = the
// three columns of a point and a zero -- in registers for the whole chunk.  No atomics until the end: the four waves' tiles are
// added in wave order through LDS and the chunk's G goes into d.red as fixed-point integers like every other contribution (one
// atomic per entry and chunk), so the result does not depend on how workgroups are scheduled.
// Points with a camera twice, or spanning more than kSchurMfCams indices in both numberings, stay with the atomic kernels.
// Measured on BA-512 (3 M observations, 512 chunks): 276 us for the plain numbering + 50 us for the seam's rotated table, against
// 856 + 45 us of the atomic window kernel; with the matrix products AND the flush compiled out the launch still takes ~180 us --
// what is left is the lanes' own loads and arithmetic (432 MB of Jacobian rows, the point blocks, 36 LDS stores per lane).  Issuing a
// batch's loads one batch ahead changed nothing (345 against 341 us, 47 spilled registers) and neither did a scene whose points are
// numbered by lowest camera, i.e. contiguous reads (465 against 487 us on a slower box: the kernel also varies 340 - 490 us box to box).
constexpr int kMfRows = 80, kMfBR = 5, kMfYPitch = 37, kMfMaxPts = 16;
constexpr int kMfWaveDoubles = 65 * kMfYPitch + kMfMaxPts;     // Y | W table (36 doubles per observation, pitch 37; row 64 = zeros) + per-point slot masks and first lanes (ints)
constexpr size_t kMfLdsBytes = sizeof(double) * (4 * kMfWaveDoubles + 6 * kSchurMfCams + kMfRows / 2);     // ... + right-hand side (u64) + the window's exponents (ints)
static_assert(4 * kMfWaveDoubles >= kMfRows * (kMfRows + 1), "the staging area is reused for the 80 x 81 result");
static_assert(kSchurMfCams <= 16 && 6 * kSchurMfCams <= kMfRows, "slot masks are 16 bits; the window's rows fit the tile grid");

// Both tables in ONE launch (round 5): workgroups [0, n_plain) take the plain numbering's chunks, the rest the seam's (camera indices
// rotated by `rot_seam`).  The seam's table is 2 % of BA-512's observations in ~100 short chunks whose fixed costs -- zeroing 120
// accumulator registers, the 80 x 81 sum through LDS, 3 240 fixed-point atomics -- made a launch of their own last 47 us; behind the
// plain chunks they fill the launch's tail.
struct SchurMfTables {
    const int32_t *slot_obs[2]; const int2 *slot_pc[2]; const int32_t *batch_slot[2]; const int32_t *chunk_batch0[2]; const int32_t *chunk_cam0[2];
    int n_plain, rot_seam;
};
__global__ __launch_bounds__(256, 2) void ba_schur_mfma_kernel(BADev d, int rhs_exp, SchurMfTables tabs)
{
    const int tb = (int)blockIdx.x >= tabs.n_plain ? 1 : 0;
    const int32_t *__restrict__ slot_obs = tabs.slot_obs[tb];
    const int2 *__restrict__ slot_pc = tabs.slot_pc[tb];
    const int32_t *__restrict__ batch_slot = tabs.batch_slot[tb];
    const int32_t *__restrict__ chunk_batch0 = tabs.chunk_batch0[tb];
    const int32_t *__restrict__ chunk_cam0 = tabs.chunk_cam0[tb];
    const int rot = tb ? tabs.rot_seam : 0;
    typedef double doublex4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) double sl[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *Yw = sl + (size_t)wave * kMfWaveDoubles;                               // [65][kMfYPitch]; row 64 stays zero
    unsigned int *pmask = reinterpret_cast<unsigned int *>(Yw + 65 * kMfYPitch);   // [kMfMaxPts] camera slots the point is seen from (bit = slot)
    int *pfirst = reinterpret_cast<int *>(pmask) + kMfMaxPts;                      // [kMfMaxPts] lane of the point's first observation
    unsigned long long *srhs = reinterpret_cast<unsigned long long *>(sl + 4 * (size_t)kMfWaveDoubles);   // [6 * kSchurMfCams]
    int *s_qe = reinterpret_cast<int *>(srhs + 6 * kSchurMfCams);                  // [kMfRows] fixed-point exponents of the window's rows
    const int n = 6 * d.n_cam, nrc = d.n_real_cam;
    const size_t n_obs = d.n_obs;
    const int chunk = (int)blockIdx.x - (tb ? tabs.n_plain : 0);
    const int cw = chunk_cam0[chunk];
    const int b0 = chunk_batch0[chunk], b1 = chunk_batch0[chunk + 1];
    auto rotated = [&](int c) { const int r = c + rot; return r >= nrc ? r - nrc : r; };
    auto true_cam = [&](int w) { int c = cw + w - rot; if (c < 0) c += nrc; return c; };
    for (int e = tid; e < 6 * kSchurMfCams; e += 256) srhs[e] = 0ull;
    // the exponents the flush converts with: fetched now, read from LDS after the batches (round 5: the flush's 25 entries per thread
    // each waited for two dependent global loads -- 58 us per workgroup, a fifth of the launch)
    if (tid < kMfRows) { const int c = true_cam(tid / 6); s_qe[tid] = (tid < 6 * kSchurMfCams && c < nrc) ? d.qexp[6 * c + tid % 6] : 0; }
    if (lane < kMfYPitch) Yw[64 * kMfYPitch + lane] = 0.0;
    __syncthreads();
    doublex4 acc[kMfBR * (kMfBR + 1) / 2];
#pragma unroll
    for (int t = 0; t < kMfBR * (kMfBR + 1) / 2; ++t) acc[t] = doublex4{0.0, 0.0, 0.0, 0.0};
    const int r16 = lane & 15, m4 = lane >> 4;          // this lane's row inside a block row, and its K index (point column; 3 = zero)
    // What a lane gathers for block row R does not depend on the point: camera slot sc = row / 6 and entry 3 a + column of the
    // observation's 36-double record.  WHICH observation is the point's business: a point's observations sit in consecutive lanes in
    // ascending slot order (the host builds the tables that way), so the one with slot sc is lane  first + popcount(mask & ((1 << sc) - 1))
    // if bit sc of the point's slot mask is set, and the zero row otherwise -- two words per point instead of a slot -> lane table
    // whose 80 entries per point had to be cleared, written and looked up (round 5).
    int fr_sc[kMfBR], fr_off[kMfBR]; unsigned int fr_low[kMfBR];
#pragma unroll
    for (int R = 0; R < kMfBR; ++R) {
        const int row = 16 * R + r16, sc = row / 6, a = row - 6 * sc;
        fr_sc[R] = sc < kSchurMfCams ? sc : 31;                      // bit 31 of a slot mask is never set
        fr_off[R] = 3 * a;
        fr_low[R] = (1u << (sc < kSchurMfCams ? sc : 0)) - 1u;
    }
    // A lane's observation, point and camera come from slot-ordered tables (contiguous, one load level) and are fetched one batch
    // AHEAD: the Jacobian rows / point block / exponents they address can then be requested the moment a batch starts -- one
    // round trip to memory per batch where the chain  slot -> observation -> point, camera -> rows  made three (8 us per batch).
    int nx_i = 0, nx_nob = 0; int2 nx_pc = make_int2(0, 0);
    auto fetch_ids = [&](int b) {
        if (b >= b1) { nx_nob = 0; return; }
        const int s0 = batch_slot[b];
        nx_nob = batch_slot[b + 1] - s0;
        const int sl_ = s0 + (lane < nx_nob ? lane : 0);
        nx_i = slot_obs[sl_]; nx_pc = slot_pc[sl_];
    };
    // ... and the ROWS of a batch are requested while the batch before it is in its matrix products (round 5; they land in the same
    // registers the products do not need: nothing is held twice).  Before that a wave waited 2.9 us per batch for them -- a third
    // of a batch's time, at the two waves per SIMD the accumulators leave room for.
    double Jc[12], Jp[6], Mi[6], ag[3];
    int qe[6];
    auto fetch_rows = [&]() {           // of the batch whose ids fetch_ids left in nx_*
        const int i = nx_i, p = nx_pc.x, ci = nx_pc.y;
#pragma unroll
        for (int q = 0; q < 12; ++q) Jc[q] = d.Jc[q * n_obs + i];
#pragma unroll
        for (int q = 0; q < 6; ++q) Jp[q] = d.Jp[q * n_obs + i];
#pragma unroll
        for (int q = 0; q < 6; ++q) Mi[q] = d.Minv[6 * (size_t)p + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) ag[q] = d.Aig[3 * (size_t)p + q];
#pragma unroll
        for (int a = 0; a < 6; ++a) qe[a] = d.qexp[6 * ci + a];
    };
    fetch_ids(b0 + wave);
    fetch_rows();
    for (int b = b0 + wave; b < b1; b += 4) {
        const int nob = nx_nob;
        const bool valid = lane < nob;
        const int p = nx_pc.x, ci = nx_pc.y;
        fetch_ids(b + 4);
        const int slot = rotated(ci) - cw;                                          // 0 .. kSchurMfCams - 1 by construction
        // local index of the lane's point inside the batch (the batch is whole points, in order)
        const int pprev = __shfl_up(p, 1);
        const bool first = valid && (lane == 0 || pprev != p);
        const unsigned long long starts = __ballot(first);
        const int q = __popcll(starts & ((2ull << lane) - 1ull)) - 1;
        const int npts = __popcll(starts);
        double W[18];                   // W_i = F_i'E_i (load_W's arithmetic)
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int m = 0; m < 3; ++m) W[3 * a + m] = Jc[a] * Jp[m] + Jc[6 + a] * Jp[3 + m];
        const double M[9] = {Mi[0], Mi[1], Mi[2], Mi[1], Mi[3], Mi[4], Mi[2], Mi[4], Mi[5]};
        const double ag0 = ag[0], ag1 = ag[1], ag2 = ag[2];
        if (lane < kMfMaxPts) pmask[lane] = 0u;
        if (valid) {
            atomicOr(&pmask[q], 1u << slot);
            if (first) pfirst[q] = lane;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double w0 = W[3 * a], w1 = W[3 * a + 1], w2 = W[3 * a + 2];
                const int ei = kFxBits - qe[a];
                atomicAdd(&srhs[6 * slot + a], fx64(-(w0 * ag0 + w1 * ag1 + w2 * ag2), ei - rhs_exp));
                double *y = Yw + lane * kMfYPitch + 3 * a;
                y[0] = w0 * M[0] + w1 * M[3] + w2 * M[6];
                y[1] = w0 * M[1] + w1 * M[4] + w2 * M[7];
                y[2] = w0 * M[2] + w1 * M[5] + w2 * M[8];
                y[18] = w0; y[19] = w1; y[20] = w2;
            }
        }
        // block rows the batch touches (wave-uniform)
        int smin = valid ? slot : kSchurMfCams, smax = valid ? slot : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { smin = min(smin, __shfl_xor(smin, o)); smax = max(smax, __shfl_xor(smax, o)); }
        const int R0 = __builtin_amdgcn_readfirstlane((6 * smin) / 16), R1 = __builtin_amdgcn_readfirstlane((6 * smax + 5) / 16);
        // The wave's own LDS writes are visible to its later reads (DS operations of a wave execute in order); the fence pair says so
        // to the COMPILER -- other lanes' stores above, a data-dependent gather below: without it nothing forbids hoisting the loads
        // (no instruction is emitted for a wavefront-scope fence).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        fetch_rows();                   // the next batch's (its ids were requested at the top; clamped to lane 0's slot past the end)
        // The K = 4 slices of one matrix instruction are four consecutive (point, column) pairs of the batch -- slice 4 t + k is column
        // (4 t + k) % 3 of point (4 t + k) / 3 -- not "three columns of one point and a zero": 3/4 of the instructions, and the matrix
        // pipe is what this loop waits for (a 16 x 16 x 4 f64 product occupies it for 64 cycles on this part -- its f64 matrix rate
        // equals its f64 vector rate -- and a ten-camera point touched 10 - 15 tiles: 2.6 us per batch of 6.4 points, 5.4 us per batch
        // and wave measured with two waves per SIMD).  A lane's slice decides its point: the point's mask and first lane come from
        // LDS by a per-lane address.  No branch: a slot the point does not have -- any slot of a block row the batch does not touch
        // is one -- and a slice past the batch's last point read the zero row.
        // (A second set of fragment registers to fetch the next step's rows under this step's products spilled at two waves per SIMD
        // and lost at one: measured, not kept.)
        const int nsteps = (3 * npts + 3) >> 2;
        for (int t = 0; t < nsteps; ++t) {
            const int sigma = 4 * t + m4;
            const int pq = (sigma * 43) >> 7;                    // sigma / 3 for sigma < 128
            const int col = sigma - 3 * pq;
            const bool live = pq < npts;
            const unsigned int pm = live ? pmask[pq & (kMfMaxPts - 1)] : 0u;
            const int pf = pfirst[pq & (kMfMaxPts - 1)];
            double fa[kMfBR], fb[kMfBR];
#pragma unroll
            for (int R = 0; R < kMfBR; ++R) {
                const int have = (int)((pm >> fr_sc[R]) & 1u);
                const int o = 64 + have * (pf + (int)__popc(pm & fr_low[R]) - 64);
                const double *y = Yw + o * kMfYPitch + fr_off[R] + col;
                fa[R] = y[0]; fb[R] = y[18];
            }
#pragma unroll
            for (int R = 0; R < kMfBR; ++R) {
                if (R < R0 || R > R1) continue;
#pragma unroll
                for (int C = 0; C <= R; ++C) {
                    if (C < R0) continue;
                    acc[R * (R + 1) / 2 + C] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[R], fb[C], acc[R * (R + 1) / 2 + C], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);       // lgkmcnt(0): the table has been read before the next batch overwrites it
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (... and the compiler may not sink this batch's reads below the next one's stores)
        __builtin_amdgcn_wave_barrier();
    }
    // the chunk's G: the waves' tiles added in wave order (fixed), lower block triangle, in the staging area
    __syncthreads();
    double *G = sl;                                // [kMfRows][kMfRows + 1]
    for (int e = tid; e < kMfRows * (kMfRows + 1); e += 256) G[e] = 0.0;
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int R = 0; R < kMfBR; ++R)
#pragma unroll
                for (int C = 0; C <= R; ++C)
#pragma unroll
                    for (int g = 0; g < 4; ++g) G[(16 * R + m4 + 4 * g) * (kMfRows + 1) + 16 * C + r16] += acc[R * (R + 1) / 2 + C][g];
        }
        __syncthreads();
    }
    // S -= G on the entry's fixed-point grid.  Window order (row >= col) is not camera order once the indices are rotated: the stored
    // triangle wants row camera >= column camera in TRUE indices, a diagonal camera block in full.
    unsigned long long *redq = reinterpret_cast<unsigned long long *>(d.red);
    for (int e = tid; e < kMfRows * kMfRows; e += 256) {
        const int row = e / kMfRows, col = e - row * kMfRows;
        if (col > row) continue;
        const int si = row / 6, a = row - 6 * si, sj = col / 6, b2 = col - 6 * sj;
        if (si >= kSchurMfCams) continue;
        const double v = G[row * (kMfRows + 1) + col];
        if (v == 0.0) continue;
        const int ci = true_cam(si), cj = true_cam(sj);
        if (ci >= nrc || cj >= nrc) continue;
        const int ri = 6 * ci + a, rj = 6 * cj + b2;
        const unsigned long long qv = fx64(-v, kFxBits - s_qe[row] - s_qe[col]);
        if (ci > cj) atomicAdd(&redq[(size_t)ri * n + rj], qv);
        else if (ci < cj) atomicAdd(&redq[(size_t)rj * n + ri], qv);
        else { atomicAdd(&redq[(size_t)ri * n + rj], qv); if (a != b2) atomicAdd(&redq[(size_t)rj * n + ri], qv); }
    }
    for (int e = tid; e < 6 * kSchurMfCams; e += 256) {
        const unsigned long long v = srhs[e];
        if (v == 0ull) continue;
        const int c = true_cam(e / 6);
        if (c < nrc) atomicAdd(&redq[(size_t)n * n + 6 * c + e % 6], v);
    }
}

// Free intrinsics: the block row of the reduced system that belongs to fx, cx, fy, cy (block index n_real_cam).
// One thread per point p.  With G_i the intrinsics columns of observation i (2 x 4, two non-zeros per row),
//   Wk_p = sum_i G_i'E_i (4x3), Yk = Wk_p M^-1:
//   S[k][k]   -= Yk Wk_p'            rhs[k] -= Wk_p M^-1 E'r
//   S[k][c_j] -= Yk W_j'  + G_j'F_j  for every observation j of p  (the second term is the F'F cross block)
// The camera-indexed part goes through an LDS copy of the block row (4 x 6 n_real_cam) when it fits, the 14 sums
// every point shares through a workgroup reduction; both are then added into d.red.  Runs after ba_schur.
__global__ __launch_bounds__(256) void ba_schur_calib_kernel(BADev d, int use_lds, int rhs_exp)
{
    extern __shared__ __attribute__((aligned(16))) double sl[];   // [8] reduction scratch, then use_lds: [4 * 6 n_real_cam]
    double *red = sl;
    double *rowblk = sl + 8;
    const int tid = threadIdx.x;
    const int nr = d.n_real_cam, n = 6 * d.n_cam, kap = 6 * nr, roww = 6 * nr;
    if (use_lds) {
        for (int e = tid; e < 4 * roww; e += 256) rowblk[e] = 0.0;
        __syncthreads();
    }
    double acc[14];
#pragma unroll
    for (int q = 0; q < 14; ++q) acc[q] = 0.0;
    const int p = blockIdx.x * 256 + tid;
    if (p < d.n_pt) {
        const int b = d.pt_start[p], e = d.pt_start[p + 1];
        if (e > b) {
            const size_t no = d.n_obs;
            double Wk[4][3];
#pragma unroll
            for (int a = 0; a < 4; ++a) Wk[a][0] = Wk[a][1] = Wk[a][2] = 0.0;
            for (int k = b; k < e; ++k) {
                const double k0 = d.Jk[k], k1 = d.Jk[no + k], k2 = d.Jk[2 * no + k], k3 = d.Jk[3 * no + k];
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const double e0 = d.Jp[m * no + k], e1 = d.Jp[(3 + m) * no + k];
                    Wk[0][m] += k0 * e0; Wk[1][m] += k1 * e0; Wk[2][m] += k2 * e1; Wk[3][m] += k3 * e1;
                }
            }
            const double *Mi = d.Minv + 6 * (size_t)p;
            const double M[9] = {Mi[0], Mi[1], Mi[2], Mi[1], Mi[3], Mi[4], Mi[2], Mi[4], Mi[5]};
            const double ag[3] = {d.Aig[3 * (size_t)p], d.Aig[3 * (size_t)p + 1], d.Aig[3 * (size_t)p + 2]};
            double Yk[4][3];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
#pragma unroll
                for (int m = 0; m < 3; ++m) Yk[a][m] = Wk[a][0] * M[m] + Wk[a][1] * M[3 + m] + Wk[a][2] * M[6 + m];
                acc[10 + a] = -(Wk[a][0] * ag[0] + Wk[a][1] * ag[1] + Wk[a][2] * ag[2]);
            }
            {
                int q = 0;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b2 = 0; b2 <= a; ++b2) acc[q++] = -(Yk[a][0] * Wk[b2][0] + Yk[a][1] * Wk[b2][1] + Yk[a][2] * Wk[b2][2]);
            }
            for (int k = b; k < e; ++k) {
                const int c = d.obs_cam[k];
                const double kk[4] = {d.Jk[k], d.Jk[no + k], d.Jk[2 * no + k], d.Jk[3 * no + k]};
                double Ej[6];
#pragma unroll
                for (int m = 0; m < 6; ++m) Ej[m] = d.Jp[m * no + k];
#pragma unroll
                for (int c2 = 0; c2 < 6; ++c2) {
                    const double f0 = d.Jc[c2 * no + k], f1 = d.Jc[(6 + c2) * no + k];
                    const double w0 = f0 * Ej[0] + f1 * Ej[3], w1 = f0 * Ej[1] + f1 * Ej[4], w2 = f0 * Ej[2] + f1 * Ej[5];
                    const int ej = d.qexp[6 * c + c2];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const double v = (a < 2 ? kk[a] * f0 : kk[a] * f1) - (Yk[a][0] * w0 + Yk[a][1] * w1 + Yk[a][2] * w2);
                        fx_add(use_lds ? &rowblk[a * roww + 6 * c + c2] : &d.red[(size_t)(kap + a) * n + 6 * c + c2], v, kFxBits - d.qexp[kap + a] - ej);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 14; ++q) {
        const double t = block_sum(acc[q], red);   // the workgroup's sum (fixed tree), rounded to the entry's grid, then exact adds
        if (tid != 0 || t == 0.0) continue;
        if (q >= 10) { fx_add(&d.red[(size_t)n * n + kap + (q - 10)], t, kFxBits - d.qexp[kap + (q - 10)] - rhs_exp); continue; }
        int a = 0, rem = q;
        while (rem > a) { rem -= a + 1; ++a; }
        fx_add(&d.red[(size_t)(kap + a) * n + kap + rem], t, kFxBits - d.qexp[kap + a] - d.qexp[kap + rem]);
    }
    if (use_lds) {
        __syncthreads();
        for (int e = tid; e < 4 * roww; e += 256) {
            const unsigned long long v = reinterpret_cast<const unsigned long long *>(rowblk)[e];
            if (v != 0ull) atomicAdd(reinterpret_cast<unsigned long long *>(&d.red[(size_t)(kap + e / roww) * n + (e % roww)]), v);
        }
    }
}

// Several free intrinsics blocks (has_calib = G > 1): block g rides as camera-side block n_real_cam + g and takes the observations of
// the cameras with cam_group[c] == g.  One thread per point p; for every group g that occurs in the track (found at its first
// observation), with Wk_g = sum_{i in p, group(i) = g} G_i'E_i (4 x 3) and Yk_g = Wk_g M^-1:
//   rhs[g]     -= Wk_g M^-1 E'r
//   S[g][c_j]  -= Yk_g W_j'  for every observation j of p,  += G_j'F_j  where group(c_j) == g
//   S[g][g2]   -= Yk_g Wk_g2'  for every group g2 <= g of the track (g2 == g: the lower triangle, as the one block's kernel writes it)
// Every addend is rounded to its entry's fixed-point grid and added as an integer -- through an LDS copy of all 4 G block rows while
// that fits (ba_calib_groups_in_lds), else into d.red directly -- so the sums do not depend on the order of arrival.  A track of T
// observations over L groups walks its rows L (L + 1) T / 2 + 2 L T times: the tracks are short.  Runs after ba_schur.
// RADIAL (also with one group): the blocks are fx, cx, fy, cy, k1, k2; Wk_g is 6 x 3 and formed from both residual rows, G_j'F_j uses
// both rows, the cross blocks are 6 x 6 and the LDS copy holds 6 G rows (calib_groups_lds_bytes).
template <bool RADIAL = false>
__global__ __launch_bounds__(256) void ba_schur_groups_kernel(BADev d, int use_lds, int rhs_exp)
{
    constexpr int NK = RADIAL ? 6 : 4;       // unknowns of a block that have columns
    extern __shared__ __attribute__((aligned(16))) unsigned long long rowq[];   // use_lds: [NK G][6 n_cam]
    const int tid = threadIdx.x;
    const int nr = d.n_real_cam, G = d.has_calib, n = 6 * d.n_cam;
    unsigned long long *redq = reinterpret_cast<unsigned long long *>(d.red);
    if (use_lds) {
        for (int e = tid; e < NK * G * n; e += 256) rowq[e] = 0ull;
        __syncthreads();
    }
    auto add = [&](int g, int a, int col, double v, int sh) {
        const unsigned long long q = fx64(v, sh);
        if (q == 0ull) return;
        if (use_lds) atomicAdd(&rowq[(size_t)(NK * g + a) * n + col], q);
        else atomicAdd(&redq[(size_t)(6 * (nr + g) + a) * n + col], q);
    };
    const size_t no = d.n_obs;
    // Wk of group g over the track [b, e)
    auto group_W = [&](int b, int e, int g, double (&Wk)[NK][3]) {
#pragma unroll
        for (int a = 0; a < NK; ++a) Wk[a][0] = Wk[a][1] = Wk[a][2] = 0.0;
        for (int k = b; k < e; ++k) {
            if (d.cam_group[d.obs_cam[k]] != g) continue;
            if constexpr (RADIAL) {
                double K[8], g0[6], g1[6];
#pragma unroll
                for (int q = 0; q < 8; ++q) K[q] = d.Jk[q * no + k];
                radial_rows(K, g0, g1);
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const double e0 = d.Jp[m * no + k], e1 = d.Jp[(3 + m) * no + k];
#pragma unroll
                    for (int a = 0; a < 6; ++a) Wk[a][m] += g0[a] * e0 + g1[a] * e1;
                }
                continue;
            }
            const double k0 = d.Jk[k], k1 = d.Jk[no + k], k2 = d.Jk[2 * no + k], k3 = d.Jk[3 * no + k];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const double e0 = d.Jp[m * no + k], e1 = d.Jp[(3 + m) * no + k];
                Wk[0][m] += k0 * e0; Wk[1][m] += k1 * e0; Wk[2][m] += k2 * e1; Wk[3][m] += k3 * e1;
            }
        }
    };
    auto first_of_group = [&](int b, int k, int g) {
        for (int j = b; j < k; ++j) if (d.cam_group[d.obs_cam[j]] == g) return false;
        return true;
    };
    const int p = blockIdx.x * 256 + tid;
    const int b = p < d.n_pt ? d.pt_start[p] : 0, e = p < d.n_pt ? d.pt_start[p + 1] : 0;
    if (e > b) {
        const double *Mi = d.Minv + 6 * (size_t)p;
        const double M[9] = {Mi[0], Mi[1], Mi[2], Mi[1], Mi[3], Mi[4], Mi[2], Mi[4], Mi[5]};
        const double ag[3] = {d.Aig[3 * (size_t)p], d.Aig[3 * (size_t)p + 1], d.Aig[3 * (size_t)p + 2]};
        for (int kl = b; kl < e; ++kl) {
            const int g = d.cam_group[d.obs_cam[kl]];
            if (!first_of_group(b, kl, g)) continue;
            const int kap = 6 * (nr + g);
            double Wk[NK][3], Yk[NK][3];
            group_W(kl, e, g, Wk);
            int qe[NK];
#pragma unroll
            for (int a = 0; a < NK; ++a) {
                qe[a] = d.qexp[kap + a];
#pragma unroll
                for (int m = 0; m < 3; ++m) Yk[a][m] = Wk[a][0] * M[m] + Wk[a][1] * M[3 + m] + Wk[a][2] * M[6 + m];
                const double v = -(Wk[a][0] * ag[0] + Wk[a][1] * ag[1] + Wk[a][2] * ag[2]);
                if (v != 0.0) fx_add(&d.red[(size_t)n * n + kap + a], v, kFxBits - qe[a] - rhs_exp);
            }
            // the camera columns of block row g
            for (int k = b; k < e; ++k) {
                const int c = d.obs_cam[k];
                const bool same = d.cam_group[c] == g;
                double kk[4] = {0.0, 0.0, 0.0, 0.0};
                double g0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g1[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // RADIAL: G_j in both residual rows
                if constexpr (RADIAL) {
                    if (same) {
                        double K[8];
#pragma unroll
                        for (int q = 0; q < 8; ++q) K[q] = d.Jk[q * no + k];
                        radial_rows(K, g0, g1);
                    }
                } else if (same) {
                    kk[0] = d.Jk[k]; kk[1] = d.Jk[no + k]; kk[2] = d.Jk[2 * no + k]; kk[3] = d.Jk[3 * no + k];
                }
                double Ej[6];
#pragma unroll
                for (int m = 0; m < 6; ++m) Ej[m] = d.Jp[m * no + k];
#pragma unroll
                for (int c2 = 0; c2 < 6; ++c2) {
                    const double f0 = d.Jc[c2 * no + k], f1 = d.Jc[(6 + c2) * no + k];
                    const double w0 = f0 * Ej[0] + f1 * Ej[3], w1 = f0 * Ej[1] + f1 * Ej[4], w2 = f0 * Ej[2] + f1 * Ej[5];
                    const int ej = d.qexp[6 * c + c2];
#pragma unroll
                    for (int a = 0; a < NK; ++a) {
                        double gf;
                        if constexpr (RADIAL) gf = g0[a] * f0 + g1[a] * f1;
                        else gf = a < 2 ? kk[a] * f0 : kk[a] * f1;
                        const double v = gf - (Yk[a][0] * w0 + Yk[a][1] * w1 + Yk[a][2] * w2);
                        add(g, a, 6 * c + c2, v, kFxBits - qe[a] - ej);
                    }
                }
            }
            // the group-by-group blocks of block row g: the groups g2 <= g of the track
            for (int k2 = b; k2 < e; ++k2) {
                const int g2 = d.cam_group[d.obs_cam[k2]];
                if (g2 > g || !first_of_group(b, k2, g2)) continue;
                double W2[NK][3];
                if (g2 == g) {
#pragma unroll
                    for (int a = 0; a < NK; ++a) { W2[a][0] = Wk[a][0]; W2[a][1] = Wk[a][1]; W2[a][2] = Wk[a][2]; }
                } else {
                    group_W(k2, e, g2, W2);
                }
                const int kap2 = 6 * (nr + g2);
#pragma unroll
                for (int a = 0; a < NK; ++a)
#pragma unroll
                    for (int b2 = 0; b2 < NK; ++b2) {
                        if (g2 == g && b2 > a) continue;
                        const double v = -(Yk[a][0] * W2[b2][0] + Yk[a][1] * W2[b2][1] + Yk[a][2] * W2[b2][2]);
                        add(g, a, kap2 + b2, v, kFxBits - qe[a] - d.qexp[kap2 + b2]);
                    }
            }
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int e2 = tid; e2 < NK * G * n; e2 += 256) {
            const unsigned long long v = rowq[e2];
            const int row = e2 / n, col = e2 % n;
            if (v != 0ull) atomicAdd(&redq[(size_t)(6 * (nr + row / NK) + row % NK) * n + col], v);
        }
    }
}

// Sum the per-workgroup slabs (fixed-point integers: exact in any order) and scatter into red = S_schur (n x n) | rhs_corr (n);
// TO_DOUBLE: converted to f64 on the way (no free intrinsics), else left in fixed point for ba_schur_calib_kernel to add to.
template <bool TO_DOUBLE>
__global__ __launch_bounds__(256) void ba_schur_reduce_kernel(BADev d, const double *__restrict__ slabs_f, int slab_doubles, int n_slabs, int rhs_exp)
{
    __shared__ unsigned long long lds[256];
    const unsigned long long *slabs = reinterpret_cast<const unsigned long long *>(slabs_f);
    const int e = blockIdx.x * kRedEnt + (threadIdx.x % kRedEnt);
    const int grp = threadIdx.x / kRedEnt;
    unsigned long long v0 = 0;
    if (e < slab_doubles) {
        for (int b = grp; b < n_slabs; b += 8 * kRedGrp) {      // eight loads in flight per round
            unsigned long long t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = (b + u * kRedGrp < n_slabs) ? slabs[(size_t)(b + u * kRedGrp) * slab_doubles + e] : 0ull;
#pragma unroll
            for (int u = 0; u < 8; ++u) v0 += t[u];
        }
    }
    lds[threadIdx.x] = v0;
    __syncthreads();
    if (threadIdx.x >= kRedEnt || e >= slab_doubles) return;
    unsigned long long t = 0;
    for (int g = 0; g < kRedGrp; ++g) t += lds[g * kRedEnt + threadIdx.x];
    const int n = 6 * d.n_cam;
    const int nblk = d.n_cam * (d.n_cam + 1) / 2;
    size_t dst; int sh;
    if (e >= nblk * 36) {
        const int r = e - nblk * 36;
        dst = (size_t)n * n + r; sh = kFxBits - d.qexp[r] - rhs_exp;
    } else {
        const int blk = e / 36, r = e % 36;
        int ci = (int)((sqrt(8.0 * (double)blk + 1.0) - 1.0) * 0.5);
        while ((ci + 1) * (ci + 2) / 2 <= blk) ++ci;
        while (ci * (ci + 1) / 2 > blk) --ci;
        const int cj = blk - ci * (ci + 1) / 2;
        const int row = 6 * ci + r / 6, col = 6 * cj + r % 6;
        dst = (size_t)row * n + col; sh = kFxBits - d.qexp[row] - d.qexp[col];
    }
    if (TO_DOUBLE) d.red[dst] = fx64_to_double(t, sh);
    else reinterpret_cast<unsigned long long *>(d.red)[dst] = t;
}

// red: fixed point -> f64 in place, block-lower triangle and right-hand side (everything else is zero in both encodings).
__global__ __launch_bounds__(256) void ba_schur_to_double_kernel(BADev d, int rhs_exp)
{
    const int n = 6 * d.n_cam;
    const int row = blockIdx.y;
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (row == n) {
        if (col < n) d.red[(size_t)n * n + col] = fx64_to_double(reinterpret_cast<const unsigned long long *>(d.red)[(size_t)n * n + col], kFxBits - d.qexp[col] - rhs_exp);
        return;
    }
    if (col >= 6 * (row / 6 + 1)) return;
    const size_t at = (size_t)row * n + col;
    const unsigned long long q = reinterpret_cast<const unsigned long long *>(d.red)[at];
    if (q != 0ull) d.red[at] = fx64_to_double(q, kFxBits - d.qexp[row] - d.qexp[col]);
}

// Multi-GPU exchange buffer of the reduced system ("packed-upper S + rhs"): only the blocks the Schur kernels
// write (row camera >= column camera) travel, row by row -- row i of block row bi holds 6 (bi + 1) doubles at
// 36 bi (bi + 1) / 2 + (i % 6) 6 (bi + 1) -- followed by the n right-hand-side entries: 36 Nc (Nc + 1) / 2 + 6 Nc doubles
// instead of (6 Nc)^2 + 6 Nc.  One workgroup per row (coalesced both ways), the last one moves the right-hand side.
__global__ __launch_bounds__(256) void ba_red_pack_kernel(BADev d, double *__restrict__ packed, int unpack)
{
    const int n = 6 * d.n_cam;
    const int i = blockIdx.x;
    const double *src; double *dst; int cnt;
    if (i < n) {
        const int bi = i / 6, r = i - 6 * bi;
        cnt = 6 * (bi + 1);
        double *full = d.red + (size_t)i * n;
        double *pk = packed + (size_t)18 * bi * (bi + 1) + (size_t)r * cnt;
        src = unpack ? pk : full; dst = unpack ? full : pk;
    } else {
        cnt = n;
        double *full = d.red + (size_t)n * n;
        double *pk = packed + (size_t)18 * d.n_cam * (d.n_cam + 1);
        src = unpack ? pk : full; dst = unpack ? full : pk;
    }
    for (int k = threadIdx.x; k < cnt; k += 256) dst[k] = src[k];
}

// ---------------------------------------------------------------------------------------------
int ba_red_pack(hipStream_t st, const BADev &d, double *packed, bool unpack)
{
    if (d.n_cam <= 0) return ESFM_OK;
    hipLaunchKernelGGL(ba_red_pack_kernel, dim3(6 * d.n_cam + 1), dim3(256), 0, st, d, packed, unpack ? 1 : 0);
    LAUNCH_CHECK();
    return ESFM_OK;
}

// e with |x| < 2^e (the exponent the right-hand side's fixed point is scaled by)
static int bound_exponent(double x)
{
    if (!(x > 1e-120)) return -400;
    if (!(x < 1e120)) return 400;
    return std::ilogb(x) + 1;
}

static int schur_to_double(hipStream_t st, const BADev &d, int rhs_exp)
{
    const int n = 6 * d.n_cam;
    hipLaunchKernelGGL(ba_schur_to_double_kernel, dim3(div_up(n, 256), n + 1), dim3(256), 0, st, d, rhs_exp);
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_schur(hipStream_t st, const BADev &d, int num_cu, double rhs_bound)
{
    const BaForms &forms = d.parts->forms;
    // (the slab path writes every entry of red anything reads -- lower blocks and right-hand side -- in its reduce kernel; the other
    // paths and the free-intrinsics kernel accumulate into it)
    const bool slab_path = forms.schur == BaForms::SCHUR_LDS_SLABS && d.n_obs > 0 && !d.has_calib;
    d.parts->red_fixed = false;
    if (!slab_path && !d.parts->red_clean) ESFM_HIP_TRY(hipMemsetAsync(d.red, 0, sizeof(double) * ba_red_doubles(d.n_cam), st));
    if (d.n_obs <= 0) return ESFM_OK;
    d.parts->red_clean = false;
    const int rhs_exp = bound_exponent(rhs_bound);
    const bool finish = !d.has_calib;    // with free intrinsics ba_schur_calib adds its block row first, then converts
    if (forms.schur == BaForms::SCHUR_LDS_SLABS) {
        const int slab_doubles = (int)ba_schur_slab_doubles(d.n_cam);
        const size_t lds_bytes = schur_lds_bytes(d.n_cam);
        constexpr int schur_threads = 1024;     // (512: 39 us, 256: 52 us against 35 us on BA-25 -- every workgroup zeroes and writes out a 96 KB slab)
        const int n_slabs = std::max(1, std::min(num_cu, div_up(d.n_obs, schur_threads)));
        double *slabs = d.slabs;
        if ((size_t)n_slabs * slab_doubles > d.slab_cap) { set_error("BA Schur: %d slabs do not fit the slab buffer", n_slabs); return ESFM_ERR_INVALID_ARG; }
        ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&ba_schur_lds_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        hipLaunchKernelGGL(ba_schur_lds_kernel, dim3(n_slabs), dim3(schur_threads), lds_bytes, st, d, slabs, slab_doubles, rhs_exp);
        LAUNCH_CHECK();
        if (finish) hipLaunchKernelGGL(ba_schur_reduce_kernel<true>, dim3(div_up(slab_doubles, kRedEnt)), dim3(256), 0, st, d, slabs, slab_doubles, n_slabs, rhs_exp);
        else hipLaunchKernelGGL(ba_schur_reduce_kernel<false>, dim3(div_up(slab_doubles, kRedEnt)), dim3(256), 0, st, d, slabs, slab_doubles, n_slabs, rhs_exp);
        LAUNCH_CHECK();
        return ESFM_OK;
    }
    // SCHUR_TABLES: every observation is in exactly one of the tables (make_ba_layout)
    // narrow tracks (nearly all of them in a sequence capture): the matrix-core kernel, plain and rotated camera numbering
    if (d.n_mchunks[0] + d.n_mchunks[1] > 0) {
        SchurMfTables tabs;
        for (int tb = 0; tb < 2; ++tb) {
            tabs.slot_obs[tb] = d.mslot_obs[tb]; tabs.slot_pc[tb] = reinterpret_cast<const int2 *>(d.mslot_pc[tb]); tabs.batch_slot[tb] = d.mbatch_slot[tb];
            tabs.chunk_batch0[tb] = d.mchunk_batch0[tb]; tabs.chunk_cam0[tb] = d.mchunk_cam0[tb];
        }
        tabs.n_plain = d.n_mchunks[0]; tabs.rot_seam = d.n_real_cam / 2;
        ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&ba_schur_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMfLdsBytes));
        hipLaunchKernelGGL(ba_schur_mfma_kernel, dim3(d.n_mchunks[0] + d.n_mchunks[1]), dim3(256), kMfLdsBytes, st, d, rhs_exp, tabs);
        LAUNCH_CHECK();
    }
    constexpr size_t win_bytes = sizeof(double) * (kWinBlocks * kSchurPitch + 6 * kWinCams);
    if (d.n_chunks > 0 || d.n_chunks_b > 0)
        ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&ba_schur_window_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)win_bytes));
    if (d.n_chunks > 0) {
        hipLaunchKernelGGL(ba_schur_window_kernel, dim3(d.n_chunks), dim3(1024), win_bytes, st, d, rhs_exp, d.slot_obs, d.chunk_slot, d.chunk_cam0, 0);
        LAUNCH_CHECK();
    }
    if (d.n_chunks_b > 0) {        // the tracks that are narrow once the camera indices are rotated by half the loop
        hipLaunchKernelGGL(ba_schur_window_kernel, dim3(d.n_chunks_b), dim3(1024), win_bytes, st, d, rhs_exp, d.slot_obs_b, d.chunk_slot_b, d.chunk_cam0_b,
                           d.n_real_cam / 2);
        LAUNCH_CHECK();
    }
    // tracks wider than the window in both index spaces go through the plain kernel, spread over the chip (inside the window
    // kernel they would all land in the chunks of the lowest cameras and the whole launch would wait for those workgroups)
    if (d.n_wide_obs > 0) {
        hipLaunchKernelGGL(ba_schur_kernel, dim3(div_up(d.n_wide_obs, 256)), dim3(256), 0, st, d, rhs_exp, d.wide_obs, d.n_wide_obs);
        LAUNCH_CHECK();
    }
    if (finish && forms.solve == BaForms::SOLVE_TILED && (d.parts->single_rank || d.sparse)) {
        // the tiled solve's assembly kernel reads red next: it converts on the way and clears what it has read (the structure-aware
        // solve of several ranks: its pack kernel does)
        d.parts->red_fixed = true; d.parts->red_rhs_exp = rhs_exp;
        return ESFM_OK;
    }
    return finish ? schur_to_double(st, d, rhs_exp) : ESFM_OK;
}

int ba_schur_calib(hipStream_t st, const BADev &d, double rhs_bound)
{
    if (!d.has_calib || d.n_pt <= 0 || d.n_obs <= 0) return ESFM_OK;
    if (ba_grouped(d)) {
        const bool rows_in_lds = ba_calib_groups_in_lds(d.n_real_cam, d.has_calib, d.radial != 0);
        const size_t bytes = rows_in_lds ? calib_groups_lds_bytes(d.n_real_cam, d.has_calib, d.radial != 0) : 0;
        const int exp = bound_exponent(rhs_bound);
        if (d.radial) hipLaunchKernelGGL(ba_schur_groups_kernel<true>, dim3(div_up(d.n_pt, 256)), dim3(256), bytes, st, d, rows_in_lds ? 1 : 0, exp);
        else hipLaunchKernelGGL(ba_schur_groups_kernel<false>, dim3(div_up(d.n_pt, 256)), dim3(256), bytes, st, d, rows_in_lds ? 1 : 0, exp);
        LAUNCH_CHECK();
        return schur_to_double(st, d, exp);
    }
    const bool use_lds = ba_calib_row_in_lds(d.n_real_cam);
    const size_t lds = use_lds ? calib_row_lds_bytes(d.n_real_cam) : calib_row_lds_bytes(0);
    const int rhs_exp = bound_exponent(rhs_bound);
    hipLaunchKernelGGL(ba_schur_calib_kernel, dim3(div_up(d.n_pt, 256)), dim3(256), lds, st, d, use_lds ? 1 : 0, rhs_exp);
    LAUNCH_CHECK();
    return schur_to_double(st, d, rhs_exp);
}

}  // namespace esfm
