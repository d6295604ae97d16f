// Device helpers that more than one stage of the bundle adjustment uses; included only by ba_linearize.hip, ba_schur.hip and
// ba_step.hip.  Reductions and the per-workgroup partial-sum protocol of the scalar sums (scal_commit / scal_reserve), the 64-bit
// fixed-point helpers, the Cauchy loss (CauchyLoss(0.5), reference cpp_code/src/ba.cpp:150), and the projection and Jacobian of
// ReprojectErrorTerm_fixcalib / _updatecalib (cpp_code/include/ba.h:108-222).  All arithmetic is f64, like Ceres; observations and
// intrinsics are f32 inputs, like the reference (ba.h:162-163).
#pragma once

#include <float.h>

#include "ba_kernels.hpp"

namespace esfm {

static inline int div_up(long long a, long long b) { return (int)((a + b - 1) / b); }
#define LAUNCH_CHECK() ESFM_HIP_TRY(hipGetLastError())

__device__ __forceinline__ double block_sum(double v, double *lds /*>= 4 doubles*/)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += lds[w];
    return s;
}

// value of lane `l` (wave-uniform index) as a scalar: two v_readlane_b32 instead of the LDS round trip of __shfl
__device__ __forceinline__ double readlane_f64(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void atomic_max_nonneg(double *addr, double v)
{
    // non-negative doubles order like their bit patterns.  A look first (L2-coherent; a value that is behind is only smaller): nearly every
    // caller loses, and thousands of read-modify-writes of ONE address queue up in one L2 channel -- ba_point_prep_chunk_kernel on BA-512,
    // 47 k waves: 151 us with the bare atomic, 54 us without its tail (round 3)
    unsigned long long *a = reinterpret_cast<unsigned long long *>(addr);
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    if (__hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= bits) return;
    atomicMax(a, bits);
}

// ba_schur_reduce_kernel sums entry e over the per-workgroup slabs with a 32 x 8 thread tile: thread (ent, grp) adds slabs grp,
// grp + 8, ... (independent loads, coalesced across ent), then the 8 partial sums are combined through LDS.
constexpr int kRedEnt = 32, kRedGrp = 8;

// Scalar sums across workgroups without f64 atomics (whose order of arrival differs from run to run): every workgroup leaves its
// block sums in d.scal_part[slot][base + blockIdx.x]; the next read-back (ba_publish_scalars / ba_scal_reduce, one workgroup) adds
// the pending partials of each slot in a fixed order -- one wave per slot, lane l takes entries l, l + 64, ..., then the shuffle tree --
// and adds the total to d.scal[slot].  The result is a function of the launch geometry only.  The host keeps the number of
// pending partials per slot (BADev::parts); `base` is where this launch's go.  vals are per-THREAD partials.
// (A first version let the last workgroup to take a ticket do the sum inside the producing kernel: the fence + ticket + tail cost
// ~10 us per kernel on the 25-camera problem, a tenth of the LM iteration.)
template <int N>
__device__ __forceinline__ void scal_commit(const BADev &d, const ScalBase &base, const int (&slots)[N], const double (&vals)[N], double *lds /* >= 8 */,
                                            int bidx = -1 /* the workgroup's index among those that commit; default blockIdx.x */)
{
    const int b = bidx < 0 ? (int)blockIdx.x : bidx;
    if (N == 1) {
        const double t = block_sum(vals[0], lds);
        if (threadIdx.x == 0) d.scal_part[(size_t)slots[0] * d.scal_cap + base.b[0] + b] = t;
        return;
    }
    // all N sums behind ONE pair of barriers (block_sum's shuffle tree and wave order per sum, hence its bits; N calls of it were 2 N
    // barriers at the end of every workgroup: twelve in the back-substitution)
    __shared__ double part[N][16];
    double t[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        t[q] = vals[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t[q] += __shfl_xor(t[q], o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) part[q][wave] = t[q];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int q = threadIdx.x;
        double sum = 0.0;
        for (int w = 0; w < nw; ++w) sum += part[q][w];
        d.scal_part[(size_t)slots[q] * d.scal_cap + base.b[q] + b] = sum;
    }
}

// scal_commit with the per-wave partials staged in the CALLER's LDS (`stage`, N * WAVES doubles; a workgroup of at most WAVES waves)
// instead of a static array: for a kernel whose dynamic LDS is sized to the last byte a workgroup may take (the Jacobian sweep:
// lin_lds_bytes, ba_forms.hpp), where 128 N static bytes beside it make the launch illegal.  The same shuffle tree and wave order, hence
// the same bits.
template <int N, int WAVES>
__device__ __forceinline__ void scal_commit_staged(const BADev &d, const ScalBase &base, const int (&slots)[N], const double (&vals)[N], double *stage)
{
    double t[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        t[q] = vals[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t[q] += __shfl_xor(t[q], o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) stage[q * WAVES + wave] = t[q];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int q = threadIdx.x;
        double sum = 0.0;
        for (int w = 0; w < nw; ++w) sum += stage[q * WAVES + w];
        d.scal_part[(size_t)slots[q] * d.scal_cap + base.b[q] + blockIdx.x] = sum;
    }
}

// 1024 threads: wave w adds the pending partials of slot w (SC_SUM_COUNT <= 16) -- lane l takes entries l, l + 64, ... in order,
// 32 loads in flight, then the fixed shuffle tree -- so all slots cost one memory round trip together.
__device__ __forceinline__ void scal_reduce_pending(const double *scal_part, int scal_cap, double *scal, const ScalCounts &c)
{
    const int slot = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (slot >= SC_SUM_COUNT) return;
    const int n = c.n[slot];
    if (n == 0) return;
    const double *part = scal_part + (size_t)slot * scal_cap;
    double v = 0.0;
    // (32 loads in flight; the adds keep the order they have always had -- entries lane, lane + 64, ... -- so the sum's bits do not
    // depend on the depth: with 8 in flight BA-512's 12 k partials per slot were 23 dependent round trips, 17 us per read-back)
    for (int b = lane; b < n; b += 32 * 64) {
        double t[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) t[u] = (b + 64 * u < n) ? part[b + 64 * u] : 0.0;
#pragma unroll
        for (int u = 0; u < 32; ++u) v += t[u];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) scal[slot] += v;
}

// host side: where the partials of a launch of `grid` workgroups go, for each of its slots
template <int N>
static int scal_reserve(hipStream_t st, const BADev &d, const int (&slots)[N], int grid, ScalBase &base)
{
    if (grid > d.scal_cap) { set_error("BA: %d workgroups exceed the scalar partial capacity %d", grid, d.scal_cap); return ESFM_ERR_INVALID_ARG; }
    bool full = false;
    for (int q = 0; q < N; ++q) full = full || d.parts->n[slots[q]] + grid > d.scal_cap;
    if (full) { if (int rc = ba_scal_reduce(st, d)) return rc; }
    for (int q = 0; q < N; ++q) { base.b[q] = d.parts->n[slots[q]]; d.parts->n[slots[q]] += grid; }
    return ESFM_OK;
}

// Exact accumulation of the Schur complement in 64-bit fixed point (BADev::qexp): fx64(v, sh) = round(v 2^sh) as an integer.
// fx64_scaled: round-to-nearest-even of an already scaled x, |x| < 2^62, to int64 WITHOUT the compiler's f64 -> i64 lowering (which,
// with the ldexp, came to ~110 VALU instructions per entry: the Schur kernel was VALU bound on it).  Two magic-number additions:
// A = x + 1.5 2^84 rounds x to a multiple of 2^32, whose quotient sits in A's low mantissa dword; xl = x - (A - 1.5 2^84) is exact,
// |xl| <= 2^31, and B = xl + 1.5 2^52 holds round(xl) as a 64-bit two's complement offset of bits(1.5 2^52).  5 f64 + 1 int op.
__device__ __forceinline__ unsigned long long fx64_scaled(double x)
{
    const double M1 = 0x1.8p84, M2 = 0x1.8p52;
    const double A = __dadd_rn(x, M1);
    const double xl = __dsub_rn(x, __dsub_rn(A, M1));
    const double B = __dadd_rn(xl, M2);
    const unsigned int hi = (unsigned int)__double2loint(A) + ((unsigned int)__double2hiint(B) - 0x43380000u);
    return ((unsigned long long)hi << 32) | (unsigned int)__double2loint(B);
}
__device__ __forceinline__ unsigned long long fx64(double v, int sh) { return fx64_scaled(ldexp(v, sh)); }
__device__ __forceinline__ void fx_add(double *slot, double v, int sh) { atomicAdd(reinterpret_cast<unsigned long long *>(slot), fx64(v, sh)); }
__device__ __forceinline__ void fx_add_scaled(double *slot, double x) { atomicAdd(reinterpret_cast<unsigned long long *>(slot), fx64_scaled(x)); }

// ceres::CauchyLoss::Evaluate [upstream]; a <= 0 selects the trivial (squared) loss.
__device__ __forceinline__ void loss_eval(double a, double s, double &rho0, double &rho1)
{
    if (a <= 0.0) { rho0 = s; rho1 = 1.0; return; }
    const double b = a * a, c = 1.0 / b;
    const double sum = 1.0 + s * c, inv = 1.0 / sum;
    rho0 = b * log(sum);
    rho1 = inv > DBL_MIN ? inv : DBL_MIN;
}

// Rotate-and-translate of ReprojectErrorTerm_fixcalib (ba.h:131-135): p = AngleAxisRotatePoint(a, X) + t,
// with ceres' two branches [upstream rotation.h].  Optionally the derivatives dp/dX (R) and dp/da (Ja):
// with alpha = sin/theta, beta = (1-cos)/theta^2,
//   p = cos X + alpha a x X + beta a (a.X)
//   dp/da_k = -alpha a_k X + gamma a_k (a x X) + alpha (e_k x X) + delta a_k (a.X) a + beta (e_k (a.X) + a X_k)
//   gamma = (cos - alpha)/theta^2, delta = (alpha - 2 beta)/theta^2.
template <bool DERIV>
__device__ __forceinline__ void transform_point(const double *__restrict__ cam, const double *__restrict__ X, double p[3],
                                                double R[9], double Ja[9])
{
    const double a0 = cam[0], a1 = cam[1], a2 = cam[2];
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    const double theta2 = a0 * a0 + a1 * a1 + a2 * a2;
    const double c0 = a1 * X2 - a2 * X1, c1 = a2 * X0 - a0 * X2, c2 = a0 * X1 - a1 * X0;  // a x X
    if (theta2 > DBL_EPSILON) {
        const double theta = sqrt(theta2);
        double s, c;
        sincos(theta, &s, &c);
        const double ti = 1.0 / theta;
        const double w0 = a0 * ti, w1 = a1 * ti, w2 = a2 * ti;
        const double tmp = (w0 * X0 + w1 * X1 + w2 * X2) * (1.0 - c);
        p[0] = X0 * c + (w1 * X2 - w2 * X1) * s + w0 * tmp;
        p[1] = X1 * c + (w2 * X0 - w0 * X2) * s + w1 * tmp;
        p[2] = X2 * c + (w0 * X1 - w1 * X0) * s + w2 * tmp;
        if (DERIV) {
            const double ti2 = ti * ti;
            const double alpha = s * ti, beta = (1.0 - c) * ti2, gamma = (c - alpha) * ti2, delta = (alpha - 2.0 * beta) * ti2;
            const double aX = a0 * X0 + a1 * X1 + a2 * X2;
            R[0] = c + beta * a0 * a0;       R[1] = -alpha * a2 + beta * a0 * a1; R[2] = alpha * a1 + beta * a0 * a2;
            R[3] = alpha * a2 + beta * a1 * a0; R[4] = c + beta * a1 * a1;       R[5] = -alpha * a0 + beta * a1 * a2;
            R[6] = -alpha * a1 + beta * a2 * a0; R[7] = alpha * a0 + beta * a2 * a1; R[8] = c + beta * a2 * a2;
            const double av[3] = {a0, a1, a2}, Xv[3] = {X0, X1, X2}, cv[3] = {c0, c1, c2};
            // e_k x X, k = 0,1,2 (columns)
            const double ex[3][3] = {{0.0, -X2, X1}, {X2, 0.0, -X0}, {-X1, X0, 0.0}};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double ak = av[k];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    double v = -alpha * ak * Xv[i] + gamma * ak * cv[i] + alpha * ex[k][i] + delta * ak * aX * av[i] + beta * av[i] * Xv[k];
                    if (i == k) v += beta * aX;
                    Ja[3 * i + k] = v;
                }
            }
        }
    } else {
        p[0] = X0 + c0; p[1] = X1 + c1; p[2] = X2 + c2;
        if (DERIV) {
            R[0] = 1.0; R[1] = -a2; R[2] = a1; R[3] = a2; R[4] = 1.0; R[5] = -a0; R[6] = -a1; R[7] = a0; R[8] = 1.0;
            Ja[0] = 0.0; Ja[1] = X2;  Ja[2] = -X1;
            Ja[3] = -X2; Ja[4] = 0.0; Ja[5] = X0;
            Ja[6] = X1;  Ja[7] = -X0; Ja[8] = 0.0;
        }
    }
    p[0] += cam[3]; p[1] += cam[4]; p[2] += cam[5];
}

// fx, cx, fy, cy of camera c: the camera's float calibration (ba.h:142-143), or the shared free block, which is
// stored behind the real cameras of the camera-side parameter vector `cams` (ba.h:199-202).  GROUPS (several free blocks, one per
// camera group): the block of the camera's group, n_real_cam + cam_group[c].
template <bool GROUPS = false>
__device__ __forceinline__ int calib_block_of(const BADev &d, int c) { return GROUPS ? d.n_real_cam + d.cam_group[c] : d.n_real_cam; }

template <bool GROUPS = false>
__device__ __forceinline__ void load_intrinsics(const BADev &d, const double *__restrict__ cams, int c, double in4[4])
{
    if (d.has_calib) {
        const double *kp = cams + 6 * (size_t)calib_block_of<GROUPS>(d, c);
        in4[0] = kp[0]; in4[1] = kp[1]; in4[2] = kp[2]; in4[3] = kp[3];
    } else {
        const float4 K = d.K4[c];
        in4[0] = (double)K.x; in4[1] = (double)K.y; in4[2] = (double)K.z; in4[3] = (double)K.w;
    }
}

// Residual and analytic Jacobian of the reprojection functor (ba.h:113-153 / 170-216) at (cam, X):
// r = uv - (x fx + cx, y fy + cy), x = p0/p2, y = p1/p2, p = R(a) X + t.  Jc[2][6], Jp[2][3]; xn, yn = x, y.
__device__ __forceinline__ void reproject_jac(const double cam[6], const double X[3], const double in4[4], float2 uv,
                                              double &r0, double &r1, double Jc[12], double Jp[6], double &xn, double &yn)
{
    double pt[3], R[9], Ja[9];
    transform_point<true>(cam, X, pt, R, Ja);
    const double iz = 1.0 / pt[2];
    const double x = pt[0] * iz, y = pt[1] * iz;
    const double fx = in4[0], cx = in4[1], fy = in4[2], cy = in4[3];
    r0 = (double)uv.x - (x * fx + cx);
    r1 = (double)uv.y - (y * fy + cy);
    // d r / d p  (rows)
    const double g0[3] = {-fx * iz, 0.0, fx * x * iz};
    const double g1[3] = {0.0, -fy * iz, fy * y * iz};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Jc[j] = g0[0] * Ja[j] + g0[1] * Ja[3 + j] + g0[2] * Ja[6 + j];
        Jc[6 + j] = g1[0] * Ja[j] + g1[1] * Ja[3 + j] + g1[2] * Ja[6 + j];
        Jc[3 + j] = g0[j];
        Jc[9 + j] = g1[j];
        Jp[j] = g0[0] * R[j] + g0[1] * R[3 + j] + g0[2] * R[6 + j];
        Jp[3 + j] = g1[0] * R[j] + g1[1] * R[3 + j] + g1[2] * R[6 + j];
    }
    xn = x; yn = y;
}

// Radial problems (BADev::radial; always the grouped path): the block of the camera's group is fx, cx, fy, cy, k1, k2.
__device__ __forceinline__ void load_intrinsics_radial(const BADev &d, const double *__restrict__ cams, int c, double in6[6])
{
    const double *kp = cams + 6 * (size_t)calib_block_of<true>(d, c);
#pragma unroll
    for (int i = 0; i < 6; ++i) in6[i] = kp[i];
}

// Residual of the radial model (OpenCV's with p1 = p2 = 0, the one esfm_undistort inverts) at the camera-frame point pt:
// x = p0/p2, y = p1/p2, r2 = x^2 + y^2, L = 1 + k1 r2 + k2 r2^2,  r = uv - (fx x L + cx, fy y L + cy).
__device__ __forceinline__ void reproject_radial(const double pt[3], const double in6[6], float2 uv, double &r0, double &r1)
{
    const double x = pt[0] / pt[2], y = pt[1] / pt[2];
    const double r2 = x * x + y * y;
    const double L = 1.0 + in6[4] * r2 + in6[5] * r2 * r2;
    r0 = (double)uv.x - (x * L * in6[0] + in6[1]);
    r1 = (double)uv.y - (y * L * in6[2] + in6[3]);
}

// reproject_jac for the radial model.  With D = 2 k1 + 4 k2 r2:  d(xL)/dx = L + x^2 D, d(xL)/dy = d(yL)/dx = x y D, d(yL)/dy = L + y^2 D,
// chained in front of d(x, y)/dp.  Jk[8]: d r0 / d(fx, cx), d r1 / d(fy, cy) -- the four the pinhole block stores -- then
// d r0 / d(k1, k2), d r1 / d(k1, k2).
__device__ __forceinline__ void reproject_jac_radial(const double cam[6], const double X[3], const double in6[6], float2 uv,
                                                     double &r0, double &r1, double Jc[12], double Jp[6], double Jk[8])
{
    double pt[3], R[9], Ja[9];
    transform_point<true>(cam, X, pt, R, Ja);
    const double iz = 1.0 / pt[2];
    const double x = pt[0] * iz, y = pt[1] * iz;
    const double fx = in6[0], cx = in6[1], fy = in6[2], cy = in6[3], k1 = in6[4], k2 = in6[5];
    const double r2 = x * x + y * y, r4 = r2 * r2;
    const double L = 1.0 + k1 * r2 + k2 * r4, D = 2.0 * k1 + 4.0 * k2 * r2;
    const double xl = x * L, yl = y * L;
    r0 = (double)uv.x - (xl * fx + cx);
    r1 = (double)uv.y - (yl * fy + cy);
    const double a00 = L + x * x * D, a01 = x * y * D, a11 = L + y * y * D;
    // d r / d p  (rows)
    const double g0[3] = {-fx * iz * a00, -fx * iz * a01, fx * (a00 * x + a01 * y) * iz};
    const double g1[3] = {-fy * iz * a01, -fy * iz * a11, fy * (a01 * x + a11 * y) * iz};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Jc[j] = g0[0] * Ja[j] + g0[1] * Ja[3 + j] + g0[2] * Ja[6 + j];
        Jc[6 + j] = g1[0] * Ja[j] + g1[1] * Ja[3 + j] + g1[2] * Ja[6 + j];
        Jc[3 + j] = g0[j];
        Jc[9 + j] = g1[j];
        Jp[j] = g0[0] * R[j] + g0[1] * R[3 + j] + g0[2] * R[6 + j];
        Jp[3 + j] = g1[0] * R[j] + g1[1] * R[3 + j] + g1[2] * R[6 + j];
    }
    Jk[0] = -xl; Jk[1] = -1.0; Jk[2] = -yl; Jk[3] = -1.0;
    Jk[4] = -fx * x * r2; Jk[5] = -fx * x * r4; Jk[6] = -fy * y * r2; Jk[7] = -fy * y * r4;
}

// The radial block's columns in the two residual rows, from the 8 stored scalars: row 0 (K0, K1, 0, 0, K4, K5), row 1 (0, 0, K2, K3, K6, K7).
__device__ __forceinline__ void radial_rows(const double K[8], double g0[6], double g1[6])
{
    g0[0] = K[0]; g0[1] = K[1]; g0[2] = 0.0; g0[3] = 0.0; g0[4] = K[4]; g0[5] = K[5];
    g1[0] = 0.0; g1[1] = 0.0; g1[2] = K[2]; g1[3] = K[3]; g1[4] = K[6]; g1[5] = K[7];
}

// W_i = F_i'E_i (6 x 3, row-major) of observation i, re-formed from its 18 Jacobian entries.  (Round 2 had the sweep store W -- 144 B
// per observation -- and the Schur kernels load it: as many loads here, 36 multiply-adds less.  Measured in round 3: without the
// store the sweep of BA-512 takes 262 us instead of 369, the Schur kernels 927 against 928 us; BA-25 29.2 against 30.7 and 41.5
// against 40.6 us.  The array is gone: 432 MB less written per sweep at BA-512, 912 MB -> 480 MB of linearisation resident.)
__device__ __forceinline__ void load_W(const BADev &d, size_t n_obs, int i, double W[18])
{
    double Jc[12], Jp[6];
#pragma unroll
    for (int q = 0; q < 12; ++q) Jc[q] = d.Jc[q * n_obs + i];
#pragma unroll
    for (int q = 0; q < 6; ++q) Jp[q] = d.Jp[q * n_obs + i];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int m = 0; m < 3; ++m) W[3 * a + m] = Jc[a] * Jp[m] + Jc[6 + a] * Jp[3 + m];
}

// e with sqrt(diag(F'F)_i) < 2^e (BADev::qexp)
__device__ __forceinline__ int qexp_of(double diag)
{
    const double sd = sqrt(fabs(diag));
    return (sd > 1e-120 && sd < 1e120) ? ilogb(sd) + 1 : -400;   // a zero column only ever contributes zeros
}

}  // namespace esfm
