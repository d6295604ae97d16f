// Bundle adjustment, linearisation stage: the part of the replacement for BundleAdjustment::solveBA's ceres::Solve (reference
// cpp_code/src/ba.cpp:132-212) that evaluates the cost functor ReprojectErrorTerm_fixcalib (cpp_code/include/ba.h:108-164) and forms
// the blocks of the normal equations.  Kernels and their launchers:
//
//   ba_linearize_kernel         residual + analytic Jacobian + Cauchy corrector per observation (the "Jacobian sweep": streams 16 B
//                               in, 160 B out per observation), plus the per-camera F'F / F'r sums in LDS
//   ba_camacc_*_kernel          the per-camera sums: slab reduction (reduce), or camera chunks (chunk, final)
//   ba_point_prep*_kernel       per point: E'E, E'r, (E'E + D^2)^-1
//   ba_jacobi_scaling_kernel, ba_camera_gradient_kernel
//
// The LM control flow (accept/reject, radius) lives in ba_solve.cpp.  DESIGN.md "Bundle adjustment".
#include "ba_device.hpp"

namespace esfm {

// Jacobian sweep: 16 B in, 160 B out per observation (+ 32 B with free intrinsics), and the per-camera sums F'F / F'r.
//
// PRIV (the 27 sums of every camera fit in LDS): each workgroup accumulates its observations' contributions in LDS as 64-bit
// FIXED-POINT integers -- integer adds are associative, so the order in which waves reach the LDS does not matter (round 1 used
// ds_add_f64 here and was not reproducible) -- and stores its private copy as one coalesced slab of doubles;
// ba_camacc_reduce_kernel adds the slabs in a fixed order.  The fixed-point scale is per workgroup, per camera and per column:
// pass 1 streams the Jacobian out and leaves  m[c][a] = max_k (J_k[a]^2 + J_k[6+a]^2)  (and max |r_k|^2) and the number of
// observations n_c of each camera in LDS (u64 max of non-negative doubles and integer adds: order-independent);
// then  sum_k f_a f_b <= sqrt(n_c m[c][a]) sqrt(n_c m[c][b]) < 2^(ex[c][a] + ex[c][b])  bounds every partial sum and pass 2 re-reads
// the workgroup's own Jacobian rows (L2) and adds round(v 2^(60 - ex[c][a] - ex[c][b])).
// !PRIV: the sweep only; ba_camacc_chunk_kernel then forms the sums by gathering each camera's observations in order.
// (Round 3, BA-25, one observation per thread: the kernel takes 29 - 31 us whether it writes 160 or 304 B per observation, re-reads
// its rows in pass 2 or keeps them in registers, shares one set of LDS sums per workgroup or keeps one per wave -- every variant
// measured.  It is one dependent chain per workgroup: index load -> parameter gather -> sincos / divide in f64 -> stores -> LDS
// maxima -> barrier -> exponents -> barrier -> 27 LDS adds -> barrier -> slab.  43 MB in 30 us is 0.18 of the HBM roofline and
// not what limits it.)
// threads per workgroup of the sweep: 512 from 2^20 observations on, 256 below (BA-25, 240 k observations, two per thread: 28.7 -> 22.8
// us -- finer workgroups get out of each other's phase and finish unevenly loaded CUs sooner; 128: 36 us, the slab count doubles;
// 1024: 33 us.  BA-512: 223 us with 512, 313 with 256)
// Round 5, BA-512 (two waves per SIMD -- 250 registers; the LDS sums of 512 cameras leave room for one workgroup per CU anyway): the
// loop's loads are issued one observation AHEAD of its stores (see the loop): 228 -> 187 us; ONE workgroup per CU instead of two in
// sequence (each paid a 9-us prologue -- LDS clear, exponents -- and an 8-us epilogue): -> 161 - 167 us.  What the loop waits for is
// neither memory nor issue slots but ITSELF (stage stamps, profiles/r05_ba512_sweep_and_schur_decomposition.txt: 5.6 us per iteration and wave = 13 400 cycles
// for 2 x 1 266 instructions): timing-only builds without the 20 stores AND the 35 LDS atomics take 177 us against 186; a build that
// takes sin / cos / 1/theta from a per-camera table -- 1 080 instructions instead of 1 266, bit-identical results -- takes exactly as
// long (5.58 against 5.60 us per iteration: measured, not kept); allowing fused multiply-adds removes 8 % of the instructions.  The
// f64 dependency chains of one observation (division -> Jacobian -> scaling -> products -> fixed point) at two waves per SIMD are the
// critical path; more waves would need the kernel in 128 registers.  A pure copy of the same 18 + 18 arrays runs at 5.9 TB/s in ANY
// layout (SoA of doubles as here, double2, tiles of 64: profiles/r05_soa_stream_ubench.txt), so the layout is not what holds the sweep back.
constexpr int kLinThreadsLarge = 512, kLinThreadsSmall = 256;

// GROUPS (several free intrinsics blocks, has_calib = G > 1; always !PRIV): the intrinsics and their column scales are those of the
// observation's camera's group, gathered with the camera's parameters; the per-group sums come from the camera chunks.
// RADIAL (a GROUPS sweep): the group's block is fx, cx, fy, cy, k1, k2 (reproject_jac_radial) and the block's columns mix the two
// residual rows, so 8 scalars per observation are stored, not 4.
template <bool PRIV, bool CALIB, int kLinThreads, bool GROUPS = false, bool RADIAL = false>
__global__ __launch_bounds__(kLinThreads, 1) void ba_linearize_kernel(BADev d, double cauchy_a, int use_scaling, ScalBase sbase, double *__restrict__ slabs,
                                                                   int prov_rexp)
{
    // prov_rexp != INT_MIN (PRIV, several observations per thread: BA-512): PROVISIONAL fixed-point exponents -- the previous
    // linearisation's global column exponents d.qexp plus one, and prov_rexp for the residual column (sqrt(2 cost) < 2^prov_rexp,
    // from the host: the accepted candidate's cost) -- let pass 1 quantise and add the rows while they are in registers.  The maxima
    // and counts are still collected, and after the loop every workgroup checks ITS bound sqrt(n_c max) < 2^exponent for every camera
    // and column: if one fails (a first linearisation, a problem that changed under the solver) the workgroup clears its sums and
    // runs the two-pass form below.  Either way the integers are exact sums on the grid the slab is converted with.  (Round 3: the
    // re-read of pass 2 was 336 MB of BA-512's sweep.)
    static_assert(!GROUPS || (CALIB && !PRIV), "the grouped sweep is a free-intrinsics sweep without LDS sums");
    static_assert(!RADIAL || GROUPS, "the radial sweep is a grouped sweep");
    constexpr int NKD = RADIAL ? 6 : 4, NJK = RADIAL ? 8 : 4;      // unknowns of the intrinsics block; scalars stored per observation
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double *red = reinterpret_cast<double *>(lds_raw);                                  // [8] reduction scratch, [10] intrinsics-block sums
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(lds_raw) + 18;     // PRIV: [n_real_cam * 27]
    unsigned long long *mx = acc + (size_t)d.n_real_cam * 27;                           //       [n_real_cam * 7]
    int *cnt = reinterpret_cast<int *>(mx + (size_t)d.n_real_cam * 7);                  //       [n_real_cam]
    int *ex = cnt + d.n_real_cam;                                                       //       [n_real_cam * 7]
    const int tid = threadIdx.x;
    const int n_obs = d.n_obs;
    const bool single_launch = PRIV && (long long)gridDim.x * kLinThreads >= n_obs;
    const bool prov = PRIV && !single_launch && prov_rexp != INT_MIN;
    if (PRIV) {
        for (int e = tid; e < d.n_real_cam * 27; e += kLinThreads) acc[e] = 0ull;
        for (int e = tid; e < d.n_real_cam * 7; e += kLinThreads) {
            mx[e] = 0ull;
            if (prov) ex[e] = e % 7 == 6 ? prov_rexp : d.qexp[6 * (e / 7) + e % 7] + 1;
        }
        for (int e = tid; e < d.n_real_cam; e += kLinThreads) cnt[e] = 0;
        if (tid == 0) red[17] = 0.0;         // the guard's verdict (red[8..17] otherwise belong to the intrinsics block, which has no provisional path)
        __syncthreads();
    }
    // the 27 fixed-point adds of one observation's rows (every factor carries 2^(30 - exponent of its column))
    auto add_rows = [&](int c, const double (&Jrow)[12], double r0, double r1) {
        double J[12];
#pragma unroll
        for (int a = 0; a < 6; ++a) { const int sh = kFxBits / 2 - ex[c * 7 + a]; J[a] = ldexp(Jrow[a], sh); J[6 + a] = ldexp(Jrow[6 + a], sh); }
        const int shr = kFxBits / 2 - ex[c * 7 + 6];
        const double q0 = ldexp(r0, shr), q1 = ldexp(r1, shr);
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) {
                atomicAdd(&acc[c * 27 + e], fx64_scaled(J[a] * J[b] + J[6 + a] * J[6 + b]));
                ++e;
            }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) atomicAdd(&acc[c * 27 + 21 + a], fx64_scaled(J[a] * q0 + J[6 + a] * q1));
    };
    double cost = 0.0, bad = 0.0;
    double kacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // PRIV, at most one observation per thread (the grid covers the observations: BA-25): pass 2 quantises the rows from REGISTERS
    // instead of re-reading the thread's own stores (112 B per observation fetched back: 33 MB of the 108 MB the kernel moved)
    const bool single = single_launch;
    double keepJ[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, keepR0 = 0.0, keepR1 = 0.0;
    int keepC = -1;
    // The loop is software-pipelined by hand.  A wave's loads and stores retire through ONE counter (vmcnt) in issue order: with
    // the next observation's index loads and parameter gathers issued AFTER this observation's 20 stores, "wait for the loads" meant
    // "wait until the stores have drained" -- two dependent round trips behind a write burst per iteration, 15 us of a 20-us iteration
    // idle at the two waves per SIMD the LDS sums leave room for.  Now the indices of observation k + 2 strides and the parameters of
    // k + stride are requested in front of the ARITHMETIC of k: they are ahead of its stores in the queue, their latency runs beside
    // 1 200 instructions, and the wait in front of the next iteration leaves the stores in flight.
    // (Unconditional loads at clamped indices: a load under `if (k + stride < n_obs)` merges with the old value, and the merge is a
    // register copy that has to wait for the load -- in front of the stores.  The camera's float calibration is converted where it
    // is used, for the same reason.)
    struct LinIdx { int c, p; float2 uv; };
    struct LinPar { float4 K; double kd[NKD], cam[6], X[3], sc[6], sp[3], ksc[NKD]; };
    auto load_idx = [&](int k, LinIdx &o) { o.c = d.obs_cam[k]; o.p = d.obs_pt[k]; o.uv = d.obs_uv[k]; };
    auto load_par = [&](const LinIdx &ix, LinPar &o) {
        if (CALIB) {         // (== d.has_calib: the free block rides behind the real cameras, load_intrinsics)
            const size_t kb = 6 * (size_t)calib_block_of<GROUPS>(d, ix.c);
            const double *kp = d.x_c + kb;
            o.kd[0] = kp[0]; o.kd[1] = kp[1]; o.kd[2] = kp[2]; o.kd[3] = kp[3];
            if (RADIAL) { o.kd[NKD - 2] = kp[4]; o.kd[NKD - 1] = kp[5]; }
            if (GROUPS) {
#pragma unroll
                for (int i = 0; i < NKD; ++i) o.ksc[i] = use_scaling ? d.scale_c[kb + i] : 1.0;
            }
        } else {
            o.K = d.K4[ix.c];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) o.cam[i] = d.x_c[6 * (size_t)ix.c + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) o.X[i] = d.x_p[3 * (size_t)ix.p + i];
        if (use_scaling) {
#pragma unroll
            for (int i = 0; i < 6; ++i) o.sc[i] = d.scale_c[6 * (size_t)ix.c + i];
#pragma unroll
            for (int i = 0; i < 3; ++i) o.sp[i] = d.scale_p[3 * (size_t)ix.p + i];
        }
    };
    double kscale[4] = {1.0, 1.0, 1.0, 1.0};      // the free intrinsics' column scales: the same for every observation, read once
    if (CALIB && !GROUPS && use_scaling) {
#pragma unroll
        for (int i = 0; i < 4; ++i) kscale[i] = d.scale_c[6 * (size_t)d.n_real_cam + i];
    }
    const int kstride = gridDim.x * kLinThreads;
    const int k_first = blockIdx.x * kLinThreads + tid;
    auto clamped = [&](long long k) { return (int)(k < n_obs ? k : n_obs - 1); };
    LinIdx ix_cur = {0, 0, make_float2(0.f, 0.f)}, ix_nxt = ix_cur;
    LinPar par_cur = {};
    if (n_obs > 0) {
        load_idx(clamped(k_first), ix_cur); load_par(ix_cur, par_cur);
        load_idx(clamped((long long)k_first + kstride), ix_nxt);
        // (vmcnt(0) here, once: the compiler's wait-count bookkeeping merges the loop's two entries, and with these loads pending on
        // the way in it would wait for "all but two" memory operations in EVERY iteration -- the stores again)
        __builtin_amdgcn_s_waitcnt(0x0f70);
    }
    for (int k = k_first; k < n_obs; k += kstride) {
        // the next observation's parameters and the indices of the one after: requested in front of this observation's arithmetic
        // (and so ahead of its stores in the queue)
        // (with free intrinsics the kernel has no registers left for that: there the requests go out after the arithmetic, in front
        // of the stores)
        LinPar par_nxt;
        LinIdx ix_nn;
        if (!CALIB) {
            load_par(ix_nxt, par_nxt);
            load_idx(clamped((long long)k + 2 * (long long)kstride), ix_nn);
            __builtin_amdgcn_sched_barrier(0);
        }
        const int c = ix_cur.c;
        const float2 uv = ix_cur.uv;
        double in4[4];
        if (CALIB) { in4[0] = par_cur.kd[0]; in4[1] = par_cur.kd[1]; in4[2] = par_cur.kd[2]; in4[3] = par_cur.kd[3]; }
        else { in4[0] = (double)par_cur.K.x; in4[1] = (double)par_cur.K.y; in4[2] = (double)par_cur.K.z; in4[3] = (double)par_cur.K.w; }
        double r0, r1, Jc[12], Jp[6], xn, yn;
        double Jk[NJK];
        if constexpr (RADIAL) {
            reproject_jac_radial(par_cur.cam, par_cur.X, par_cur.kd, uv, r0, r1, Jc, Jp, Jk);
            xn = Jk[0]; yn = Jk[2];          // (for the finite check: the rest of Jk is products of these, the intrinsics and r2)
#pragma unroll
            for (int i = 4; i < NJK; ++i) { if (!isfinite(Jk[i])) xn = Jk[i]; }
        } else {
            reproject_jac(par_cur.cam, par_cur.X, in4, uv, r0, r1, Jc, Jp, xn, yn);
            // intrinsics columns (ba.h:199-206): u = x fx + cx, v = y fy + cy
            Jk[0] = -xn; Jk[1] = -1.0; Jk[2] = -yn; Jk[3] = -1.0;
        }
        const double s = r0 * r0 + r1 * r1;
        bool fin = isfinite(s);
#pragma unroll
        for (int i = 0; i < 12; ++i) fin = fin && isfinite(Jc[i]);
#pragma unroll
        for (int i = 0; i < 6; ++i) fin = fin && isfinite(Jp[i]);
        fin = fin && isfinite(xn) && isfinite(yn);
        if (!fin) {
            bad += 1.0; r0 = r1 = 0.0;
#pragma unroll
            for (int i = 0; i < 12; ++i) Jc[i] = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) Jp[i] = 0.0;
#pragma unroll
            for (int i = 0; i < NJK; ++i) Jk[i] = 0.0;
        } else {
            double rho0, rho1;
            loss_eval(cauchy_a, s, rho0, rho1);
            cost += 0.5 * rho0;
            const double sq = sqrt(rho1);  // corrector, rho'' <= 0 branch [upstream corrector.cc]
            r0 *= sq; r1 *= sq;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double sc = use_scaling ? sq * par_cur.sc[i] : sq;
                Jc[i] *= sc; Jc[6 + i] *= sc;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double sp = use_scaling ? sq * par_cur.sp[i] : sq;
                Jp[i] *= sp; Jp[3 + i] *= sp;
            }
            if (CALIB) {
#pragma unroll
                for (int i = 0; i < 4; ++i) Jk[i] *= sq * (GROUPS ? par_cur.ksc[i] : kscale[i]);
                if constexpr (RADIAL) {
#pragma unroll
                    for (int i = 4; i < NJK; ++i) Jk[i] *= sq * par_cur.ksc[4 + (i & 1)];      // columns k1, k2 of row 0, then of row 1
                }
            }
        }
        if (CALIB) {
#pragma unroll
            for (int i = 0; i < NJK; ++i) d.Jk[(size_t)i * n_obs + k] = Jk[i];
            if (PRIV) {
                // G'G (upper triangle of the 4x4: rows fx, cx | fy, cy never mix) and G'r, kept in registers over the sweep
                kacc[0] += Jk[0] * Jk[0]; kacc[1] += Jk[0] * Jk[1]; kacc[2] += Jk[1] * Jk[1];
                kacc[3] += Jk[2] * Jk[2]; kacc[4] += Jk[2] * Jk[3]; kacc[5] += Jk[3] * Jk[3];
                kacc[6] += Jk[0] * r0; kacc[7] += Jk[1] * r0; kacc[8] += Jk[2] * r1; kacc[9] += Jk[3] * r1;
            }
        }
        if (CALIB) {
            load_par(ix_nxt, par_nxt);
            load_idx(clamped((long long)k + 2 * (long long)kstride), ix_nn);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) d.Jc[(size_t)i * n_obs + k] = Jc[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) d.Jp[(size_t)i * n_obs + k] = Jp[i];
        d.res[k] = r0; d.res[(size_t)n_obs + k] = r1;
        if (PRIV) {
            atomicAdd(&cnt[c], 1);
#pragma unroll
            for (int a = 0; a < 6; ++a) atomicMax(&mx[c * 7 + a], (unsigned long long)__double_as_longlong(Jc[a] * Jc[a] + Jc[6 + a] * Jc[6 + a]));
            atomicMax(&mx[c * 7 + 6], (unsigned long long)__double_as_longlong(r0 * r0 + r1 * r1));
            if (single) {
#pragma unroll
                for (int i = 0; i < 12; ++i) keepJ[i] = Jc[i];
                keepR0 = r0; keepR1 = r1; keepC = c;
            }
            if (prov && !CALIB) add_rows(c, Jc, r0, r1);
        }
        ix_cur = ix_nxt; ix_nxt = ix_nn; par_cur = par_nxt;
    }
    {
        const int slots[2] = {SC_COST, SC_LIN_BAD};
        const double vals[2] = {cost, bad};
        // staged in red[0 .. 2 waves): no static LDS beside lin_lds_bytes, which takes a compute unit's LDS to within 144 bytes at 538
        // cameras (red[8 .. 16] are written further down, red[17] is the guard's verdict)
        static_assert(2 * (kLinThreads / 64) <= 17, "the sweep's 18 doubles of scratch hold the staged partials in front of the verdict");
        scal_commit_staged<2, kLinThreads / 64>(d, sbase, slots, vals, red);
    }
    if (!PRIV) return;
    if (CALIB) {
#pragma unroll
        for (int q = 0; q < 10; ++q) {
            const double v = block_sum(kacc[q], red);     // a fixed tree
            if (tid == 0) red[8 + q] = v;
        }
    }
    __syncthreads();
    bool two_pass = !(prov && !CALIB);
    if (!two_pass) {
        // the guard: this workgroup's bound on every partial sum against the provisional grid
        bool viol = false;
        for (int e = tid; e < d.n_real_cam * 7; e += kLinThreads) {
            if (cnt[e / 7] == 0) continue;
            const double b = sqrt((double)cnt[e / 7] * __longlong_as_double((long long)mx[e]));
            const int need = (b > 1e-120 && b < 1e120) ? ilogb(b) + 1 : (b >= 1e120 || b != b ? INT_MAX : -400);
            viol = viol || need > ex[e];
        }
        if (viol) red[17] = 1.0;
        __syncthreads();
        two_pass = red[17] != 0.0;            // (workgroup-uniform)
        if (two_pass) {
            for (int e = tid; e < d.n_real_cam * 27; e += kLinThreads) acc[e] = 0ull;
        }
        __syncthreads();
    }
    if (two_pass) {
        for (int e = tid; e < d.n_real_cam * 7; e += kLinThreads) {
            const double b = sqrt((double)cnt[e / 7] * __longlong_as_double((long long)mx[e]));   // > sqrt(sum): every term is <= the maximum
            ex[e] = (b > 1e-120 && b < 1e120) ? ilogb(b) + 1 : -400;
        }
        __syncthreads();
    }
    for (int k = blockIdx.x * kLinThreads + tid; two_pass && k < n_obs; k += gridDim.x * kLinThreads) {
        int c;
        double J[12], r0, r1;
        if (single) {
            c = keepC; r0 = keepR0; r1 = keepR1;
#pragma unroll
            for (int i = 0; i < 12; ++i) J[i] = keepJ[i];
        } else {
            c = d.obs_cam[k];
#pragma unroll
            for (int i = 0; i < 12; ++i) J[i] = d.Jc[(size_t)i * n_obs + k];    // this thread's own stores
            r0 = d.res[k]; r1 = d.res[(size_t)n_obs + k];
        }
        add_rows(c, J, r0, r1);
    }
    __syncthreads();
    // one coalesced slab of doubles per workgroup; ba_camacc_reduce_kernel sums them in a fixed order
    double *out = slabs + (size_t)blockIdx.x * d.n_cam * 27;
    for (int e = tid; e < d.n_real_cam * 27; e += kLinThreads) {
        const int c = e / 27, q = e % 27;
        int a = 0, b2 = 6;                      // q >= 21: column a = q - 21 against the residual
        if (q >= 21) a = q - 21;
        else { int rem = q; while (rem >= 6 - a) { rem -= 6 - a; ++a; } b2 = a + rem; }
        out[e] = fx64_to_double(acc[e], kFxBits - ex[c * 7 + a] - ex[c * 7 + b2]);
    }
    if (CALIB) {
        // the intrinsics block rides as camera-side block n_real_cam.  Packed index of (a, b), a <= b: a*6 - a(a-1)/2 + b - a.
        const int slot[10] = {0, 1, 6, 11, 12, 15, 21, 22, 23, 24};
        if (tid < 27) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 10; ++q) if (slot[q] == tid) v = red[8 + q];
            out[(size_t)d.n_real_cam * 27 + tid] = v;
        }
    }
}

// Camera part of max|gradient| (needs the all-reduced F'r): |F'r_i / scale_i|, or for bounded problems the norm of
// x - Plus(x, -gradient)  (trust_region_minimizer.cc, projected gradient step).
__device__ __forceinline__ double camera_gradient_entry(const BADev &d, int i, double ftr)
{
    double g = ftr / d.scale_c[i];
    if (d.constrained) {
        const double x = d.x_c[i];
        g = x - fmin(fmax(x - g, d.lo_c[i]), d.up_c[i]);
    }
    return fabs(g);
}

// Sum of entry e over n_slabs per-workgroup slabs, computed by a 32 x 8 thread tile: thread (ent, grp) adds slabs grp, grp + 8, ...
// (independent loads, coalesced across ent), then the 8 partial sums are combined in a fixed order through LDS.  Deterministic.
__device__ __forceinline__ void camacc_reduce_block(const BADev &d, const double *__restrict__ slabs, int n_slabs, int with_gradient, int bidx, double *lds /* 256 */)
{
    const int e = bidx * kRedEnt + (threadIdx.x % kRedEnt);
    const int per = d.n_cam * 27;
    const int grp = threadIdx.x / kRedEnt;
    // thread (ent, grp) adds slabs grp, grp + 8, ... in that order; 32 loads in flight per round (512 slabs: two round trips; the loop
    // used to wait for every load, ~1 us each, then for every eighth)
    double v0 = 0.0;
    if (e < per) {
        for (int b = grp; b < n_slabs; b += 32 * kRedGrp) {
            double t[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) t[u] = (b + u * kRedGrp < n_slabs) ? slabs[(size_t)(b + u * kRedGrp) * per + e] : 0.0;
#pragma unroll
            for (int u = 0; u < 32; ++u) v0 += t[u];
        }
    }
    lds[threadIdx.x] = v0;
    __syncthreads();
    if (threadIdx.x >= kRedEnt || e >= per) return;
    double v = 0.0;
    for (int g = 0; g < kRedGrp; ++g) v += lds[g * kRedEnt + threadIdx.x];
    const int c = e / 27, q = e % 27;
    if (q >= 21) {
        d.camacc[36 * (size_t)d.n_cam + 6 * (size_t)c + (q - 21)] = v;
        // one rank: this IS the gradient's camera part, max-reduced here instead of in a launch of its own
        if (with_gradient) { const double g = camera_gradient_entry(d, 6 * c + (q - 21), v); if (g > 0.0) atomic_max_nonneg(&d.scal[SC_GMAX], g); }
        return;
    }
    int a = 0, rem = q;
    while (rem >= 6 - a) { rem -= 6 - a; ++a; }
    const int b2 = a + rem;
    d.camacc[36 * (size_t)c + 6 * a + b2] = v;
    d.camacc[36 * (size_t)c + 6 * b2 + a] = v;
    if (a == b2) d.qexp[6 * c + a] = qexp_of(v);
}

__global__ __launch_bounds__(256) void ba_camacc_reduce_kernel(BADev d, const double *__restrict__ slabs, int n_slabs, int with_gradient)
{
    __shared__ double lds[256];
    camacc_reduce_block(d, slabs, n_slabs, with_gradient, blockIdx.x, lds);
}

// Per-camera sums from the stored Jacobian, chunk by chunk: ONE WAVE per chunk adds F'F (upper triangle, 21), F'r (6) -- and with
// free intrinsics the 10 sums of the shared block, G'G (6) and G'r (4) -- over the (up to kCamChunk = 256) observations
// cam_obs[beg, end) of ONE camera.  Lane l takes observations l, l + 64, l + 128, l + 192 in that order (all four index loads,
// then all Jacobian loads, are issued before the first use: the kernel is two memory round trips deep, not eight); the 37 sums
// then go through the wave shuffle tree.  A fixed association: bit-reproducible.
// RADIAL: the block of the camera's group is 6 wide and its columns mix the two residual rows: G'G is the full upper triangle (21)
// and G'r has 6 entries, from the 8 stored scalars; they go to cam_part_k (the ten sums of the pinhole block are not formed).
// (This instance compiles to exactly 256 VGPRs, the most a wave may have without AGPR copies, and no scratch
// (profiles/r14_ba_radial_kernel_resources.txt): four observations' 12 + 8 + 2 values and 27 + 27 sums in f64.  Check the scratch
// count after a compiler change; if it ever spills, form the 27 radial sums in a second pass over K, r0, r1 -- the order of the adds,
// hence the bits, stays.)
template <bool CALIB, bool RADIAL = false>
__global__ __launch_bounds__(64) void ba_camacc_chunk_kernel(BADev d)
{
    const int lane = threadIdx.x;
    const int beg = d.cchunk_beg[blockIdx.x], end = d.cchunk_end[blockIdx.x];
    const size_t n = d.n_obs;
    constexpr int U = kCamChunk / 64;
    int k[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const int idx = beg + lane + 64 * u; k[u] = idx < end ? d.cam_obs[idx] : -1; }
    constexpr int NJK = RADIAL ? 8 : 4;
    double J[U][12], r0[U], r1[U], K[U][NJK];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int kk = k[u] < 0 ? 0 : k[u];
#pragma unroll
        for (int a = 0; a < 12; ++a) J[u][a] = d.Jc[a * n + kk];
        r0[u] = d.res[kk]; r1[u] = d.res[n + kk];
        if (CALIB) {
#pragma unroll
            for (int a = 0; a < NJK; ++a) K[u][a] = d.Jk[a * n + kk];
        }
    }
    double acc[kCamPart];
#pragma unroll
    for (int q = 0; q < kCamPart; ++q) acc[q] = 0.0;
    double acck[RADIAL ? kRadialPart : 1];
    if constexpr (RADIAL) {
#pragma unroll
        for (int q = 0; q < kRadialPart; ++q) acck[q] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (k[u] < 0) continue;
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[e++] += J[u][a] * J[u][b] + J[u][6 + a] * J[u][6 + b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] += J[u][a] * r0[u] + J[u][6 + a] * r1[u];
        if constexpr (RADIAL) {
            double g0[6], g1[6];
            radial_rows(K[u], g0, g1);
            int e2 = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) acck[e2++] += g0[a] * g0[b] + g1[a] * g1[b];
#pragma unroll
            for (int a = 0; a < 6; ++a) acck[21 + a] += g0[a] * r0[u] + g1[a] * r1[u];
        } else if (CALIB) {
            const double k0 = K[u][0], k1 = K[u][1], k2 = K[u][2], k3 = K[u][3];
            acc[27] += k0 * k0; acc[28] += k0 * k1; acc[29] += k1 * k1; acc[30] += k2 * k2; acc[31] += k2 * k3; acc[32] += k3 * k3;
            acc[33] += k0 * r0[u]; acc[34] += k1 * r0[u]; acc[35] += k2 * r1[u]; acc[36] += k3 * r1[u];
        }
    }
    constexpr int NQ = RADIAL ? 27 : CALIB ? kCamPart : 27;
    double mine = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double v = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == q) mine = v;
    }
    if (lane < NQ) d.cam_part[(size_t)blockIdx.x * kCamPart + lane] = mine;
    if constexpr (RADIAL) {
        double minek = 0.0;
#pragma unroll
        for (int q = 0; q < kRadialPart; ++q) {
            double v = acck[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == q) minek = v;
        }
        if (lane < kRadialPart) d.cam_part_k[(size_t)blockIdx.x * kRadialPart + lane] = minek;
    }
}

// camacc = F'F (36 per camera, both triangles) | F'r (6 per camera): a camera's chunk sums added in chunk order; the
// intrinsics block (free calibration) adds ALL chunks in order.  Every entry of camacc is written (cameras without observations get
// zeros), and the diagonal entries also leave their fixed-point exponent in qexp.
__global__ __launch_bounds__(256) void ba_camacc_final_kernel(BADev d)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int nr = d.n_real_cam;
    if (e < nr * 27) {
        const int c = e / 27, q = e % 27;
        double v = 0.0;
        for (int b = d.cam_chunk0[c]; b < d.cam_chunk0[c + 1]; ++b) v += d.cam_part[(size_t)b * kCamPart + q];
        if (q >= 21) { d.camacc[36 * (size_t)d.n_cam + 6 * (size_t)c + (q - 21)] = v; return; }
        int a = 0, rem = q;
        while (rem >= 6 - a) { rem -= 6 - a; ++a; }
        const int b2 = a + rem;
        d.camacc[36 * (size_t)c + 6 * a + b2] = v;
        d.camacc[36 * (size_t)c + 6 * b2 + a] = v;
        if (a == b2) d.qexp[6 * c + a] = qexp_of(v);
        return;
    }
    const int q = e - nr * 27;
    if (d.has_calib != 1 || d.radial || q >= 42) return;     // (several blocks, or a radial one: ba_camacc_groups_kernel)
    // the shared intrinsics block rides as camera-side block nr: 6 x 6 with the 4 x 4 part G'G (fx, cx | fy, cy never mix), then G'r
    const int kc = nr;
    if (q < 36) {
        const int a = q / 6, b2 = q % 6;
        const int lo = a < b2 ? a : b2, hi = a < b2 ? b2 : a;
        int src = -1;
        if (lo == 0 && hi == 0) src = 27; else if (lo == 0 && hi == 1) src = 28; else if (lo == 1 && hi == 1) src = 29;
        else if (lo == 2 && hi == 2) src = 30; else if (lo == 2 && hi == 3) src = 31; else if (lo == 3 && hi == 3) src = 32;
        double v = 0.0;
        if (src >= 0) for (int b = 0; b < d.n_cchunks; ++b) v += d.cam_part[(size_t)b * kCamPart + src];
        d.camacc[36 * (size_t)kc + q] = v;
        if (a == b2) d.qexp[6 * kc + a] = qexp_of(v);
    } else {
        const int a = q - 36;
        double v = 0.0;
        if (a < 4) for (int b = 0; b < d.n_cchunks; ++b) v += d.cam_part[(size_t)b * kCamPart + 33 + a];
        d.camacc[36 * (size_t)d.n_cam + 6 * (size_t)kc + a] = v;
    }
}

// Several free intrinsics blocks: block g rides as camera-side block n_real_cam + g, and its sums G'G / G'r are the sums 27..36 of the
// chunks of ITS cameras (a chunk belongs to one camera, hence to one group).  One WAVE per entry of the block's 6 x 6 and of its
// right-hand side: lane l takes chunks l, l + 64, ... in that order -- a chunk of another group adds 0.0 -- then the wave shuffle
// tree: a fixed association whatever the launch timing.  (One thread per entry walking all chunks was a chain of three dependent
// loads per chunk: 2 ms per sweep at 938 chunks.)  A group without observations gets zeros.
// RADIAL: every entry of the 6 x 6 and of the right-hand side has a sum, among the chunk's 27 of cam_part_k.
template <bool RADIAL = false>
__global__ __launch_bounds__(64) void ba_camacc_groups_kernel(BADev d)
{
    const int g = blockIdx.x / 42, q = blockIdx.x % 42, lane = threadIdx.x;
    const int kc = d.n_real_cam + g;
    const double *part = RADIAL ? d.cam_part_k : d.cam_part;
    constexpr int kPart = RADIAL ? kRadialPart : kCamPart;
    int src = -1;
    if constexpr (RADIAL) {
        if (q < 36) {
            const int a = q / 6, b2 = q % 6;
            const int lo = a < b2 ? a : b2, hi = a < b2 ? b2 : a;
            src = lo * 6 - lo * (lo - 1) / 2 + hi - lo;      // packed index of (lo, hi) in the upper triangle
        } else src = 21 + (q - 36);
    } else if (q < 36) {
        const int a = q / 6, b2 = q % 6;
        const int lo = a < b2 ? a : b2, hi = a < b2 ? b2 : a;
        if (lo == 0 && hi == 0) src = 27; else if (lo == 0 && hi == 1) src = 28; else if (lo == 1 && hi == 1) src = 29;
        else if (lo == 2 && hi == 2) src = 30; else if (lo == 2 && hi == 3) src = 31; else if (lo == 3 && hi == 3) src = 32;
    } else if (q - 36 < 4) src = 33 + (q - 36);
    double v = 0.0;
    if (src >= 0) {
        constexpr int U = 4;
        for (int b0 = lane; b0 < d.n_cchunks; b0 += 64 * U) {
            double t[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int b = b0 + 64 * u;
                const bool mine = b < d.n_cchunks && d.cam_group[d.cchunk_cam[b < d.n_cchunks ? b : 0]] == g;
                t[u] = mine ? part[(size_t)b * kPart + src] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) v += t[u];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    }
    if (lane != 0) return;
    if (q < 36) {
        d.camacc[36 * (size_t)kc + q] = v;
        if (q / 6 == q % 6) d.qexp[6 * kc + q / 6] = qexp_of(v);
    } else {
        d.camacc[36 * (size_t)d.n_cam + 6 * (size_t)kc + (q - 36)] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// Per point: E'E, E'r (only when the Jacobian is fresh), then M^-1 = (E'E + clamp(diag)/radius)^-1
// via a 3x3 Cholesky (ceres InvertPSDMatrix), M^-1 E'r, and the point part of max|gradient|.
// M = E'E + D^2 of one point, its inverse (closed-form 3 x 3 Cholesky) and M^-1 E'r; returns 1.0 when M is not positive definite
__device__ __forceinline__ double point_block_invert(const BADev &d, int p, const double (&A)[6], const double (&g)[3], double radius, double min_diag,
                                                     double max_diag)
{
    double sing = 0.0;
    // M = E'E + D^2, D^2 = clamp(diag(E'E)) / radius  (levenberg_marquardt_strategy.cc)
    const double m00 = A[0] + fmin(fmax(A[0], min_diag), max_diag) / radius;
    const double m11 = A[3] + fmin(fmax(A[3], min_diag), max_diag) / radius;
    const double m22 = A[5] + fmin(fmax(A[5], min_diag), max_diag) / radius;
    const double m10 = A[1], m20 = A[2], m21 = A[4];
    double Mi[6] = {0, 0, 0, 0, 0, 0};
    bool ok = m00 > 0.0;
    const double l00 = sqrt(m00);
    const double l10 = m10 / l00, l20 = m20 / l00;
    const double t11 = m11 - l10 * l10;
    ok = ok && (t11 > 0.0);
    const double l11 = sqrt(t11);
    const double l21 = (m21 - l20 * l10) / l11;
    const double t22 = m22 - l20 * l20 - l21 * l21;
    ok = ok && (t22 > 0.0);
    const double l22 = sqrt(t22);
    if (ok) {
        const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
        const double i10 = -l10 * i00 * i11;
        const double i21 = -l21 * i11 * i22;
        const double i20 = -(l20 * i00 + l21 * i10) * i22;
        Mi[0] = i00 * i00 + i10 * i10 + i20 * i20;  // xx
        Mi[1] = i10 * i11 + i20 * i21;              // xy
        Mi[2] = i20 * i22;                          // xz
        Mi[3] = i11 * i11 + i21 * i21;              // yy
        Mi[4] = i21 * i22;                          // yz
        Mi[5] = i22 * i22;                          // zz
    } else {
        sing = 1.0;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) d.Minv[6 * (size_t)p + i] = Mi[i];
    d.Aig[3 * (size_t)p + 0] = Mi[0] * g[0] + Mi[1] * g[1] + Mi[2] * g[2];
    d.Aig[3 * (size_t)p + 1] = Mi[1] * g[0] + Mi[3] * g[1] + Mi[4] * g[2];
    d.Aig[3 * (size_t)p + 2] = Mi[2] * g[0] + Mi[4] * g[1] + Mi[5] * g[2];
    return sing;
}

// one thread = one point: (fresh) E'E and E'r from the track, then the damped 3 x 3 inverse; returns its |gradient| share and singular flag
__device__ __forceinline__ void point_prep_thread(const BADev &d, int p, double radius, double min_diag, double max_diag, int fresh, double &gmax, double &sing)
{
    gmax = 0.0; sing = 0.0;
    if (p >= d.n_pt) return;
    const int b = d.pt_start[p], e = d.pt_start[p + 1];
    if (e <= b) return;
    double A[6], g[3];
    if (fresh) {
#pragma unroll
        for (int i = 0; i < 6; ++i) A[i] = 0.0;
        g[0] = g[1] = g[2] = 0.0;
        const size_t n = d.n_obs;
        for (int k = b; k < e; ++k) {
            const double j0 = d.Jp[k], j1 = d.Jp[n + k], j2 = d.Jp[2 * n + k];
            const double j3 = d.Jp[3 * n + k], j4 = d.Jp[4 * n + k], j5 = d.Jp[5 * n + k];
            const double r0 = d.res[k], r1 = d.res[n + k];
            A[0] += j0 * j0 + j3 * j3; A[1] += j0 * j1 + j3 * j4; A[2] += j0 * j2 + j3 * j5;
            A[3] += j1 * j1 + j4 * j4; A[4] += j1 * j2 + j4 * j5; A[5] += j2 * j2 + j5 * j5;
            g[0] += j0 * r0 + j3 * r1; g[1] += j1 * r0 + j4 * r1; g[2] += j2 * r0 + j5 * r1;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) d.EtE[6 * (size_t)p + i] = A[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            d.Etr[3 * (size_t)p + i] = g[i];
            gmax = fmax(gmax, fabs(g[i] / d.scale_p[3 * (size_t)p + i]));  // gradient of the unscaled problem
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) A[i] = d.EtE[6 * (size_t)p + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i] = d.Etr[3 * (size_t)p + i];
    }
    sing = point_block_invert(d, p, A, g, radius, min_diag, max_diag);
}

__global__ __launch_bounds__(64) void ba_point_prep_kernel(BADev d, double radius, double min_diag, double max_diag, int fresh, ScalBase sbase)
{
    __shared__ double red[8];
    double gmax, sing;
    point_prep_thread(d, blockIdx.x * 64 + threadIdx.x, radius, min_diag, max_diag, fresh, gmax, sing);
    if (fresh) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, o));
        if ((threadIdx.x & 63) == 0 && gmax > 0.0) atomic_max_nonneg(&d.scal[SC_GMAX], gmax);
    }
    const int slots[1] = {SC_PT_SINGULAR};
    const double vals[1] = {sing};
    scal_commit<1>(d, sbase, slots, vals, red);
}

// The per-point blocks of a fresh Jacobian AND the reduction of the sweep's per-camera slabs in one launch (one rank, small
// problems): the two are independent -- the slab sums are first needed by the reduced solve -- and each leaves most of the chip
// idle (22 workgroups for 25 cameras; a latency-bound walk over the tracks), so back to back they cost 8 + 12 us of a 180-us
// LM iteration on BA-25 and together 12.  The first n_red workgroups are ba_camacc_reduce_kernel's, the others take 256 points
// each (the singular-point count is an integer-valued sum and the gradient maximum a maximum: the wider workgroup changes no bit).
__global__ __launch_bounds__(256, 1) void ba_point_prep_camacc_kernel(BADev d, double radius, double min_diag, double max_diag, ScalBase sbase,
                                                                   const double *__restrict__ slabs, int n_slabs, int with_gradient, int n_red)
{
    __shared__ double lds[256];
    if ((int)blockIdx.x < n_red) { camacc_reduce_block(d, slabs, n_slabs, with_gradient, blockIdx.x, lds); return; }
    const int pb = (int)blockIdx.x - n_red;
    double gmax, sing;
    point_prep_thread(d, pb * 256 + threadIdx.x, radius, min_diag, max_diag, 1, gmax, sing);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, o));
    if ((threadIdx.x & 63) == 0 && gmax > 0.0) atomic_max_nonneg(&d.scal[SC_GMAX], gmax);
    const int slots[1] = {SC_PT_SINGULAR};
    const double vals[1] = {sing};
    scal_commit<1>(d, sbase, slots, vals, lds, pb);
}

// The fresh-Jacobian variant for large problems, one workgroup per point chunk (pchunk_pt0, <= 256 observations): thread =
// observation forms its nine products from ONE coalesced read of its Jp / res rows -> LDS; thread = point adds them in observation
// order (the same order, hence the same bits, as ba_point_prep_kernel's walk over the track) and inverts its block.  Throughput
// against latency: on BA-512 (3M observations) the walk costs 0.27 ms, this form 0.15 ms; on BA-25 (240k) this form is
// slower (17.6 us against 12 us: the 3 x 3 inverse's sqrt / divide chain runs in one half-filled wave per chunk), so the
// launcher picks by size.  A single point with more observations than a chunk holds walks its track like the plain kernel.
__global__ __launch_bounds__(kPtChunkObs) void ba_point_prep_chunk_kernel(BADev d, double radius, double min_diag, double max_diag, ScalBase sbase)
{
    __shared__ double red[8];
    __shared__ double prod[kPtChunkObs][9];
    const int tid = threadIdx.x;
    const int4 ci4 = d.pchunk_info[blockIdx.x];          // (one load where p0 / p1, then pt_start[p0] / pt_start[p1], were two dependent ones)
    const int p0 = ci4.x, p1 = ci4.y, k0 = ci4.z, k1 = ci4.w;
    const int nobs = k1 - k0;
    const size_t n = d.n_obs;
    double gmax = 0.0, sing = 0.0;
    const bool small = nobs <= kPtChunkObs;
    // what the point phase needs from memory is requested NOW, in front of the rows (round 5): behind the barrier it was two more
    // dependent round trips in a workgroup whose whole life is five, with 9 of 10 threads idle
    const bool is_pt = tid < p1 - p0;
    int pt_b = 0, pt_e = 0;
    double pt_sc[3] = {1.0, 1.0, 1.0};
    if (is_pt) {
        pt_b = d.pt_start[p0 + tid]; pt_e = d.pt_start[p0 + tid + 1];
#pragma unroll
        for (int q = 0; q < 3; ++q) pt_sc[q] = d.scale_p[3 * (size_t)(p0 + tid) + q];
    }
    if (small && tid < nobs) {
        const int k = k0 + tid;
        const double j0 = d.Jp[k], j1 = d.Jp[n + k], j2 = d.Jp[2 * n + k];
        const double j3 = d.Jp[3 * n + k], j4 = d.Jp[4 * n + k], j5 = d.Jp[5 * n + k];
        const double r0 = d.res[k], r1 = d.res[n + k];
        prod[tid][0] = j0 * j0 + j3 * j3; prod[tid][1] = j0 * j1 + j3 * j4; prod[tid][2] = j0 * j2 + j3 * j5;
        prod[tid][3] = j1 * j1 + j4 * j4; prod[tid][4] = j1 * j2 + j4 * j5; prod[tid][5] = j2 * j2 + j5 * j5;
        prod[tid][6] = j0 * r0 + j3 * r1; prod[tid][7] = j1 * r0 + j4 * r1; prod[tid][8] = j2 * r0 + j5 * r1;
    }
    __syncthreads();
    if (is_pt) {
        const int p = p0 + tid;
        const int b = pt_b, e = pt_e;
        if (e > b) {
            double A[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
            if (small) {
                for (int o = b - k0; o < e - k0; ++o) {
#pragma unroll
                    for (int q = 0; q < 6; ++q) A[q] += prod[o][q];
#pragma unroll
                    for (int q = 0; q < 3; ++q) g[q] += prod[o][6 + q];
                }
            } else {
                for (int k = b; k < e; ++k) {
                    const double j0 = d.Jp[k], j1 = d.Jp[n + k], j2 = d.Jp[2 * n + k];
                    const double j3 = d.Jp[3 * n + k], j4 = d.Jp[4 * n + k], j5 = d.Jp[5 * n + k];
                    const double r0 = d.res[k], r1 = d.res[n + k];
                    A[0] += j0 * j0 + j3 * j3; A[1] += j0 * j1 + j3 * j4; A[2] += j0 * j2 + j3 * j5;
                    A[3] += j1 * j1 + j4 * j4; A[4] += j1 * j2 + j4 * j5; A[5] += j2 * j2 + j5 * j5;
                    g[0] += j0 * r0 + j3 * r1; g[1] += j1 * r0 + j4 * r1; g[2] += j2 * r0 + j5 * r1;
                }
            }
#pragma unroll
            for (int q = 0; q < 6; ++q) d.EtE[6 * (size_t)p + q] = A[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                d.Etr[3 * (size_t)p + q] = g[q];
                gmax = fmax(gmax, fabs(g[q] / pt_sc[q]));  // gradient of the unscaled problem
            }
            sing = point_block_invert(d, p, A, g, radius, min_diag, max_diag);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, o));
    if ((threadIdx.x & 63) == 0 && gmax > 0.0) atomic_max_nonneg(&d.scal[SC_GMAX], gmax);
    const int slots[1] = {SC_PT_SINGULAR};
    const double vals[1] = {sing};
    scal_commit<1>(d, sbase, slots, vals, red);
}

// Jacobi scaling 1/(1 + sqrt(squared column norm)) from the unscaled linearisation
// (trust_region_minimizer.cc, iteration 0).  Point norms = diag(E'E); camera norms = diag(F'F).
__global__ void ba_jacobi_scaling_kernel(BADev d)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * d.n_pt) {
        const int p = i / 3, a = i % 3;
        const int di = a == 0 ? 0 : (a == 1 ? 3 : 5);
        const bool active = d.pt_start[p + 1] > d.pt_start[p];
        d.scale_p[i] = active ? 1.0 / (1.0 + sqrt(d.EtE[6 * (size_t)p + di])) : 1.0;
    }
    if (i < 6 * d.n_cam) {
        const int c = i / 6, a = i % 6;
        d.scale_c[i] = 1.0 / (1.0 + sqrt(d.camacc[36 * (size_t)c + 7 * a]));
    }
}

__global__ void ba_camera_gradient_kernel(BADev d)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double g = 0.0;
    if (i < 6 * d.n_cam) g = camera_gradient_entry(d, i, d.camacc[36 * (size_t)d.n_cam + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) g = fmax(g, __shfl_xor(g, o));
    if ((threadIdx.x & 63) == 0 && g > 0.0) atomic_max_nonneg(&d.scal[SC_GMAX], g);
}

// ---------------------------------------------------------------------------------------------
int ba_linearize(hipStream_t st, const BADev &d, int num_cu, double cauchy_a, bool use_scaling, esfm_ctx *timing_ctx, int *deferred_slabs, double cost_bound)
{
    const BaForms &forms = d.parts->forms;
    // provisional exponent of the residual column (see the kernel): sqrt(sum r^2) <= sqrt(2 cost) < 2^prov_rexp
    int prov_rexp = INT_MIN;
    if (cost_bound > 0.0 && cost_bound < 1e300) prov_rexp = std::ilogb(std::sqrt(2.0 * cost_bound)) + 1;
    if (deferred_slabs) *deferred_slabs = 0;
    if (d.n_obs <= 0 || d.n_cchunks <= 0) {
        ESFM_HIP_TRY(hipMemsetAsync(d.camacc, 0, sizeof(double) * ba_camacc_doubles(d.n_cam), st));
        ESFM_HIP_TRY(hipMemsetAsync(d.qexp, 0, sizeof(int32_t) * 6 * (size_t)d.n_cam, st));
        return ESFM_OK;
    }
    const size_t priv_bytes = lin_lds_bytes(d.n_real_cam);
    const bool small = !forms.large;
    const int kLinThreads = small ? kLinThreadsSmall : kLinThreadsLarge;
    // (the 512-thread form fills a CU's registers with ONE workgroup -- 250 registers x 8 waves -- so a second workgroup per CU only runs
    // after the first, paying the 9-us prologue (LDS clear, exponents) and the 8-us epilogue (guard, slab) again: one per CU)
    const int grid = std::min(div_up(d.n_obs, kLinThreads), std::max(1, num_cu) * (small ? 2 : 1));
    const bool priv = forms.sweep_sums_in_lds;
    if (priv && ba_grouped(d)) { set_error("BA sweep: several intrinsics blocks, or a radial one, take the camera-chunk sums"); return ESFM_ERR_INVALID_ARG; }
    if (priv && (size_t)grid * ba_lin_slab_doubles(d.n_cam) > d.lin_slab_cap) { set_error("BA sweep: %d slabs do not fit lin_slabs", grid); return ESFM_ERR_INVALID_ARG; }
    ScalBase sbase;
    { const int slots[2] = {SC_COST, SC_LIN_BAD}; if (int rc = scal_reserve<2>(st, d, slots, grid, sbase)) return rc; }
    if (priv) {
        auto kern = small ? (d.has_calib ? &ba_linearize_kernel<true, true, kLinThreadsSmall> : &ba_linearize_kernel<true, false, kLinThreadsSmall>)
                          : (d.has_calib ? &ba_linearize_kernel<true, true, kLinThreadsLarge> : &ba_linearize_kernel<true, false, kLinThreadsLarge>);
        ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)priv_bytes));
        {
            KernelTimer tm(timing_ctx, ESFM_K_BA_LINEARIZE);   // the Jacobian sweep with its in-LDS camera sums (not the slab reduction)
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kLinThreads), priv_bytes, st, d, cauchy_a, use_scaling ? 1 : 0, sbase, d.lin_slabs, prov_rexp);
        }
        LAUNCH_CHECK();
        d.parts->grad_done = d.parts->single_rank;
        // one rank, per-point blocks by the walking kernel next: the slab reduction rides in that launch (ba_point_prep_camacc)
        if (deferred_slabs && d.parts->single_rank && !(d.n_pchunks > 0 && forms.large) && d.n_pt > 0) { *deferred_slabs = grid; return ESFM_OK; }
        hipLaunchKernelGGL(ba_camacc_reduce_kernel, dim3(div_up(d.n_cam * 27, kRedEnt)), dim3(256), 0, st, d, d.lin_slabs, grid, d.parts->single_rank ? 1 : 0);
        LAUNCH_CHECK();
        return ESFM_OK;
    }
    {
        KernelTimer tm(timing_ctx, ESFM_K_BA_LINEARIZE);   // the Jacobian sweep alone
        auto kern = small ? (d.has_calib ? &ba_linearize_kernel<false, true, kLinThreadsSmall> : &ba_linearize_kernel<false, false, kLinThreadsSmall>)
                          : (d.has_calib ? &ba_linearize_kernel<false, true, kLinThreadsLarge> : &ba_linearize_kernel<false, false, kLinThreadsLarge>);
        if (d.has_calib > 1) kern = small ? &ba_linearize_kernel<false, true, kLinThreadsSmall, true> : &ba_linearize_kernel<false, true, kLinThreadsLarge, true>;
        if (d.radial) kern = small ? &ba_linearize_kernel<false, true, kLinThreadsSmall, true, true> : &ba_linearize_kernel<false, true, kLinThreadsLarge, true, true>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kLinThreads), 18 * sizeof(double), st, d, cauchy_a, use_scaling ? 1 : 0, sbase, (double *)nullptr, INT_MIN);
    }
    LAUNCH_CHECK();
    if (d.radial) hipLaunchKernelGGL((ba_camacc_chunk_kernel<true, true>), dim3(d.n_cchunks), dim3(64), 0, st, d);
    else if (d.has_calib) hipLaunchKernelGGL(ba_camacc_chunk_kernel<true>, dim3(d.n_cchunks), dim3(64), 0, st, d);
    else hipLaunchKernelGGL(ba_camacc_chunk_kernel<false>, dim3(d.n_cchunks), dim3(64), 0, st, d);
    hipLaunchKernelGGL(ba_camacc_final_kernel, dim3(div_up(d.n_real_cam * 27 + 42, 256)), dim3(256), 0, st, d);
    LAUNCH_CHECK();
    if (d.radial) {
        hipLaunchKernelGGL(ba_camacc_groups_kernel<true>, dim3(d.has_calib * 42), dim3(64), 0, st, d);
        LAUNCH_CHECK();
    } else if (d.has_calib > 1) {
        hipLaunchKernelGGL(ba_camacc_groups_kernel<false>, dim3(d.has_calib * 42), dim3(64), 0, st, d);
        LAUNCH_CHECK();
    }
    return ESFM_OK;
}

int ba_point_prep(hipStream_t st, const BADev &d, double radius, double min_diag, double max_diag, bool fresh, int deferred_slabs)
{
    ScalBase sbase;
    const int slots[1] = {SC_PT_SINGULAR};
    if (deferred_slabs > 0) {      // ba_linearize left the slab reduction to this launch (it checked that this path is taken)
        const int n_red = div_up(d.n_cam * 27, kRedEnt), n_prep = div_up(d.n_pt, 256);
        if (int rc = scal_reserve<1>(st, d, slots, n_prep, sbase)) return rc;
        hipLaunchKernelGGL(ba_point_prep_camacc_kernel, dim3(n_red + n_prep), dim3(256), 0, st, d, radius, min_diag, max_diag, sbase, d.lin_slabs,
                           deferred_slabs, 1, n_red);
        LAUNCH_CHECK();
        return ESFM_OK;
    }
    if (d.n_pt <= 0) return ESFM_OK;
    if (fresh && d.n_pchunks > 0 && d.parts->forms.large) {        // (see ba_point_prep_chunk_kernel for the crossover)
        if (int rc = scal_reserve<1>(st, d, slots, d.n_pchunks, sbase)) return rc;
        hipLaunchKernelGGL(ba_point_prep_chunk_kernel, dim3(d.n_pchunks), dim3(kPtChunkObs), 0, st, d, radius, min_diag, max_diag, sbase);
        LAUNCH_CHECK();
        return ESFM_OK;
    }
    if (int rc = scal_reserve<1>(st, d, slots, div_up(d.n_pt, 64), sbase)) return rc;
    hipLaunchKernelGGL(ba_point_prep_kernel, dim3(div_up(d.n_pt, 64)), dim3(64), 0, st, d, radius, min_diag, max_diag, fresh ? 1 : 0, sbase);
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_jacobi_scaling(hipStream_t st, const BADev &d)
{
    const int m = std::max(3 * d.n_pt, 6 * d.n_cam);
    if (m <= 0) return ESFM_OK;
    hipLaunchKernelGGL(ba_jacobi_scaling_kernel, dim3(div_up(m, 256)), dim3(256), 0, st, d);
    LAUNCH_CHECK();
    return ESFM_OK;
}

int ba_camera_gradient(hipStream_t st, const BADev &d)
{
    if (d.parts->grad_done) { d.parts->grad_done = false; return ESFM_OK; }    // ba_camacc_reduce_kernel has done it (one rank)
    if (d.n_cam <= 0) return ESFM_OK;
    hipLaunchKernelGGL(ba_camera_gradient_kernel, dim3(div_up(6 * d.n_cam, 256)), dim3(256), 0, st, d);
    LAUNCH_CHECK();
    return ESFM_OK;
}

}  // namespace esfm
