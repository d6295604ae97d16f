// L2 matching on f32 operands: the row norms, the f32-input MFMA distance
// pass with its fused top-3 and certificate (128-float rows; 64-float rows under ESFM_L2_PASS=f32), the exact brute-force scan
// (widths without an MFMA build, audit mode 2, the f32 pass's certificate failures) and its latency-aware 64-float form.
#include "match_kernels.hpp"
#include "match_device.hpp"

#include <float.h>
#include <type_traits>
#include <stdlib.h>
#include <string.h>

namespace esfm {

// ---------------------------------------------------------------------------------------------
// |row|^2 for every descriptor row (float chain; only used by the approximate pass + certificate)
__global__ void l2_row_norms_kernel(const float *__restrict__ desc, int dim, long long n_rows, float *__restrict__ norms)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const float *p = desc + r * dim;
    float s = 0.f;
    for (int k = 0; k < dim; ++k) s = fmaf(p[k], p[k], s);
    norms[r] = s;
}

// ---------------------------------------------------------------------------------------------
// MFMA distance pass.
//
// One workgroup (4 waves) owns QB = 128 query rows of one pair and streams the whole train set
// through LDS in tiles of TT = 64 rows.  Each wave owns 32 queries for the entire kernel: their
// descriptors, scaled by -2, stay in HALF = DIM/2 VGPRs per lane as the MFMA B operand
// (lane l: query l&31, features [HALF*(l>>5), HALF*(l>>5)+HALF)).  A train sub-tile of 32 rows is
// the A operand, read from LDS with ds_read_b128 (XOR-swizzled 16-B slots: conflict-free).  The
// accumulator starts at |t|^2, so after DIM/2 MFMAs D[t][q] = |t|^2 - 2 q.t  (= d^2 - |q|^2) with
// no epilogue arithmetic.  C/D layout: lane l, reg r -> train row (r&3)+8*(r>>2)+4*(l>>5), query
// l&31, i.e. the 16 values in a lane belong to ONE query, so the running top-3 is lane-local.
template <int DIM, int TT>
__global__ __launch_bounds__(256) void l2_knn_mfma_kernel(const float *__restrict__ desc, const float *__restrict__ norms,
                                                          const PairDesc *__restrict__ pairs, int n_pairs,
                                                          int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist,
                                                          int32_t *__restrict__ flagged, int32_t *__restrict__ counters,
                                                          int flag_cap)
{
    constexpr int QB = 128, HALF = DIM / 2, NCH = HALF / 4, SLOTS = DIM / 4;
    constexpr int STAGE = TT * SLOTS / 256;  // float4 per thread per tile
    static_assert(DIM % 8 == 0 && STAGE >= 1, "DIM");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *lds_tile = reinterpret_cast<float4 *>(smem);                       // [2][TT*SLOTS]
    float *lds_norm = reinterpret_cast<float *>(smem + 2 * TT * SLOTS * 16);   // [2][TT]
    float *lds_red = lds_norm + 2 * TT;                                        // [4]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = find_pair_by_block(pairs, n_pairs, lb);
    const PairDesc pd = pairs[pi];
    const int nq = pd.nq, nt = pd.nt;
    const float *__restrict__ Q = desc + (size_t)pd.q_row0 * DIM;
    const float *__restrict__ T = desc + (size_t)pd.t_row0 * DIM;
    const float *__restrict__ tn = norms + pd.t_row0;
    const int qrow = (lb - pd.blk_off) * QB + wave * 32 + j;
    const bool qvalid = qrow < nq;

    // B operand: this lane's half of its query row, times -2 (exact scaling).
    float breg[HALF];
    {
        const float4 *qp = reinterpret_cast<const float4 *>(Q + (size_t)(qvalid ? qrow : 0) * DIM + h * HALF);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            float4 v = qvalid ? qp[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            breg[4 * c + 0] = -2.f * v.x; breg[4 * c + 1] = -2.f * v.y; breg[4 * c + 2] = -2.f * v.z; breg[4 * c + 3] = -2.f * v.w;
        }
    }

    // Running top-3, two levels.
    //
    // On gfx950 the f32-input MFMA runs at the f32 VECTOR rate and VALU work does NOT hide under it
    // (measured: every VALU instruction next to v_mfma_f32_32x32x2_f32 adds ~3 cycles per SIMD), so
    // the fold is budgeted in instructions per element.  Level 1 (per element, 4 VALU ops, no
    // compares): the low 8 mantissa bits of s are replaced by an 8-bit position code
    // (key = (s & ~0xFF) | code, one v_and_or_b32) and the three smallest keys of the current
    // 512-row segment are kept with v_med3_f32 / v_med3_f32 / v_min -- as floats, the keys order like
    // s truncated to 15 mantissa bits.  Level 2 (once per segment = 256 elements per lane): the three
    // segment keys are decoded to (key, train row) and merged into the lane's master top-3 with the
    // compare/select chain.  The truncation error (< 2^-14 |key|) is charged to the certificate.
    constexpr float kBig = 3.0e38f;       // finite "empty slot" sentinel; padded train rows carry |t|^2 = kBig too
    constexpr int kSegSub = 16;           // sub-tiles (32 rows) per segment -> 8-bit codes
    float k0 = kBig, k1 = kBig, k2 = kBig;             // segment keys
    float v0 = kBig, v1 = kBig, v2 = kBig;             // master keys
    int c0 = -1, c1 = -1, c2 = -1;                     // master train rows
    float tmax = 0.f;  // max |t|^2 seen by this thread (threads < TT only)
    int poison = 0;    // a train row with a non-finite norm (inf / NaN entries, or an overflowing |t|^2): its scores can be NaN, and a NaN key
                       // corrupts the v_med3 network -- no query of this workgroup is certified, the exact re-scan decides
    unsigned kmask = 0xFFFFFF00u;
    asm volatile("" : "+v"(kmask));   // keep the mask in a VGPR: v_and_or_b32 can then take the code as its one SGPR operand
    auto fold = [&](float s, int code /* wave-uniform */) {
        float key;
        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(key) : "v"(s), "v"(kmask), "s"(code));
        k2 = __builtin_amdgcn_fmed3f(k1, k2, key);
        k1 = __builtin_amdgcn_fmed3f(k0, k1, key);
        k0 = __builtin_amdgcn_fmed3f(k0, key, -kBig);   // min without the NaN-quieting v_max pair
    };
    auto master_insert = [&](float key, int seg_sub0) {
        // decode: code = 16 * (sub-tile within segment) + accumulator register
        const int code = (int)(__float_as_uint(key) & 0xFFu);
        const int r = code & 15;
        const int t = (seg_sub0 + (code >> 4)) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool live = key < 1.0e38f;
        const bool l2 = live && key < v2, l1 = live && key < v1, l0 = live && key < v0;
        const int t2 = l2 ? t : c2;
        const int t1 = l1 ? t : c1;
        c2 = l1 ? c1 : t2;
        c1 = l0 ? c0 : t1;
        c0 = l0 ? t : c0;
        const float n2 = l2 ? key : v2;
        const float n1 = l1 ? key : v1;
        v2 = l1 ? v1 : n2;
        v1 = l0 ? v0 : n1;
        v0 = l0 ? key : v0;
    };
    auto flush = [&](int seg_sub0) {
        master_insert(k0, seg_sub0); master_insert(k1, seg_sub0); master_insert(k2, seg_sub0);
        k0 = k1 = k2 = kBig;
    };

    const int ntiles = (nt + TT - 1) / TT;
    float4 stage[STAGE];
    float stage_n = kBig;
    // Staging loads go through a buffer descriptor over the train set: rows past nt read as zeros in
    // hardware, the per-thread byte offset is one loop-invariant VGPR and the tile offset is scalar, so
    // a tile costs no address VALU (VALU does not overlap the f32 MFMA, every instruction counts).
    const __amdgpu_buffer_rsrc_t trsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(T), 0, nt * DIM * 4, 0x00020000);
    const int voff = (tid / SLOTS) * (DIM * 4) + (tid % SLOTS) * 16;   // row-in-pass * row bytes + slot * 16
    auto gload = [&](int tile) {
#pragma unroll
        for (int i = 0; i < STAGE; ++i) {
            const int soff = (tile * TT + i * (256 / SLOTS)) * (DIM * 4);   // wave-uniform
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(trsrc, voff, soff, 0);
            stage[i] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
        }
        const int t = tile * TT + (tid & (TT - 1));
        const float nv = tn[min(t, nt - 1)];
        stage_n = (t < nt) ? nv : kBig;
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < STAGE; ++i) {
            const int s = tid + 256 * i, row = s / SLOTS, slot = s % SLOTS;
            lds_tile[buf * TT * SLOTS + row * SLOTS + (slot ^ (row & 15))] = stage[i];
        }
        if (tid < TT) { lds_norm[buf * TT + tid] = stage_n; if (stage_n < 1.0e38f) tmax = fmaxf(tmax, stage_n); else if (!(stage_n == kBig)) poison = 1; }
    };

    if (ntiles > 0) { gload(0); lstore(0); }
    __syncthreads();

    static_assert(TT % 64 == 0 && TT <= 256, "a tile is a whole number of 64-row sub-tile pairs");
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        gload(min(tile + 1, ntiles - 1));  // next tile in flight under the MFMAs below (last trip: harmless re-load)
#pragma unroll
        for (int sp = 0; sp < TT / 64; ++sp) {
            const int base = sp * 64;
            floatx16 acc0, acc1;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 n0 = *reinterpret_cast<const float4 *>(&lds_norm[buf * TT + base + 8 * g + 4 * h]);
                const float4 n1 = *reinterpret_cast<const float4 *>(&lds_norm[buf * TT + base + 32 + 8 * g + 4 * h]);
                acc0[4 * g + 0] = n0.x; acc0[4 * g + 1] = n0.y; acc0[4 * g + 2] = n0.z; acc0[4 * g + 3] = n0.w;
                acc1[4 * g + 0] = n1.x; acc1[4 * g + 1] = n1.y; acc1[4 * g + 2] = n1.z; acc1[4 * g + 3] = n1.w;
            }
            float4 a0[NCH], a1[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {   // (base + 32 + j) & 15 == j & 15
                a0[c] = lds_tile[buf * TT * SLOTS + (base + j) * SLOTS + ((h * NCH + c) ^ (j & 15))];
                a1[c] = lds_tile[buf * TT * SLOTS + (base + 32 + j) * SLOTS + ((h * NCH + c) ^ (j & 15))];
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[c].x, breg[4 * c + 0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[c].x, breg[4 * c + 0], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[c].y, breg[4 * c + 1], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[c].y, breg[4 * c + 1], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[c].z, breg[4 * c + 2], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[c].z, breg[4 * c + 2], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[c].w, breg[4 * c + 3], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[c].w, breg[4 * c + 3], acc1, 0, 0, 0);
            }
            // The fold reads the accumulators from inline asm, for which hipcc pads no hazards: an MFMA's
            // result needs ~18 wait states (16-pass op) before a non-MFMA reader.  Routing both
            // accumulators through this statement orders every fold after the last MFMA plus the pad.
            asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc0), "+v"(acc1));
            const int sub = tile * (TT / 32) + 2 * sp;  // global sub-tile index of acc0
            const int cb = __builtin_amdgcn_readfirstlane((sub % kSegSub) * 16);   // code base inside the segment (SGPR)
#pragma unroll
            for (int r = 0; r < 16; ++r) fold(acc0[r], cb + r);
#pragma unroll
            for (int r = 0; r < 16; ++r) fold(acc1[r], cb + 16 + r);
            if ((sub + 2) % kSegSub == 0) flush(sub + 2 - kSegSub);
        }
        if (tile + 1 < ntiles) lstore(buf ^ 1);
        __syncthreads();
    }
    {
        const int nsub = ntiles * (TT / 32);
        if (nsub % kSegSub != 0) flush((nsub / kSegSub) * kSegSub);
    }

    // max |t|^2 over the train set (for the certificate's error bound)
    {
        float m = tmax;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) lds_red[wave] = m;
        poison = __syncthreads_or(poison);
        tmax = fmaxf(fmaxf(lds_red[0], lds_red[1]), fmaxf(lds_red[2], lds_red[3]));
    }

    // ---- exact re-rank of this lane's 3 candidates in the oracle's order ----
    Cand b0 = {FLT_MAX, -1, 0.f}, b1 = {FLT_MAX, -1, 0.f};
    float ed[3], ed2[3];
    int ei[3];
    {
        const int cc[3] = {c0, c1, c2};
        const float *qp = Q + (size_t)(qvalid ? qrow : 0) * DIM;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            ei[m] = -1; ed[m] = FLT_MAX; ed2[m] = 0.f;
            if (cc[m] >= 0 && qvalid) {
                const int t = cc[m];
                const float d2 = l2sqr_canonical<true>(qp, T + (size_t)t * DIM, DIM);
                ei[m] = t; ed2[m] = d2; ed[m] = sqrt_rn_f32(d2);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) best2_insert(b0, b1, ed[m], ei[m], ed2[m]);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const float pd_ = __shfl_xor(ed[m], 32), pd2 = __shfl_xor(ed2[m], 32);
        const int pi_ = __shfl_xor(ei[m], 32);
        best2_insert(b0, b1, pd_, pi_, pd2);
    }
    const float tau = fminf(v2, __shfl_xor(v2, 32));  // every train outside the 6 candidates has s >= tau

    if (qvalid && h == 0) {
        const size_t o = 2 * ((size_t)pd.out_off + qrow);
        knn_idx[o] = b0.i; knn_idx[o + 1] = b1.i;
        knn_dist[o] = b0.d; knn_dist[o + 1] = b1.d;
        // Certificate: |(|q|^2 + s(t)) - D(t)| <= 2^-16 (|q|^2 + max|t|^2) for every train t, and
        // every train outside the candidates has key >= tau, hence s >= tau - 2^-14 |tau| (truncation);
        // the candidate set provably contains the two best iff |q|^2 + tau - eps exceeds the second
        // best exact d^2 by more than sqrt's rounding can hide.
        bool certified = (tau >= 1.0e38f) && !poison;   // an empty slot in either lane: every train row is a candidate (a NaN tau is NOT certified)
        if (!certified && b1.i >= 0 && !poison) {
            const double qn = (double)norms[pd.q_row0 + qrow];
            const double eps = (qn + (double)tmax) * (1.0 / 65536.0) + fabs((double)tau) * (1.0 / 16384.0);
            certified = (qn + (double)tau - eps) > (double)b1.d2 * (1.0 + 1.0 / 2097152.0);
        }
        if (!certified) {
            const int slot = atomicAdd(&counters[0], 1);
            if (slot < flag_cap) { flagged[2 * slot] = pi; flagged[2 * slot + 1] = qrow; }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Exact brute-force 2-NN for listed queries (flagged != NULL: entries [0, counters[0])) or for
// every query of every pair (flagged == NULL: entries [0, total_queries)).  One workgroup per
// entry, threads stride over the train rows, lexicographic (distance, index) reduction.
template <bool VEC>
__global__ __launch_bounds__(256) void l2_exact_scan_kernel(const float *__restrict__ desc, int dim,
                                                            const PairDesc *__restrict__ pairs, int n_pairs,
                                                            const int32_t *__restrict__ flagged,
                                                            const int32_t *__restrict__ counters, long long total_queries,
                                                            int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist)
{
    __shared__ float s_d[2][256];
    __shared__ int s_i[2][256];
    const int tid = threadIdx.x;
    const long long n_entries = flagged ? (long long)counters[0] : total_queries;
    for (long long e = blockIdx.x; e < n_entries; e += gridDim.x) {
        int pi, qrow;
        if (flagged) { pi = flagged[2 * e]; qrow = flagged[2 * e + 1]; }
        else { pi = find_pair_by_query(pairs, n_pairs, e); qrow = (int)(e - pairs[pi].out_off); }
        const PairDesc pd = pairs[pi];
        const float *q = desc + ((size_t)pd.q_row0 + qrow) * dim;
        const float *T = desc + (size_t)pd.t_row0 * dim;
        Cand b0 = {FLT_MAX, -1, 0.f}, b1 = {FLT_MAX, -1, 0.f};
        for (int t = tid; t < pd.nt; t += 256) {
            const float d2 = l2sqr_canonical<VEC>(q, T + (size_t)t * dim, dim);
            best2_insert(b0, b1, sqrt_rn_f32(d2), t, d2);
        }
        s_d[0][tid] = b0.d; s_i[0][tid] = b0.i; s_d[1][tid] = b1.d; s_i[1][tid] = b1.i;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) {
                Cand a0 = {s_d[0][tid], s_i[0][tid], 0.f}, a1 = {s_d[1][tid], s_i[1][tid], 0.f};
                best2_insert(a0, a1, s_d[0][tid + w], s_i[0][tid + w], 0.f);
                best2_insert(a0, a1, s_d[1][tid + w], s_i[1][tid + w], 0.f);
                s_d[0][tid] = a0.d; s_i[0][tid] = a0.i; s_d[1][tid] = a1.d; s_i[1][tid] = a1.i;
            }
            __syncthreads();
        }
        if (tid == 0) {
            const size_t o = 2 * ((size_t)pd.out_off + qrow);
            knn_idx[o] = s_i[0][0]; knn_idx[o + 1] = s_i[1][0];
            knn_dist[o] = s_i[0][0] >= 0 ? s_d[0][0] : FLT_MAX;
            knn_dist[o + 1] = s_i[1][0] >= 0 ? s_d[1][0] : FLT_MAX;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// (Measured alternative, round 2: one workgroup per PAIR, its uncertified queries -- 2.2 on average -- sharing every train row a
// thread loads: fewer bytes, but eight candidate states and two train rows per thread spill, 0.35 ms against 0.105 ms.)
// The rescan of the queries the certificate rejects, 64-float rows: same result as l2_exact_scan_kernel, but latency-aware --
// the handful of flagged queries (0.06 % on M-SURF-4k) leaves the chip nearly empty, so a thread keeps its query row in
// registers and has the loads of two train rows in flight at a time, and the (distance, index) reduction runs on wave
// shuffles.  l2sqr64_canonical_regs is l2sqr_canonical on register operands: the same 8 chains, the same final order.
__global__ __launch_bounds__(256) void l2_rescan64_kernel(const float *__restrict__ desc, const PairDesc *__restrict__ pairs,
                                                          const int32_t *__restrict__ flagged, const int32_t *__restrict__ counters,
                                                          int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist)
{
    __shared__ float s_d[2][4];
    __shared__ int s_i[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_entries = counters[0];
    for (int e = blockIdx.x; e < n_entries; e += gridDim.x) {
        const int pi = flagged[2 * e], qrow = flagged[2 * e + 1];
        const PairDesc pd = pairs[pi];
        const float4 *qp = reinterpret_cast<const float4 *>(desc + ((size_t)pd.q_row0 + qrow) * 64);
        const float4 *T = reinterpret_cast<const float4 *>(desc + (size_t)pd.t_row0 * 64);
        float4 qv[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) qv[c] = qp[c];
        Cand b0 = {FLT_MAX, -1, 0.f}, b1 = {FLT_MAX, -1, 0.f};
        for (int t = tid; t < pd.nt; t += 512) {
            const int t2 = t + 256;
            const bool two = t2 < pd.nt;
            float4 ta[16], tb[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) ta[c] = T[(size_t)t * 16 + c];
#pragma unroll
            for (int c = 0; c < 16; ++c) tb[c] = T[(size_t)(two ? t2 : t) * 16 + c];
            const float da = l2sqr64_canonical_regs(qv, ta), db = l2sqr64_canonical_regs(qv, tb);
            best2_insert(b0, b1, sqrt_rn_f32(da), t, da);
            if (two) best2_insert(b0, b1, sqrt_rn_f32(db), t2, db);
        }
        // (distance, index) is a total order: the merge order does not matter
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float d0 = __shfl_xor(b0.d, o), d1 = __shfl_xor(b1.d, o);
            const int i0 = __shfl_xor(b0.i, o), i1 = __shfl_xor(b1.i, o);
            best2_insert(b0, b1, d0, i0, 0.f);
            best2_insert(b0, b1, d1, i1, 0.f);
        }
        if (lane == 0) { s_d[0][wave] = b0.d; s_i[0][wave] = b0.i; s_d[1][wave] = b1.d; s_i[1][wave] = b1.i; }
        __syncthreads();
        if (tid == 0) {
            Cand a0 = {FLT_MAX, -1, 0.f}, a1 = {FLT_MAX, -1, 0.f};
            for (int w = 0; w < 4; ++w) { best2_insert(a0, a1, s_d[0][w], s_i[0][w], 0.f); best2_insert(a0, a1, s_d[1][w], s_i[1][w], 0.f); }
            const size_t o = 2 * ((size_t)pd.out_off + qrow);
            knn_idx[o] = a0.i; knn_idx[o + 1] = a1.i;
            knn_dist[o] = a0.i >= 0 ? a0.d : FLT_MAX;
            knn_dist[o + 1] = a1.i >= 0 ? a1.d : FLT_MAX;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// launchers

static inline int div_up(long long a, long long b) { return (int)((a + b - 1) / b); }

int launch_l2_norms(hipStream_t st, const float *desc, int dim, long long n_rows, float *norms)
{
    if (n_rows <= 0) return ESFM_OK;
    hipLaunchKernelGGL(l2_row_norms_kernel, dim3(div_up(n_rows, 256)), dim3(256), 0, st, desc, dim, n_rows, norms);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

bool l2_mfma_supported(int dim) { return dim == 64 || dim == 128; }

int launch_l2_knn_mfma(hipStream_t st, int dim, const float *desc, const float *norms, const PairDesc *pairs, int n_pairs,
                       int n_blocks, int32_t *knn_idx, float *knn_dist, int32_t *flagged, int32_t *counters, int flag_cap)
{
    if (n_blocks <= 0) return ESFM_OK;
    // train tile = 128 rows (one barrier per 128 MFMAs per wave); LDS = 2 x TT x DIM x 4 B + norms
    if (dim == 64) {
        constexpr int TT = 128;
        constexpr size_t lds = 2 * TT * 16 * 16 + 2 * TT * 4 + 16;
        hipLaunchKernelGGL((l2_knn_mfma_kernel<64, TT>), dim3(n_blocks), dim3(256), lds, st, desc, norms, pairs, n_pairs, knn_idx,
                           knn_dist, flagged, counters, flag_cap);
    } else if (dim == 128) {
        constexpr int TT = 64;
        constexpr size_t lds = 2 * TT * 32 * 16 + 2 * TT * 4 + 16;
        hipLaunchKernelGGL((l2_knn_mfma_kernel<128, TT>), dim3(n_blocks), dim3(256), lds, st, desc, norms, pairs, n_pairs, knn_idx,
                           knn_dist, flagged, counters, flag_cap);
    } else {
        set_error("l2 MFMA kernel is built for dim 64 and 128 only (got %d)", dim);
        return ESFM_ERR_UNSUPPORTED;
    }
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_l2_exact_scan(hipStream_t st, int dim, const float *desc, const PairDesc *pairs, int n_pairs,
                         const int32_t *flagged, const int32_t *counters, long long total_queries, int grid,
                         int32_t *knn_idx, float *knn_dist)
{
    if (grid <= 0) return ESFM_OK;
    if (dim == 64 && flagged)
        hipLaunchKernelGGL(l2_rescan64_kernel, dim3(grid), dim3(256), 0, st, desc, pairs, flagged, counters, knn_idx, knn_dist);
    else if (dim % 4 == 0)
        hipLaunchKernelGGL(l2_exact_scan_kernel<true>, dim3(grid), dim3(256), 0, st, desc, dim, pairs, n_pairs, flagged, counters,
                           total_queries, knn_idx, knn_dist);
    else
        hipLaunchKernelGGL(l2_exact_scan_kernel<false>, dim3(grid), dim3(256), 0, st, desc, dim, pairs, n_pairs, flagged, counters,
                           total_queries, knn_idx, knn_dist);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

}  // namespace esfm
