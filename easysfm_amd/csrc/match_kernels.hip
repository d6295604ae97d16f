// The matcher's default L2 path, the two kernels the metric times (sections 4.1 and 4.2):
// l2_knn_bf16x1_kernel -- one bf16 product per f32 product, fused top-K fold, ratio screen -- and l2_finish_kernel -- exact re-rank,
// certificate, threshold filter, brute force, ratio test + compaction --, with their launchers and switches.  The other families
// have files of their own: match_l2_bf16x3.hip (which also writes this pass's images), match_l2_f32.hip, match_hamming.hip,
// match_lists.hip; match_device.hpp is what all of them share.
#include "match_kernels.hpp"
#include "match_plan.hpp"              // fused_grid_of
#include "match_device.hpp"
#include "l2x1_segment_gfx950.inc"     // ESFM_L2X1_SEGMENT_ASM, ESFM_L2X1_KEEP: the one-product pass's main loop (gen_l2x1_segment_asm.py)

#include <float.h>
#include <type_traits>
#include <stdlib.h>
#include <string.h>

namespace esfm {

// The one-product pass's bound E1 on |(|q|^2 + score) - D| for every train row (D = the canonical float d^2; see the comment of
// l2_knn_bf16x1_kernel): operand rounding (rB T + (2 |q| + rB) R), the three-product pass's 2^-15 (|q|^2 + max |t|^2) for norms, MFMA
// accumulation and the canonical distance, and an ABSOLUTE floor of 2^-118 for whatever is flushed to zero or loses bits as a
// denormal on the way (64 products and sums below 2^-126 each, in the norms, the matrix pipe and the residual norms: descriptors of
// magnitude ~1e-20 and less).  Used by the first pass's certificate and ratio screen and by the threshold-filter pass: one formula.
__device__ __forceinline__ double l2x1_e1(double qn, double rq, double sqrt_tmax, double tmax, double rmax)
{
    return (rq * sqrt_tmax + (2.0 * sqrt(qn) + rq) * rmax) * (1.0 + 1.0 / 512.0) + (qn + tmax) * (1.0 / 32768.0) + 0x1p-118;
}

// ---------------------------------------------------------------------------------------------
// The ONE-product distance pass (round 3; reshaped in round 4): q.t ~ bf16(q).bf16(t), four v_mfma_f32_32x32x16_bf16 per 32 x 32 x 64
// tile instead of the three-product pass's twelve, a fused fold that keeps the K = ESFM_L2X1_KEEP smallest GROUP keys per lane and
// query set (groups of ESFM_L2X1_GRP results, the position in the low mantissa bits), and a ratio screen on those keys.
//  * the operand rounding is part of every bound.  With B = bf16(-2 q), a = bf16(t), rB = |(-2 q) - B|_2 and
//    rho_t = |t - a|_2 (both measured per row by l2_split_bf16_kernel):  |(-2 q).t - B.a| <= rB |t| + |B| rho_t, so
//        E1 = (rB T + (2 |q| + rB) R) (1 + 2^-9) + 2^-15 (|q|^2 + max|t|^2) + 2^-118,   T = max |t|,  R = max rho_t  over the train set,
//    bounds |(|q|^2 + score) - d^2| for every train row (l2x1_e1; the 2^-15 term is the three-product pass's whole budget: norms, MFMA
//    accumulation, the canonical distance).  For unit-norm descriptors E1 ~ 0.008 against 6e-5: K = 4 groups per lane push tau -- the
//    bound on every row outside the kept groups -- about as many ranks out as the larger error needs (simulated on M-SURF-4k:
//    K = 3 leaves 6.9 % of the queries uncertified, K = 4 0.6 %, K = 6 0.01 %; the reference's own
//    fountain descriptors 37 % / 15 % / 3.6 %);
//  * this kernel ends with the keys: the screen drops the queries that provably fail the ratio test, every other query leaves a
//    48-byte survivor entry.  l2_finish_kernel does the rest -- exact re-rank of the kept groups in the oracle's order, certificate,
//    threshold-filter pass over what stays uncertified, brute force of what overflows that, ratio test and compaction -- so the
//    result stays bit-identical to the oracle whatever the data;
//  * 512 queries per item (four sets of 32 per wave), a ring of two 32-KiB tiles of bf16(t) rows fed by LDS-DMA, 12-bit position
//    codes in the group keys: l2x1_segment_gfx950.inc (gen_l2x1_segment_asm.py) is the whole main loop.  Train sets the code cannot
//    number skip this pass (l2_x1_supported).  Since round 10 the loop itself runs on v_mfma_f32_16x16x32_bf16 -- eight K = 32
//    instructions per 32 x 32 x 64 tile, a wave's sets split into eight of 16 queries (ESFM_L2X1_QSETS), a fold group per lane
//    quarter, the quarters of a lane half merged at the end of the block -- and leaves the keys of the 32-query sets as before.
constexpr int l2x1_query_block_c = 128 * ESFM_L2X1_SETS;
// Cross-lane moves without an address register (__shfl_xor goes through ds_bpermute_b32, whose lane addresses the compiler hoists out
// of l2_knn_bf16x1_kernel's item loop and then has to keep in scratch memory across the main loop's asm block).
// max over the wave, the same value in every lane: rotations inside the rows of 16 lanes (DPP), then the four rows through SGPRs
__device__ __forceinline__ float wave_max_dpp(float x)
{
#define ESFM_ROR(n) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x120 + (n), 0xF, 0xF, false))
    x = fmaxf(x, ESFM_ROR(8)); x = fmaxf(x, ESFM_ROR(4)); x = fmaxf(x, ESFM_ROR(2)); x = fmaxf(x, ESFM_ROR(1));
#undef ESFM_ROR
    const int xi = __float_as_int(x);
    const float a = __int_as_float(__builtin_amdgcn_readlane(xi, 0)), b = __int_as_float(__builtin_amdgcn_readlane(xi, 16));
    const float c = __int_as_float(__builtin_amdgcn_readlane(xi, 32)), d = __int_as_float(__builtin_amdgcn_readlane(xi, 48));
    return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
// A 16-byte piece of a survivor entry.  COH: a write-through store (`sc1`), for entries that a finish workgroup of the SAME launch
// reads (l2_fused_kernel); the caller waits for it (s_waitcnt vmcnt(0)) before it counts its block.
template <bool COH>
__device__ __forceinline__ void st_entry(float4 *p, float4 v)
{
    if (COH) {
        const u32x4 w = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
        asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(w) : "memory");
    } else {
        *p = v;
    }
}
// One unit of the one-product pass's work: 512 queries (block qblk) of pair pi against the pair's whole train set.
struct X1Item { int32_t q_row0, nq, t_row0, nt; int64_t out_off; int32_t pi, qblk; };

// The pass's body, shared by l2_knn_bf16x1_kernel (bid = blockIdx.x, G = gridDim.x) and by the pass role of l2_fused_kernel (FUSED:
// G = n_blocks, one block per workgroup; the survivor entries leave through write-through stores and the block ends by adding 1 to
// pass_done[pair] -- the hand-over to the pair's finish workgroups of the same launch, see l2_fused_kernel).
template <bool FUSED>
__device__ __forceinline__ void l2_knn_bf16x1_body(const int bid, const int G, const float *__restrict__ desc, const u32x4 *__restrict__ hi_t,
                                                   const u32x4 *__restrict__ hi_q, const float *__restrict__ norms,
                                                   const float *__restrict__ rho_t, const float *__restrict__ rho_q,
                                                   const float2 *__restrict__ blkmax,
                                                   const PairDesc *__restrict__ pairs, const int32_t *__restrict__ blk_pair, int n_blocks,
                                                   int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist,
                                                   int32_t *__restrict__ counters, int flag_cap,
                                                   int32_t *__restrict__ surv_cnt, float4 *__restrict__ surv_list,
                                                   double ratio2m, int markers, int32_t *__restrict__ rejected,
                                                   int32_t *__restrict__ zero_a, int32_t *__restrict__ zero_b, int zero_n,
                                                   int32_t *__restrict__ zero_counters, int32_t *__restrict__ pass_done)
{
    // The per-pair list counters and the global counters exist twice: this launch fills one phase and zeroes the other for the NEXT
    // call (whose finish kernel needs them immutable while it runs) -- no memset launch, no zeroing pass in front of this one.
    if (threadIdx.x == 0) for (int e = bid; e < zero_n; e += G) { zero_a[e] = 0; zero_b[e] = 0; }
    if (bid == 0 && threadIdx.x < 16) zero_counters[threadIdx.x] = 0;
    constexpr int TT = ESFM_L2X1_TT, NS = ESFM_L2X1_SETS, K = ESFM_L2X1_KEEP, RING = ESFM_L2X1_RING;
    constexpr int QB = 128 * NS, HS = 8;                         // HS: 16-B slots per row of the hi images
    constexpr int TILE_BYTES = TT * HS * 16;
    static_assert(NS == 4, "operand list below is written for four query sets");
    static_assert(RING * TT == 2 * 256, "a thread stages two norms of the ring's first tiles");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    u32x4 *lds_tile = reinterpret_cast<u32x4 *>(smem);                         // [RING][TT * HS]: 64 KiB; the main loop leaves the keys here
    float *lds_norm = reinterpret_cast<float *>(smem + RING * TILE_BYTES);     // [RING][TT]   (the asm block assumes norms right behind the ring)
    float *lds_red = lds_norm + RING * TT;                                     // [2][8]: max |t|^2 and max rho_t of an item's train set, per wave
    float *lds_qn = lds_red + 16;                                              // [2][QB]: |q|^2 of an item's queries
    float *lds_rq = lds_qn + 2 * QB;                                           // [2][QB]: their residual norms

    // Nothing that depends on the thread index may stay live across the main loop's asm block (64 operand registers in, 184
    // clobbered: whatever the compiler keeps it keeps in scratch memory and fetches back in the tail's critical path): the thread's
    // coordinates are re-derived from an opaque copy of the index behind every pass of the block.
    int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    auto rederive = [&]() {
        int l;             // (the lane index from scratch: not even the thread index has to survive the block)
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        lane = l; wave = wave_s; tid = wave_s * 64 + l; j = l & 31; h = l >> 5;
    };
    const uint32_t lds_tile_addr = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds_tile);   // LDS byte address

    // ---- A workgroup takes the 512-query blocks b, b + G, b + 2 G, ... of the launch (G = gridDim.x, a multiple of 8 when there is
    // more than one round: all of a workgroup's blocks map to its XCD's contiguous range of the numbering, xcd_remap) and overlaps the
    // memory round trips of block k + 1's set-up -- query operands, the ring's first tiles, norms, maxima -- with block k's tail.
    // The launcher's default is G = number of blocks (one block per workgroup, the loop runs once): persistent workgroups, two per
    // CU, were measured 2 - 4 % SLOWER on the metric's workload and on config 4 (0.517 - 0.540 against 0.498 - 0.513 ms; 191.5 against
    // 187.9 ms) although they take a block's set-up from 16 us to one round trip -- the hardware's dispatcher refills a CU the
    // moment a workgroup leaves, whatever the other one is doing, and a lone workgroup runs its main loop 60 % faster, so the set-up
    // was hidden already; what the static schedule adds is the last round's imbalance.  (ESFM_X1_GRID sets G for measurements; what
    // the restructuring did buy is the short set-up itself: a block -> pair table instead of nine dependent loads of a binary search,
    // maxima from a per-256-row table, 5 % on the launch.)
    auto lb_of = [&](int k) -> int {
        const long long v = (long long)bid + (long long)k * G;
        return v < (long long)n_blocks ? xcd_remap((int)v, n_blocks) : -1;
    };
    auto make_item = [&](int lb, int pi) -> X1Item {
        X1Item it = {0, 0, 0, 0, 0, -1, 0};
        if (pi >= 0) {
            const PairDesc d = pairs[pi];
            it = X1Item{__builtin_amdgcn_readfirstlane(d.q_row0), __builtin_amdgcn_readfirstlane(d.nq), __builtin_amdgcn_readfirstlane(d.t_row0),
                        __builtin_amdgcn_readfirstlane(d.nt),
                        (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)d.out_off >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)d.out_off)),
                        pi, lb - __builtin_amdgcn_readfirstlane(d.blk_off2)};
        }
        return it;
    };

    // what the set-up of an item leaves in registers until its round trip is over
    constexpr int QS = ESFM_L2X1_QSETS;  // sets of 16 queries per wave: set 2 s + b = queries 16 b .. 16 b + 15 of the 32-query set s
    static_assert(QS == 2 * NS, "the main loop's 16-query sets halve the tail's 32-query sets");
    u32x4 bq[QS][2];                     // B operands: bf16(-2 q), this lane's 8 features of both 32-feature K-steps
    float st_norm[2], st_qn[2], st_rq[2], st_m, st_r;
    // set-up, part 1: every load of the item goes out (and the ring's first tiles: LDS-DMA, wave w rows [TT/4 w, TT/4 (w + 1)) of a
    // tile, 8 rows = 1 KiB per instruction, lane l -> row l >> 3, physical slot l & 7 = logical slot (l & 7) ^ (((row >> 1) & 3) | ((row >> 2) & 4)): the generator's lds_phys_slot)
    auto stage_issue = [&](const X1Item &it) {
        const int nt = it.nt, nq = it.nq;
        const int ntiles = (nt + TT - 1) / TT;
        const u32x4 trsrc = raw_buffer_rsrc(hi_t + (size_t)it.t_row0 * HS, (uint32_t)nt * (HS * 16));   // reads past it return 0
        // LDS under rows that are never transferred (past nt in the last tile) must not hold huge values (the previous item's keys)
        if (ntiles * TT != nt || ntiles < RING) {
            uint32_t z;          // (as a hoisted constant vector the zeros would be carried through the main loop's asm block)
            asm volatile("v_mov_b32 %0, 0" : "=v"(z));
            for (int i = tid; i < RING * TT * HS; i += 256) lds_tile[i] = u32x4{z, z, z, z};
            __syncthreads();
        }
#pragma unroll
        for (int b = 0; b < RING; ++b) {
#pragma unroll
            for (int i = 0; i < TT / 32; ++i) {
                const int row = wave_s * (TT / 4) + 8 * i + (lane >> 3);
                const int voff = row * (HS * 16) + (((lane & 7) ^ (((row >> 1) & 3) | ((row >> 2) & 4))) * 16);
                lds_dma_b128(lds_tile_addr + (uint32_t)(b * TILE_BYTES + (wave_s * (TT / 4) + 8 * i) * (HS * 16)), voff, trsrc, b * TILE_BYTES);
            }
        }
        const int qbase = it.qblk * QB + wave * 32 * NS;
        const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4 *>(hi_q + (size_t)it.q_row0 * HS), 0, nq * (HS * 16), 0x00020000);   // rows past nq read as zeros
#pragma unroll
        for (int s = 0; s < QS; ++s) {        // lane (n = lane & 15, c = lane >> 4): query n of the set, slot 4 ks + c of its row
            const int voff = (qbase + 16 * s + (lane & 15)) * (HS * 16) + (lane >> 4) * 16;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) bq[s][ks] = __builtin_amdgcn_raw_buffer_load_b128(qrsrc, voff + 64 * ks, 0, 0);
        }
        const float *__restrict__ tn = norms + it.t_row0;
        const float *__restrict__ tr = rho_t + it.t_row0;
        float big;           // (kBig out of an SGPR written here: as a hoisted constant it would be one more register to carry through the block)
        asm volatile("s_mov_b32 %0, 0x7f61b1e6" : "=s"(big));
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + 256 * u, q = it.qblk * QB + t;
            st_norm[u] = t < nt ? tn[t] : big;            // norms of the ring's first tiles, rows past nt as kBig
            st_qn[u] = norms[it.q_row0 + (q < nq ? q : 0)];
            st_rq[u] = rho_q[it.q_row0 + (q < nq ? q : 0)];
        }
        // max |t|^2 and max rho_t over the train set (the certificate's bound needs both in the tail): whole 256-row blocks of the
        // bank from l2_blockmax_kernel's table, the rows in front of and behind them one by one
        float m = 0.f, r = 0.f;
        const int t0 = it.t_row0, t1 = t0 + nt, b0 = (t0 + 255) >> 8, b1 = t1 >> 8;
        if (b0 >= b1) {
            for (int t = tid; t < nt; t += 256) { m = fmaxf(m, tn[t]); r = fmaxf(r, tr[t]); }      // < 512 rows
        } else {
            if (tid < b0 * 256 - t0) { m = fmaxf(m, tn[tid]); r = fmaxf(r, tr[tid]); }
            if (tid < t1 - b1 * 256) { m = fmaxf(m, norms[b1 * 256 + tid]); r = fmaxf(r, rho_t[b1 * 256 + tid]); }
            for (int b = b0 + tid; b < b1; b += 256) { const float2 v = blkmax[b]; m = fmaxf(m, v.x); r = fmaxf(r, v.y); }
        }
        st_m = m; st_r = r;
    };
    // set-up, part 2 (every load has landed): what the main loop and the tail read from LDS
    auto stage_commit = [&](int par) {
        lds_norm[tid] = st_norm[0]; lds_norm[tid + 256] = st_norm[1];
        lds_qn[par * QB + tid] = st_qn[0]; lds_qn[par * QB + tid + 256] = st_qn[1];
        lds_rq[par * QB + tid] = st_rq[0]; lds_rq[par * QB + tid + 256] = st_rq[1];
        const float m = wave_max_dpp(st_m), r = wave_max_dpp(st_r);
        if (lane == 0) { lds_red[par * 8 + wave] = m; lds_red[par * 8 + 4 + wave] = r; }
    };

    // items k, k + 1 and the pair index of item k + 2 (the table look-ups run two items ahead, the pair descriptors one)
    int lb_c = lb_of(0), lb_n = lb_of(1), lb_nn = lb_of(2);
    if (lb_c < 0) return;
    int pi_nn = lb_nn >= 0 ? blk_pair[lb_nn] : -1;
    X1Item cur = make_item(lb_c, blk_pair[lb_c]);
    X1Item nxt = make_item(lb_n, lb_n >= 0 ? blk_pair[lb_n] : -1);
    stage_issue(cur);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stage_commit(0);
    __syncthreads();

    static_assert(K == 4, "a survivor entry carries a lane's keys as one 16-byte piece");
    constexpr double kTrunc = 1.0001 / (double)(1 << (23 - ESFM_L2X1_CODE_BITS));     // the key's mantissa bits under the position code
    for (int k = 0;; ++k) {
        const int par = k & 1;
        const int nq = cur.nq, nt = cur.nt, pi = cur.pi;
        const int ntiles = (nt + TT - 1) / TT;
        if (ntiles > 0) {
            const u32x4 trsrc = raw_buffer_rsrc(hi_t + (size_t)cur.t_row0 * HS, (uint32_t)nt * (HS * 16));
            const u32x4 nrsrc = raw_buffer_rsrc(norms + cur.t_row0, (uint32_t)nt * 4u);
            asm volatile(ESFM_L2X1_SEGMENT_ASM
                         :
                         : "v"(bq[0][0]), "v"(bq[0][1]), "v"(bq[1][0]), "v"(bq[1][1]), "v"(bq[2][0]), "v"(bq[2][1]), "v"(bq[3][0]), "v"(bq[3][1]),
                           "v"(bq[4][0]), "v"(bq[4][1]), "v"(bq[5][0]), "v"(bq[5][1]), "v"(bq[6][0]), "v"(bq[6][1]), "v"(bq[7][0]), "v"(bq[7][1]),
                           "s"(ntiles), "s"(nt), "s"(trsrc), "s"(nrsrc), "s"(lds_tile_addr), "s"(wave_s)
                         : ESFM_L2X1_SEGMENT_CLOBBERS);
        }
        rederive();
        st_norm[0] = st_norm[1] = st_qn[0] = st_qn[1] = st_rq[0] = st_rq[1] = st_m = st_r = 0.f;      // (dead here: not carried through the block)
        // the block left this thread's keys in LDS: key i of set s at float (K s + i) * 256 + tid  (replaced when no tile ran)
        float keys[NS][K];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int i = 0; i < K; ++i) {
                keys[s][i] = reinterpret_cast<const float *>(smem)[(K * s + i) * 256 + tid];
            }
        }
        if (ntiles == 0) {
            float big;
            asm volatile("s_mov_b32 %0, 0x7f61b1e6" : "=s"(big));
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int i = 0; i < K; ++i) keys[s][i] = big;
        }
        const float tmax = fmaxf(fmaxf(lds_red[par * 8 + 0], lds_red[par * 8 + 1]), fmaxf(lds_red[par * 8 + 2], lds_red[par * 8 + 3]));
        const float rmax = fmaxf(fmaxf(lds_red[par * 8 + 4], lds_red[par * 8 + 5]), fmaxf(lds_red[par * 8 + 6], lds_red[par * 8 + 7]));
        const int qbase = cur.qblk * QB + wave * 32 * NS;
        float qn_s[NS], rq_s[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) { qn_s[s] = lds_qn[par * QB + wave * 32 * NS + 32 * s + j]; rq_s[s] = lds_rq[par * QB + wave * 32 * NS + 32 * s + j]; }
        __syncthreads();                  // the ring (and the keys in it) is free: every wave has left the main loop and read its keys

        // ---- the RATIO SCREEN (round 4), all that is left of this kernel's tail.  The reference keeps a query only if d0 < ratio d1
        // (feature_matching.cpp:133); everything else is dropped one kernel later, and on the metric's workload that is > 90 % of the
        // queries.  With k0 <= kb the two smallest of a query's 2 K group keys (two groups, hence two different train rows: the groups'
        // minima) and E1 the pass's bound on |(|q|^2 + score) - D| (D = the canonical float d^2), kTrunc the key's truncation:
        //     every train row has   D >= L0 = |q|^2 + k0 - kTrunc |k0| - E1        (k0 is the smallest key of all groups),
        //     two rows have         D <= U1 = |q|^2 + kb + kTrunc |kb| + E1,
        // so the nearest has D0 >= L0 and the second nearest D1 <= U1.  If L0 >= ratio^2 (1 + 2^-20) U1 then sqrtf(D0) >= ratio sqrtf(D1)
        // whatever the two roundings of sqrtf and the double product do (their relative error is < 2^-22 together): the query cannot
        // pass the test.  It gets a marker (train index -2) and nothing more is done for it.  A SURVIVOR leaves one 48-byte entry -- its
        // 2 K keys, its row, |q|^2 and E1 (as a float, rounded up) -- in the pair's slice of surv_list; l2_finish_kernel re-ranks the
        // survivors' kept groups exactly.  (Until the middle of round 4 the re-rank ran here, per wave, beside the other workgroup's
        // main loop whose VALU and LDS ports it shares: 0.06 - 0.075 of 0.605 ms, measured against a build without it; in a kernel of its
        // own it has the chip to itself.)  ratio2m = ratio^2 (1 + 2^-20); +inf switches the screen off (the knn2 entry points).
        const double sqrt_tmax = sqrt((double)tmax);
        int nsurv = 0;
        int myslot[NS];
        float e1_s[NS];
        uint32_t rejmask = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int qrow = qbase + 32 * s + j;
            const bool qvalid = qrow < nq;
            const float v0 = keys[s][0], v1 = keys[s][1];
            const float p0 = other_half(v0, h != 0), p1 = other_half(v1, h != 0);
            const float k0 = fminf(v0, p0), kb = fminf(fmaxf(v0, p0), fminf(v1, p1));     // the two smallest of the 2 K keys
            const double qn = (double)qn_s[s];
            const double e1 = l2x1_e1(qn, (double)rq_s[s], sqrt_tmax, (double)tmax, (double)rmax);
            const double L0 = qn + (double)k0 - e1 - fabs((double)k0) * kTrunc;
            const double U1 = qn + (double)kb + e1 + fabs((double)kb) * kTrunc;
            const bool rej = qvalid && (L0 >= ratio2m * U1);                              // false on NaN / inf: re-rank
            const bool surv = qvalid && !rej;
            const uint32_t m = (uint32_t)__ballot(surv);                                  // lanes 0 .. 31 (both halves agree)
            myslot[s] = surv ? nsurv + __popc(m & ((1u << j) - 1u)) : -1;
            float ef = (float)e1;
            if ((double)ef < e1) ef = __uint_as_float(__float_as_uint(ef) + 1u);          // rounded up: e1 > 0, and ef < e1 makes ef finite (NaN: every compare false)
            e1_s[s] = ef;
            if (rej) rejmask |= 1u << s;
            nsurv += __popc(m);
        }
        // the one round trip of the tail -- the survivors' place in the pair's slice -- and the next item's set-up share their latency
        int base = 0;
        if (nsurv > 0 && lane == 0) { base = atomicAdd(&surv_cnt[pi], nsurv); atomicAdd(&counters[2], nsurv); }
        const bool more = nxt.pi >= 0;
        const int lb_3 = lb_of(k + 3);
        int pi_3 = -1;
        X1Item nn = {0, 0, 0, 0, 0, -1, 0};
        if (more) {
            stage_issue(nxt);
            nn = make_item(lb_nn, pi_nn);
            pi_3 = lb_3 >= 0 ? blk_pair[lb_3] : -1;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (more) stage_commit(par ^ 1);
        // the tail's stores go out last: nothing waits for them (the main loop's first hand-over, eight steps on, finds them done)
        float fltmax;        // (FLT_MAX out of an SGPR written here, like kBig in the set-up)
        asm volatile("s_mov_b32 %0, 0x7f7fffff" : "=s"(fltmax));
        int minus2;
        asm volatile("s_mov_b32 %0, -2" : "=s"(minus2));
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int qrow = qbase + 32 * s + j;
            if (markers && h == 0 && ((rejmask >> s) & 1u)) {
                const size_t o = 2 * ((size_t)cur.out_off + qrow);
                *reinterpret_cast<int2 *>(knn_idx + o) = make_int2(minus2, minus2);
                *reinterpret_cast<float2 *>(knn_dist + o) = make_float2(fltmax, fltmax);
                if (rejected) {          // audit of the screen: what it dropped, on the global list
                    const int slot = atomicAdd(&counters[0], 1);
                    if (slot < flag_cap) { rejected[2 * slot] = pi; rejected[2 * slot + 1] = qrow; }
                }
            }
        }
        if (nsurv > 0) {
            base = __builtin_amdgcn_readfirstlane(base);
            float4 *ent = surv_list + 3 * ((size_t)cur.out_off + base);                   // (a pair's slice holds nq entries: it cannot overflow)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (myslot[s] >= 0) {
                    st_entry<FUSED>(ent + 3 * myslot[s] + h, make_float4(keys[s][0], keys[s][1], keys[s][2], keys[s][3]));
                    if (h == 0) st_entry<FUSED>(ent + 3 * myslot[s] + 2, make_float4(__int_as_float(qbase + 32 * s + j), qn_s[s], e1_s[s], 0.f));
                }
            }
        }
        if (FUSED) {
            // hand-over: every wave's entries (write-through) and the count's atomic are acknowledged, then the block is counted
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) __hip_atomic_fetch_add(&pass_done[pi], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!more) break;
        __syncthreads();                  // the next item's norms, maxima and query norms are in LDS, its first tile has landed
        cur = nxt; nxt = nn; lb_nn = lb_3; pi_nn = pi_3;
    }
}

__global__ __launch_bounds__(256, 2) void l2_knn_bf16x1_kernel(const float *__restrict__ desc, const u32x4 *__restrict__ hi_t,
                                                               const u32x4 *__restrict__ hi_q, const float *__restrict__ norms,
                                                               const float *__restrict__ rho_t, const float *__restrict__ rho_q,
                                                               const float2 *__restrict__ blkmax,
                                                               const PairDesc *__restrict__ pairs, const int32_t *__restrict__ blk_pair, int n_blocks,
                                                               int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist,
                                                               int32_t *__restrict__ counters, int flag_cap,
                                                               int32_t *__restrict__ surv_cnt, float4 *__restrict__ surv_list,
                                                               double ratio2m, int markers, int32_t *__restrict__ rejected,
                                                               int32_t *__restrict__ zero_a, int32_t *__restrict__ zero_b, int zero_n,
                                                               int32_t *__restrict__ zero_counters)
{
    l2_knn_bf16x1_body<false>(blockIdx.x, gridDim.x, desc, hi_t, hi_q, norms, rho_t, rho_q, blkmax, pairs, blk_pair, n_blocks, knn_idx, knn_dist, counters,
                              flag_cap, surv_cnt, surv_list, ratio2m, markers, rejected, zero_a, zero_b, zero_n, zero_counters, nullptr);
}

// ---------------------------------------------------------------------------------------------
// Everything behind the one-product pass's main loop and ratio screen in ONE launch (round 4; round 3 had three: a threshold-filter kernel,
// l2_rescan64_pairs_kernel, ratio_compact_kernel, and every launch boundary costs 5 - 10 us on this part):
//   (1) the exact RE-RANK of the screen's survivors (surv_cnt / surv_list: one 48-byte entry per survivor): the rows of the kept
//       groups in the oracle's order, the certificate, and the ratio verdicts that make most second neighbours unnecessary
//       (finish_rerank_vset below).  Uncertified and undecided queries go on the pair's list (unc_cnt / unc_list, knn_d2);
//   (2) the second pass over that list -- a THRESHOLD FILTER instead of a second top-k.  For such a query (1) has left the exact
//       two best of its candidates; U = an upper bound of the second-best d^2.  Every train row that can still change the answer
//       has d^2 <= U, hence a one-product score s <= U - |q|^2 + E1 (E1: l2x1_e1).  So: the same bf16(-2 q).bf16(t) product on the
//       matrix cores over the whole train set, a compare of every score with the query's threshold, the few rows that pass (0.1 -
//       1.2 per query on simulated data) evaluated exactly in the oracle's order and merged;
//   (3) the exact brute force of a chunk whose hit list overflows (adversarial inputs: every row inside the error);
//   (4) the ratio test and the ordered compaction of the pair's survivors (ratio_compact_pair).
// Work split: S workgroups per pair (blockIdx = slice * n_pairs + pair).  Stage (1) is shared: the pair's virtual sets of seven
// survivors are dealt out over the S x 4 waves.  Then every workgroup arrives at the pair's counter and the LAST one runs (2) - (4)
// alone (after the screen and the verdicts (2) and (3) see a handful of queries per launch).  Nobody waits for anybody: no
// assumption about which workgroups are resident.  What stage (1) writes for the last workgroup -- results, list entries -- travels
// through relaxed agent-scope atomics (write-through stores, L2-bypassing loads), not through agent-scope fences: on this part a
// release is a write-back of the XCD's whole L2, an acquire an invalidation, and hundreds of workgroups would queue for them.
constexpr int kFinThreads = 256, kFinCap = 2048, kFinWaves = kFinThreads / 64;

// exact 2-NN of up to 32 listed queries of one pair by the whole workgroup, the oracle's arithmetic and (distance, index) order:
// thread = train row (16 x 16 B in registers), the queries as LDS broadcasts; the 64 keys of a wave's rows are reduced to the two
// smallest by shuffles and merged into lane k's running pair for query k.  The fallback of the fallback: ~3 us per query.
__device__ __forceinline__ void finish_bruteforce_chunk(const float *__restrict__ desc, const PairDesc &pd, const int32_t *__restrict__ qrows /* LDS, nqc */,
                                                        int nqc, float4 (*s_q)[16] /* LDS [32][16] */, unsigned long long (*s_keys)[32][2] /* LDS [waves][32][2] */,
                                                        int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist)
{
    typedef unsigned long long u64;
    constexpr u64 kEmpty = ~0ull;
    auto key_of = [](float d, int t) { return d < FLT_MAX ? (((u64)__float_as_uint(d) << 32) | (u64)(uint32_t)t) : ~0ull; };   // FLT_MAX, +inf, NaN: never a neighbour
    auto insert2 = [](u64 &b0, u64 &b1, u64 k) {
        const u64 hi = k > b0 ? k : b0;
        b0 = k > b0 ? b0 : k;
        b1 = hi < b1 ? hi : b1;
    };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float4 *Q = reinterpret_cast<const float4 *>(desc + (size_t)pd.q_row0 * 64);
    const float4 *T = reinterpret_cast<const float4 *>(desc + (size_t)pd.t_row0 * 64);
    for (int e = tid; e < nqc * 16; e += kFinThreads) s_q[e >> 4][e & 15] = Q[(size_t)qrows[e >> 4] * 16 + (e & 15)];
    __syncthreads();
    u64 m0 = kEmpty, m1 = kEmpty;                    // lane k: query k's two best over this wave's rows
    for (int t0 = wave * 64; t0 < pd.nt; t0 += kFinThreads) {
        const int t = t0 + lane;
        float4 ta[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) ta[c] = t < pd.nt ? T[(size_t)t * 16 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < nqc; ++k) {
            float4 qa[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) qa[c] = s_q[k][c];
            const float d2 = l2sqr64_canonical_regs(qa, ta);
            u64 x0 = t < pd.nt ? key_of(sqrt_rn_f32(d2), t) : kEmpty, x1 = kEmpty;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const u64 y0 = __shfl_xor(x0, o), y1 = __shfl_xor(x1, o);
                insert2(x0, x1, y0);
                insert2(x0, x1, y1);
            }
            if (lane == k) { insert2(m0, m1, x0); insert2(m0, m1, x1); }
        }
    }
    if (lane < 32) { s_keys[wave][lane][0] = m0; s_keys[wave][lane][1] = m1; }
    __syncthreads();
    if (tid < nqc) {
        u64 x0 = kEmpty, x1 = kEmpty;
        for (int w = 0; w < kFinWaves; ++w) { insert2(x0, x1, s_keys[w][tid][0]); insert2(x0, x1, s_keys[w][tid][1]); }
        const size_t o = 2 * ((size_t)pd.out_off + qrows[tid]);
        const int i0 = (int)(uint32_t)x0, i1 = (int)(uint32_t)x1;
        st_coh_i(knn_idx + o, i0); st_coh_i(knn_idx + o + 1, i1);           // (read back by the ratio stage past the L2)
        st_coh_f(knn_dist + o, i0 >= 0 ? __uint_as_float((uint32_t)(x0 >> 32)) : FLT_MAX);
        st_coh_f(knn_dist + o + 1, i1 >= 0 ? __uint_as_float((uint32_t)(x1 >> 32)) : FLT_MAX);
    }
    __syncthreads();
}

// Stage (1) for ONE virtual set of up to QV = 7 survivors, by one wave, DENSE: eight lanes per query.  In round r lane l (query slot
// l >> 3, i = l & 7) evaluates row i of the query's group of rank r -- a kept group is eight rows: two runs of four, eight apart -- so
// a round is ONE batch of row transfers into the wave's 16-KiB landing zone (56 candidate rows, 16 lanes per 256-B row: every cache
// line touched once; round 0 also brings the seven query rows, which stay in the slots 56 .. 62) and every lane computes one
// distance, straight from LDS.
//  * a candidate is ONE 64-bit key, (bits of the distance) << 32 | train row: key order is the oracle's (distance, index) order; the
//    two best of a query's eight are reduced over its eight lanes by min / max exchanges and merged into (m0, m1), which all eight
//    lanes carry.  The bounds need d^2, not the canonical float D the distance is the root of: sqrtf is correctly rounded, so D lies
//    in d^2 (1 -+ 2^-22), and each use takes the side that keeps it conservative;
//  * round 0 needs the two smallest of the 2 K keys only (its group, the verdict's bound): the heads of the two sorted key lists; the
//    ranking by counting is made in the later rounds -- when a query is still undecided after its best group.
// Between the rounds the ratio test may already be DECIDED (the match entry points only; the reference emits queryIdx, trainIdx and d0
// of a survivor, never d1): with (m0, m1) the exact two best of the rows evaluated so far and lrest a lower bound on the D of every
// other row (the groups of the next ranks, everything outside the kept groups; rows of a group skipped as `cannot` are farther than
// the two rows that bound U anyway),
//   verdict 1, cannot pass:  D1 <= m1 and D0 >= min(m0, lrest) >= ratio^2 (1 + 2^-20) m1;
//   verdict 2, passes:       lrest > m0 (1 + 2^-20), so m0 IS the nearest row, and m0 (1 + 2^-18) < ratio^2 (1 + 2^-20) min(m1, lrest),
//                            so sqrtf(m0) < ratio sqrtf(D1) whatever the second nearest turns out to be -- it is not looked for
//                            (second index -3: "not determined, the test passes").
// On the metric's workload nearly every survivor is a true match whose best group alone decides it: one transfer round trip.  A
// query that ends neither certified nor decided goes on the pair's list for the threshold filter, with an upper bound of its
// second-best d^2 as the filter's threshold.
struct FinRerankArgs {
    const float4 *ent;                 // the pair's survivor entries
    __amdgpu_buffer_rsrc_t ersrc;      // ... as a buffer (COH: the entries were written by pass blocks of this launch, read with `sc1` loads)
    int nsv, per;                      // ... their number; entries per virtual set (<= kFinQV)
    PairDesc pd; int p;
    __amdgpu_buffer_rsrc_t frsrc_t, frsrc_q;   // buffer descriptors of the train / query set's float rows (rows past a set read as zeros)
    double ratio2m;
    int32_t *knn_idx; float *knn_dist; float *knn_d2;
    int32_t *unc_cnt, *unc_list;       // the pair's list of queries for the threshold filter
    int32_t *counters, *audit_unc, *audit_rej; int flag_cap;
};
constexpr int kFinQV = 7;
// What the re-rank keeps of a query between two rounds: its survivor entry (two half-waves' K keys, row / |q|^2 / E1) and the exact
// two best rows so far.  64 bytes.
struct FinPending { float4 ka, kb, mi; unsigned long long m0, m1; };
constexpr int kFinPend = 112;        // pending queries of a wave (16 virtual sets' worth): 7 KiB of LDS per wave

// Stage (1) for ONE WAVE's share of a pair's survivors: the virtual sets v0, v0 + vstride, ... < nvs.
// Round 5 -- COMPACTION BY ROUND.  Until then a virtual set of seven ran all of its rounds together and advanced at the pace of its
// slowest query: on real, clustered descriptors (M-SURF-4k-hard) a set took 3.24 rounds for queries that needed 1.8 on average, and
// every round costs the same whatever it holds.  Now round 0 runs over the wave's sets as before; a query that is neither decided
// nor out of groups afterwards is parked in the wave's LDS list (FinPending); the later rounds are run over that list, seven
// queries at a time, each round re-packing what is still undecided.  A query's arithmetic depends on nothing but its own state, so
// the results are bit-identical; on the metric's workload (one set per wave, 1.6 rounds) nothing changes.
template <bool SINGLE, bool COH>
__device__ __forceinline__ void finish_rerank_wave(const FinRerankArgs &A, int v0, int vstride, int nvs, FinPending *pend)
{
    typedef unsigned long long u64;
    constexpr int K = ESFM_L2X1_KEEP, GRP = ESFM_L2X1_GRP, NG = 16 / GRP, QV = kFinQV;
    static_assert(K == 4 && GRP == 8, "an entry carries 2 x 4 keys; eight lanes evaluate the eight rows of a group");
    constexpr u64 kNone = ~0ull;
    constexpr float kBig = 3.0e38f;
    constexpr uint32_t kCodeMask = (1u << ESFM_L2X1_CODE_BITS) - 1u;
    constexpr double kTrunc = 1.0001 / (double)(1 << (23 - ESFM_L2X1_CODE_BITS));
    const int lane = threadIdx.x & 63;
    const int ri = (lane & 3) + 8 * ((lane >> 2) & 1);     // row of the group this lane evaluates (lanes 8 e .. 8 e + 7: entry e of the virtual set)
    const int nt = A.pd.nt, nq = A.pd.nq;
    const double ratio2m = A.ratio2m;
    const bool screen = ratio2m < 1.0e300;
    auto row0_of = [&](float key, int hh) {
        const int code = (int)(__float_as_uint(key) & kCodeMask);
        return key < 1.0e38f ? (code / NG) * 32 + (32 / NG) * (code % NG) + 4 * hh : -1;
    };
    auto kmin = [](u64 x, u64 y) { return x < y ? x : y; };
    auto kmax = [](u64 x, u64 y) { return x < y ? y : x; };
    // ---- the state of the query this lane works for (the same in its eight lanes)
    int nv = 0;                                                  // wave-uniform: queries of the current set
    bool qvalid = false;
    int qrow = 0;
    double qn = 0.0, e1 = 0.0, U = 0.0;
    float a_[4], b_[4], tau = kBig;
    float4 s_ka, s_kb, s_mi;                                     // (the entry as it came: what is parked when the query stays undecided)
    u64 m0 = kNone, m1 = kNone;                                  // the query's exact two best so far
    int verdict = 0;
    // the 2 K keys' order, once per parked query (round 6): position p of the ascending (key, index) order holds key number
    // (ord >> 3 p) & 7 (0 .. 3: half 0's keys, 4 .. 7: half 1's); kOrdValid marks a computed order.  It travels with the parked query in
    // the entry's unused fourth word.  (Until then every later round ranked the eight keys by counting TWICE -- once to decide whether
    // to park, once when the round ran: 8 x 7 compares each, a third of the later rounds' instructions on clustered descriptors.)
    constexpr int kOrdValid = 1 << 24;
    int ord = 0;
    auto take = [&](float4 ka, float4 kb4, float4 mi, bool valid, u64 b0, u64 b1) {
        s_ka = ka; s_kb = kb4; s_mi = mi;
        ord = __float_as_int(mi.w);                                // 0 in an entry as the pass wrote it
        qvalid = valid;
        qrow = qvalid ? __float_as_int(mi.x) : nq;               // nq: past the descriptor, zeros
        qn = (double)mi.y; e1 = (double)mi.z;
        a_[0] = qvalid ? ka.x : kBig; a_[1] = qvalid ? ka.y : kBig; a_[2] = qvalid ? ka.z : kBig; a_[3] = qvalid ? ka.w : kBig;
        b_[0] = qvalid ? kb4.x : kBig; b_[1] = qvalid ? kb4.y : kBig; b_[2] = qvalid ? kb4.z : kBig; b_[3] = qvalid ? kb4.w : kBig;
        tau = fminf(a_[3], b_[3]);
        // the two smallest keys (ties: half 0 first -- any fixed rule will do, the eight lanes only have to agree)
        const bool c0 = a_[0] <= b_[0];
        const float r1k = fminf(c0 ? a_[1] : a_[0], c0 ? b_[0] : b_[1]);
        U = (qn + (double)r1k + e1 + fabs((double)r1k) * kTrunc) * (1.0 + 1.0 / 1048576.0);
        m0 = b0; m1 = b1; verdict = 0;
    };
    // the group of rank r among the query's 2 K keys (by counting), and the smallest key behind it
    auto rank_group = [&](int r, float &key, int &row0, float &nkey) {
        key = kBig; nkey = kBig; row0 = -1;
#pragma unroll
        for (int x = 0; x < 2 * K; ++x) {
            const float kx = x < K ? a_[x & 3] : b_[x & 3];
            int rank = 0;
#pragma unroll
            for (int y = 0; y < 2 * K; ++y) {
                const float ky = y < K ? a_[y & 3] : b_[y & 3];
                if (y != x) rank += (ky < kx || (ky == kx && y < x)) ? 1 : 0;
            }
            if (rank == r) { key = kx; row0 = row0_of(kx, x < K ? 0 : 1); }
            if (rank == r + 1) nkey = kx;
        }
    };
    auto compute_ord = [&]() {
        int o = kOrdValid;
#pragma unroll
        for (int x = 0; x < 2 * K; ++x) {
            const float kx = x < K ? a_[x & 3] : b_[x & 3];
            int rank = 0;
#pragma unroll
            for (int y = 0; y < 2 * K; ++y) {
                const float ky = y < K ? a_[y & 3] : b_[y & 3];
                if (y != x) rank += (ky < kx || (ky == kx && y < x)) ? 1 : 0;
            }
            o |= x << (3 * rank);
        }
        ord = o;
    };
    auto key_number = [&](int x) {           // key number x of the query's eight (a chain of selects: a register array indexed by data would go to scratch)
        // (through opaque copies: hipcc otherwise folds the chain into an indexed load from a stack copy of the keys, the kernel's only
        // scratch memory -- which in l2_fused_kernel every pass workgroup would be given as well)
        float k0 = a_[0], k1 = a_[1], k2 = a_[2], k3 = a_[3], k4 = b_[0], k5 = b_[1], k6 = b_[2], k7 = b_[3];
        asm volatile("" : "+v"(k0), "+v"(k1), "+v"(k2), "+v"(k3), "+v"(k4), "+v"(k5), "+v"(k6), "+v"(k7));
        float k = k0;
        k = x == 1 ? k1 : k; k = x == 2 ? k2 : k; k = x == 3 ? k3 : k;
        k = x == 4 ? k4 : k; k = x == 5 ? k5 : k; k = x == 6 ? k6 : k; k = x == 7 ? k7 : k;
        return k;
    };
    // rank_group from the stored order: the same (key, row0, nkey)
    auto ordered_group = [&](int r, float &key, int &row0, float &nkey) {
        const int x = (ord >> (3 * r)) & 7;
        key = key_number(x);
        row0 = row0_of(key, x >> 2);
        nkey = r + 1 < 2 * K ? key_number((ord >> (3 * (r + 1))) & 7) : kBig;
    };
    // does a round on the group (key, row0) still have to look at rows?  (false once: false for every later rank -- the keys ascend)
    auto wanted = [&](float key, int row0) {
        const bool cannot = (qn + (double)key - e1 - fabs((double)key) * kTrunc) > U;   // false on NaN: re-rank
        return row0 >= 0 && qvalid && !cannot && verdict == 0;
    };
    // one round: the group (key, row0) of the query, nkey = the smallest key of the groups the later rounds would fetch
    auto do_round = [&](bool last, float key, int row0, float nkey) __attribute__((always_inline)) {
        const bool need = wanted(key, row0);
        if (__ballot(need) == 0ull) return;
        const int trow = row0 + ri;
        const int rsel = need ? trow : nt;                       // nt: past the descriptor, zeros
        // 16 lanes fetch one 256-B row INTO REGISTERS: load i brings the rows of the lanes 4 i .. 4 i + 3 (i < 2 nv: the candidate
        // rows), lane l of the wave its 16-byte piece l & 15 of the row of lane 4 i + (l >> 4); the query rows of the entries
        // 0 .. nv - 1 the same way (every 16-lane row holds a copy).  Distances across the 16 lanes of a row in the oracle's order
        // (l2sqr64_canonical_row16), handed to the lane that owns the candidate by one ds_bpermute per load.
        // (Until the end of round 4 the rows landed in a 16-KiB LDS zone per wave -- LDS-DMA -- and every lane summed its own row
        // from there: eight waves per CU, 56 queries in flight, and the zone idle for 60 % of a virtual set's 10 us.  Registers
        // hold the same 14 KiB per wave, but sixteen waves fit a CU.)
        int rs[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) rs[i] = __builtin_amdgcn_ds_bpermute((4 * i + (lane >> 4)) * 4, rsel) * 256 + (lane & 15) * 16;
        u32x4 qv[QV], rowv[14];
#pragma unroll
        for (int e = 0; e < QV; ++e)
            if (e < nv) qv[e] = __builtin_amdgcn_raw_buffer_load_b128(A.frsrc_q, __builtin_amdgcn_readlane(qrow, 8 * e) * 256 + (lane & 15) * 16, 0, 0);
#pragma unroll
        for (int i = 0; i < 14; ++i)
            if (i < 2 * nv) rowv[i] = __builtin_amdgcn_raw_buffer_load_b128(A.frsrc_t, rs[i], 0, 0);
        float da = 0.f;
        float got[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) {
            got[i] = 0.f;
            if (i < 2 * nv) {
                const float dr = l2sqr64_canonical_row16(qv[i >> 1], rowv[i]);
                got[i] = __int_as_float(__builtin_amdgcn_ds_bpermute(((lane & 3) * 16 + 15) * 4, __float_as_int(dr)));
            }
            __builtin_amdgcn_sched_barrier(0);       // (one row group at a time: interleaved, the fourteen chains took 296 registers)
        }
#pragma unroll
        for (int i = 0; i < 14; ++i)
            if ((lane >> 2) == i) da = got[i];
        // this lane's candidate as a key (+inf, NaN, rows past the set: none); then the two best of the query's eight lanes
        const float dda = sqrt_rn_f32(da);
        u64 c0k = (need && trow < nt && dda < FLT_MAX) ? (((u64)__float_as_uint(dda) << 32) | (u64)(uint32_t)trow) : kNone, c1k = kNone;
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            const u64 p0 = __shfl_xor(c0k, o), p1 = __shfl_xor(c1k, o);
            const u64 lo = kmin(c0k, p0), hi = kmax(c0k, p0);
            c1k = kmin(hi, kmin(c1k, p1));
            c0k = lo;
        }
        {
            const u64 lo = kmin(m0, c0k), hi = kmax(m0, c0k);
            m1 = kmin(hi, kmin(m1, c1k));
            m0 = lo;
        }
        if (screen && !last) {
            const float nk = fminf(nkey, tau);                   // the smallest key of anything not evaluated yet
            const double lrest = qn + (double)nk - e1 - fabs((double)nk) * kTrunc;
            const double d0 = (double)__uint_as_float((uint32_t)(m0 >> 32)), d1 = (double)__uint_as_float((uint32_t)(m1 >> 32));
            const double m0lo = d0 * d0 * (1.0 - 1.0 / 4194304.0), m0hi = d0 * d0 * (1.0 + 1.0 / 4194304.0);
            const double m1lo = d1 * d1 * (1.0 - 1.0 / 4194304.0), m1hi = d1 * d1 * (1.0 + 1.0 / 4194304.0);
            const bool two = m1 != kNone;
            const double r1 = ratio2m * m1hi;
            const bool fail = two && lrest >= r1 && m0lo >= r1;                                                    // (every compare false on NaN)
            const double dlo = lrest < m1lo ? lrest : m1lo;
            const bool pass = two && lrest > m0hi * (1.0 + 1.0 / 1048576.0) && m0hi * (1.0 + 1.0 / 262144.0) < ratio2m * dlo;
            if (verdict == 0 && qvalid) verdict = fail ? 1 : (pass ? 2 : 0);
        }
    };
    // the query is through: its record, and -- neither certified nor decided -- its place on the pair's list for the threshold filter
    auto finalize = [&]() {
        const size_t o = 2 * ((size_t)A.pd.out_off + qrow);
        const bool one = m0 != kNone, two = m1 != kNone;
        const double d0 = (double)__uint_as_float((uint32_t)(m0 >> 32)), d1 = (double)__uint_as_float((uint32_t)(m1 >> 32));
        const double m0lo = d0 * d0 * (1.0 - 1.0 / 4194304.0), m1hi = d1 * d1 * (1.0 + 1.0 / 4194304.0);
        bool certified = (tau >= 1.0e38f);       // the empty-slot sentinel: every train row is a candidate (a NaN tau compares false)
        double lmiss = 0.0;
        if (!certified && two) {
            const double eps = e1 + fabs((double)tau) * kTrunc;
            lmiss = qn + (double)tau - eps;                                                    // every row outside the kept groups has D >= lmiss
            certified = lmiss > m1hi * (1.0 + 1.0 / 2097152.0);     // false on NaN (e1 of non-finite rows)
        }
        // Not certified, but the ratio test is already decided: the true second-nearest has D1 <= m1, the true nearest
        // D0 >= min(m0, lmiss); if that is >= ratio^2 (1 + 2^-20) m1 the query cannot pass whatever the other rows are.
        const bool lost = verdict == 1 || (verdict == 0 && !certified && two && lmiss >= ratio2m * m1hi && m0lo >= ratio2m * m1hi);   // false on NaN
        if (lost) {
            st_coh_i(A.knn_idx + o, -2); st_coh_i(A.knn_idx + o + 1, -2);
            st_coh_f(A.knn_dist + o, FLT_MAX); st_coh_f(A.knn_dist + o + 1, FLT_MAX);
            if (A.audit_rej) {       // audit of the screen: what it dropped, on the global list
                const int slot = atomicAdd(&A.counters[0], 1);
                if (slot < A.flag_cap) { A.audit_rej[2 * slot] = A.p; A.audit_rej[2 * slot + 1] = qrow; }
            }
        } else {
            st_coh_i(A.knn_idx + o, one ? (int)(uint32_t)m0 : -1); st_coh_i(A.knn_idx + o + 1, verdict == 2 ? -3 : (two ? (int)(uint32_t)m1 : -1));
            st_coh_f(A.knn_dist + o, one ? __uint_as_float((uint32_t)(m0 >> 32)) : FLT_MAX);
            st_coh_f(A.knn_dist + o + 1, two ? __uint_as_float((uint32_t)(m1 >> 32)) : FLT_MAX);
        }
        if (!certified && !lost && verdict == 0) {
            atomicAdd(&A.counters[1], 1);
            float u2 = two ? (float)m1hi : FLT_MAX;              // the threshold filter's bound: an upper bound of the exact second best so far
            if (two && (double)u2 < m1hi) u2 = nextafterf(u2, FLT_MAX);
            st_coh_f(A.knn_d2 + A.pd.out_off + qrow, u2);
            if (A.audit_unc) {       // audit of THIS pass's certificate: its failures on the global list
                const int slot = atomicAdd(&A.counters[0], 1);
                if (slot < A.flag_cap) { A.audit_unc[2 * slot] = A.p; A.audit_unc[2 * slot + 1] = qrow; }
            }
            const int k = __hip_atomic_fetch_add(&A.unc_cnt[A.p], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            st_coh_i(A.unc_list + A.pd.out_off + k, qrow);
        }
    };
    // after round r: a query whose group of rank r + 1 is still wanted is parked at pend[*npend ...] (the leaders of the wave's
    // queries take consecutive slots), every other one is finalised
    auto park_or_finalize = [&](int r, int *npend) {
        float key = kBig, nkey; int row0 = -1;
        if (r + 1 < 2 * K) {
            if (!(ord & kOrdValid)) compute_ord();
            ordered_group(r + 1, key, row0, nkey);
        }
        const bool leader = qvalid && (lane & 7) == 0;
        const bool again = leader && r + 1 < 2 * K && wanted(key, row0);
        const unsigned long long bal = __ballot(again);
        if (again) {
            FinPending &dst = pend[*npend + __popcll(bal & ((1ull << lane) - 1ull))];
            dst.ka = s_ka; dst.kb = s_kb; dst.mi = make_float4(s_mi.x, s_mi.y, s_mi.z, __int_as_float(ord)); dst.m0 = m0; dst.m1 = m1;
        }
        if (leader && !again) finalize();
        *npend += __popcll(bal);
    };
    // the later rounds over the parked queries, seven at a time, re-packed in place after every round (a set is read into
    // registers before anything of it is written back, and what is written never passes what has been read)
    auto drain = [&](int npend) {
#pragma unroll 1
        for (int r = 1; r < 2 * K && npend > 0; ++r) {
            int nout = 0;
#pragma unroll 1
            for (int k = 0; k < npend; k += QV) {
                nv = min(QV, npend - k);
                const int e = lane >> 3;
                const FinPending src = pend[k + min(e, nv - 1)];
                __builtin_amdgcn_wave_barrier();
                take(src.ka, src.kb, src.mi, e < nv, src.m0, src.m1);
                float key, nkey; int row0;
                ordered_group(r, key, row0, nkey);                 // (a parked query carries its order)
                do_round(r + 1 == 2 * K, key, row0, nkey);
                park_or_finalize(r, &nout);
                __builtin_amdgcn_wave_barrier();
            }
            npend = nout;
        }
    };
    // ---- round 0 over the wave's virtual sets (the next set's entries are loaded while this one waits for its rows)
    const int eq = lane >> 3 < QV ? lane >> 3 : QV - 1;
    auto entry_of = [&](int v, int part) {
        const int e = v * A.per + eq;
        if (COH) {       // (aux 16: sc1 -- served past this XCD's L2; entries past the pair's count read as zeros)
            const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(A.ersrc, (v < nvs && e < A.nsv) ? e * 48 + part * 16 : 0x7fffffff, 0, 16);
            return make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
        }
        return (v < nvs && e < A.nsv) ? A.ent[3 * (size_t)e + part] : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    int npend = 0;
    int v = v0;
    float4 e0 = entry_of(v, 0), e1v = entry_of(v, 1), e2 = entry_of(v, 2);
#pragma unroll 1
    for (; v < nvs; v += vstride) {
        const float4 n0 = entry_of(v + vstride, 0), n1 = entry_of(v + vstride, 1), n2 = entry_of(v + vstride, 2);
        nv = min(A.per, A.nsv - v * A.per);                      // wave-uniform: queries of this virtual set
        take(e0, e1v, e2, (lane >> 3) < nv, kNone, kNone);
        {
            const bool c0 = a_[0] <= b_[0];
            const float r0k = c0 ? a_[0] : b_[0];
            const float r1k = fminf(c0 ? a_[1] : a_[0], c0 ? b_[0] : b_[1]);
            do_round(false, r0k, row0_of(r0k, c0 ? 0 : 1), r1k);
        }
        if (SINGLE) {
            // the wave's only set (the metric's workload: a pair's survivors are one set per wave): its later rounds straight away, in
            // the registers the state is in -- parking and re-loading five queries costs more than their idle lanes do.  (SINGLE is a
            // template parameter, the kernel branches once per wave: compiled into one body with the parking form, this path -- round
            // 4's, instruction for instruction -- came out 3 us slower per launch.)
#pragma unroll 1
            for (int r = 1; r < 2 * K; ++r) {
                float key, nkey; int row0;
                rank_group(r, key, row0, nkey);
                if (__ballot(wanted(key, row0)) == 0ull) break;
                do_round(r + 1 == 2 * K, key, row0, nkey);
            }
            if (qvalid && (lane & 7) == 0) finalize();
        } else {
            park_or_finalize(0, &npend);
            if (npend + QV > kFinPend) { __builtin_amdgcn_wave_barrier(); drain(npend); npend = 0; }
        }
        e0 = n0; e1v = n1; e2 = n2;
    }
    if (!SINGLE) {
        __builtin_amdgcn_wave_barrier();
        drain(npend);
    }
}

// Stage (2)'s sweep over a wave's share [st0, st1) of the train set's 32-row steps, for the (up to) 64 queries of a sweep: the same
// bf16(-2 q) . bf16(t) product as the pass on the matrix cores, every score compared with its query's threshold, the rows that pass
// appended to the workgroup's hit list ((query slot) << 21 | train row).  Lane j of either half-wave owns the queries j and 32 + j.
// Branch-free loads through buffer descriptors (rows past nt read as zeros; their norms become kBig), the next step's eight loads in
// flight during this step's MFMAs.  (The first version guarded every load with `row < nt`: hipcc turned each into a branch and waited
// for every fragment before its MFMA -- 6.5 us per step.)  A function of its OWN, not inlined: inside l2_finish_kernel's body the
// register allocator -- 168 registers for three workgroups per CU, cut for the re-rank -- kept the operands of this loop in scratch
// memory and re-loaded them in front of every matrix instruction (6 us per step on M-SURF-4k-hard, round 5).
// (l2_fused_kernel's finish role, cut for 256 registers, takes the body INLINE: its operands then never pass through scratch memory,
// which the fused kernel's pass role must not be made to allocate.)
__device__ __forceinline__ void finish_filter_sweep_body(const u32x4 *hi_rows /* the train set's bf16 images */, const float *tn /* its |row|^2 */, int st0, int st1, int nt_, int j,
                                                         int h, bool two, const bf16x8 (&bq_)[2][4], const float (&thr2_)[2], int *s_nhit, int *s_h)
{
    constexpr int HS = 8, CAP = kFinCap;
    constexpr float kBig = 3.0e38f;
    // (arguments of a non-inlined function arrive in vector registers: the descriptors are rebuilt from values the compiler can see
    // are wave-uniform, or every buffer load becomes a waterfall loop)
    auto uniform_ptr = [](const void *p) {
        const unsigned long long v = (unsigned long long)(uintptr_t)p;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return reinterpret_cast<void *>((uintptr_t)(((unsigned long long)hi << 32) | lo));
    };
    const int nt = __builtin_amdgcn_readfirstlane(nt_);
    st0 = __builtin_amdgcn_readfirstlane(st0); st1 = __builtin_amdgcn_readfirstlane(st1);
    const __amdgpu_buffer_rsrc_t rsrc_t = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(hi_rows), 0, nt * (HS * 16), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_n = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(tn), 0, nt * 4, 0x00020000);
    // the query operands and thresholds arrive by reference, i.e. in the caller's scratch memory: into registers ONCE (left as
    // references, every matrix instruction of every step re-loaded its operand with a flat load: 2.7 us per step)
    bf16x8 lbq[2][4]; float lthr[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float tv = thr2_[u];
        asm volatile("" : "+v"(tv));
        lthr[u] = tv;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 v = __builtin_bit_cast(u32x4, bq_[u][ks]);
            asm volatile("" : "+v"(v));
            lbq[u][ks] = __builtin_bit_cast(bf16x8, v);
        }
    }
    const bf16x8 (&bq)[2][4] = lbq; const float (&thr2)[2] = lthr;
    auto load_step = [&](int st, u32x4 (&a)[4], u32x4 (&nv)[4]) {
        const int voff = (st * 32 + j) * (HS * 16) + h * 16;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a[ks] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_t, voff + 32 * ks, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) nv[g] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_n, (st * 32 + 8 * g + 4 * h) * 4, 0, 0);
    };
    // one step: scores of the step's 32 rows against the sweep's queries, the rows under a query's threshold appended to the hit list
    auto step = [&](int st, const u32x4 (&ca)[4], const u32x4 (&cn)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u == 1 && !two) break;                       // (workgroup-uniform: a sweep of at most 32 queries runs one accumulator)
            floatx16 acc;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int x = 0; x < 4; ++x) acc[4 * g + x] = (st * 32 + 8 * g + 4 * h + x) < nt ? __uint_as_float(cn[g][x]) : kBig;
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ca[ks]), bq[u][ks], acc, 0, 0, 0);
            float m = kBig;
#pragma unroll
            for (int r = 0; r < 16; ++r) m = fminf(m, acc[r]);       // (fminf drops NaN scores: never neighbours)
            if (__ballot(m <= thr2[u]) != 0ull) {
                uint32_t mask = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int t = st * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    mask |= (acc[r] <= thr2[u] && t < nt) ? (1u << r) : 0u;
                }
                if (mask) {                         // one atomic per lane with hits, then its slots in order
                    int k = atomicAdd(s_nhit, __popc(mask));
                    while (mask) {
                        const int r = __ffs(mask) - 1;
                        mask &= mask - 1;
                        if (k < CAP) s_h[k] = ((32 * u + j) << 21) | (st * 32 + (r & 3) + 8 * (r >> 2) + 4 * h);
                        ++k;
                    }
                }
            }
        }
    };
    // two operand sets: the loads of step s + 2 are issued right behind the use of step s.  (A ring of three was measured: the third
    // set pushes two of the query operands into scratch memory, re-loaded in front of their matrix instructions: slower.)
    u32x4 a0[4], n0[4], a1[4], n1[4];
    load_step(st0, a0, n0); load_step(st0 + 1, a1, n1);      // (steps past the set read zeros; past st1 they are not used)
    for (int st = st0; st < st1; st += 2) {
        step(st, a0, n0);
        if (st + 2 < st1) load_step(st + 2, a0, n0);
        if (st + 1 < st1) { step(st + 1, a1, n1); if (st + 3 < st1) load_step(st + 3, a1, n1); }
    }
}

__device__ __noinline__ void finish_filter_sweep(const u32x4 *hi_rows, const float *tn, int st0, int st1, int nt_, int j, int h, bool two,
                                                 const bf16x8 (&bq_)[2][4], const float (&thr2_)[2], int *s_nhit, int *s_h)
{
    finish_filter_sweep_body(hi_rows, tn, st0, st1, nt_, j, h, two, bq_, thr2_, s_nhit, s_h);
}

constexpr size_t kFinTailLds = 8192 + 8192 + (size_t)kFinWaves * 32 * 2 * 8;        // the buffers of stages (2) - (4)
constexpr size_t kFinLdsBytes = kFinTailLds + (size_t)kFinWaves * kFinPend * sizeof(FinPending);   // + the re-rank's parked queries (its rows live in registers)

// the small per-workgroup variables of the finish stages (static LDS in l2_finish_kernel; behind the dynamic part in l2_fused_kernel,
// whose pass role wants the ring at LDS address 0 as in its own kernel)
struct FinShared {
    int s_nhit, s_last;
    float s_red[2 * kFinWaves];
    int s_qrows[64];
    unsigned long long s_best[2][64];            // stage 2: the running (distance, index) keys of a sweep's queries
    int s_wave[kFinWaves], s_base;
};
constexpr long long kHandoverTicks = 200000000;  // the fused finish role's bound on its wait for the pair's pass blocks: 2 s of the 100-MHz wall clock

// The finish stages' body, shared by l2_finish_kernel (fb = blockIdx.x of nfb = gridDim.x) and the finish role of l2_fused_kernel
// (FUSED: fb counts from the role's first workgroup; the pair's pass blocks run in the SAME launch, see the wait below).
template <bool FUSED>
__device__ __forceinline__ void l2_finish_body(const int fb, const int nfb, FinShared &sh, const float *__restrict__ desc, const u32x4 *__restrict__ hi_t,
                                               const u32x4 *__restrict__ hi_q, const float *__restrict__ norms,
                                               const float *__restrict__ rho_t, const float *__restrict__ rho_q,
                                               const PairDesc *__restrict__ pairs, const int32_t *__restrict__ pair_order, int n_pairs, int S,
                                               const int32_t *surv_cnt, const float4 *surv_list,
                                               int32_t *__restrict__ unc_cnt, int32_t *__restrict__ unc_list, float *__restrict__ knn_d2,
                                               int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist,
                                               int32_t *__restrict__ counters, int32_t *__restrict__ flagged, int flag_cap,
                                               int32_t *__restrict__ done, int audit, int do_ratio, double ratio, double ratio2m,
                                               int32_t *__restrict__ query_idx, int32_t *__restrict__ train_idx,
                                               float *__restrict__ distance, int32_t *__restrict__ n_out,
                                               int32_t *pass_done, int32_t *handover_fail)
{
    constexpr int CAP = kFinCap, HS = 8, NW = kFinWaves;
    constexpr float kBig = 3.0e38f;
    static_assert(kFinThreads == 256, "the later stages' buffers are laid out for four waves");
    extern __shared__ __attribute__((aligned(16))) char fin_smem[];         // kFinLdsBytes
    // stages (2) - (4) reuse the landing zones
    int *s_h = reinterpret_cast<int *>(fin_smem);                             // [CAP] hits of the sweep: (query slot in the sweep) << 21 | train row
    float4 (*s_q)[16] = reinterpret_cast<float4 (*)[16]>(fin_smem + 8192);   // [32][16]
    unsigned long long (*s_keys)[32][2] = reinterpret_cast<unsigned long long (*)[32][2]>(fin_smem + 8192 + 8192);   // [NW][32][2]
    int &s_nhit = sh.s_nhit, &s_last = sh.s_last, &s_base = sh.s_base;
    float (&s_red)[2 * NW] = sh.s_red;
    int (&s_qrows)[64] = sh.s_qrows, (&s_wave)[NW] = sh.s_wave;
    unsigned long long (&s_best)[2][64] = sh.s_best;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    // Blocks are dispatched round-robin over the XCDs; xcd_remap gives every XCD a contiguous range of logical blocks, and the logical
    // order is pair-major over the pairs SORTED BY TRAIN SET: the S workgroups of a pair and the pairs of one train set run on one
    // XCD, whose L2 (4 MiB) then holds the one or two train sets their row fetches go to -- the re-rank is bound by those fetches
    // (51 k survivors x 9 rows x 256 B per step on the metric's workload).
    const int lb = xcd_remap(fb, nfb);
    const int sl = lb % S, p = pair_order[lb / S];
    const PairDesc pd = pairs[p];
    const int nq = pd.nq, nt = pd.nt;

    if (FUSED) {
        // ---- (0) the HAND-OVER: this pair's pass blocks run in this launch; each adds 1 to pass_done[p] once its survivor entries
        // (write-through stores) and its surv_cnt add are acknowledged.  One thread polls until all of the pair's 512-query blocks
        // are counted (a pair without queries has none: ready at once).  Why no wait can stall the launch:
        //   * every pass block has a lower workgroup id than every finish workgroup (the grid is [pass | padding | finish]);
        //   * within an XCD workgroups start in id order, so a finish workgroup starts only after ALL of its XCD's pass blocks have
        //     started; a waiting finish workgroup therefore never holds a slot that an unstarted pass block of its XCD needs;
        //   * pass blocks wait for nothing, and the awaited ones sit on their own XCDs, each of which has started its pass blocks
        //     before its finish workgroups for the same reason -- or starts them as soon as slots free up, which waiting finish
        //     workgroups of OTHER XCDs cannot prevent;
        //   * so every awaited pass block is running or done, or will start without this workgroup's help.
        // The spin is still bounded by wall clock: on expiry the workgroup raises the context's failure word and leaves; the API
        // turns the word into an error at its next synchronising call (as chol_sparse_kernel does for a lost flag).
        // What the pass wrote is read past this XCD's L2 from here on (surv_cnt: ld_coh_i; the entries: `sc1` loads).
        if (tid == 0) {
            const int need = (nq + l2x1_query_block_c - 1) / l2x1_query_block_c;
            int ok = 1;
            if (need > 0) {
                const long long t0 = wall_clock64();
                while (ld_coh_i(pass_done + p) != need) {
                    __builtin_amdgcn_s_sleep(8);
                    if (wall_clock64() - t0 > kHandoverTicks) { st_coh_i(handover_fail, 1); ok = 0; break; }
                }
            }
            s_last = ok;
        }
        __syncthreads();
        if (!s_last) return;       // (s_last is next written behind the arrival's barrier)
    }
    const int nsv_pair = min(FUSED ? ld_coh_i(surv_cnt + p) : surv_cnt[p], nq);

    // ---- (1) re-rank of the survivors: virtual sets dealt out over the pair's S x NW waves
    {
        FinRerankArgs A;
        A.nsv = nsv_pair;
        // the survivors dealt out EVENLY over the pair's S x NW waves while a wave's share fits one virtual set (a set costs its
        // latency chain whatever it holds: 25 sets of seven for 20 waves made five of them -- and their workgroups -- last twice as long)
        A.per = max(1, min(kFinQV, (A.nsv + S * NW - 1) / (S * NW)));
        A.ent = surv_list + 3 * (size_t)pd.out_off;
        A.ersrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(A.ent), 0, A.nsv * 48, 0x00020000);
        A.pd = pd; A.p = p;
        A.frsrc_t = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(desc + (size_t)pd.t_row0 * 64), 0, nt * 256, 0x00020000);   // rows past the set read as zeros, no memory access
        A.frsrc_q = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(desc + (size_t)pd.q_row0 * 64), 0, nq * 256, 0x00020000);
        A.ratio2m = ratio2m;
        A.knn_idx = knn_idx; A.knn_dist = knn_dist; A.knn_d2 = knn_d2;
        A.unc_cnt = unc_cnt; A.unc_list = unc_list;
        A.counters = counters; A.audit_unc = audit == 3 ? flagged : nullptr; A.audit_rej = audit == 4 ? flagged : nullptr; A.flag_cap = flag_cap;
        const int nvs = (A.nsv + A.per - 1) / A.per;
        if (sl * NW + wave + S * NW >= nvs)      // (wave-uniform) at most one virtual set for this wave
            finish_rerank_wave<true, FUSED>(A, sl * NW + wave, S * NW, nvs, nullptr);
        else
            finish_rerank_wave<false, FUSED>(A, sl * NW + wave, S * NW, nvs, reinterpret_cast<FinPending *>(fin_smem + kFinTailLds) + wave * kFinPend);
    }
    // (Round 5, measured and not kept: every workgroup settling ITS OWN uncertified queries by exact brute force right here instead
    // of leaving them to the pair's last workgroup -- M-SURF-4k-hard: 16 695 such queries per step, the finish kernel 1.43 -> 1.71 ms:
    // 4096 exact distances per query are as many VALU instructions again as the whole re-rank; the threshold filter's MFMA pass is
    // what keeps the second pass cheap, and what it needed was a shorter serial tail, see stage (2).)
    // arrive; the last of the pair's S workgroups goes on alone.  Every wave waits for its own write-through stores to be
    // acknowledged before the barrier lets the arrival out.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (S > 1) {
        if (tid == 0) s_last = __hip_atomic_fetch_add(&done[p], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S - 1;
        __syncthreads();
        if (!s_last) return;
        if (tid == 0) __hip_atomic_store(&done[p], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (everybody has arrived: nobody touches it again in this launch)
    }
    if (FUSED && tid == 0) st_coh_i(pass_done + p, 0);       // (... nor the hand-over counter: every slice has seen it full)
    if (audit == 3 || audit == 4) return;          // the first pass alone: its answers, its own lists

    // ---- (2), (3): the pair's uncertified queries, chunks of 32, the whole train set by this workgroup's four waves
    const int cnt = min(ld_coh_i(unc_cnt + p), nq);
    constexpr int kSmall = 8;      // uncertified queries of a pair up to which the exact brute force beats the threshold filter's fixed ~100-us chain
    if (cnt > 0 && cnt <= kSmall) {
        // a handful of queries: their exact 2-NN over the whole train set straight away (the threshold filter below is a chain of
        // nt / 128 dependent MFMA steps per chunk of 32 whatever the chunk holds: ~100 us for ONE query; this: a few us per query).
        // Audit mode 1 lists them like the product path does and leaves them the re-rank's answer (it used to send them through the
        // threshold filter instead, and its flagged list came out shorter than the product path's count of re-scanned queries).
        if (tid < 32) s_qrows[tid] = tid < cnt ? ld_coh_i(unc_list + pd.out_off + tid) : 0;
        __syncthreads();
        if (tid < cnt) {
            const int sl2 = atomicAdd(&counters[0], 1);
            if (sl2 < flag_cap) { flagged[2 * sl2] = p; flagged[2 * sl2 + 1] = s_qrows[tid]; }
        }
        if (audit != 1) finish_bruteforce_chunk(desc, pd, s_qrows, cnt, s_q, s_keys, knn_idx, knn_dist);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    } else if (cnt > 0) {
        // Round 5: a sweep over the train set serves SIXTY-FOUR queries (two MFMA accumulators per operand load) and the hits are merged
        // by 64-bit LDS atomic minima of (distance, index) keys.  Until then a sweep took 32 queries and one thread per query walked the
        // whole hit list: on real descriptors (M-SURF-4k-hard: 55 uncertified queries per pair, 13 hits per query) the pair's last
        // workgroup spent 2.2 x (104 us of sweep + 68 us of hits) here while every other workgroup of the pair had left.
        typedef unsigned long long u64;
        const int nchunks = (cnt + 63) >> 6;
        const float *__restrict__ tn = norms + pd.t_row0;
        const float *__restrict__ tr = rho_t + pd.t_row0;
        {   // max |t|^2 and max rho_t over the train set
            float m = 0.f, r = 0.f;
            for (int t = tid; t < nt; t += kFinThreads) { m = fmaxf(m, tn[t]); r = fmaxf(r, tr[t]); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o)); r = fmaxf(r, __shfl_xor(r, o)); }
            if (lane == 0) { s_red[wave] = m; s_red[NW + wave] = r; }
        }
        __syncthreads();
        float tmax = 0.f, rmax = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) { tmax = fmaxf(tmax, s_red[w2]); rmax = fmaxf(rmax, s_red[NW + w2]); }
        const double sqrt_tmax = sqrt((double)tmax);
        // this wave's share of the train set, in steps of 32 rows
        const int nsteps = (nt + 31) / 32;
        const int st0 = (nsteps * wave) / NW, st1 = (nsteps * (wave + 1)) / NW;
        auto key_of = [](float d, int t) { return (t >= 0 && d < FLT_MAX) ? (((u64)__float_as_uint(d) << 32) | (u64)(uint32_t)t) : ~0ull; };   // FLT_MAX, +inf, NaN: never a neighbour
        for (int c = 0; c < nchunks; ++c) {
            if (tid == 0) s_nhit = 0;
            const int nqc = min(64, cnt - c * 64);
            // lane j of either half-wave owns the queries j and 32 + j of the sweep
            int qrow2[2]; float thr2[2]; bf16x8 bq[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int slot = c * 64 + 32 * u + j;
                const bool qok = slot < cnt;
                const int qrow = qok ? ld_coh_i(unc_list + pd.out_off + slot) : 0;
                qrow2[u] = qrow;
                // threshold on the score: s <= U - |q|^2 + E1, rounded up
                float thr = -kBig;
                if (qok) {
                    const double qn = (double)norms[pd.q_row0 + qrow], rq = (double)rho_q[pd.q_row0 + qrow];
                    const double e1 = l2x1_e1(qn, rq, sqrt_tmax, (double)tmax, (double)rmax);
                    const double uu = (double)ld_coh_f(knn_d2 + pd.out_off + qrow);
                    const double x = uu * (1.0 + 1.0 / 1048576.0) - qn + e1;
                    const double xs = x + fabs(x) * (1.0 / 1048576.0);
                    thr = xs < 3.0e38 ? (float)xs : kBig;                 // (NaN compares false: kBig, everything passes -> overflow -> brute force)
                    if (!(xs < 3.0e38)) thr = kBig;
                    if ((double)thr < xs) thr = nextafterf(thr, kBig);
                }
                thr2[u] = thr;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    u32x4 v = qok ? hi_q[((size_t)pd.q_row0 + qrow) * HS + 2 * ks + h] : u32x4{0u, 0u, 0u, 0u};
                    bq[u][ks] = __builtin_bit_cast(bf16x8, v);
                }
            }
            if (tid < 32) { s_qrows[tid] = qrow2[0]; s_qrows[32 + tid] = qrow2[1]; }
            // the running two best of every query of the sweep start from what the re-rank left
            if (tid < nqc) {
                const size_t o = 2 * ((size_t)pd.out_off + ld_coh_i(unc_list + pd.out_off + c * 64 + tid));
                s_best[0][tid] = key_of(ld_coh_f(knn_dist + o), ld_coh_i(knn_idx + o));
                s_best[1][tid] = key_of(ld_coh_f(knn_dist + o + 1), ld_coh_i(knn_idx + o + 1));
            }
            __syncthreads();
            if (FUSED) finish_filter_sweep_body(hi_t + (size_t)pd.t_row0 * HS, tn, st0, st1, nt, j, h, nqc > 32, bq, thr2, &s_nhit, s_h);
            else finish_filter_sweep(hi_t + (size_t)pd.t_row0 * HS, tn, st0, st1, nt, j, h, nqc > 32, bq, thr2, &s_nhit, s_h);
            __syncthreads();
            const int nhit = s_nhit;
            if (nhit <= CAP) {
                // exact distances of the hits in the oracle's order (a thread per hit), merged as (distance, index) keys: the smallest
                // key of a query by a 64-bit LDS atomic minimum, then the smallest of the others (two different rows never share a key;
                // a hit that IS one of the two rows the re-rank left carries that row's key and changes nothing)
                u64 keyv[CAP / kFinThreads];
#pragma unroll
                for (int x = 0; x < CAP / kFinThreads; ++x) {
                    const int k = tid + kFinThreads * x;
                    keyv[x] = ~0ull;
                    if (k < nhit) {
                        const int hk = s_h[k];
                        const float4 *qp = reinterpret_cast<const float4 *>(desc + ((size_t)pd.q_row0 + s_qrows[hk >> 21]) * 64);
                        const float4 *tp = reinterpret_cast<const float4 *>(desc + ((size_t)pd.t_row0 + (hk & 0x1FFFFF)) * 64);
                        float4 qa[16], tb[16];
#pragma unroll
                        for (int e = 0; e < 16; ++e) { qa[e] = qp[e]; tb[e] = tp[e]; }
                        keyv[x] = key_of(sqrt_rn_f32(l2sqr64_canonical_regs(qa, tb)), hk & 0x1FFFFF);
                    }
                }
                u64 init0 = ~0ull;
                if (tid < nqc) init0 = s_best[0][tid];
                __syncthreads();
#pragma unroll
                for (int x = 0; x < CAP / kFinThreads; ++x) {
                    const int k = tid + kFinThreads * x;
                    if (k < nhit && keyv[x] != ~0ull) atomicMin(&s_best[0][s_h[k] >> 21], keyv[x]);
                }
                __syncthreads();
#pragma unroll
                for (int x = 0; x < CAP / kFinThreads; ++x) {
                    const int k = tid + kFinThreads * x;
                    if (k < nhit && keyv[x] != ~0ull && keyv[x] != s_best[0][s_h[k] >> 21]) atomicMin(&s_best[1][s_h[k] >> 21], keyv[x]);
                }
                if (tid < nqc && init0 != s_best[0][tid]) atomicMin(&s_best[1][tid], init0);      // (the re-rank's best, displaced by a hit)
                __syncthreads();
                if (tid < nqc) {
                    const size_t o = 2 * ((size_t)pd.out_off + s_qrows[tid]);
                    const u64 k0 = s_best[0][tid], k1 = s_best[1][tid];
                    st_coh_i(knn_idx + o, k0 != ~0ull ? (int)(uint32_t)k0 : -1); st_coh_i(knn_idx + o + 1, k1 != ~0ull ? (int)(uint32_t)k1 : -1);
                    st_coh_f(knn_dist + o, k0 != ~0ull ? __uint_as_float((uint32_t)(k0 >> 32)) : FLT_MAX);
                    st_coh_f(knn_dist + o + 1, k1 != ~0ull ? __uint_as_float((uint32_t)(k1 >> 32)) : FLT_MAX);
                }
                __syncthreads();
            } else {
                // too many rows inside the error bound: exact brute force of the sweep's queries, 32 at a time
                if (tid < nqc) {
                    const int sl2 = atomicAdd(&counters[0], 1);
                    if (sl2 < flag_cap) { flagged[2 * sl2] = p; flagged[2 * sl2 + 1] = s_qrows[tid]; }
                }
                __syncthreads();
                if (audit != 1) {
                    finish_bruteforce_chunk(desc, pd, s_qrows, min(32, nqc), s_q, s_keys, knn_idx, knn_dist);
                    if (nqc > 32) finish_bruteforce_chunk(desc, pd, s_qrows + 32, nqc - 32, s_q, s_keys, knn_idx, knn_dist);
                }
                __syncthreads();
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (the write-through stores above, before the ratio stage reads them back)
        __syncthreads();
    }
    if (do_ratio) {
        if (ratio2m < 1.0e300)            // the screen ran: only its survivors have records
            ratio_compact_pair_sparse<kFinThreads, FUSED>(pd, surv_list + 3 * (size_t)pd.out_off, nsv_pair, knn_idx, knn_dist, ratio, query_idx, train_idx,
                                                   distance, n_out + p, reinterpret_cast<uint32_t *>(fin_smem), s_wave, &s_base);
        else
            ratio_compact_pair<kFinThreads, 4096 / kFinThreads, true>(pd, knn_idx, knn_dist, ratio, query_idx, train_idx, distance, n_out + p, s_wave, &s_base);
    }
}

constexpr int kFinOcc = 3;        // workgroups per CU the register budget is cut for: 3 = 168 registers, no spill in the re-rank (64.5 us per step;
                                  // 1: 342 registers, 113 us; 2: 76 us; 4: 128 registers, 42 spills in the re-rank, 80 - 87 us; the query rows parked in LDS: 66 / 84 us at 3 / 4)
__global__ __launch_bounds__(kFinThreads, kFinOcc) void l2_finish_kernel(const float *__restrict__ desc, const u32x4 *__restrict__ hi_t,
                                                                const u32x4 *__restrict__ hi_q, const float *__restrict__ norms,
                                                                const float *__restrict__ rho_t, const float *__restrict__ rho_q,
                                                                const PairDesc *__restrict__ pairs, const int32_t *__restrict__ pair_order, int n_pairs, int S,
                                                                const int32_t *__restrict__ surv_cnt, const float4 *__restrict__ surv_list,
                                                                int32_t *__restrict__ unc_cnt, int32_t *__restrict__ unc_list, float *__restrict__ knn_d2,
                                                                int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist,
                                                                int32_t *__restrict__ counters, int32_t *__restrict__ flagged, int flag_cap,
                                                                int32_t *__restrict__ done, int audit, int do_ratio, double ratio, double ratio2m,
                                                                int32_t *__restrict__ query_idx, int32_t *__restrict__ train_idx,
                                                                float *__restrict__ distance, int32_t *__restrict__ n_out)
{
    __shared__ FinShared sh;
    l2_finish_body<false>(blockIdx.x, gridDim.x, sh, desc, hi_t, hi_q, norms, rho_t, rho_q, pairs, pair_order, n_pairs, S, surv_cnt, surv_list, unc_cnt, unc_list,
                          knn_d2, knn_idx, knn_dist, counters, flagged, flag_cap, done, audit, do_ratio, ratio, ratio2m, query_idx, train_idx, distance, n_out,
                          nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// The pass and the finish stages in ONE launch (the match-list path outside the audit modes 3 / 4).  Grid:
//     [ n_blocks pass blocks, padded to n_pad = a multiple of 8 | n_pairs * S finish workgroups ]
// Workgroups below n_blocks run l2_knn_bf16x1_body, one 512-query block each; padding workgroups return at once; the others run
// l2_finish_body, which waits for ITS pair's pass blocks only (the hand-over, stage (0) there).  Each role keeps its own xcd_remap
// numbering over its own range, and because n_pad is a multiple of 8 a finish workgroup's XCD is (its index in the role) % 8 as in
// a launch of its own: a pair's finish workgroups land where the pair order (sorted by train set) wants them.  The hardware's
// dispatcher starts the finish workgroups as the pass's last round frees slots, instead of after the whole grid has drained and a
// second launch has come up; the finish role runs at this kernel's two workgroups per CU.
__global__ __launch_bounds__(256, 2) void l2_fused_kernel(const float *__restrict__ desc, const u32x4 *__restrict__ hi_t,
                                                          const u32x4 *__restrict__ hi_q, const float *__restrict__ norms,
                                                          const float *__restrict__ rho_t, const float *__restrict__ rho_q,
                                                          const float2 *__restrict__ blkmax,
                                                          const PairDesc *__restrict__ pairs, const int32_t *__restrict__ blk_pair, int n_blocks, int n_pad,
                                                          const int32_t *__restrict__ pair_order, int n_pairs, int S,
                                                          int32_t *knn_idx, float *knn_dist, int32_t *counters, int32_t *flagged, int flag_cap,
                                                          int32_t *surv_cnt, float4 *surv_list,
                                                          int32_t *unc_cnt, int32_t *unc_list, float *knn_d2,
                                                          int32_t *zero_a, int32_t *zero_b, int zero_n, int32_t *zero_counters,
                                                          int32_t *done, int32_t *pass_done, int32_t *handover_fail,
                                                          int audit, double ratio, double ratio2m,
                                                          int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    static_assert(kFinThreads == 256, "both roles run 256 threads");
    extern __shared__ __attribute__((aligned(16))) char fused_smem[];
    const int bid = blockIdx.x;
    if (bid < n_pad) {
        if (bid >= n_blocks) return;
        l2_knn_bf16x1_body<true>(bid, n_blocks, desc, hi_t, hi_q, norms, rho_t, rho_q, blkmax, pairs, blk_pair, n_blocks, knn_idx, knn_dist, counters, flag_cap,
                                 surv_cnt, surv_list, ratio2m, 0, nullptr, zero_a, zero_b, zero_n, zero_counters, pass_done);
    } else {
        l2_finish_body<true>(bid - n_pad, n_pairs * S, *reinterpret_cast<FinShared *>(fused_smem + kFinLdsBytes), desc, hi_t, hi_q, norms, rho_t, rho_q, pairs,
                             pair_order, n_pairs, S, surv_cnt, surv_list, unc_cnt, unc_list, knn_d2, knn_idx, knn_dist, counters, flagged, flag_cap, done, audit, 1,
                             ratio, ratio2m, query_idx, train_idx, distance, n_out, pass_done, handover_fail);
    }
}

// ---------------------------------------------------------------------------------------------
// launchers

bool l2_one_product_pass()
{
    static const bool off = [] { const char *e = getenv("ESFM_L2_PASS"); return e && strcmp(e, "bf16x3") == 0; }();
    return !off;
}

// the ratio screen's constant: ratio^2 (1 + 2^-20); a ratio that is not a finite number >= 0 switches the screen off
static inline double l2_ratio2m(double ratio) { return (ratio >= 0.0 && ratio < 1.0e150) ? ratio * ratio * (1.0 + 1.0 / 1048576.0) : (double)INFINITY; }

int l2_x1_query_block() { return l2x1_query_block_c; }
bool l2_x1_supported(int max_nt) { return max_nt <= (1 << (ESFM_L2X1_CODE_BITS - (ESFM_L2X1_GRP == 4 ? 2 : 1))) * 32; }   // the position code names a 32-row step and one of its 16 / GRP groups

int l2_x1_forced_grid()
{
    static const int forced = [] { const char *e = getenv("ESFM_X1_GRID"); return e ? atoi(e) : 0; }();     // (measurement)
    return forced;
}

int launch_l2_knn_bf16x1(hipStream_t st, int num_cu, const float *desc, const void *hi, long long total_rows, const float *norms, const PairDesc *pairs,
                         const int32_t *blk_pair, int n_blocks, int32_t *knn_idx, float *knn_dist, int32_t *counters, int flag_cap,
                         int32_t *surv_cnt, void *surv_list, double ratio, bool markers, int32_t *rejected,
                         int32_t *zero_a, int32_t *zero_b, int zero_n, int32_t *zero_counters)
{
    if (n_blocks <= 0) return ESFM_OK;
    // ring of bf16 tiles, their norms, two sets of reductions, two sets of query norms and residual norms
    constexpr size_t lds = 4 * 128 * 128 + 4 * 128 * 4 + 64 + 4 * l2x1_query_block_c * 4;
    static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
    // (set on every launch, like the other large-LDS kernels: the attribute belongs to the current device)
    ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&l2_knn_bf16x1_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void *h = const_cast<void *>(hi);
    // one workgroup per block by default (see the kernel); ESFM_X1_GRID = persistent workgroups (a multiple of 8, e.g. 2 x CUs)
    const int forced = l2_x1_forced_grid();
    (void)num_cu;
    const int grid = forced > 0 && forced < n_blocks ? std::max(8, forced / 8 * 8) : n_blocks;
    hipLaunchKernelGGL(l2_knn_bf16x1_kernel, dim3(grid), dim3(256), lds, st, desc,
                       reinterpret_cast<const u32x4 *>(l2_hi_part(h, total_rows, 0)), reinterpret_cast<const u32x4 *>(l2_hi_part(h, total_rows, 1)), norms,
                       reinterpret_cast<const float *>(l2_hi_part(h, total_rows, 2)), reinterpret_cast<const float *>(l2_hi_part(h, total_rows, 3)),
                       reinterpret_cast<const float2 *>(l2_hi_part(h, total_rows, 4)),
                       pairs, blk_pair, n_blocks, knn_idx, knn_dist, counters, flag_cap, surv_cnt, reinterpret_cast<float4 *>(surv_list), l2_ratio2m(ratio), markers ? 1 : 0, rejected,
                       zero_a, zero_b, zero_n, zero_counters);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

static int forced_fin_slices()
{
    static const int forced = [] { const char *e = getenv("ESFM_FIN_SLICES"); return e ? atoi(e) : 0; }();     // (measurement)
    return forced;
}
int l2_finish_slices(int n_pairs)
{
    if (forced_fin_slices() > 0) return forced_fin_slices();
    return std::max(1, std::min(8, 2304 / std::max(n_pairs, 1)));      // (300 pairs, three workgroups per CU, survivors dealt evenly: 7 slices 60 us, 4: 70, 5: 65, 6: 66, 8: 63)
}

int launch_l2_finish(hipStream_t st, const float *desc, const void *hi, long long total_rows, const float *norms, const PairDesc *pairs,
                     const int32_t *pair_order, int n_pairs, const int32_t *surv_cnt, const void *surv_list, int32_t *unc_cnt, int32_t *unc_list, float *knn_d2,
                     int32_t *knn_idx, float *knn_dist, int32_t *counters, int32_t *flagged, int flag_cap, int32_t *done,
                     int audit, bool do_ratio, double ratio, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    if (n_pairs <= 0) return ESFM_OK;
    const int S = l2_finish_slices(n_pairs);
    ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&l2_finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFinLdsBytes));
    void *h = const_cast<void *>(hi);
    hipLaunchKernelGGL(l2_finish_kernel, dim3((unsigned)n_pairs * (unsigned)S), dim3(kFinThreads), kFinLdsBytes, st, desc,
                       reinterpret_cast<const u32x4 *>(l2_hi_part(h, total_rows, 0)), reinterpret_cast<const u32x4 *>(l2_hi_part(h, total_rows, 1)), norms,
                       reinterpret_cast<const float *>(l2_hi_part(h, total_rows, 2)), reinterpret_cast<const float *>(l2_hi_part(h, total_rows, 3)),
                       pairs, pair_order, n_pairs, S, surv_cnt, reinterpret_cast<const float4 *>(surv_list), unc_cnt, unc_list, knn_d2, knn_idx, knn_dist, counters, flagged,
                       flag_cap, done, audit, do_ratio ? 1 : 0, ratio, l2_ratio2m(ratio), query_idx, train_idx, distance, n_out);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_l2_fused(hipStream_t st, const float *desc, const void *hi, long long total_rows, const float *norms, const PairDesc *pairs,
                    const int32_t *blk_pair, int n_blocks, const int32_t *pair_order, int n_pairs, int32_t *knn_idx, float *knn_dist, int32_t *counters,
                    int32_t *flagged, int flag_cap, int32_t *surv_cnt, void *surv_list, int32_t *unc_cnt, int32_t *unc_list, float *knn_d2,
                    int32_t *zero_a, int32_t *zero_b, int zero_n, int32_t *zero_counters, int32_t *done, int32_t *pass_done, int32_t *handover_fail,
                    int audit, double ratio, int32_t *query_idx, int32_t *train_idx, float *distance, int32_t *n_out)
{
    if (n_blocks <= 0 || n_pairs <= 0) return ESFM_OK;
    const FusedGrid g = fused_grid_of(n_blocks, n_pairs, forced_fin_slices() > 0 ? forced_fin_slices() : fused_slices_default(n_pairs));
    if (g.total >= (1LL << 31)) { set_error("too many workgroups for one launch; split the pair list"); return ESFM_ERR_INVALID_ARG; }
    // dynamic LDS: the larger of the two roles' needs (the pass's, as in launch_l2_knn_bf16x1; the finish role's buffers + its FinShared)
    constexpr size_t lds_pass = 4 * 128 * 128 + 4 * 128 * 4 + 64 + 4 * l2x1_query_block_c * 4;
    constexpr size_t lds_fin = kFinLdsBytes + ((sizeof(FinShared) + 15) & ~(size_t)15);
    constexpr size_t lds = lds_pass > lds_fin ? lds_pass : lds_fin;
    static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
    ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&l2_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void *h = const_cast<void *>(hi);
    hipLaunchKernelGGL(l2_fused_kernel, dim3((unsigned)g.total), dim3(256), lds, st, desc,
                       reinterpret_cast<const u32x4 *>(l2_hi_part(h, total_rows, 0)), reinterpret_cast<const u32x4 *>(l2_hi_part(h, total_rows, 1)), norms,
                       reinterpret_cast<const float *>(l2_hi_part(h, total_rows, 2)), reinterpret_cast<const float *>(l2_hi_part(h, total_rows, 3)),
                       reinterpret_cast<const float2 *>(l2_hi_part(h, total_rows, 4)),
                       pairs, blk_pair, n_blocks, (int)g.n_pad, pair_order, n_pairs, g.slices, knn_idx, knn_dist, counters, flagged, flag_cap, surv_cnt,
                       reinterpret_cast<float4 *>(surv_list), unc_cnt, unc_list, knn_d2, zero_a, zero_b, zero_n, zero_counters, done, pass_done, handover_fail,
                       audit, ratio, l2_ratio2m(ratio), query_idx, train_idx, distance, n_out);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}
size_t l2_survivor_entry_bytes() { return 48; }

}  // namespace esfm
