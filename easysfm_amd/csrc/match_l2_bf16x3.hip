// The three-product bf16 L2 pass (64-float rows with ESFM_L2_PASS=bf16x3 or train sets
// beyond the one-product pass's position code): the split kernel -- which also writes the one-product pass's images, layout
// l2_hi_part() in match_kernels.hpp --, the block maxima, the distance pass and the per-pair re-scan of its uncertified queries.
#include "match_kernels.hpp"
#include "match_device.hpp"
#include "l2_segment_gfx950.inc"       // ESFM_L2_SEGMENT_ASM: the matcher's hand-scheduled main loop (gen_l2_segment_asm.py)

#include <float.h>
#include <type_traits>
#include <stdlib.h>
#include <string.h>

namespace esfm {

// ---------------------------------------------------------------------------------------------
// Split-bf16 distance pass (64-float descriptors): the same kernel shape as l2_knn_mfma_kernel, with the f32 MFMA (157 TFLOP/s,
// no VALU co-execution) replaced by three bf16 MFMAs (2.5 PFLOP/s, VALU runs beside them).  Every float a is split into
// hi = bf16(a) and lo = bf16(a - hi) (round to nearest even; a = hi + lo + e, |e| <= 2^-18 |a|), and
//   q.t ~ sum hi_q hi_t + hi_q lo_t + lo_q hi_t          (the dropped terms are <= 3.01 * 2^-18 sum |q_i t_i|)
// is accumulated by v_mfma_f32_32x32x16_bf16 on top of |t|^2, with -2 folded into the query operand.  bf16 products are exact
// in f32; the accumulation error and the split error go into the certificate's eps (2^-15 instead of 2^-16 of |q|^2 + max|t|^2,
// DESIGN.md), so the exact re-rank and the rescan of uncertified queries keep the result bit-identical to the oracle's.
// The split image (l2_split_bf16_kernel) has the f32 rows' size: per 16 features 32 B of hi then 32 B of lo, so a lane's A
// fragment of K-step ks is the 16-B slot 4 ks + h (hi) or 4 ks + 2 + h (lo) of its train row -- the staging code, the XOR
// swizzle and the conflict-free ds_read_b128 of the f32 kernel carry over unchanged.
// Each wave owns TWO sets of 32 queries (B operands: 64 VGPRs), so an A fragment feeds two MFMAs and a workgroup covers 256
// queries (half the L2 -> LDS traffic of the f32 kernel).  The fold of step n runs in the shadow of step n+1's MFMAs.

__device__ __forceinline__ uint32_t bf16_rne_bits(float a)
{
    const uint32_t u = __float_as_uint(a);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// hi / lo halves of 2 consecutive floats packed into one dword each (element 0 in the low half)
__device__ __forceinline__ void bf16_split2(float a0, float a1, uint32_t &hi, uint32_t &lo)
{
    const uint32_t h0 = bf16_rne_bits(a0), h1 = bf16_rne_bits(a1);
    const float r0 = __fsub_rn(a0, __uint_as_float(h0 << 16)), r1 = __fsub_rn(a1, __uint_as_float(h1 << 16));   // exact
    hi = h0 | (h1 << 16);
    lo = bf16_rne_bits(r0) | (bf16_rne_bits(r1) << 16);
}

// One thread per 16-B piece of a row (4 floats): the load and both stores of a wave are contiguous kilobytes.  A 16-B piece of
// the image holds the hi (or lo) halves of EIGHT floats, so neighbouring lanes swap what the other one assembles: the even lane
// of a pair stores the hi piece, the odd lane the lo piece -- slots 0, 2, 1, 3 of the 64-B group for four consecutive lanes.
// Twice (train image, query image = the same split of -2 x); the 16 lanes of a row also leave |row|^2 (the approximate pass and
// the certificate only need it to 64 u: the summation order is free).  The launch also zeroes the pass's counters (the global
// list's and one per pair): two memset launches less per call.
// (Round 1: one thread per 16-feature group, four loads and eight stores of 16 B at a 64-B lane stride: 31 us per 25 x 4096 rows.)
__global__ __launch_bounds__(256) void l2_split_bf16_kernel(const float4 *__restrict__ desc, long long n_pieces, u32x4 *__restrict__ out,
                                                            u32x4 *__restrict__ out_q, float *__restrict__ norms,
                                                            int32_t *__restrict__ counters, int32_t *__restrict__ pair_cnt, int n_pairs,
                                                            u32x4 *__restrict__ hi_t, u32x4 *__restrict__ hi_q, float *__restrict__ rho_t,
                                                            float *__restrict__ rho_q, int32_t *__restrict__ pair_cnt2)
{
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < 16) counters[f] = 0;
    if (f < n_pairs) { pair_cnt[f] = 0; if (pair_cnt2) pair_cnt2[f] = 0; }
    const bool ok = f < n_pieces;
    const float4 v = ok ? desc[f] : make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
    s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 8);
    const bool odd = (threadIdx.x & 1) != 0;
    const long long g = f >> 2;                                  // 16-feature group
    const int slot = (odd ? 2 : 0) + (int)((f >> 1) & 1);        // hi pieces: slots 0, 1; lo pieces: 2, 3
#pragma unroll
    for (int img = 0; img < 2; ++img) {
        const float sc = img == 0 ? 1.f : -2.f;                 // scaling by -2 is exact and commutes with the split
        uint32_t h0, l0, h1, l1;
        bf16_split2(sc * v.x, sc * v.y, h0, l0);
        bf16_split2(sc * v.z, sc * v.w, h1, l1);
        // the even lane needs its partner's hi halves, the odd lane its partner's lo halves
        const uint32_t r0 = __shfl_xor(odd ? h0 : l0, 1), r1 = __shfl_xor(odd ? h1 : l1, 1);
        const u32x4 piece = odd ? u32x4{r0, r1, l0, l1} : u32x4{h0, h1, r0, r1};
        if (ok && out) (img == 0 ? out : out_q)[4 * g + slot] = piece;      // (the hi / lo images: the three-product pass's operands only)
        if (hi_t) {
            // The one-product pass (l2_knn_bf16x1_kernel) multiplies the hi halves only.  Its images are dense -- 128 B per row, the
            // even lane's piece IS the 16-B slot of eight consecutive features -- and its certificate needs |x - hi(x)|_2 of every
            // row in both roles (x = t and x = -2 q: the same number times two, except for denormals).  The residuals are exact in
            // f32; the sum is rounded up by more than its 64-term error.
            if (ok && !odd) (img == 0 ? hi_t : hi_q)[f >> 1] = piece;
            const float e0 = __fsub_rn(sc * v.x, __uint_as_float(h0 << 16)), e1 = __fsub_rn(sc * v.y, __uint_as_float(h0 & 0xFFFF0000u));
            const float e2 = __fsub_rn(sc * v.z, __uint_as_float(h1 << 16)), e3 = __fsub_rn(sc * v.w, __uint_as_float(h1 & 0xFFFF0000u));
            // (summed in double: the squares of residuals below ~1e-19 are denormal or zero in f32, and a residual norm that comes out
            // too small would make the certificate's bound too small)
            double r = (double)e0 * (double)e0 + (double)e1 * (double)e1 + (double)e2 * (double)e2 + (double)e3 * (double)e3;
            r += __shfl_xor(r, 1);
            r += __shfl_xor(r, 2);
            r += __shfl_xor(r, 4);
            r += __shfl_xor(r, 8);
            if (ok && (f & 15) == 0) {
                const double rd = sqrt(r) * 1.0005;
                float rf = (float)rd;
                if ((double)rf < rd) rf = nextafterf(rf, FLT_MAX);     // rounded up
                (img == 0 ? rho_t : rho_q)[f >> 4] = rf;
            }
        }
    }
    if (ok && (f & 15) == 0) norms[f >> 4] = s;
}

__global__ __launch_bounds__(256, 2) void l2_knn_bf16_kernel(const float *__restrict__ desc, const u32x4 *__restrict__ split,
                                                             const u32x4 *__restrict__ split_q, const float *__restrict__ norms, const PairDesc *__restrict__ pairs,
                                                             int n_pairs, int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist,
                                                             int32_t *__restrict__ flagged, int32_t *__restrict__ counters, int flag_cap,
                                                             int32_t *__restrict__ pair_cnt, int32_t *__restrict__ pair_list)
{
    constexpr int TT = 128, NS = 2, GRP = 4;                     // train rows per LDS tile, query sets of 32 per wave, rows per fold group
    constexpr int DIM = 64, QB = 128 * NS, SLOTS = 16, KS = 4;
    constexpr int NDMA = TT / 16;             // LDS-DMA instructions per wave per tile (4 rows = 1 KiB each)

    extern __shared__ __attribute__((aligned(16))) char smem[];
    u32x4 *lds_tile = reinterpret_cast<u32x4 *>(smem);                         // [2][TT*SLOTS]
    float *lds_norm = reinterpret_cast<float *>(smem + 2 * TT * SLOTS * 16);   // [2][TT]   (the asm segment assumes norms right behind the tiles)
    float *lds_red = lds_norm + 2 * TT;                                        // [4]
    float *lds_master = lds_red + 4;                                           // [NS][6][256]: per-thread master top-3 (keys, segments)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = find_pair_by_block(pairs, n_pairs, lb);
    const PairDesc pd = pairs[pi];
    const int nq = pd.nq, nt = pd.nt;
    const float *__restrict__ Q = desc + (size_t)pd.q_row0 * DIM;
    const float *__restrict__ T = desc + (size_t)pd.t_row0 * DIM;
    const float *__restrict__ tn = norms + pd.t_row0;
    const int qbase = (lb - pd.blk_off) * QB + wave * 32 * NS;
    auto row_of_slot = [&](int q) { return q; };

    // Running top-3 per query set, TWO levels deep in the hot loop (l2_segment_gfx950.inc).  A lane's 16 results of a 32-train
    // step are four groups of four consecutive train rows (accumulator registers 4g .. 4g+3 = rows 8g + 4h + 0..3).  Per group:
    // the minimum of the four raw scores (two v_min3_f32 seeded with kBig: a NaN score loses every minimum), the 8-bit position
    // code (6 bits step in segment, 2 bits group) into the low mantissa bits of that minimum (one v_and_or_b32), and the
    // three-smallest network on the group key (three v_med3_f32): 6 VALU per 4 results instead of 16.  The two nearest trains of a
    // query lie in the (at most two) groups with the smallest minima; the third group key bounds every row outside the kept
    // groups, which is what the certificate needs.  The tail re-ranks the kept groups' rows exactly -- four consecutive 256-B rows
    // per group.
    // (Measured on MI355X, profiles/r02_ubench_mfma_issue.txt: in SHADER CYCLES up to six VALU instructions hide behind every bf16 MFMA --
    // the 5.33-per-MFMA fold of round 1 included; what they cost is POWER: the chip is clock-limited on random operands, 1660 TFLOP/s
    // with the 4-per-result fold beside the MFMAs against 1805 with this one and 1690-1940 with none.)
    constexpr float kBig = 3.0e38f;
    constexpr int NG = 16 / GRP;              // groups per lane per 32-train step
    constexpr int kSegSub = 256 / NG;         // steps per segment: the 8-bit code is (step in segment) * NG + group
    constexpr int kSegTiles = kSegSub / (TT / 32);
    // The master top-3 (key, first step of the key's segment) is touched once per segment (2048 trains): it lives in LDS, a
    // private column per thread, so that the main loop's registers go to the pipeline.
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int m = 0; m < 3; ++m) { lds_master[(6 * s + m) * 256 + tid] = kBig; lds_master[(6 * s + 3 + m) * 256 + tid] = __int_as_float(-1); }
    }
    float tmax;
    // the master keeps (key, first step of the key's segment); the group's rows are decoded from the two once, at the end
    struct Master { float v0, v1, v2; int c0, c1, c2; };
    auto master_load = [&](int s) {
        Master m;
        m.v0 = lds_master[(6 * s + 0) * 256 + tid]; m.v1 = lds_master[(6 * s + 1) * 256 + tid]; m.v2 = lds_master[(6 * s + 2) * 256 + tid];
        m.c0 = __float_as_int(lds_master[(6 * s + 3) * 256 + tid]); m.c1 = __float_as_int(lds_master[(6 * s + 4) * 256 + tid]);
        m.c2 = __float_as_int(lds_master[(6 * s + 5) * 256 + tid]);
        return m;
    };
    auto master_store = [&](int s, const Master &m) {
        lds_master[(6 * s + 0) * 256 + tid] = m.v0; lds_master[(6 * s + 1) * 256 + tid] = m.v1; lds_master[(6 * s + 2) * 256 + tid] = m.v2;
        lds_master[(6 * s + 3) * 256 + tid] = __int_as_float(m.c0); lds_master[(6 * s + 4) * 256 + tid] = __int_as_float(m.c1);
        lds_master[(6 * s + 5) * 256 + tid] = __int_as_float(m.c2);
    };
    auto master_insert = [&](Master &m, float key, int seg_sub0 /* wave-uniform */) {
        const bool live = key < 1.0e38f;
        const bool l2 = live && key < m.v2, l1 = live && key < m.v1, l0 = live && key < m.v0;
        const int t2 = l2 ? seg_sub0 : m.c2;
        const int t1 = l1 ? seg_sub0 : m.c1;
        m.c2 = l1 ? m.c1 : t2;
        m.c1 = l0 ? m.c0 : t1;
        m.c0 = l0 ? seg_sub0 : m.c0;
        const float n2 = l2 ? key : m.v2;
        const float n1 = l1 ? key : m.v1;
        m.v2 = l1 ? m.v1 : n2;
        m.v1 = l0 ? m.v0 : n1;
        m.v0 = l0 ? key : m.v0;
    };
    // first of the GRP consecutive train rows of the group a key names (-1: empty slot): accumulator register r holds row
    // (r & 3) + 8 (r >> 2) + 4 h of its step
    auto group_row0_of = [&](float key, int seg_sub0) {
        const int code = (int)(__float_as_uint(key) & 0xFFu);
        const int r0 = GRP * (code % NG);
        return key < 1.0e38f ? (seg_sub0 + code / NG) * 32 + (r0 & 3) + 8 * (r0 >> 2) + 4 * h : -1;
    };

    const int ntiles = (nt + TT - 1) / TT;
    // Staging is LDS-DMA (buffer_load_dwordx4 ... lds): a wave instruction moves 4 train rows (1 KiB) straight into LDS, lane l
    // to byte 16 l of the destination, so the XOR swizzle is applied on the SOURCE side (lane l fetches slot (l & 15) ^ (row & 15)
    // of its row) -- no staging VGPRs, no ds_write pass.  Rows past nt read as zeros through the buffer descriptor; their norm
    // is kBig.  Tiles 0 and 1 are issued here, tile t + 2 by the segment code when tile t hands its buffer over.
    const u32x4 trsrc = raw_buffer_rsrc(split + (size_t)pd.t_row0 * SLOTS, (uint32_t)nt * (DIM * 4));   // reads past it return 0
    const u32x4 nrsrc = raw_buffer_rsrc(tn, (uint32_t)nt * 4u);
    const uint32_t lds_tile_addr = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds_tile);   // LDS byte address
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int wrow0 = wave_s * (TT / 4);                                   // this wave stages rows [wrow0, wrow0 + TT / 4) of a tile
    auto dma_tile = [&](int tile, int buf) {
        int voff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wrow0 + 4 * i + (lane >> 4);
            voff[i] = row * (DIM * 4) + (((lane & 15) ^ (row & 15)) * 16);   // rows 16 apart share the swizzle: i and i + 4
        }
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            const uint32_t dst = lds_tile_addr + (uint32_t)((buf * TT * SLOTS + (wrow0 + 4 * i) * SLOTS) * 16);
            const int soff = (tile * TT + (i >= 4 ? 16 : 0)) * (DIM * 4);    // wave-uniform
            lds_dma_b128(dst, voff[i & 3], trsrc, soff);
        }
    };
    auto norm_load = [&](int tile) {
        const int t = tile * TT + tid;
        return (tid < TT && t < nt) ? tn[t] : kBig;
    };
    auto norm_store = [&](int buf, float nv) { if (tid < TT) lds_norm[buf * TT + tid] = nv; };

    // rows past nt of the last tile are not transferred (their norm kBig keeps them out of every top-3): what they hold must
    // at least be finite, so the buffers start out zeroed (NaN keys would corrupt the v_med3 network)
    if (ntiles * TT != nt) {
        for (int i = tid; i < 2 * TT * SLOTS; i += 256) lds_tile[i] = u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
    }
    if (ntiles > 0) {
        norm_store(0, norm_load(0));
        dma_tile(0, 0);
        if (ntiles > 1) { norm_store(1, norm_load(1)); dma_tile(1, 1); }
    }

    // (issued after the first two tiles' DMA so that their latencies overlap)
    // B operands: -2 q split into hi and lo (the query image of l2_split_bf16_kernel), this lane's 8 features of every K-step
    u32x4 bhi[NS][KS], blo[NS][KS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int qrow = row_of_slot(qbase + 32 * s + j);
        const bool ok = qrow < nq;
        const u32x4 *qp = split_q + ((size_t)pd.q_row0 + (ok ? qrow : 0)) * SLOTS + h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 hi = qp[4 * ks], lo = qp[4 * ks + 2];
            if (!ok) { hi = u32x4{0u, 0u, 0u, 0u}; lo = hi; }
            bhi[s][ks] = hi;
            blo[s][ks] = lo;
        }
    }

    // max |t|^2 over the train set (the certificate's error bound needs it in the tail): reduced here, while the first tiles are
    // on their way, and published through LDS -- the segment code's first barrier orders it for the whole workgroup
    {
        float m = 0.f;
        for (int t = tid; t < nt; t += 256) m = fmaxf(m, tn[t]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) lds_red[wave] = m;
    }

    // Main loop: one hand-scheduled asm block per segment of <= 16 tiles (gen_l2_segment_asm.py has the schedule: software-pipelined
    // by two K-steps, LDS-DMA of tile t + 2 issued when tile t hands its buffer over, one barrier per tile).  It returns the
    // segment's three smallest group keys per query set; they go into the master top-3 between segments.
    for (int t0 = 0; t0 < ntiles; t0 += kSegTiles) {
        const int t1 = min(t0 + kSegTiles, ntiles);
        float k0[NS], k1[NS], k2[NS];
        asm volatile(ESFM_L2_SEGMENT_ASM
                     : "=&v"(k0[0]), "=&v"(k1[0]), "=&v"(k2[0]), "=&v"(k0[1]), "=&v"(k1[1]), "=&v"(k2[1])
                     : "v"(bhi[0][0]), "v"(bhi[0][1]), "v"(bhi[0][2]), "v"(bhi[0][3]), "v"(bhi[1][0]), "v"(bhi[1][1]), "v"(bhi[1][2]), "v"(bhi[1][3]),
                       "v"(blo[0][0]), "v"(blo[0][1]), "v"(blo[0][2]), "v"(blo[0][3]), "v"(blo[1][0]), "v"(blo[1][1]), "v"(blo[1][2]), "v"(blo[1][3]),
                       "s"(t0), "s"(t1), "s"(nt), "s"(trsrc), "s"(nrsrc), "s"(lds_tile_addr), "s"(wave_s)
                     : ESFM_L2_SEGMENT_CLOBBERS);
        const int seg_sub0 = t0 * (TT / 32);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            Master m = master_load(s);
            master_insert(m, k0[s], seg_sub0); master_insert(m, k1[s], seg_sub0); master_insert(m, k2[s], seg_sub0);
            master_store(s, m);
        }
    }

    if (ntiles == 0) __syncthreads();   // no segment ran, so no barrier has published lds_red yet
    tmax = fmaxf(fmaxf(lds_red[0], lds_red[1]), fmaxf(lds_red[2], lds_red[3]));

    // ---- exact re-rank of the kept groups' rows in the oracle's order, certificate ----
    // A query's six kept groups (three per half-wave lane) are ranked by key across the two lanes and dealt out alternately --
    // global rank 2 r + h goes to lane half h in round r -- so the two groups that usually matter cost ONE round of four rows
    // whichever lanes found them.  A group is skipped when it provably cannot hold one of the two nearest: with ka <= kb the two
    // smallest of the six keys (two groups, hence two different rows: the groups' minima), both of those rows' exact d^2 are
    // <= U = |q|^2 + kb + E(kb), E(k) = 2^-15 (|q|^2 + max|t|^2) + 2^-15 |k| being the certificate's bound on |(|q|^2 + key) - d^2|;
    // every row of a group with |q|^2 + k - E(k) > U (1 + 2^-20) -- k its minimum -- is farther than both even after sqrtf's
    // rounding.  Keys only grow with the rank, so the rounds stop at the first one no lane of the wave needs.
    //
    // The rows come in by LDS-DMA (round 2, second half).  With one row per lane a load instruction touches 64 cache lines and the
    // L1 looks up about one line per clock: the 160 such instructions per wave kept the texture path busy for ~21 us per workgroup
    // (measured: 0.40 ms per launch with one workgroup per CU, 0.22 ms with two) and the OTHER workgroup's tile transfers queued
    // behind them -- with wave-uniform (coalesced) addresses in the same instructions the kernel ran 0.10 ms faster.  Now 16 lanes
    // fetch one 256-B row (4 rows = 1 KiB per wave instruction, every line touched once) into the wave's quarter of the idle tile
    // area, XOR-swizzled on the source side like the tiles, and lane l reads "its" row back with 16 conflict-free ds_read_b128; the
    // row of sub-round u + 1 is in flight while row u is compared.  A wave's chain is now latency-bound (ten sub-rounds of
    // ~1.3 us), which costs little: the other workgroup of the CU alone keeps the matrix pipe 93 % busy (measured, one workgroup
    // per CU without tail: 1.39 ms against 1.29).  Measured: 1.50-1.52 -> 1.42-1.44 ms per launch.
    // (Measured and dropped: s_setprio 3 for the main loop / 0 for the tail, 1.50 ms; the query rows by per-lane loads in the
    // shadow of the first row transfer instead of their own sub-round, 1.50 ms -- 32 lines per instruction are enough to disturb
    // the tile transfers again; starting the second workgroup of every CU half a run time late, no gain.)
    // The segment code issues the transfer of tile t + 2 unconditionally (a tile that does not exist reads zeros through the
    // descriptor): the last two of them are still in flight, aimed at rows of the tile area that now become OTHER waves' landing
    // zones -- every wave drains its own before the barrier.
    lds_dma_wait();
    __syncthreads();   // every wave is through its last tile: the tile area becomes four private 16-KiB landing zones
    const u32x4 frsrc_t = raw_buffer_rsrc(T, (uint32_t)nt * 256u);   // rows past the set read as zeros, no memory access
    const u32x4 frsrc_q = raw_buffer_rsrc(Q, (uint32_t)nq * 256u);
    const uint32_t lds_land = lds_tile_addr + (uint32_t)wave_s * 16384u;
    const float4 *land = reinterpret_cast<const float4 *>(smem) + (size_t)wave * 1024;
    int swz[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) swz[i] = (4 * i + (lane >> 4)) * 256 + (((lane & 15) ^ ((4 * i + (lane >> 4)) & 15)) * 16);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int qrow = row_of_slot(qbase + 32 * s + j);
        const bool qvalid = qrow < nq;
        // the two best (distance, index, d^2) as plain scalars, updated without a branch (the struct form went through scratch
        // memory here, and every scratch access waits for the row transfer in flight)
        float b0d = FLT_MAX, b1d = FLT_MAX, b0q = 0.f, b1q = 0.f; int b0i = -1, b1i = -1;
        auto insert2 = [&](bool valid, float d, int i, float d2) {
            const bool c1 = valid && (d < b1d || (d == b1d && i < b1i));     // (an empty slot holds FLT_MAX: +inf and NaN never enter, like the oracle's `d < d1`)
            const bool c0 = valid && (d < b0d || (d == b0d && i < b0i));
            b1d = c0 ? b0d : (c1 ? d : b1d); b1i = c0 ? b0i : (c1 ? i : b1i); b1q = c0 ? b0q : (c1 ? d2 : b1q);
            b0d = c0 ? d : b0d; b0i = c0 ? i : b0i; b0q = c0 ? d2 : b0q;
        };
        // the 32 query rows of this set -> landing slots 0..31 (lanes j and j + 32 read the same slot); the group ranking below
        // runs in the transfer's shadow
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 8; ++i)
            lds_dma_b128(lds_land + (uint32_t)i * 1024u, (qbase + 32 * s) * 256 + (i >> 2) * 4096 + swz[i & 3], frsrc_q, 0);
        const Master mst = master_load(s);
        const float qnorm_s = norms[pd.q_row0 + (qvalid ? qrow : 0)];
        const float vk[3] = {mst.v0, mst.v1, mst.v2};
        const int g0[3] = {group_row0_of(mst.v0, mst.c0), group_row0_of(mst.v1, mst.c1), group_row0_of(mst.v2, mst.c2)};
        float pk[3]; int pg[3], rank_own[3], rank_par[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { pk[i] = __shfl_xor(vk[i], 32); pg[i] = __shfl_xor(g0[i], 32); }
#pragma unroll
        for (int i = 0; i < 3; ++i) {        // ties between the halves: half 0 first (both lanes must agree on the order)
            rank_own[i] = i; rank_par[i] = i;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                rank_own[i] += (pk[k] < vk[i] || (pk[k] == vk[i] && h == 1)) ? 1 : 0;
                rank_par[i] += (vk[k] < pk[i] || (vk[k] == pk[i] && h == 0)) ? 1 : 0;
            }
        }
        const float kb = fminf(fmaxf(vk[0], pk[0]), fminf(vk[1], pk[1]));
        const double qn = (double)qnorm_s;
        const double e1 = (qn + (double)tmax) * (1.0 / 32768.0);
        constexpr double kTrunc = 1.0001 / 32768.0;
        const double U = (qn + (double)kb + e1 + fabs((double)kb) * kTrunc) * (1.0 + 1.0 / 1048576.0);
        float4 qv[16];
        lds_dma_wait();
#pragma unroll
        for (int c = 0; c < 16; ++c) qv[c] = land[j * 16 + (c ^ (j & 15))];
        for (int r = 0; r < 3; ++r) {
            const int want = 2 * r + h;
            float key = kBig; int row0 = -1;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (rank_own[i] == want) { key = vk[i]; row0 = g0[i]; }
                if (rank_par[i] == want) { key = pk[i]; row0 = pg[i]; }
            }
            const bool cannot = (qn + (double)key - e1 - fabs((double)key) * kTrunc) > U;   // false on NaN: re-rank
            const bool need = row0 >= 0 && qvalid && !cannot;
            if (__ballot(need) == 0ull) break;
            // 16 lanes fetch one 256-B row: DMA instruction i serves the lanes 4 i .. 4 i + 3 (their row of sub-round u)
            const int rsel = need ? row0 : nt;          // nt: past the descriptor, zeros
            int rowsrc[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) rowsrc[i] = __builtin_amdgcn_ds_bpermute((4 * i + (lane >> 4)) * 4, rsel) * 256 + (swz[i & 3] & 255);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the zone's previous contents are in registers
#pragma unroll
            for (int i = 0; i < 16; ++i) lds_dma_b128(lds_land + (uint32_t)i * 1024u, rowsrc[i], frsrc_t, 0);
#pragma unroll
            for (int u = 0; u < GRP; ++u) {
                float4 ra_[16];
                lds_dma_wait();
#pragma unroll
                for (int c = 0; c < 16; ++c) ra_[c] = land[lane * 16 + (c ^ (lane & 15))];
                if (u + 1 < GRP) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                    for (int i = 0; i < 16; ++i) lds_dma_b128(lds_land + (uint32_t)i * 1024u, rowsrc[i] + (u + 1) * 256, frsrc_t, 0);
                }
                const float da = l2sqr64_canonical_regs(qv, ra_);
                const int ta_ = row0 + u;
                insert2(need && ta_ < nt, sqrt_rn_f32(da), ta_, da);
            }
        }
        {
            const float pd0 = __shfl_xor(b0d, 32), pq0 = __shfl_xor(b0q, 32), pd1 = __shfl_xor(b1d, 32), pq1 = __shfl_xor(b1q, 32);
            const int pi0 = __shfl_xor(b0i, 32), pi1 = __shfl_xor(b1i, 32);
            insert2(pi0 >= 0, pd0, pi0, pq0);
            insert2(pi1 >= 0, pd1, pi1, pq1);
        }
        const float tau = fminf(mst.v2, __shfl_xor(mst.v2, 32));
        if (qvalid && h == 0) {
            const size_t o = 2 * ((size_t)pd.out_off + qrow);
            knn_idx[o] = b0i; knn_idx[o + 1] = b1i;
            knn_dist[o] = b0d; knn_dist[o + 1] = b1d;
            bool certified = (tau >= 1.0e38f);       // the empty-slot sentinel; a NaN tau compares false and goes to the re-scan
            if (!certified && b1i >= 0) {
                const double eps = (qn + (double)tmax) * (1.0 / 32768.0) + fabs((double)tau) * (1.0001 / 32768.0);
                certified = (qn + (double)tau - eps) > (double)b1q * (1.0 + 1.0 / 2097152.0);
            }
            if (!certified) {
                const int slot = atomicAdd(&counters[0], 1);
                if (slot < flag_cap) { flagged[2 * slot] = pi; flagged[2 * slot + 1] = qrow; }
                pair_list[pd.out_off + atomicAdd(&pair_cnt[pi], 1)] = qrow;
            }
        }
    }
}

// max |row|^2 and max rho_t of every 256-row block of the bank (l2_knn_bf16x1_kernel takes the maxima over a train set from here: the
// whole blocks inside the set from this table, the rows in front of and behind them one by one).  Launched behind l2_split_bf16_kernel.
__global__ __launch_bounds__(256) void l2_blockmax_kernel(const float *__restrict__ norms, const float *__restrict__ rho_t, long long total_rows,
                                                          float2 *__restrict__ blkmax)
{
    __shared__ float red[8];
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    float m = row < total_rows ? norms[row] : 0.f, r = row < total_rows ? rho_t[row] : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o)); r = fmaxf(r, __shfl_xor(r, o)); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = m; red[4 + (threadIdx.x >> 6)] = r; }
    __syncthreads();
    if (threadIdx.x == 0)
        blkmax[blockIdx.x] = make_float2(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));
}

// ---------------------------------------------------------------------------------------------
// The re-scan of l2_knn_bf16_kernel's uncertified queries, pair by pair.  l2_rescan64_kernel above streams a whole train set per
// QUERY (662 MiB through the L2s for the 662 queries of M-SURF-4k, 295 GB for the 148 k of M-SURF-8k) with one row per lane: a
// load instruction touches 64 cache lines, and the L1 looks up one line per clock -- measured, a workgroup's pass over 1 MiB
// took ~50 us whatever else the chip was doing.  Here
//  * a workgroup takes up to `chunk` uncertified queries of ONE pair (the distance pass bins them per pair) and every train row
//    is compared with all of them; workgroup (p, c) of the chunks_per_pair workgroups of pair p takes the chunks c,
//    c + chunks_per_pair, ... of the pair's list, so one pair with thousands of uncertified queries (duplicated descriptors)
//    still spreads over the chip;
//  * train rows come in by LDS-DMA, 16 lanes per 256-B row (4 rows = 1 KiB per wave instruction, every line touched once), XOR
//    swizzled on the source side like the distance pass's tiles; a wave stages exactly the 64 rows its own lanes consume -- lane l
//    reads row l back with 16 conflict-free ds_read_b128 -- so no workgroup barrier is involved, and the next 64 rows are in
//    flight into the same LDS slice while the current ones (now in registers) are compared;
//  * the queries sit in LDS and are read as broadcasts (every lane the same address); through the scalar cache -- no vector
//    registers at all -- the four s_load_dwordx16 of a row came back one after the other into the same SGPRs, ~1 us per query
//    and group; a thread's two best keys per query live in LDS too (a private 16-B slot per query: the query loop is a real
//    loop, NQ x 4 registers indexed by it would go to scratch).
// Same arithmetic as l2_exact_scan_kernel (l2sqr_canonical's 8 chains and final order, sqrtf, (distance, index) order): the
// result is identical.
template <int NQ>
__global__ __launch_bounds__(256) void l2_rescan64_pairs_kernel(const float *__restrict__ desc, const PairDesc *__restrict__ pairs,
                                                                const int32_t *__restrict__ pair_cnt, const int32_t *__restrict__ pair_list,
                                                                int chunks_per_pair, int chunk /* <= NQ */, int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist)
{
    // (distance, train index) as one 64-bit key: distances are >= +0 and not NaN for finite descriptors, so the bit pattern of the
    // float orders like the float and key order is the (distance, index) order of best2_insert; the two smallest keys are kept
    // without a branch.  ~0 is the empty slot (index -1).
    typedef unsigned long long u64;
    constexpr u64 kEmpty = ~0ull;
    auto key_of = [](float d, int t) { return d < FLT_MAX ? (((u64)__float_as_uint(d) << 32) | (u64)(uint32_t)t) : ~0ull; };   // FLT_MAX, +inf, NaN: never a neighbour (oracle: `d < d1`)
    auto insert2 = [](u64 &b0, u64 &b1, u64 k) {
        const u64 hi = k > b0 ? k : b0;
        b0 = k > b0 ? b0 : k;
        b1 = hi < b1 ? hi : b1;
    };
    __shared__ float4 s_q[NQ][16];
    __shared__ int s_qrow[NQ];
    __shared__ u64 s_k[2][NQ][4];
    extern __shared__ __attribute__((aligned(16))) char smem_rescan[];
    float4 *s_rows = reinterpret_cast<float4 *>(smem_rescan);                                 // [4 waves][64 rows][16 slots]
    ulonglong2 *s_state = reinterpret_cast<ulonglong2 *>(smem_rescan + 4 * 64 * 256);         // [NQ][256]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x / chunks_per_pair, c0 = blockIdx.x - p * chunks_per_pair;
    const PairDesc pd = pairs[p];
    const int cnt = min(pair_cnt[p], pd.nq);
    if (c0 * chunk >= cnt) return;
    const float *Q = desc + (size_t)pd.q_row0 * 64;
    const u32x4 trsrc = raw_buffer_rsrc(desc + (size_t)pd.t_row0 * 64, (uint32_t)pd.nt * 256u);   // rows past nt read as zeros
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t lds_rows = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)s_rows) + (uint32_t)wave_s * (64 * 256);
    const float4 *my_row = s_rows + (size_t)(wave * 64 + lane) * 16;
    int voff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 4 * i + (lane >> 4);                       // rows 16 apart share the swizzle
        voff[i] = row * 256 + (((lane & 15) ^ (row & 15)) * 16);
    }
    const int ngroups = (pd.nt + 255) / 256;                       // 256 train rows per step of the workgroup, 64 per wave
    auto dma_rows = [&](int g) {
        // the whole offset travels in the per-lane operand, which is what the descriptor's range check covers
        const int base = (g * 256 + wave_s * 64) * 256;            // byte offset of this wave's 64 rows
#pragma unroll
        for (int i = 0; i < 16; ++i) lds_dma_b128(lds_rows + (uint32_t)i * 1024u, voff[i & 3] + base + (i >> 2) * (16 * 256), trsrc, 0);
    };
    for (int c = c0; c * chunk < cnt; c += chunks_per_pair) {
        const int nqc = min(chunk, cnt - c * chunk);       // workgroup-uniform
        if (tid < nqc * 16) {
            const int k = tid >> 4, qrow = pair_list[pd.out_off + c * chunk + k];
            s_q[k][tid & 15] = reinterpret_cast<const float4 *>(Q)[(size_t)qrow * 16 + (tid & 15)];
            if ((tid & 15) == 0) s_qrow[k] = qrow;
        }
        for (int k = 0; k < nqc; ++k) s_state[k * 256 + tid] = make_ulonglong2(kEmpty, kEmpty);
        if (ngroups > 0) dma_rows(0);
        __syncthreads();
        for (int g = 0; g < ngroups; ++g) {
            const int t = g * 256 + wave * 64 + lane;
            float4 ta[16];
            lds_dma_wait();
#pragma unroll
            for (int j = 0; j < 16; ++j) ta[j] = my_row[j ^ (lane & 15)];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the slice is in registers: the next rows may overwrite it
            if (g + 1 < ngroups) dma_rows(g + 1);
            for (int k = 0; k < nqc; ++k) {
                const float4 *qk = s_q[k];       // every lane the same address: LDS broadcast reads
                float2v acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};      // l2sqr64_canonical_regs, packed
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float2v av[4] = {{ta[2 * j].x, ta[2 * j].y}, {ta[2 * j].z, ta[2 * j].w}, {ta[2 * j + 1].x, ta[2 * j + 1].y}, {ta[2 * j + 1].z, ta[2 * j + 1].w}};
                    const float4 q0 = qk[2 * j], q1 = qk[2 * j + 1];
                    const float2v qe[4] = {{q0.x, q0.y}, {q0.z, q0.w}, {q1.x, q1.y}, {q1.z, q1.w}};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float2v d = qe[e] - av[e];
                        acc[e] = acc[e] + d * d;
                    }
                }
                const float2v s01 = acc[0] + acc[2], s23 = acc[1] + acc[3];
                const float da = __fadd_rn(__fadd_rn(__fadd_rn(s01.x, s01.y), s23.x), s23.y);
                ulonglong2 st = s_state[k * 256 + tid];
                insert2(st.x, st.y, t < pd.nt ? key_of(sqrt_rn_f32(da), t) : kEmpty);
                s_state[k * 256 + tid] = st;
            }
        }
        for (int k = 0; k < nqc; ++k) {
            const ulonglong2 st = s_state[k * 256 + tid];
            u64 x0 = st.x, x1 = st.y;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const u64 y0 = __shfl_xor(x0, o), y1 = __shfl_xor(x1, o);
                insert2(x0, x1, y0);
                insert2(x0, x1, y1);
            }
            if (lane == 0) { s_k[0][k][wave] = x0; s_k[1][k][wave] = x1; }
        }
        __syncthreads();
        if (tid < nqc) {
            u64 x0 = kEmpty, x1 = kEmpty;
            for (int w = 0; w < 4; ++w) { insert2(x0, x1, s_k[0][tid][w]); insert2(x0, x1, s_k[1][tid][w]); }
            const size_t o = 2 * ((size_t)pd.out_off + s_qrow[tid]);
            const int i0 = (int)(uint32_t)x0, i1 = (int)(uint32_t)x1;
            knn_idx[o] = i0; knn_idx[o + 1] = i1;
            knn_dist[o] = i0 >= 0 ? __uint_as_float((uint32_t)(x0 >> 32)) : FLT_MAX;
            knn_dist[o + 1] = i1 >= 0 ? __uint_as_float((uint32_t)(x1 >> 32)) : FLT_MAX;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// launchers

// 64-float descriptors take the split-bf16 pass (256 queries per workgroup); ESFM_L2_PASS=f32 in the environment keeps them on
// the f32-MFMA kernel (measurement only: bench.py reports both)
bool l2_bf16_pass(int dim)
{
    static const bool forced_f32 = [] { const char *e = getenv("ESFM_L2_PASS"); return e && strcmp(e, "f32") == 0; }();
    return dim == 64 && !forced_f32;
}
constexpr int kL2RescanQueries = 8;   // uncertified queries of one pair that share a pass over the train set (l2_rescan64_pairs_kernel)
constexpr int kL2BfSets = 2;     // query sets of 32 per wave in l2_knn_bf16_kernel (1: 3 waves per SIMD, measured 7-15 % slower)
int l2_query_block(int dim) { return l2_bf16_pass(dim) ? 128 * kL2BfSets : 128; }
size_t l2_split_bytes(int dim, long long total_rows) { return l2_bf16_pass(dim) ? (size_t)512 * (size_t)std::max(total_rows, 1LL) : 0; }

int launch_l2_split_bf16(hipStream_t st, const float *desc, long long total_rows, void *split, float *norms, int32_t *counters,
                         int32_t *pair_cnt, int n_pairs, void *hi, int32_t *pair_cnt2)
{
    // `split` holds two images of 256 B per row: the train operand, then the query operand (-2 x); NULL when only the one-product
    // pass and its refine pass follow (they read the dense hi images in `hi`): 52 MB less to write per 25 x 4096 rows
    const long long n_pieces = std::max(total_rows * 16, (long long)std::max(n_pairs, 16));     // the launch also zeroes counters / pair_cnt
    hipLaunchKernelGGL(l2_split_bf16_kernel, dim3((unsigned)((n_pieces + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const float4 *>(desc), total_rows * 16, reinterpret_cast<u32x4 *>(split),
                       split ? reinterpret_cast<u32x4 *>(split) + (size_t)std::max(total_rows, 1LL) * 16 : nullptr, norms, counters, pair_cnt, n_pairs,
                       hi ? reinterpret_cast<u32x4 *>(l2_hi_part(hi, total_rows, 0)) : nullptr,
                       hi ? reinterpret_cast<u32x4 *>(l2_hi_part(hi, total_rows, 1)) : nullptr,
                       hi ? reinterpret_cast<float *>(l2_hi_part(hi, total_rows, 2)) : nullptr,
                       hi ? reinterpret_cast<float *>(l2_hi_part(hi, total_rows, 3)) : nullptr, pair_cnt2);
    ESFM_HIP_TRY(hipGetLastError());
    if (hi && total_rows > 0) {
        hipLaunchKernelGGL(l2_blockmax_kernel, dim3((unsigned)((total_rows + 255) / 256)), dim3(256), 0, st, norms,
                           reinterpret_cast<const float *>(l2_hi_part(hi, total_rows, 2)), total_rows, reinterpret_cast<float2 *>(l2_hi_part(hi, total_rows, 4)));
        ESFM_HIP_TRY(hipGetLastError());
    }
    return ESFM_OK;
}

int launch_l2_knn_bf16(hipStream_t st, const float *desc, const void *split, long long total_rows, const float *norms, const PairDesc *pairs,
                       int n_pairs, int n_blocks, int32_t *knn_idx, float *knn_dist, int32_t *flagged, int32_t *counters, int flag_cap,
                       int32_t *pair_cnt, int32_t *pair_list)
{
    if (n_blocks <= 0) return ESFM_OK;
    constexpr int TT = 128;   // train rows per LDS tile: one barrier per 96 MFMAs per wave
    constexpr size_t lds = 2 * TT * 16 * 16 + 2 * TT * 4 + 16 + kL2BfSets * 6 * 256 * 4;   // two tiles, their norms, the master top-3
    static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
    const u32x4 *sp = reinterpret_cast<const u32x4 *>(split);
    const u32x4 *sq = sp + (size_t)std::max(total_rows, 1LL) * 16;
    hipLaunchKernelGGL(l2_knn_bf16_kernel, dim3(n_blocks), dim3(256), lds, st, desc, sp, sq, norms, pairs,
                       n_pairs, knn_idx, knn_dist, flagged, counters, flag_cap, pair_cnt, pair_list);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_l2_rescan64_pairs(hipStream_t st, const float *desc, const PairDesc *pairs, int n_pairs, const int32_t *pair_cnt,
                             const int32_t *pair_list, int32_t *knn_idx, float *knn_dist)
{
    if (n_pairs <= 0) return ESFM_OK;
    // about 4096 workgroups whatever the pair count: a workgroup without work leaves after one load.  Few pairs: the launch is as
    // long as its longest workgroup (a 16-step latency chain per 4096 train rows), so the chunks are small -- more workgroups, two
    // per CU; many pairs: throughput counts, the chunks are as large as the kernel's LDS allows (M-SURF-8k-like launch of 2415
    // pairs: 1.85 ms with chunks of 2, 1.33 with 3, 1.28 with 8).
    const int chunks_per_pair = std::max(1, std::min(512, 4096 / n_pairs));
    ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&l2_rescan64_pairs_kernel<kL2RescanQueries>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 256 + kL2RescanQueries * 256 * 16));
    const int chunk = n_pairs >= 2048 ? kL2RescanQueries : 3;     // 3: 64 + 12 + 3 KB of LDS, still two workgroups per CU (measured 1: 69, 2: 65, 3: 60, 4: 92 us)
    hipLaunchKernelGGL(l2_rescan64_pairs_kernel<kL2RescanQueries>, dim3((unsigned)n_pairs * (unsigned)chunks_per_pair), dim3(256),
                       (size_t)4 * 64 * 256 + (size_t)chunk * 256 * 16, st, desc, pairs,
                       pair_cnt, pair_list, chunks_per_pair, chunk, knn_idx, knn_dist);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

}  // namespace esfm
