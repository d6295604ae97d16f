// Hamming matching (DESIGN.md section 4.4, rows HM_FP4, HM_I8 and HM_VALU): XOR-popcount for 128- and 512-bit rows, the byte-per-bit
// i8-MFMA kernel and the nibble-per-bit FP4-MFMA kernel for 256-bit rows, and the two expanders that write their operand images.
#include "match_kernels.hpp"
#include "match_device.hpp"
#include "hmx1_segment_gfx950.inc"     // ESFM_HMX1_SEGMENT_ASM: the one-product loop around v_mfma_f32_32x32x64_f8f6f4 on FP4 operands (256-bit Hamming)

#include <float.h>
#include <type_traits>
#include <stdlib.h>
#include <string.h>

namespace esfm {

// ---------------------------------------------------------------------------------------------
// Hamming 2-NN (ORB).  One thread per query row, descriptor words in VGPRs; the train row is
// wave-uniform, so it is fetched through the scalar cache (s_load) and XOR'd against the VGPRs.
// key = distance << 22 | train index: one u32 min orders by (distance, index) exactly.
template <int NW>
__global__ __launch_bounds__(256) void hamming_knn_kernel(const uint32_t *__restrict__ desc, const PairDesc *__restrict__ pairs,
                                                          int n_pairs, int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist)
{
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = find_pair_by_block(pairs, n_pairs, lb);
    const PairDesc pd = pairs[pi];
    const int qrow = (lb - pd.blk_off) * 256 + threadIdx.x;
    const bool qvalid = qrow < pd.nq;
    uint32_t qw[NW];
    {
        const uint32_t *qp = desc + ((size_t)pd.q_row0 + (qvalid ? qrow : 0)) * NW;
#pragma unroll
        for (int w = 0; w < NW; ++w) qw[w] = qp[w];
    }
    const uint32_t *__restrict__ T = desc + (size_t)pd.t_row0 * NW;
    uint32_t k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu;
    const int nt = pd.nt;
#pragma unroll 16
    for (int t = 0; t < nt; ++t) {
        const uint32_t *tp = T + (size_t)t * NW;  // wave-uniform address
        uint32_t d = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) d += __popc(qw[w] ^ tp[w]);
        const uint32_t key = (d << 22) | (uint32_t)t;
        const uint32_t hi = max(k0, key);
        k0 = min(k0, key);
        k1 = min(k1, hi);
    }
    if (qvalid) {
        const size_t o = 2 * ((size_t)pd.out_off + qrow);
        const bool h0 = nt >= 1, h1 = nt >= 2;
        knn_idx[o] = h0 ? (int)(k0 & 0x3FFFFFu) : -1;
        knn_idx[o + 1] = h1 ? (int)(k1 & 0x3FFFFFu) : -1;
        knn_dist[o] = h0 ? (float)(k0 >> 22) : FLT_MAX;
        knn_dist[o + 1] = h1 ? (float)(k1 >> 22) : FLT_MAX;
    }
}

// ---------------------------------------------------------------------------------------------
// Hamming 2-NN for 256-bit descriptors (ORB) on the i8 matrix cores.  Bits are stored as 0/1 bytes; the query operand
// enters the MFMA doubled (0/2) and each train's accumulator starts at 256 - popcount(t), so that
//   acc = 256 - popcount(t) + 2 popcount(t & q) = 256 + popcount(q) - hamming(q, t),
// an exact integer identity: `v_mfma_i32_32x32x32_i8` ranks 32 trains x 32 queries x 32 bits at a time (larger acc =
// closer), and the per-query constant is removed when the two winners are written.  The operand encoding is chosen for
// the matrix pipe's power draw, which is what sets its clock here: on the symmetric +-1 expansion (dot = 256 - 2 ham, half
// the bytes 0xFF) the same kernel is 18 % slower, and bare MFMA loops over this workload's 2.6 POP take 0.68 ms on 0/1
// x 0/1 operands, 0.73 ms on zeros x +-1 and 0.87 ms on +-1 x +-1 -- a "peak" measured on constant operands overstates
// what random descriptors reach, and 0/1 trains against +-1 queries gain nothing: both operands have to be sparse.
// A = train rows (so that a lane's 16 results belong to ONE query, column lane & 31, and 16 different trains), B = query
// columns held in registers for the whole kernel (2 sets of 32 queries per wave: 64 VGPRs), train tiles of 64 rows
// staged through LDS (LDS-DMA, 16-B slots XOR-swizzled with row & 15: conflict-free ds_read_b128) together with their 64
// start values, shared by the 4 waves.  K is contracted in whatever order the hardware pairs the 16 bytes a lane supplies -- A and B are loaded with
// the same lane->byte convention, and the sum does not depend on it.
// Top-2: running (best, second) pairs of keys acc << 21 | (2^21 - 1 - L), largest first, with L = 16 * (32-train group
// number) + accumulator register -- a wave-uniform scalar, so a result costs v_lshl_add + v_max_u32 + v_med3_u32.  Within
// a lane L grows with the train index (row(r) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) is monotonic in r), so key order =
// (distance ascending, train index ascending); four independent pairs per query set give the VALU chain some slack.
// The train index is rebuilt from L at the end, where the slots and the two lane halves are merged.
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

constexpr int kHmTT = 64;          // trains per LDS tile
constexpr int kHmQB = 256;         // queries per workgroup (4 waves x 2 sets x 32)
constexpr uint32_t kHmLMask = 0x1FFFFFu;

// bits -> 0/1 bytes, one 32-bit word (32 output bytes) per thread; the 8 threads of a row also leave 256 - popcount(row)
__global__ __launch_bounds__(256) void hamming_expand_kernel(const uint32_t *__restrict__ desc, long long n_words, uint32_t *__restrict__ out,
                                                             int32_t *__restrict__ start)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const uint32_t w = i < n_words ? desc[i] : 0u;
    int pop = __popc(w);
    pop += __shfl_xor(pop, 1);
    pop += __shfl_xor(pop, 2);
    pop += __shfl_xor(pop, 4);
    if (i >= n_words) return;
    if ((i & 7) == 0) start[i >> 3] = 256 - pop;
    uint32_t o[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const uint32_t x = (w >> (4 * g)) & 0xFu;
        o[g] = (x & 1u) | ((x & 2u) << 7) | ((x & 4u) << 14) | ((x & 8u) << 21);   // one 0/1 byte per bit
    }
    uint4 *dst = reinterpret_cast<uint4 *>(out + i * 8);
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// keeps the two largest keys seen, m1 >= m2
__device__ __forceinline__ void key_insert_max(uint32_t &m1, uint32_t &m2, uint32_t key)
{
    uint32_t med;   // second largest of (m1 >= m2, key); operands are VALU results, no MFMA hazard to pad
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(med) : "v"(m1), "v"(m2), "v"(key));
    m1 = max(m1, key);
    m2 = med;
}

__global__ __launch_bounds__(256, 2) void hamming_knn_mfma_kernel(const unsigned char *__restrict__ ex, const int32_t *__restrict__ start,
                                                               const uint32_t *__restrict__ packed, const PairDesc *__restrict__ pairs, int n_pairs,
                                                               int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][kHmTT * 256];   // 256-B rows, 16-B slots XOR-swizzled with row & 15
    __shared__ __attribute__((aligned(16))) int32_t lds_start[2][kHmTT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = find_pair_by_block(pairs, n_pairs, lb);
    const PairDesc pd = pairs[pi];
    const int nq = pd.nq, nt = pd.nt;
    const unsigned char *__restrict__ Q = ex + (size_t)pd.q_row0 * 256;
    const unsigned char *__restrict__ T = ex + (size_t)pd.t_row0 * 256;
    const int32_t *__restrict__ TS = start + pd.t_row0;
    const int qbase = (lb - pd.blk_off) * kHmQB + wave * 64;

    // B operand: the query rows doubled (0/2 bytes), 8 K-chunks of 32 bytes, this lane's 16
    i32x4 bq[2][8];
    int qpop[2];   // set bits of this lane's query (both lane halves hold the same query)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int qrow = qbase + 32 * s + j;
        const bool ok = qrow < nq;
        const i32x4 *qp = reinterpret_cast<const i32x4 *>(Q + (size_t)(ok ? qrow : 0) * 256 + h * 16);
        int pop = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            i32x4 v = qp[2 * c];
            if (!ok) v = i32x4{0, 0, 0, 0};
            pop += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
            bq[s][c] = i32x4{v.x << 1, v.y << 1, v.z << 1, v.w << 1};
        }
        qpop[s] = pop + __shfl_xor(pop, 32);
    }
    // Two-level top-2, as in l2_knn_bf16_kernel: a lane's 16 results of a 32-train step are four groups of four consecutive
    // train rows (accumulator registers 4g .. 4g+3 = rows 8g + 4h + 0..3); the hot loop keeps the two best GROUPS per lane
    // (key = group maximum << 21 | 2^21 - 1 - (4 step + g): two v_max3, one v_lshl_add, max + med3 = 5 VALU per 4 results instead of
    // 12), and the tail counts the bits of the kept groups' rows exactly.  No certificate is involved: the scores are exact
    // integers, the two nearest rows lie in the two groups with the best maxima of the lane half that holds them (a group that
    // precedes the second nearest row's group in key order contains a row that precedes that row in (distance, index) order, and
    // there is only one such row), and ties between groups go to the lower train index like ties between rows.
    uint32_t m1[2][2], m2[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 2; ++r) { m1[s][r] = 0u; m2[s][r] = 0u; }

    const int n_tiles = (nt + kHmTT - 1) / kHmTT;
    const int n_full = nt / kHmTT;       // tiles with all 64 rows inside the set: the software-pipelined loop
    // Staging is LDS-DMA (buffer_load_dwordx4 ... lds, 4 rows = 1 KiB per wave instruction) with the swizzle applied on the
    // source side, issued from inline asm so that hipcc does not order the tile's LDS reads behind the transfer, and waited for
    // explicitly in front of the barrier -- the scheme of l2_knn_bf16_kernel.  Start values go through a register, loaded
    // before the tile's DMA and stored at the end of the iteration.
    const u32x4 trsrc = raw_buffer_rsrc(T, (uint32_t)nt * 256u);
    const uint32_t lds_addr = (uint32_t)(uintptr_t)&lds[0][0];
    const int wrow0 = __builtin_amdgcn_readfirstlane(wave * 16);             // this wave moves rows [wrow0, wrow0 + 16) of a tile
    int voff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = wrow0 + 4 * i + (lane >> 4);
        voff[i] = row * 256 + (((lane & 15) ^ (row & 15)) * 16);
    }
    auto dma_tile = [&](int tile, int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t dst = lds_addr + (uint32_t)(buf * kHmTT * 256 + (wrow0 + 4 * i) * 256);
            const int soff = tile * kHmTT * 256;
            lds_dma_b128(dst, voff[i], trsrc, soff);
        }
    };
    auto start_load = [&](int tile) { return (tid < kHmTT && tile * kHmTT + tid < nt) ? TS[tile * kHmTT + tid] : 0; };
    auto start_store = [&](int buf, int32_t sv) { if (tid < kHmTT) lds_start[buf][tid] = sv; };
    if (n_tiles > 0) {
        const int32_t sv = start_load(0);
        start_store(0, sv);
        dma_tile(0, 0);
    }
    lds_dma_wait();
    __syncthreads();

    // the accumulator start values of a 32-train step, in the C/D register order: rows 8 g + 4 h + (0..3), g = 0..3
    auto load_start = [&](int buf, int sub) {
        const i32x4 *sp = reinterpret_cast<const i32x4 *>(&lds_start[buf][sub * 32 + 4 * h]);
        const i32x4 g0 = sp[0], g1 = sp[2], g2 = sp[4], g3 = sp[6];
        return i32x16{g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x, g2.y, g2.z, g2.w, g3.x, g3.y, g3.z, g3.w};
    };
    // group g of a step's results p (set s) into the lane's two best groups; pK = 2^21 - 1 - 4 (step number of p)
    auto group_insert = [&](int s, int g, const i32x16 &p, uint32_t pK) {
        const int gm = max(max(p[4 * g], p[4 * g + 1]), max(p[4 * g + 2], p[4 * g + 3]));
        key_insert_max(m1[s][g & 1], m2[s][g & 1], ((uint32_t)gm << 21) + (pK - g));
    };
    // One 32-train step: 16 MFMAs into (c0, c1), with the fold of the PREVIOUS step's results (p0, p1) issued in their shadow --
    // one group insert (5 VALU) behind every second MFMA of a set -- so the matrix pipe and the VALU run concurrently.
    // arow = the lane's train row in LDS; its K-chunk c is the 16-B slot 2 c + h, stored at slot ^ (row & 15) = ^ (j & 15)
    auto step = [&](const unsigned char *arow, const i32x16 &c_init, i32x16 &c0, i32x16 &c1, const i32x16 &p0, const i32x16 &p1, uint32_t pK) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const i32x4 a = *reinterpret_cast<const i32x4 *>(arow + (((2 * c + h) ^ (j & 15)) * 16));
            c0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[0][c], c == 0 ? c_init : c0, 0, 0, 0);
            if (c & 1) group_insert(0, c >> 1, p0, pK);
            c1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[1][c], c == 0 ? c_init : c1, 0, 0, 0);
            if (c & 1) group_insert(1, c >> 1, p1, pK);
        }
    };
    // start-up placeholders: acc 0 with pK = 15 gives keys 12..15, below every real key (real 4 step + g < 2^21 - 16)
    i32x16 pa0, pa1, pb0, pb1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { pb0[r] = 0; pb1[r] = 0; }
    uint32_t pbK = 15u;
    for (int tile = 0; tile < n_full; ++tile) {
        const int buf = tile & 1;
        const bool more = tile + 1 < n_tiles;
        int32_t nxt_start = 0;
        if (more) {
            nxt_start = start_load(tile + 1);
            dma_tile(tile + 1, buf ^ 1);                                       // lands under this tile's MFMAs
        }
        const unsigned char *arow = &lds[buf][j * 256];
        step(arow, load_start(buf, 0), pa0, pa1, pb0, pb1, pbK);                                        // sub 0, folding the previous tile's sub 1
        step(arow + 32 * 256, load_start(buf, 1), pb0, pb1, pa0, pa1, kHmLMask - (uint32_t)(tile * 2) * 4u);   // sub 1, folding sub 0
        pbK = kHmLMask - (uint32_t)(tile * 2 + 1) * 4u;
        __builtin_amdgcn_sched_barrier(0);
        if (more) start_store(buf ^ 1, nxt_start);
        lds_dma_wait();                                                        // the DMA issued above has landed
        __syncthreads();
    }
    // drain the pipeline
#pragma unroll
    for (int g = 0; g < 4; ++g) { group_insert(0, g, pb0, pbK); group_insert(1, g, pb1, pbK); }
    // the partial tile at the end of the set; rows past it are zero-filled with start value 0: their score 0 is the worst there
    // is, and the tail skips them by index
    if (n_full < n_tiles) {
        const int tile = n_full, buf = tile & 1;
#pragma unroll 1
        for (int sub = 0; sub < 2; ++sub) {
            const i32x16 c_init = load_start(buf, sub);
            i32x16 acc0 = c_init, acc1 = c_init;
            const unsigned char *arow = &lds[buf][(sub * 32 + j) * 256];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const i32x4 a = *reinterpret_cast<const i32x4 *>(arow + (((2 * c + h) ^ (j & 15)) * 16));
                acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[0][c], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[1][c], acc1, 0, 0, 0);
            }
            const uint32_t K0 = kHmLMask - (uint32_t)(tile * 2 + sub) * 4u;
#pragma unroll
            for (int g = 0; g < 4; ++g) { group_insert(0, g, acc0, K0); group_insert(1, g, acc1, K0); }
        }
    }
    // ---- tail: the kept groups' rows counted exactly on the packed descriptors (32 B per row) ----
    // The two nearest rows of a query lie in the two best groups of ALL its groups, so the four kept ones (two per lane half) are
    // first merged -- keys rebuilt with the group's first train row in the position field, which orders groups of different lane
    // halves like their rows -- and each lane of the pair counts ONE group: 4 rows, 8 loads.
    // row key = distance << 21 | train index: the smallest two are the (distance, index)-first two.
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    auto key_insert_min = [](uint32_t &k1, uint32_t &k2, uint32_t key) {
        const uint32_t hi = max(k1, key);
        k1 = min(k1, key);
        k2 = min(k2, hi);
    };
    const u32x4 *P = reinterpret_cast<const u32x4 *>(packed);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int qrow = qbase + 32 * s + j;
        const bool qvalid = qrow < nq;
        uint32_t g1 = 0u, g2 = 0u;
#pragma unroll
        for (int r = 0; r < 2; ++r) { key_insert_max(g1, g2, m1[s][r]); key_insert_max(g1, g2, m2[s][r]); }
        // position field: 2^21 - 1 - (first row / 4) = 2^21 - 1 - (8 step + 2 g + h); placeholders (below 16) become 0
        auto global_key = [&](uint32_t k) {
            const uint32_t L = kHmLMask - (k & kHmLMask);
            return k < 16u ? 0u : ((k & ~kHmLMask) | (kHmLMask - (2u * L + (uint32_t)h)));
        };
        g1 = global_key(g1); g2 = global_key(g2);
        const uint32_t p1 = __shfl_xor(g1, 32), p2 = __shfl_xor(g2, 32);
        key_insert_max(g1, g2, p1);
        key_insert_max(g1, g2, p2);                                        // both lanes of the pair now hold the query's two best groups
        const uint32_t mine = h == 0 ? g1 : g2;
        const bool live = mine != 0u && qvalid;
        const int row0 = (int)(kHmLMask - (mine & kHmLMask)) * 4;
        const u32x4 *qp = P + ((size_t)pd.q_row0 + (qvalid ? qrow : 0)) * 2;
        const u32x4 q0 = qp[0], q1 = qp[1];
        u32x4 t0[4], t1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = min(row0 + u, max(nt - 1, 0));
            const u32x4 *tp = P + ((size_t)pd.t_row0 + (live ? t : 0)) * 2;
            t0[u] = tp[0]; t1[u] = tp[1];
        }
        uint32_t k1 = kNone, k2 = kNone;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = row0 + u;
            const int dist = __popc(q0.x ^ t0[u].x) + __popc(q0.y ^ t0[u].y) + __popc(q0.z ^ t0[u].z) + __popc(q0.w ^ t0[u].w) +
                             __popc(q1.x ^ t1[u].x) + __popc(q1.y ^ t1[u].y) + __popc(q1.z ^ t1[u].z) + __popc(q1.w ^ t1[u].w);
            key_insert_min(k1, k2, (live && t < nt) ? (((uint32_t)dist << 21) | (uint32_t)t) : kNone);
        }
        const uint32_t o1 = __shfl_xor(k1, 32), o2 = __shfl_xor(k2, 32);
        key_insert_min(k1, k2, o1);
        key_insert_min(k1, k2, o2);
        if (h == 0 && qvalid) {
            const size_t o = 2 * ((size_t)pd.out_off + qrow);
            const bool h0 = k1 != kNone, h1 = k2 != kNone;
            knn_idx[o] = h0 ? (int)(k1 & kHmLMask) : -1;
            knn_idx[o + 1] = h1 ? (int)(k2 & kHmLMask) : -1;
            knn_dist[o] = h0 ? (float)(k1 >> 21) : FLT_MAX;
            knn_dist[o + 1] = h1 ? (float)(k2 >> 21) : FLT_MAX;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 256-bit Hamming on the FP4 matrix cores (round 4).  hamming(q, t) = pop(q) + pop(t) - 2 q.t, and q.t over 0/1 bits is a dot product
// of 256 NIBBLES: t's bits as e2m1 1.0 (0x2), q's as -2.0 (0xC), accumulated in f32 on top of a start value pop(t) + 512 --
// exact small integers, positive, with 14 zero bits at the low end of the mantissa.  A row of 256 nibbles is 128 B = four K-steps of
// v_mfma_f32_32x32x64_f8f6f4 (cbsz = blgp = 4: FP4 x FP4, 16 B per lane and K-step): byte for byte the shapes of the one-product L2
// pass, so the whole main loop -- LDS-DMA ring of two 256-row tiles, four query sets per wave, fold groups of eight with the
// position in the low mantissa bits -- is that pass's generator with another instruction (hmx1_segment_gfx950.inc).  The FP4
// instruction moves 64 K per 8 passes where v_mfma_i32_32x32x32_i8 moves 32 (measured 7.7 against 4.2 Pop/s by a
// microbenchmark that also checked the products exact), at half the operand bytes of the byte-per-bit form.
// No certificate: the scores are exact, a group key IS the group's smallest score.  With code order = row order inside a lane half,
// the nearest row sits in the half's smallest key's group and the second nearest in one of its two smallest (a group in front of it
// would hold a row in front of it in (distance, index) order, and there is only one such row), and a group whose score exceeds the
// second smallest score of all eight keys holds neither.  The tail counts the bits of those groups' rows exactly on the packed
// descriptors, in (distance, index) order.  Ratio screen as in the L2 pass, exact here: d0 = score(k0) - 512 + pop(q) is the nearest
// distance, the second smallest key bounds the second nearest from above, and (double) d0 >= ratio (double) U1 rejects (marker -2).
typedef int i32x4h __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void hamming_expand_fp4_kernel(const uint32_t *__restrict__ desc, long long n_words, u32x4 *__restrict__ img_t,
                                                                 u32x4 *__restrict__ img_q, float *__restrict__ start)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const uint32_t w = i < n_words ? desc[i] : 0u;
    int pop = __popc(w);
    pop += __shfl_xor(pop, 1);
    pop += __shfl_xor(pop, 2);
    pop += __shfl_xor(pop, 4);
    if (i >= n_words) return;
    if ((i & 7) == 0) start[i >> 3] = (float)(pop + 512);
    u32x4 t, q;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        uint32_t b = (w >> (8 * d)) & 0xFFu, x = 0u;
#pragma unroll
        for (int n = 0; n < 8; ++n) x |= ((b >> n) & 1u) << (4 * n + 1);      // nibble n = bit 8 d + n as 0x2 (e2m1 1.0)
        t[d] = x; q[d] = x * 6u;                                              // 0x2 -> 0xC (-2.0): no carries between nibbles
    }
    img_t[i] = t; img_q[i] = q;
}

__global__ __launch_bounds__(256, 2) void hamming_fp4_kernel(const uint32_t *__restrict__ packed, const u32x4 *__restrict__ img_t,
                                                             const u32x4 *__restrict__ img_q, const float *__restrict__ start,
                                                             const PairDesc *__restrict__ pairs, const int32_t *__restrict__ blk_pair, int n_blocks,
                                                             int32_t *__restrict__ knn_idx, float *__restrict__ knn_dist, double ratio,
                                                             int32_t *__restrict__ done, int n_pairs, int32_t *__restrict__ query_idx,
                                                             int32_t *__restrict__ train_idx, float *__restrict__ distance, int32_t *__restrict__ n_out)
{
    // (a pair without queries has no block: nobody would write its count)
    if (done && blockIdx.x == 0) for (int p = threadIdx.x; p < n_pairs; p += 256) if (pairs[p].nq == 0) n_out[p] = 0;
    constexpr int TT = ESFM_HMX1_TT, NS = ESFM_HMX1_SETS, K = ESFM_HMX1_KEEP, RING = ESFM_HMX1_RING, GRP = ESFM_HMX1_GRP, NG = 16 / GRP;
    constexpr int QB = 128 * NS, HS = 8;
    constexpr int TILE_BYTES = TT * HS * 16;
    static_assert(NS == 4 && (GRP == 8 || GRP == 16) && RING * TT == 512 && K >= 2, "written for the L2 one-product pass's shapes");
    constexpr uint32_t kCodeMask = (1u << ESFM_HMX1_CODE_BITS) - 1u;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u32x4 *lds_tile = reinterpret_cast<u32x4 *>(smem);
    float *lds_norm = reinterpret_cast<float *>(smem + RING * TILE_BYTES);
    int lane = threadIdx.x & 63;
    const int wave_s = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int tid = threadIdx.x, j = lane & 31, h = lane >> 5;
    const uint32_t lds_tile_addr = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds_tile);
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = blk_pair[lb];
    const PairDesc pd = pairs[pi];
    const int nq = __builtin_amdgcn_readfirstlane(pd.nq), nt = __builtin_amdgcn_readfirstlane(pd.nt);
    const int q_row0 = __builtin_amdgcn_readfirstlane(pd.q_row0), t_row0 = __builtin_amdgcn_readfirstlane(pd.t_row0);
    const int qblk = lb - __builtin_amdgcn_readfirstlane(pd.blk_off2);
    const int ntiles = (nt + TT - 1) / TT;
    const float *__restrict__ tn = start + t_row0;
    const u32x4 trsrc = raw_buffer_rsrc(img_t + (size_t)t_row0 * HS, (uint32_t)nt * (HS * 16));
    const u32x4 nrsrc = raw_buffer_rsrc(tn, (uint32_t)nt * 4u);
    if (ntiles * TT != nt || ntiles < RING) {
        for (int i = tid; i < RING * TT * HS; i += 256) lds_tile[i] = u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
    }
#pragma unroll
    for (int b = 0; b < RING; ++b) {
#pragma unroll
        for (int i = 0; i < TT / 32; ++i) {
            const int row = wave_s * (TT / 4) + 8 * i + (lane >> 3);
            const int voff = row * (HS * 16) + (((lane & 7) ^ ((row >> 1) & 7)) * 16);
            lds_dma_b128(lds_tile_addr + (uint32_t)(b * TILE_BYTES + (wave_s * (TT / 4) + 8 * i) * (HS * 16)), voff, trsrc, b * TILE_BYTES);
        }
    }
    u32x4 bq[NS][4];
    {
        const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4 *>(img_q + (size_t)q_row0 * HS), 0, nq * (HS * 16), 0x00020000);
        const int qbase0 = qblk * QB + wave_s * 32 * NS;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int voff = (qbase0 + 32 * s + j) * (HS * 16) + h * 16;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) bq[s][ks] = __builtin_amdgcn_raw_buffer_load_b128(qrsrc, voff + 32 * ks, 0, 0);
        }
    }
    {
        float big;
        asm volatile("s_mov_b32 %0, 0x7f61b1e6" : "=s"(big));
#pragma unroll
        for (int u = 0; u < 2; ++u) { const int t = tid + 256 * u; lds_norm[t] = t < nt ? tn[t] : big; }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (ntiles > 0) {
        asm volatile(ESFM_HMX1_SEGMENT_ASM
                     :
                     : "v"(bq[0][0]), "v"(bq[0][1]), "v"(bq[0][2]), "v"(bq[0][3]), "v"(bq[1][0]), "v"(bq[1][1]), "v"(bq[1][2]), "v"(bq[1][3]),
                       "v"(bq[2][0]), "v"(bq[2][1]), "v"(bq[2][2]), "v"(bq[2][3]), "v"(bq[3][0]), "v"(bq[3][1]), "v"(bq[3][2]), "v"(bq[3][3]),
                       "s"(ntiles), "s"(nt), "s"(trsrc), "s"(nrsrc), "s"(lds_tile_addr), "s"(wave_s)
                     : ESFM_HMX1_SEGMENT_CLOBBERS);
    }
    {   // (nothing thread-dependent lives across the block: see l2_knn_bf16x1_kernel)
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        lane = l; tid = wave_s * 64 + l; j = l & 31; h = l >> 5;
    }
    float key0[NS], key1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        key0[s] = reinterpret_cast<const float *>(smem)[(K * s + 0) * 256 + tid];
        key1[s] = reinterpret_cast<const float *>(smem)[(K * s + 1) * 256 + tid];
    }
    if (ntiles == 0) {
        float big;
        asm volatile("s_mov_b32 %0, 0x7f61b1e6" : "=s"(big));
#pragma unroll
        for (int s = 0; s < NS; ++s) { key0[s] = big; key1[s] = big; }
    }
    // ---- tail: exact (distance, index)-first two rows of every query that the screen lets through
    constexpr uint32_t kNone = 0xFFFFFFFFu, kIdxMask = 0x1FFFFFu;
    auto key_insert_min = [](uint32_t &k1, uint32_t &k2, uint32_t key) {
        const uint32_t hi = max(k1, key);
        k1 = min(k1, key);
        k2 = min(k2, hi);
    };
    const u32x4 *P = reinterpret_cast<const u32x4 *>(packed);
    const int qbase = qblk * QB + wave_s * 32 * NS;
    float fltmax; int minus2;
    asm volatile("s_mov_b32 %0, 0x7f7fffff" : "=s"(fltmax));
    asm volatile("s_mov_b32 %0, -2" : "=s"(minus2));
#pragma unroll 1                         // (unrolled by 2 / 4 -- the four sets' row loads in flight together -- measured: 0.442 / 0.441 ms against 0.443)
    for (int s = 0; s < NS; ++s) {
        const int qrow = qbase + 32 * s + j;
        const bool qvalid = qrow < nq;
        const float v0 = s == 0 ? key0[0] : (s == 1 ? key0[1] : (s == 2 ? key0[2] : key0[3]));
        const float v1 = s == 0 ? key1[0] : (s == 1 ? key1[1] : (s == 2 ? key1[2] : key1[3]));
        const float p0 = other_half(v0, h != 0), p1 = other_half(v1, h != 0);
        const float k0 = fminf(v0, p0), kb = fminf(fmaxf(v0, p0), fminf(v1, p1));           // the two smallest of the eight keys
        const float thr = __uint_as_float(__float_as_uint(kb) & ~kCodeMask);                   // ... the second one's score
        const float qpop = start[q_row0 + (qvalid ? qrow : 0)] - 512.f;
        // ratio screen (exact): d0 and an upper bound of d1
        const double d0 = (double)(__uint_as_float(__float_as_uint(k0) & ~kCodeMask) - 512.f + qpop), U1 = (double)(thr - 512.f + qpop);
        const bool rej = qvalid && kb < 1.0e38f && d0 >= ratio * U1;                           // (+inf ratio: never; one row only: re-rank)
        uint32_t k1 = kNone, k2 = kNone;
        const u32x4 *qp = P + ((size_t)q_row0 + (qvalid ? qrow : 0)) * 2;
        const u32x4 q0 = qp[0], q1 = qp[1];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float key = i == 0 ? v0 : v1;
            const float score = __uint_as_float(__float_as_uint(key) & ~kCodeMask);
            const bool need = qvalid && !rej && key < 1.0e38f && score <= thr;
            if (need) {
                const int code = (int)(__float_as_uint(key) & kCodeMask);
                const int row0 = (code / NG) * 32 + (32 / NG) * (code % NG) + 4 * h;
#pragma unroll
                for (int hb = 0; hb < GRP / 8; ++hb) {         // eight rows at a time: rows {0..3, 8..11} (+ 16 hb) of the step, + 4 h
                    u32x4 t0[8], t1[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int t = min(row0 + 16 * hb + (u & 3) + 8 * (u >> 2), max(nt - 1, 0));
                        const u32x4 *tp = P + ((size_t)t_row0 + t) * 2;
                        t0[u] = tp[0]; t1[u] = tp[1];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int t = row0 + 16 * hb + (u & 3) + 8 * (u >> 2);
                        const int dist = __popc(q0[0] ^ t0[u][0]) + __popc(q0[1] ^ t0[u][1]) + __popc(q0[2] ^ t0[u][2]) + __popc(q0[3] ^ t0[u][3]) +
                                         __popc(q1[0] ^ t1[u][0]) + __popc(q1[1] ^ t1[u][1]) + __popc(q1[2] ^ t1[u][2]) + __popc(q1[3] ^ t1[u][3]);
                        key_insert_min(k1, k2, t < nt ? (((uint32_t)dist << 21) | (uint32_t)t) : kNone);
                    }
                }
            }
        }
        const uint32_t o1 = __float_as_uint(other_half(__uint_as_float(k1), h != 0)), o2 = __float_as_uint(other_half(__uint_as_float(k2), h != 0));
        key_insert_min(k1, k2, o1);
        key_insert_min(k1, k2, o2);
        if (h == 0 && qvalid) {
            const size_t o = 2 * ((size_t)pd.out_off + qrow);
            const bool h0 = !rej && k1 != kNone, h1 = !rej && k2 != kNone;
            const int i0 = rej ? minus2 : (h0 ? (int)(k1 & kIdxMask) : -1), i1 = rej ? minus2 : (h1 ? (int)(k2 & kIdxMask) : -1);
            const float f0 = h0 ? (float)(k1 >> 21) : fltmax, f1 = h1 ? (float)(k2 >> 21) : fltmax;
            if (done) {       // another workgroup of this launch reads the records (the ratio stage below): write-through stores
                st_coh_i(knn_idx + o, i0); st_coh_i(knn_idx + o + 1, i1); st_coh_f(knn_dist + o, f0); st_coh_f(knn_dist + o + 1, f1);
            } else {
                *reinterpret_cast<int2 *>(knn_idx + o) = make_int2(i0, i1);
                *reinterpret_cast<float2 *>(knn_dist + o) = make_float2(f0, f1);
            }
        }
    }
    // ---- the match entry points: ratio test + ordered compaction of the pair by the workgroup that brings its last block (the
    // protocol of l2_finish_kernel: stores acknowledged, barrier, one relaxed agent-scope arrival; `done` reads 0 again afterwards)
    if (done) {
        __shared__ int s_last, s_wave[4], s_base;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int nblk = (nq + QB - 1) / QB;
        if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&done[pi], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblk - 1;
        __syncthreads();
        if (!s_last) return;
        if (threadIdx.x == 0) __hip_atomic_store(&done[pi], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ratio_compact_pair<256, 16, true>(pd, knn_idx, knn_dist, ratio, query_idx, train_idx, distance, n_out + pi, s_wave, &s_base);
    }
}

// ---------------------------------------------------------------------------------------------
// launchers

// queries per workgroup of the kernel that serves this descriptor width (the pair plan's block count depends on it)
int hamming_query_block(int nbytes) { return 256; }

// the 0/1 byte image of every descriptor followed by one start value (256 - popcount) per row
size_t hamming_expanded_bytes(int nbytes, long long total_rows) { return nbytes == 32 ? (size_t)(256 + 4) * (size_t)std::max(total_rows, 1LL) : 0; }

int launch_hamming_expand(hipStream_t st, int nbytes, const void *desc, long long total_rows, void *exp_scratch)
{
    if (nbytes != 32 || !exp_scratch || total_rows <= 0) return ESFM_OK;
    const long long n_words = total_rows * 8;
    int32_t *start = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(exp_scratch) + (size_t)256 * (size_t)std::max(total_rows, 1LL));
    hipLaunchKernelGGL(hamming_expand_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(desc), n_words,
                       reinterpret_cast<uint32_t *>(exp_scratch), start);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_hamming_knn(hipStream_t st, int nbytes, const void *desc, long long total_rows, void *exp_scratch, const PairDesc *pairs,
                       int n_pairs, int n_blocks, int32_t *knn_idx, float *knn_dist, bool expanded)
{
    if (n_blocks <= 0) return ESFM_OK;
    const uint32_t *d = reinterpret_cast<const uint32_t *>(desc);
    if (nbytes == 32 && exp_scratch) {
        int32_t *start = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(exp_scratch) + (size_t)256 * (size_t)std::max(total_rows, 1LL));
        if (!expanded)
            if (int rc = launch_hamming_expand(st, nbytes, desc, total_rows, exp_scratch)) return rc;
        hipLaunchKernelGGL(hamming_knn_mfma_kernel, dim3(n_blocks), dim3(256), 0, st, reinterpret_cast<const unsigned char *>(exp_scratch),
                           start, d, pairs, n_pairs, knn_idx, knn_dist);
    } else if (nbytes == 32)
        hipLaunchKernelGGL(hamming_knn_kernel<8>, dim3(n_blocks), dim3(256), 0, st, d, pairs, n_pairs, knn_idx, knn_dist);
    else if (nbytes == 64)
        hipLaunchKernelGGL(hamming_knn_kernel<16>, dim3(n_blocks), dim3(256), 0, st, d, pairs, n_pairs, knn_idx, knn_dist);
    else if (nbytes == 16)
        hipLaunchKernelGGL(hamming_knn_kernel<4>, dim3(n_blocks), dim3(256), 0, st, d, pairs, n_pairs, knn_idx, knn_dist);
    else {
        set_error("hamming kernel is built for 16/32/64-byte descriptors (got %d)", nbytes);
        return ESFM_ERR_UNSUPPORTED;
    }
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

bool hamming_fp4_pass()
{
    static const bool off = [] { const char *e = getenv("ESFM_HM_PASS"); return e && strcmp(e, "i8") == 0; }();
    return !off;
}
bool hamming_fp4_supported(int nbytes, int max_nt) { return nbytes == 32 && hamming_fp4_pass() && max_nt <= (1 << (ESFM_HMX1_CODE_BITS - 1)) * 32 && max_nt < (1 << 21); }

// the FP4 form's operands: nibble images of every row in both roles (128 B each) and pop(row) + 512 as a float -- the same 260 B per
// row as the byte image + start value of the i8 form (hamming_expanded_bytes)
int launch_hamming_expand_fp4(hipStream_t st, const void *desc, long long total_rows, void *exp_scratch)
{
    if (!exp_scratch || total_rows <= 0) return ESFM_OK;
    const long long n_words = total_rows * 8;
    unsigned char *base = static_cast<unsigned char *>(exp_scratch);
    const size_t n = (size_t)std::max(total_rows, 1LL);
    hipLaunchKernelGGL(hamming_expand_fp4_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(desc), n_words,
                       reinterpret_cast<u32x4 *>(base), reinterpret_cast<u32x4 *>(base + 128 * n), reinterpret_cast<float *>(base + 256 * n));
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

int launch_hamming_fp4(hipStream_t st, const void *desc, long long total_rows, void *exp_scratch, const PairDesc *pairs, const int32_t *blk_pair,
                       int n_blocks, int32_t *knn_idx, float *knn_dist, double ratio, bool expanded, int32_t *done, int n_pairs, int32_t *query_idx,
                       int32_t *train_idx, float *distance, int32_t *n_out)
{
    if (n_blocks <= 0) return ESFM_OK;
    if (!expanded)
        if (int rc = launch_hamming_expand_fp4(st, desc, total_rows, exp_scratch)) return rc;
    constexpr size_t lds = 4 * 128 * 128 + 4 * 128 * 4 + 64;      // ring of nibble tiles, their start values (the keys leave through the ring)
    ESFM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&hamming_fp4_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    unsigned char *base = static_cast<unsigned char *>(exp_scratch);
    const size_t n = (size_t)std::max(total_rows, 1LL);
    // (the ratio test's own compare is `(double) d0 < ratio * (double) d1`: a NaN or negative ratio rejects nothing here)
    const double r = (ratio >= 0.0 && ratio < 1.0e150) ? ratio : (double)INFINITY;
    hipLaunchKernelGGL(hamming_fp4_kernel, dim3(n_blocks), dim3(256), lds, st, reinterpret_cast<const uint32_t *>(desc), reinterpret_cast<const u32x4 *>(base),
                       reinterpret_cast<const u32x4 *>(base + 128 * n), reinterpret_cast<const float *>(base + 256 * n), pairs, blk_pair, n_blocks, knn_idx,
                       knn_dist, done ? ratio : r, done, n_pairs, query_idx, train_idx, distance, n_out);
    ESFM_HIP_TRY(hipGetLastError());
    return ESFM_OK;
}

}  // namespace esfm
