// What every matcher kernel shares (device code; included by .hip files only): vector types, the LDS-DMA staging, the block -> pair
// look-ups, the CANONICAL DISTANCE -- l2sqr_canonical and its register / row16 / LDS forms, the oracle's summation order
// (oracle/match_ref.c esfm_ref_l2sqr), bit-exact by contract -- the (distance, index) order, the coherent accesses and the ratio test
// with its ordered compaction.  This header is the single home of these: the five matcher .hip files and guided_kernels.hip all include it, so
// "guided with an infinite threshold equals the plain matcher" holds by construction.
#pragma once

#include <float.h>

#include "pair_desc.hpp"

namespace esfm {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------
// LDS-DMA staging (buffer_load_dwordx4 ... lds): lane l of the wave writes its 16 bytes to lds_dst + 16 l, from byte
// voff (per lane) + soff (wave-uniform) of the buffer.  Issued from inline asm on purpose: through the builtin hipcc orders
// every later LDS read behind vmcnt(0) (it cannot tell a double buffer's halves apart) and the transfer would serialise with the
// compute it is meant to hide under.  The asm is invisible to the waitcnt pass, so the CALLER waits: lds_dma_wait() in front of
// the barrier that publishes the tile.  M0 (the LDS base of the transfer) is saved and restored around the instruction.
__device__ __forceinline__ u32x4 raw_buffer_rsrc(const void *base, uint32_t bytes)
{
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    u32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((uint32_t)b);
    r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32) & 0xFFFFu);   // stride 0: raw buffer
    r[2] = __builtin_amdgcn_readfirstlane(bytes);                            // the per-lane offset is range-checked against it
    r[3] = 0x00020000u;
    return r;
}
__device__ __forceinline__ void lds_dma_b128(uint32_t lds_dst /* wave-uniform */, int voff, u32x4 rsrc, int soff /* wave-uniform */)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_dst), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
__device__ __forceinline__ void lds_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---------------------------------------------------------------------------------------------
// helpers

__device__ __forceinline__ int xcd_remap(int bid, int nb)
{
    // Blocks are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8).  Give each XCD a
    // contiguous range of logical blocks so that the blocks sharing one pair's train set hit the
    // same 4 MiB L2.  Bijective for any nb.
    const int q = nb >> 3, r = nb & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

__device__ __forceinline__ int find_pair_by_block(const PairDesc *pairs, int n_pairs, int lb)
{
    int lo = 0, hi = n_pairs - 1;  // last p with blk_off[p] <= lb
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (pairs[mid].blk_off <= lb) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int find_pair_by_query(const PairDesc *pairs, int n_pairs, long long gq)
{
    int lo = 0, hi = n_pairs - 1;  // last p with out_off[p] <= gq
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (pairs[mid].out_off <= gq) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Squared L2 distance in the oracle's canonical order (oracle/match_ref.c esfm_ref_l2sqr):
// 8 partial sums over blocks of 8, separate multiply and add (no FMA), (acc[c]+acc[c+4]) summed
// left to right, then the scalar tail.  Bit-exact with the CPU restatement.
template <bool VEC>
__device__ __forceinline__ float l2sqr_canonical(const float *__restrict__ a, const float *__restrict__ b, int n)
{
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int j = 0;
    for (; j <= n - 8; j += 8) {
        float av[8], bv[8];
        if (VEC) {
            const float4 a0 = *reinterpret_cast<const float4 *>(a + j), a1 = *reinterpret_cast<const float4 *>(a + j + 4);
            const float4 b0 = *reinterpret_cast<const float4 *>(b + j), b1 = *reinterpret_cast<const float4 *>(b + j + 4);
            av[0] = a0.x; av[1] = a0.y; av[2] = a0.z; av[3] = a0.w; av[4] = a1.x; av[5] = a1.y; av[6] = a1.z; av[7] = a1.w;
            bv[0] = b0.x; bv[1] = b0.y; bv[2] = b0.z; bv[3] = b0.w; bv[4] = b1.x; bv[5] = b1.y; bv[6] = b1.z; bv[7] = b1.w;
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) { av[c] = a[j + c]; bv[c] = b[j + c]; }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float t = __fsub_rn(av[c], bv[c]);
            acc[c] = __fadd_rn(acc[c], __fmul_rn(t, t));
        }
    }
    const float s0 = __fadd_rn(acc[0], acc[4]);
    const float s1 = __fadd_rn(acc[1], acc[5]);
    const float s2 = __fadd_rn(acc[2], acc[6]);
    const float s3 = __fadd_rn(acc[3], acc[7]);
    float d = __fadd_rn(s0, s1);
    d = __fadd_rn(d, s2);
    d = __fadd_rn(d, s3);
    for (; j < n; ++j) {
        const float t = __fsub_rn(a[j], b[j]);
        d = __fadd_rn(d, __fmul_rn(t, t));
    }
    return d;
}

// l2sqr_canonical for 64-float rows held in registers: the same 8 chains, the same final order.
// (Measured in the distance pass's tail: the packed form below made the whole kernel 1.5 % SLOWER -- 1.499 -> 1.522 ms; the
// tail's arithmetic runs beside the other workgroup's MFMAs and the chip is power-limited there -- so the tail keeps this one.)
__device__ __forceinline__ float l2sqr64_canonical_regs(const float4 (&a)[16], const float4 (&b)[16])
{
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float av[8] = {a[2 * j].x, a[2 * j].y, a[2 * j].z, a[2 * j].w, a[2 * j + 1].x, a[2 * j + 1].y, a[2 * j + 1].z, a[2 * j + 1].w};
        const float bv[8] = {b[2 * j].x, b[2 * j].y, b[2 * j].z, b[2 * j].w, b[2 * j + 1].x, b[2 * j + 1].y, b[2 * j + 1].z, b[2 * j + 1].w};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float t = __fsub_rn(av[c], bv[c]);
            acc[c] = __fadd_rn(acc[c], __fmul_rn(t, t));
        }
    }
    const float s0 = __fadd_rn(acc[0], acc[4]);
    const float s1 = __fadd_rn(acc[1], acc[5]);
    const float s2 = __fadd_rn(acc[2], acc[6]);
    const float s3 = __fadd_rn(acc[3], acc[7]);
    float d = __fadd_rn(s0, s1);
    d = __fadd_rn(d, s2);
    return __fadd_rn(d, s3);
}
// The same with a row spread over SIXTEEN LANES (lane l of a 16-lane DPP row holds floats 4 l .. 4 l + 3 of both operands): float
// 4 l + x belongs to chain c = 4 (l & 1) + x at step j = l >> 1, so a chain runs over the lanes of equal parity in lane order --
// seven `row_shr:2` additions  A_k[l] = A_(k-1)[l - 2] + d[l]  (A_0 = d; the chain's 0 + d_0 is d_0) leave chains 0 .. 3 in lane 14
// and 4 .. 7 in lane 15; lane 15 then forms s_x = acc[x] + acc[x + 4] and ((s0 + s1) + s2) + s3.  The result is valid in lane 15
// of every row (four rows per wave).  Same operations on the same operands in the same order as l2sqr64_canonical_regs.
__device__ __forceinline__ float dpp_row_shr_f(float v, int n_is_2)
{
    return n_is_2 ? __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xF, 0xF, true))
                  : __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, true));
}
__device__ __forceinline__ float l2sqr64_canonical_row16(const u32x4 a, const u32x4 b)
{
    float d[4], acc[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const float t = __fsub_rn(__uint_as_float(a[x]), __uint_as_float(b[x]));
        d[x] = __fmul_rn(t, t);
        acc[x] = d[x];
    }
#pragma unroll
    for (int k = 1; k < 8; ++k)
#pragma unroll
        for (int x = 0; x < 4; ++x) acc[x] = __fadd_rn(dpp_row_shr_f(acc[x], 1), d[x]);
    float sx[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) sx[x] = __fadd_rn(dpp_row_shr_f(acc[x], 0), acc[x]);      // lane 15: acc[x] of lane 14 + acc[x + 4] of its own
    float r = __fadd_rn(sx[0], sx[1]);
    r = __fadd_rn(r, sx[2]);
    return __fadd_rn(r, sx[3]);
}
// The same on two rows that sit in LDS as 16 x 16 B with their slots XOR-swizzled (slot c of a row at piece c ^ sw): the pieces are
// read as they are used, so neither row has to be held in 64 registers.  a_row / b_row: LDS byte address of the row, a_sw16 / b_sw16:
// 16 sw.  The 32 piece addresses are formed HERE, every time, from operands the compiler cannot see through (one v_xad_u32 each): as
// ordinary loop invariants they are hoisted out of the caller's loops, live across everything, get spilled, and every LDS read then
// waits for the scratch reload of its own address (seen in the re-rank: 219 spilled registers).  Same 8 chains, same final order.
typedef float floatx4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const floatx4_t *lds_cf4p;
__device__ __forceinline__ float l2sqr64_canonical_lds(uint32_t a_row, uint32_t a_sw16, uint32_t b_row, uint32_t b_sw16)
{
    asm volatile("" : "+v"(a_sw16), "+v"(b_sw16));
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const floatx4_t a0 = *(lds_cf4p)(uintptr_t)((a_sw16 ^ (uint32_t)(32 * j)) + a_row), a1 = *(lds_cf4p)(uintptr_t)((a_sw16 ^ (uint32_t)(32 * j + 16)) + a_row);
        const floatx4_t b0 = *(lds_cf4p)(uintptr_t)((b_sw16 ^ (uint32_t)(32 * j)) + b_row), b1 = *(lds_cf4p)(uintptr_t)((b_sw16 ^ (uint32_t)(32 * j + 16)) + b_row);
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float t = __fsub_rn(av[c], bv[c]);
            acc[c] = __fadd_rn(acc[c], __fmul_rn(t, t));
        }
    }
    const float s0 = __fadd_rn(acc[0], acc[4]);
    const float s1 = __fadd_rn(acc[1], acc[5]);
    const float s2 = __fadd_rn(acc[2], acc[6]);
    const float s3 = __fadd_rn(acc[3], acc[7]);
    float d = __fadd_rn(s0, s1);
    d = __fadd_rn(d, s2);
    return __fadd_rn(d, s3);
}
// Two neighbouring chains of l2sqr64_canonical_regs per packed instruction (v_pk_add_f32 / v_pk_mul_f32: every half is an IEEE single
// operation, the result is bit-identical): l2_rescan64_pairs_kernel, which has the chip to itself, sums on these.
typedef float float2v __attribute__((ext_vector_type(2)));

// Correctly rounded f32 square root.  NOT __fsqrt_rn: in this toolchain that maps to
// __ocml_native_sqrt_f32 (about 1 ulp), while sqrtf is IEEE-exact under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt and matches the CPU's sqrtss bit for bit.
__device__ __forceinline__ float sqrt_rn_f32(float x) { return sqrtf(x); }

// (distance, index) ordered pair; "better" = the order a stable ascending scan with strict-<
// insertion produces (OpenCV batchDistance): smaller distance, ties to the lower train index.
struct Cand { float d; int i; float d2; };

__device__ __forceinline__ bool cand_better(float d, int i, const Cand &b)
{
    // an empty slot holds FLT_MAX: like the oracle's strict `d < d1`, a distance of FLT_MAX, +inf or NaN is never a neighbour
    return (i >= 0) && (d < b.d || (d == b.d && i < b.i));
}

__device__ __forceinline__ void best2_insert(Cand &b0, Cand &b1, float d, int i, float d2)
{
    if (cand_better(d, i, b1)) {
        if (cand_better(d, i, b0)) { b1 = b0; b0.d = d; b0.i = i; b0.d2 = d2; }
        else { b1.d = d; b1.i = i; b1.d2 = d2; }
    }
}

// the value of lane ^ 32 (v_permlane32_swap, gfx950: the upper half of its first operand changes places with the lower half of the
// second); upper = this lane is in the upper half
__device__ __forceinline__ float other_half(float x, bool upper)
{
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(upper ? r[0] : r[1]);
}

// ---------------------------------------------------------------------------------------------
// coherent (agent-scope, relaxed) accesses to what one workgroup of a pair writes and another reads inside l2_finish_kernel's launch
__device__ __forceinline__ void st_coh_i(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_coh_f(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t ld_coh_i(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_coh_f(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// N x 16 contiguous bytes (dword aligned) with agent-scope coherence (`sc1`: the load is served past this XCD's L2), all in flight at once
template <int N>
__device__ __forceinline__ void ld_coh_block(const void *p, uint32_t *out /* 4 N */)
{
    static_assert(N == 4 || N == 8 || N == 2, "offsets below are immediates");
    u32x4 v[N];
    if constexpr (N == 8)
        asm volatile("global_load_dwordx4 %0, %8, off sc1\n\tglobal_load_dwordx4 %1, %8, off offset:16 sc1\n\tglobal_load_dwordx4 %2, %8, off offset:32 sc1\n\t"
                     "global_load_dwordx4 %3, %8, off offset:48 sc1\n\tglobal_load_dwordx4 %4, %8, off offset:64 sc1\n\tglobal_load_dwordx4 %5, %8, off offset:80 sc1\n\t"
                     "global_load_dwordx4 %6, %8, off offset:96 sc1\n\tglobal_load_dwordx4 %7, %8, off offset:112 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7]) : "v"(p) : "memory");
    else if constexpr (N == 4)
        asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %4, off offset:16 sc1\n\tglobal_load_dwordx4 %2, %4, off offset:32 sc1\n\t"
                     "global_load_dwordx4 %3, %4, off offset:48 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(p) : "memory");
    else
        asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(v[0]), "=&v"(v[1]) : "v"(p) : "memory");
#pragma unroll
    for (int i = 0; i < N; ++i) { out[4 * i] = v[i][0]; out[4 * i + 1] = v[i][1]; out[4 * i + 2] = v[i][2]; out[4 * i + 3] = v[i][3]; }
}

// ---------------------------------------------------------------------------------------------
// Lowe ratio test (feature_matching.cpp:88 / :133: float < double * float, i.e. in double) and an order-preserving compaction of one
// pair's survivors, by the THREADS threads of a workgroup, THREADS * kRatioPer queries per sweep (one round of loads for a 4096-row
// set in either instantiation).  A thread takes kRatioPer CONSECUTIVE queries (their 2-NN records are
// 32 + 32 contiguous bytes), so the survivors' order is thread order, then query order inside the thread: an exclusive scan of the
// threads' counts places them.  A train index < 0 (no neighbour; -2: dropped by the one-product pass's ratio screen) never passes; a
// SECOND index of -3 says that pass has proved d0 < ratio d1 without looking for the second neighbour.
// (Round 1: 256 threads, one query each, 16 sweeps of three barriers for a 4096-row set: 14 us per launch.)
// The reference's test on one 2-NN record (i0, i1, d0, d1): every filter that applies it calls this one predicate
// (ratio_compact_pair, ratio_compact_pair_sparse, cross_check_compact_kernel), so ratio+cross can only keep what ratio keeps.
__device__ __forceinline__ bool ratio_ok(int i0, int i1, float d0, float d1, double ratio)
{
    return i0 >= 0 && (i1 == -3 || (i1 >= 0 && (double)d0 < ratio * (double)d1));     // -3: the one-product pass proved the test
}

template <int THREADS, int kRatioPer, bool COHERENT = false>
__device__ __forceinline__ void ratio_compact_pair(const PairDesc &pd, const int32_t *__restrict__ knn_idx, const float *__restrict__ knn_dist,
                                                   double ratio, int32_t *__restrict__ query_idx, int32_t *__restrict__ train_idx,
                                                   float *__restrict__ distance, int32_t *__restrict__ n_out_p, int *s_wave /* [THREADS / 64] */,
                                                   int *s_base)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) *s_base = 0;
    __syncthreads();
    for (int q0 = 0; q0 < pd.nq; q0 += THREADS * kRatioPer) {
        const int qa = q0 + tid * kRatioPer;
        int ti[kRatioPer]; float d0[kRatioPer]; bool pass[kRatioPer];
        int cnt = 0;
        // COHERENT: the records may have been written by another workgroup of this launch (l2_finish_kernel, through write-through
        // stores): they are read past this XCD's L2 -- `sc1` loads -- sixteen bytes at a time (one asm statement per array: as
        // 4-byte atomic loads the same reads took 80 us per launch)
        int iv[2 * kRatioPer]; float dv[2 * kRatioPer];
        if (COHERENT && (kRatioPer % 2) == 0 && qa + kRatioPer <= pd.nq) {
            ld_coh_block<kRatioPer / 2>(knn_idx + 2 * ((size_t)pd.out_off + qa), reinterpret_cast<uint32_t *>(iv));
            ld_coh_block<kRatioPer / 2>(knn_dist + 2 * ((size_t)pd.out_off + qa), reinterpret_cast<uint32_t *>(dv));
        } else {
#pragma unroll
            for (int u = 0; u < kRatioPer; ++u) {
                const size_t o = 2 * ((size_t)pd.out_off + min(qa + u, max(pd.nq - 1, 0)));
                iv[2 * u] = COHERENT ? ld_coh_i(knn_idx + o) : knn_idx[o]; iv[2 * u + 1] = COHERENT ? ld_coh_i(knn_idx + o + 1) : knn_idx[o + 1];
                dv[2 * u] = COHERENT ? ld_coh_f(knn_dist + o) : knn_dist[o]; dv[2 * u + 1] = COHERENT ? ld_coh_f(knn_dist + o + 1) : knn_dist[o + 1];
            }
        }
#pragma unroll
        for (int u = 0; u < kRatioPer; ++u) {
            const int q = qa + u;
            const int i0 = iv[2 * u], i1 = iv[2 * u + 1];
            const float d1 = dv[2 * u + 1];
            d0[u] = dv[2 * u]; ti[u] = i0;
            pass[u] = q < pd.nq && ratio_ok(i0, i1, d0[u], d1, ratio);
            cnt += pass[u] ? 1 : 0;
        }
        // exclusive scan of cnt over the workgroup: inside the wave by shuffles, across waves through LDS
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int off = *s_base;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        size_t o = (size_t)pd.out_off + off + (incl - cnt);
#pragma unroll
        for (int u = 0; u < kRatioPer; ++u) {
            if (pass[u]) { query_idx[o] = qa + u; train_idx[o] = ti[u]; distance[o] = d0[u]; ++o; }
        }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < THREADS / 64; ++w) t += s_wave[w]; *s_base += t; }
        __syncthreads();
    }
    if (tid == 0) *n_out_p = *s_base;
}

// The same over the ratio screen's SURVIVORS only (l2_finish_kernel when the screen ran): whatever is not on the pair's survivor list
// has been dropped by the screen and has no record at all (the one-product pass writes no markers outside the audit modes: 16 bytes
// per query it does not store and this stage does not read -- 19.6 of 19.7 MB per step on the metric's workload).  A sweep of
// THREADS * 16 queries: the survivors' rows set bits in an LDS bitmap, a thread looks at its 16 consecutive queries' bits and reads
// the records of the set ones; order and compaction as above.
// COH: the survivor entries too were written by other workgroups of this launch (l2_fused_kernel): their rows are read with ld_coh_f.
template <int THREADS, bool COH = false>
__device__ __forceinline__ void ratio_compact_pair_sparse(const PairDesc &pd, const float4 *__restrict__ ent, int nsv,
                                                          const int32_t *__restrict__ knn_idx, const float *__restrict__ knn_dist,
                                                          double ratio, int32_t *__restrict__ query_idx, int32_t *__restrict__ train_idx,
                                                          float *__restrict__ distance, int32_t *__restrict__ n_out_p,
                                                          uint32_t *s_bits /* [THREADS / 2] */, int *s_wave /* [THREADS / 64] */, int *s_base)
{
    constexpr int PER = 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) *s_base = 0;
    for (int q0 = 0; q0 < pd.nq; q0 += THREADS * PER) {
        for (int w = tid; w < THREADS / 2; w += THREADS) s_bits[w] = 0u;
        __syncthreads();
        for (int k = tid; k < nsv; k += THREADS) {
            const float rowf = COH ? ld_coh_f(reinterpret_cast<const float *>(ent) + 12 * (size_t)k + 8) : ent[3 * (size_t)k + 2].x;
            const uint32_t r = (uint32_t)(__float_as_int(rowf) - q0);
            if (r < (uint32_t)(THREADS * PER)) atomicOr(&s_bits[r >> 5], 1u << (r & 31));
        }
        __syncthreads();
        const int qa = q0 + tid * PER;
        uint32_t bits = (s_bits[tid >> 1] >> ((tid & 1) * PER)) & 0xFFFFu;
        int ti[PER]; float d0[PER];
        uint32_t passm = 0;
        for (uint32_t b = bits; b; b &= b - 1) {
            const int u = __ffs(b) - 1;
            const size_t o = 2 * ((size_t)pd.out_off + qa + u);
            uint32_t iv[4];          // (records written by other workgroups of this launch: read past this XCD's L2)
            asm volatile("global_load_dwordx2 %0, %2, off sc1\n\tglobal_load_dwordx2 %1, %3, off sc1\n\ts_waitcnt vmcnt(0)"
                         : "=&v"(*reinterpret_cast<uint2 *>(iv)), "=&v"(*reinterpret_cast<uint2 *>(iv + 2)) : "v"(knn_idx + o), "v"(knn_dist + o) : "memory");
            const int i0 = (int)iv[0], i1 = (int)iv[1];
            const float dd0 = __uint_as_float(iv[2]), dd1 = __uint_as_float(iv[3]);
            const bool pass = qa + u < pd.nq && ratio_ok(i0, i1, dd0, dd1, ratio);
            // (static indexing keeps ti / d0 in registers)
#pragma unroll
            for (int e = 0; e < PER; ++e) if (e == u) { ti[e] = i0; d0[e] = dd0; }
            passm |= pass ? (1u << u) : 0u;
        }
        const int cnt = __popc(passm);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int off = *s_base;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        size_t o = (size_t)pd.out_off + off + (incl - cnt);
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if ((passm >> u) & 1u) { query_idx[o] = qa + u; train_idx[o] = ti[u]; distance[o] = d0[u]; ++o; }
        }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < THREADS / 64; ++w) t += s_wave[w]; *s_base += t; }
        __syncthreads();
    }
    if (tid == 0) *n_out_p = *s_base;
}

}  // namespace esfm
