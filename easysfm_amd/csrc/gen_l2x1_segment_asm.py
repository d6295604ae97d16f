#!/usr/bin/env python3
"""Generates the hand-scheduled main loop of the ONE-product distance passes, as ONE inline-asm block for a wave's 128 queries over
the whole train set with the fused top-K fold:
  l2x1_segment_gfx950.inc  (default)            the bf16 L2 pass, l2_knn_bf16x1_kernel and the fused kernel (match_kernels.hip):
                                                q.t ~ bf16(q).bf16(t) on v_mfma_f32_16x16x32_bf16 -- the "16x16x32" schedule;
  hmx1_segment_gfx950.inc  (ESFM_GEN_MFMA=fp4)  the 256-bit Hamming matcher: v_mfma_f32_32x32x64_f8f6f4 on e2m1 nibbles, one per bit
                                                -- the "32x32" schedule.
The schedule follows from the instruction.  Switches: ESFM_GEN_MFMA (bf16 | fp4), ESFM_GEN_KEEP (K, keys per lane and set),
ESFM_GEN_STEP_BITS, ESFM_GEN_PREFIX (macro prefix of the file); the Makefile sets them.

1. THE RING -- what both schedules share (the emit_* functions below; a schedule hands them its register map and its step)

  train image  rows of 128 bytes (64 bf16 features / 256 nibbles) = eight 16-byte slots.  In LDS, slot s of ring row r sits at
            physical slot s ^ key(r) (lds_phys_slot), so that every 16-lane group of a ds_read_b128 covers the 64 banks exactly
            once; the key is the schedule's (swz32, swz16) and repeats every 32 rows.
  ring      RING tile buffers of TT rows, 64 KiB, the tiles' |t|^2 behind them (RING x TT floats).  Wave w stages rows
            [WROWS w, WROWS (w + 1)) of a tile by LDS-DMA, 8 rows (1 KiB) per instruction: lane l fetches, into physical slot l & 7
            of row l >> 3 of the piece, the logical slot (l & 7) ^ key(row) (dma_write).  Pieces i and i + 4 are 32 rows apart and
            share the source-offset register.  LDS-DMA destinations stay below 64 KiB: M0 carries the address (saved in s43).  A
            tile's |t|^2 travel through one VGPR per ring slot.
  step      32 train rows x 128 queries.  The A fragments and the start values (|t|^2 of the step's rows) are prefetched a whole
            step ahead, into the registers of the other step parity.
  hand-over of tile t = the top of its last step: every read of the tile was issued a step ago and is waited for, the wave's own
            transfers of tile t + 1 are waited for (vmcnt) and its norms written to LDS -- kBig for rows past nt --, barrier; then
            the norm load and the NP DMA pieces of tile t + RING ride behind the MFMAs of that last step (a tile that does not
            exist reads zeros through the descriptors into a buffer nobody reads again: unconditional).  The caller has staged
            the first RING tiles and written their norms.
  fold      a GROUP is 8 results of a lane: group G (0, 1) of lane half h of a step = train rows 16 G + 4 h + (0..3) and
            16 G + 8 + 4 h + (0..3).  4 v_min3 give its minimum, v_and_or puts the POSITION CODE (step << 1 | G, CODE_BITS =
            STEP_BITS + 1 bits) into the low mantissa bits, K v_med3 insert the key into the set's K sorted keys.  No segments, no
            master list: the keys a block ends with name their rows directly.  11 step bits are 65 536 rows (larger train sets
            skip the L2 pass); the coarser keys (2^-11 relative) are noise next to the bf16 operand rounding (2^-8).  The FP4
            form's scores are small integers that leave 14 zero mantissa bits: 13 step bits, 262 144 rows.  K > 3 for the L2 pass's
            certificate; exact scores need none: two keys per lane half are enough there.
  keys      leave through LDS once the ring is dead (every wave is past its last step, every transfer has landed): key i of the
            32-query set s of thread tid at float (K s + i) * 256 + tid.
  registers v[112 : 112 + K nsets) keys: set s, rank i = v[112 + K s + i]; the rest behind them in one order (reg_map): a_addr,
            n_addr, 4 DMA source offsets, norm source offset, norm LDS address, 4 ring norm registers, 4 scratch, 4 fold temporaries,
            key mask, then the schedule's own.  All are clobbered.
            s40 tile  s43 saved M0  s48-s51 scratch  s52 kBig  s53 -kBig
  operands  (inputs only)  %0-%15 B fragments, set major;  %16 tile count;  %17 nt;  %18 train image buffer descriptor;  %19 train
            norms buffer descriptor;  %20 LDS address of the ring;  %21 wave index.

2. THE 32x32 SCHEDULE (gen32; the fp4 form)

  lanes     FOUR sets of 32 queries.  Lane l = (j = l & 31, h = l >> 5) reads, as its A fragment of K-step ks (64 nibbles), slot
            2 ks + h of row j of the step (a_read32); key(r) = (r >> 1) & 7 (swz32): within a 16-lane group j >> 1 takes eight
            values twice, once per 128-byte half.  Start values: the lane's 16 of the step's 32.
  slots     16 MFMAs.  Six accumulator register sets for the four query sets: sets 2 and 3 have ONE each, sets 0 and 1 alternate
            between two (even / odd steps).  MFMA order inside a step
      slot   0      1      2      3      4      5      6      7      8      9      10     11     12     13     14     15
      MFMA  (0,0)  (1,0)  (2,0)  (3,0)  (2,1)  (3,1)  (2,2)  (3,2)  (2,3)  (3,3)  (0,1)  (1,1)  (0,2)  (1,2)  (0,3)  (1,3)     (set, K-step)
            so that the single-buffered sets finish at slots 8 / 9 and are overwritten at slots 2 / 3 of the next step: their folds
            (two slots after the last MFMA: the results must have left the pipe) take the eight gaps behind slots 10 .. 15, 0', 1';
            the folds of sets 0 and 1 (whose registers are not touched by the next step) the eight gaps behind slots 2' .. 9'.  A
            gap carries a QUARTER of a set's fold: quarter 2 G the minimum and the code of group G (5 VALU), quarter 2 G + 1 its
            K v_med3 -- 4.5 VALU per MFMA at K = 4.  Two accumulators per set do not fit beside 64 registers of B operands; a
            first version with four register sets folded each set right in front of the MFMA that overwrote it: no overlap at
            all, fold and matrix time simply added up (0.47 + 0.21 = 0.68 ms).
  registers v[0:15] v[16:31]   accumulators of query sets 0, 1 in even steps      acc_odd (32, behind the key mask)  ... in odd steps
            v[32:47] v[48:63]  accumulators of query sets 2, 3
            v[64:79] v[80:95]  A fragments of even / odd steps: K-step ks = v[64 + 16 par + 4 ks : +3]
            v[96:111]          start values;   a_addr: one per K-step (4)
            s41 code base of the step being folded  s42 step index  s44, s45 codes of the two groups
  operands  %0-%15 = B[s][ks], 4 sets x 4 K-steps.

3. THE 16x16x32 SCHEDULE (gen16; the bf16 form).  The chip holds a higher clock on v_mfma_f32_16x16x32_bf16 than on 32x32x16 at equal
   cycles per FLOP; everything that leaves the block is what the 32x32 schedule leaves.

  lanes     EIGHT sets of 16 queries: set 2 s + b = queries 16 b .. 16 b + 15 of the 32-query set s.  Lane l = (n = l & 15,
            c = l >> 4) holds query n of each set; its B fragment of K-step ks (32 features) is slot 4 ks + c of the query's row.
            A 32-train step is two VIRTUAL 16-row tiles v = 0, 1 per set.  A-fragment lane (n, c) reads slot 4 ks + c of train row
            16 G + 8 v + 4 h + i of the step, n = 8 h + 4 G + i (a_read).  Output lane (n, c) holds virtual rows 4 c .. 4 c + 3 of
            query n: with c = 2 h + G ("quarter" c) these are the eight rows of group G of lane half h.  One quarter folds one
            group per set and step, under the lane's code (a VGPR); K keys per quarter and set.
            key(r) = ((r >> 1) & 3) | ((r >> 2) & 4) (swz16): the 16 rows {0..7, 16..23} + 8 v of a read cover the 64 banks once
            per 16-lane group.  v and the ring buffer are address offsets (the key ignores bit 3); the two K-steps are two
            address registers.
  slots     32 MFMAs, set pairs (2 p, 2 p + 1) in octets  a00 a10 b00 b10 a01 a11 b01 b11  (set, v, ks): an accumulator's two
            K-steps are four MFMAs apart, every accumulator is single-buffered (a set is live for 8 of the step's 32 slots).  The
            fold of pair p rides behind the MFMAs of octet p + 1 (set a behind its slots 0..3, set b behind 4..7: three MFMAs at
            least after the set's last), pair 3's behind octet 0 of the NEXT step -- with the previous step's code: the two code
            registers alternate, the other step's is set behind slot 7.  The next step's four fragments and two start-value reads
            go out behind slots 1, 5, .., 21; one lgkmcnt(0) at the top of a step.
  block end the two quarters of a half (lanes 16 apart) are merged into the half's K smallest keys: v_permlane16_swap_b32 brings
            a lane the partner's list of the set it answers for (b = c & 1), K x K v_med3 insert it.  Distinct position codes
            make the K smallest of the union of two top-K lists the top-K of the union: the keys name the groups the 32x32
            schedule's keys name.
  registers v[0:63]     accumulators: set s, virtual tile v = v[8 s + 4 v : +3]
            v[64:95]    A fragments: parity par, tile v, K-step ks = v[64 + 16 par + 8 v + 4 ks : +3]
            v[96:111]   start values: parity par, tile v = v[96 + 8 par + 4 v : +3]
            a_addr: one per K-step (2);   behind the key mask: the codes of even / odd steps (2)
  operands  %0-%15 = B[s][ks], 8 sets x 2 K-steps.

4. MEASURED, and no longer generated (each had a switch here once; DESIGN.md section 4 and profiles/ have the write-ups)

  * four query sets per wave (512 queries per workgroup): with a third of the three-product pass's MFMAs per train row the
    L2 -> LDS stream, the LDS reads and the per-tile barrier of the 256-query shape were as long as the matrix work (0.26 ms of
    0.66 with all arithmetic removed: no fold, no MFMA).  Loops without the barrier, without the hand-over's vmcnt wait and without
    the LDS reads or their waits -- wrong results by design -- sized what each of those costs;
  * two tiles of 256 rows: one hand-over (drain of the LDS queue, barrier, nine transfers to issue) per 128 MFMA slots.  Four
    tiles of 128 rows, on the same box: 0.91 - 0.92 ms against 0.89;
  * groups of 8: groups of 4 results (a 13-bit code, 3 + K VALU per group, 7 VALU per MFMA at K = 4) were the first form.  One
    group of 16 per lane and step, Hamming form only (a kept group costs the exact tail 16 rows of 32 B there, of 256 B in the
    L2 pass): 1 509 instead of 1 728 instructions, 3 % SLOWER -- the tail counts twice the rows;
  * the bf16 pass ran the 32x32 schedule on v_mfma_f32_32x32x16_bf16 before it moved to 16x16x32.
"""
import os
import sys
from types import SimpleNamespace

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:      # (asm_inc sits beside this file, however it was loaded)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asm_inc import Emit, render_inc  # noqa: E402

MFMA = os.environ.get("ESFM_GEN_MFMA", "bf16")
assert MFMA in ("bf16", "fp4")
SHAPE = "16x16x32" if MFMA == "bf16" else "32x32"
KEEP = int(os.environ.get("ESFM_GEN_KEEP", "4"))
assert (2 if MFMA == "fp4" else 3) <= KEEP <= 6
STEP_BITS = int(os.environ.get("ESFM_GEN_STEP_BITS", "11"))
PREFIX = os.environ.get("ESFM_GEN_PREFIX", "ESFM_L2X1")
NS = 4                                # sets of 32 queries per wave
GRP = 8                               # results per fold group
NG = 16 // GRP                        # groups per lane half and 32-train step
CODE_BITS = STEP_BITS + 1             # position code: step, one bit group
KBIG = 0x7F61B1E6                     # 3.0e38f
NKBIG = 0xFF61B1E6
TT = 256                              # train rows per tile
RING = 2                              # tile buffers
ROW_BYTES = 128
assert TT * RING * ROW_BYTES == 65536
STEPS = TT // 32                      # 32-train steps per tile
NP = TT // 32                         # LDS-DMA pieces (8 rows = 1 KiB) per wave and tile
WROWS = TT // 4                       # rows of a tile staged by one wave
TILE_BYTES = TT * ROW_BYTES
NORM_BASE = RING * TILE_BYTES         # the ring's norms sit behind the tiles: RING x TT floats
assert STEPS % 2 == 0                 # a tile's last step has parity 1

OP_NTILES, OP_NT, OP_TRSRC, OP_NRSRC, OP_LDS, OP_WAVE = (f"%{16 + i}" for i in range(6))
KEY = lambda s, i: f"v{112 + KEEP * s + i}"


def reg_map(nsets, n_a_addr, own, n_own):
    """name -> first VGPR of everything behind the keys of `nsets` sets (registers are packed: beside 64 registers of B operands
    every one counts); `own` names the schedule's n_own registers at the end.  .end is the number of VGPRs the block clobbers."""
    m, r = SimpleNamespace(nsets=nsets), 112 + nsets * KEEP
    for name, n in (("a_addr", n_a_addr), ("n_addr", 1), ("dma_off", 4), ("nsrc_off", 1), ("nlds", 1), ("nr", 4), ("scr", 4),
                    ("ftmp", 4), ("mask", 1), (own, n_own)):
        setattr(m, name, r)
        r += n
    m.end = r
    return m


def insert_key(s, x):
    """Insert register x into the sorted keys of set s."""
    out = [f"v_med3_f32 {KEY(s, i)}, {KEY(s, i - 1)}, {KEY(s, i)}, {x}" for i in range(KEEP - 1, 0, -1)]
    return out + [f"v_med3_f32 {KEY(s, 0)}, {KEY(s, 0)}, {x}, s53"]


# ------------------------------------------------------------------------------------------------ address maps (pure functions)
def swz32(row):
    """XOR key of a ring row's eight 16-byte slots, 32x32 schedule."""
    return (row >> 1) & 7


def swz16(row):
    """XOR key of a ring row's eight 16-byte slots, 16x16x32 schedule."""
    return ((row >> 1) & 3) | ((row >> 2) & 4)


def lds_phys_slot(row, slot, swz=swz16):
    """Physical 16-byte slot of logical slot `slot` of ring row `row`."""
    return slot ^ swz(row)


def a_read32(lane, ks):
    """(row of the 32-train step, logical slot) that `lane` reads as its A fragment of K-step ks, 32x32 schedule."""
    return lane & 31, 2 * ks + (lane >> 5)


def a_read(lane, v, ks):
    """(row of the 32-train step, logical slot) that `lane` reads as its A fragment of virtual tile v, K-step ks (16x16x32)."""
    n, c = lane & 15, lane >> 4
    h, G, i = n >> 3, (n >> 2) & 1, n & 3
    return 16 * G + 8 * v + 4 * h + i, 4 * ks + c


def dma_write(wave, piece, lane, swz=swz16):
    """(row of the tile, physical slot, logical slot) that `lane` of `wave` moves in LDS-DMA piece `piece` of a tile."""
    row = WROWS * wave + 8 * piece + (lane >> 3)
    return row, lane & 7, (lane & 7) ^ swz(row)


# ------------------------------------------------------------------------------------------------ the ring: shared emitters
def emit_lane(e, m):
    e("s_mov_b32 s43, m0")
    e(f"v_mbcnt_lo_u32_b32 v{m.scr}, -1, 0")
    e(f"v_mbcnt_hi_u32_b32 v{m.scr}, -1, v{m.scr}")           # lane


def emit_dma_offsets(e, m, emit_swz, swz):
    """LDS-DMA source offsets (lane in scr): 128 row + 16 (logical slot fetched into the lane's physical slot) for pieces 0 .. 3.
    emit_swz(dst, row, tmp) emits the key `swz` of the row in register `row`."""
    for wave in range(4):
        for piece in range(NP):
            for lane in range(64):      # the arithmetic below; the piece's register and the scalar offset of dma_piece
                row = WROWS * wave + (lane >> 3) + 8 * (piece & 3)
                assert dma_write(wave, piece, lane, swz) == (row + 32 * (piece >> 2), lane & 7, swz(row) ^ (lane & 7))
    e(f"s_mul_i32 s48, {OP_WAVE}, {WROWS}")
    e(f"v_lshrrev_b32 v{m.scr + 1}, 3, v{m.scr}")             # lane >> 3
    e(f"v_and_b32 v{m.scr + 3}, 7, v{m.scr}")                 # lane & 7: physical slot
    for i in range(4):
        e(f"v_add_u32 v{m.ftmp}, s48, v{m.scr + 1}")
        e(f"v_add_u32 v{m.ftmp}, {8 * i}, v{m.ftmp}")         # row in the tile
        emit_swz(m.ftmp + 1, m.ftmp, m.ftmp + 2)
        e(f"v_xor_b32 v{m.ftmp + 1}, v{m.ftmp + 1}, v{m.scr + 3}")
        e(f"v_lshlrev_b32 v{m.ftmp + 1}, 4, v{m.ftmp + 1}")
        e(f"v_lshl_add_u32 v{m.dma_off + i}, v{m.ftmp}, 7, v{m.ftmp + 1}")


def emit_norm_addrs(e, m):
    """Lane l of wave w moves |t|^2 of row WROWS w + (l & (WROWS - 1)) of a tile (lanes that share a row move the same value)."""
    e(f"v_and_b32 v{m.ftmp}, {WROWS - 1}, v{m.scr}")
    e(f"v_add_u32 v{m.ftmp}, s48, v{m.ftmp}")                 # row in the tile (s48: emit_dma_offsets)
    e(f"v_lshlrev_b32 v{m.nsrc_off}, 2, v{m.ftmp}")           # byte offset inside a tile's norms
    e(f"v_add_u32 v{m.nlds}, {OP_LDS}, v{m.nsrc_off}")
    e(f"v_add_u32 v{m.nlds}, {NORM_BASE}, v{m.nlds}")         # lds_norm + 4 row (ring slot 0)


def emit_constants(e, m, placeholders):
    """kBig, -kBig, the key mask, every key = kBig; kBig as well in `placeholders`, the registers that the first step folds as
    the results of the step before it (never live)."""
    e(f"s_mov_b32 s52, 0x{KBIG:08x}")
    e(f"s_mov_b32 s53, 0x{NKBIG:08x}")
    e(f"v_mov_b32 v{m.mask}, 0x{(0xFFFFFFFF << CODE_BITS) & 0xFFFFFFFF:08x}")
    for s in range(m.nsets):
        for i in range(KEEP):
            e(f"v_mov_b32 {KEY(s, i)}, s52")
    for r in placeholders:
        e(f"v_mov_b32 v{r}, s52")
    e("s_mov_b32 s40, 0")


def dma_piece(m, i, buf):
    out = [f"s_add_u32 s50, s49, {buf * TILE_BYTES + i * 1024}",
           "s_mov_b32 m0, s50"]
    if i >= 4:
        out.append(f"s_add_u32 s50, s48, {(i >> 2) * 32 * ROW_BYTES}")
    out.append(f"buffer_load_dwordx4 v{m.dma_off + (i & 3)}, {OP_TRSRC}, {'s50' if i >= 4 else 's48'} offen lds")
    return out


def emit_tile(e, m, step, buf):
    """The steps of the tile in ring buffer `buf`, the hand-over at the top of the last.  step(par, nbuf, nstep, extra=None) emits
    one 32-train step on the registers of parity `par` that prefetches step nstep of buffer nbuf and issues the instruction
    lists of `extra`, one list behind an MFMA each."""
    nb = (buf + 1) % RING
    for st in range(STEPS - 1):
        step(st & 1, buf, st + 1)
    e("s_waitcnt lgkmcnt(0)")                                  # every read of this tile has landed
    e(f"s_waitcnt vmcnt({(RING - 2) * NP})")                   # this wave's transfers of tile + 1 have landed (younger tiles may fly;
    #                                                            counted in pieces only: the caller's first tiles come without norm loads)
    # norms of tile + 1 -> LDS, rows past nt as kBig (the first RING tiles' norms were written by the caller)
    e(f"s_cmp_lt_u32 s40, {RING - 1}")
    e(f"s_cbranch_scc1 L_nonorm_t{buf}_%=")
    e("s_add_u32 s48, s40, 1")
    e(f"s_mul_i32 s48, s48, {TT}")
    e(f"v_lshrrev_b32 v{m.scr}, 2, v{m.nsrc_off}")
    e(f"v_add_u32 v{m.scr}, s48, v{m.scr}")                    # train row of this lane's norm
    e(f"v_cmp_gt_u32 vcc, {OP_NT}, v{m.scr}")
    e(f"v_mov_b32 v{m.scr + 1}, s52")
    e(f"v_cndmask_b32 v{m.scr + 1}, v{m.scr + 1}, v{m.nr + nb}, vcc")
    e(f"ds_write_b32 v{m.nlds}, v{m.scr + 1} offset:{nb * TT * 4}")
    e("s_waitcnt lgkmcnt(0)")
    e(f"L_nonorm_t{buf}_%=:")
    e("s_barrier")
    e(f"s_add_u32 s48, s40, {RING}")
    e(f"s_mul_i32 s51, s48, {TT * 4}")                         # (tile + RING) * TT * 4: its norms
    e(f"s_mul_i32 s48, s48, {TILE_BYTES}")                     # ... its rows
    e(f"s_mul_i32 s49, {OP_WAVE}, {WROWS * ROW_BYTES}")        # this wave's rows inside a tile
    e(f"s_add_u32 s49, s49, {OP_LDS}")
    pcs = [[f"buffer_load_dword v{m.nr + buf}, v{m.nsrc_off}, {OP_NRSRC}, s51 offen"]] + [dma_piece(m, i, buf) for i in range(NP)]
    step(1, nb, 0, extra=pcs)
    e("s_add_u32 s40, s40, 1")


def emit_ring(e, m, step):
    """The loop over the tiles, the ring unrolled; ends with the matrix pipe drained and every LDS read landed."""
    e("L_top_%=:")
    for buf in range(RING):
        emit_tile(e, m, step, buf)
        if buf < RING - 1:
            e(f"s_cmp_ge_u32 s40, {OP_NTILES}")
            e("s_cbranch_scc1 L_done_%=")
    e(f"s_cmp_lt_u32 s40, {OP_NTILES}")
    e("s_cbranch_scc1 L_top_%=")
    e("L_done_%=:")
    e("s_nop 15")                                              # the last step's results leave the matrix pipe
    e("s_nop 15")
    e("s_waitcnt lgkmcnt(0)")                                  # the prefetches past the end land in dead registers


def emit_tail(e, m, key):
    """Keys -> LDS (the ring is dead once every wave is here and every transfer has landed); key(s, i): rank i of 32-query set s."""
    e("s_waitcnt vmcnt(0)")
    e("s_barrier")
    e(f"v_mbcnt_lo_u32_b32 v{m.scr}, -1, 0")
    e(f"v_mbcnt_hi_u32_b32 v{m.scr}, -1, v{m.scr}")
    e(f"s_lshl_b32 s48, {OP_WAVE}, 6")
    e(f"v_add_u32 v{m.scr}, s48, v{m.scr}")                    # tid
    e(f"v_lshlrev_b32 v{m.scr}, 2, v{m.scr}")
    e(f"v_add_u32 v{m.scr}, {OP_LDS}, v{m.scr}")
    for s in range(NS):
        for i in range(KEEP):
            e(f"ds_write_b32 v{m.scr}, {key(s, i)} offset:{(KEEP * s + i) * 1024}")
    e("s_waitcnt lgkmcnt(0)")
    e("s_mov_b32 m0, s43")


# ------------------------------------------------------------------------------------------------ the 32x32 schedule
M32 = reg_map(NS, 4, "acc_odd", 32)


def gen32():
    e, m = Emit(), M32
    SCR, FTMP = m.scr, m.ftmp
    OP_B = lambda s, ks: f"%{4 * s + ks}"
    acc = lambda s, par: 16 * s if (s >= 2 or par == 0) else m.acc_odd + 16 * s
    accr = lambda s, par: f"v[{acc(s, par)}:{acc(s, par) + 15}]"
    fr = lambda ks, par: f"v[{64 + 16 * par + 4 * ks}:{64 + 16 * par + 4 * ks + 3}]"

    def emit_swz(dst, row, tmp):
        e(f"v_bfe_u32 v{dst}, v{row}, 1, 3")
    for row in range(TT * RING):
        assert swz32(row) == (row >> 1) & 7 == swz32(row + 32)
    for lane in range(64):          # the set-up's arithmetic below, lane by lane
        for ks in range(4):
            assert a_read32(lane, ks) == (lane & 31, (2 * ks) | (lane >> 5))
    # ------------------------------------------------------------------ set-up
    emit_lane(e, m)
    e(f"v_and_b32 v{SCR + 1}, 31, v{SCR}")                   # j
    e(f"v_lshrrev_b32 v{SCR + 2}, 5, v{SCR}")                # h
    emit_swz(SCR + 3, SCR + 1, None)                         # the row's swizzle
    e(f"v_lshlrev_b32 v{m.nlds}, 7, v{SCR + 1}")             # j * 128
    e(f"v_add_u32 v{m.nlds}, {OP_LDS}, v{m.nlds}")           # row j of buffer 0, step 0
    for ks in range(4):
        e(f"v_or_b32 v{FTMP}, {2 * ks}, v{SCR + 2}")          # logical slot 2 ks + h
        e(f"v_xor_b32 v{FTMP}, v{FTMP}, v{SCR + 3}")
        e(f"v_lshl_add_u32 v{m.a_addr + ks}, v{FTMP}, 4, v{m.nlds}")
    e(f"v_lshlrev_b32 v{m.n_addr}, 4, v{SCR + 2}")
    e(f"v_add_u32 v{m.n_addr}, {OP_LDS}, v{m.n_addr}")
    e(f"v_add_u32 v{m.n_addr}, {NORM_BASE}, v{m.n_addr}")     # n_addr = lds_norm + 16 h
    emit_dma_offsets(e, m, emit_swz, swz32)
    emit_norm_addrs(e, m)
    # (the fold temporaries are placeholders too: the second half of a fold of the step before the first runs in the first step's slots 0 / 1)
    emit_constants(e, m, list(range(0, 64)) + list(range(m.acc_odd, m.acc_odd + 32)) + [FTMP + 1, FTMP + 3])
    e("s_mov_b32 s41, 0")
    e("s_mov_b32 s42, 0")
    for g in range(NG):
        e(f"s_mov_b32 s{44 + g}, {g}")
    # tile 0 has landed for every wave (the caller's barrier).  Pipeline fill: the start values and the four fragments of step 0
    for g in range(4):
        e(f"ds_read_b128 v[{96 + 4 * g}:{99 + 4 * g}], v{m.n_addr} offset:{32 * g}")
    for ks in range(4):
        e(f"ds_read_b128 {fr(ks, 0)}, v{m.a_addr + ks}")

    def fold_quarter(s, q, par):
        """Quarter q (0..3) of the fold of set s' 16 results of the step with parity `par`.  Groups are register octets (0..7 = rows
        {0..3, 8..11} + 4 h of the step, 8..15 = rows {16..19, 24..27} + 4 h); quarter 2 G is the first half of group G's fold -- the
        minimum of its eight scores and the position code, into the set parity's temporary -- quarter 2 G + 1 the second half: the
        K v_med3 (it reads the temporary only, so it may run after the octet has been overwritten)."""
        G, half = q >> 1, q & 1
        t, key = FTMP + 2 * (s & 1), FTMP + 1 + 2 * (s & 1)        # sets of equal parity never have a fold in flight at the same time
        if half:
            return insert_key(s, f"v{key}")
        b = acc(s, par) + 8 * G
        return [f"v_min3_f32 v{t}, v{b}, s52, v{b + 1}",
                f"v_min3_f32 v{t}, v{t}, v{b + 2}, v{b + 3}",
                f"v_min3_f32 v{t}, v{t}, v{b + 4}, v{b + 5}",
                f"v_min3_f32 v{t}, v{t}, v{b + 6}, v{b + 7}",
                f"v_and_or_b32 v{key}, v{t}, v{m.mask}, s{44 + G}"]

    # slot -> (set, K-step)
    ORDER = [(0, 0), (1, 0), (2, 0), (3, 0), (2, 1), (3, 1), (2, 2), (3, 2), (2, 3), (3, 3), (0, 1), (1, 1), (0, 2), (1, 2), (0, 3), (1, 3)]
    # fold quarter behind each slot: ("cur", set, quarter) = this step's results, ("prev", ...) = the previous step's
    GAP = {10: ("cur", 2, 0), 11: ("cur", 3, 0), 12: ("cur", 2, 1), 13: ("cur", 3, 1), 14: ("cur", 2, 2), 15: ("cur", 3, 2),
           0: ("prev", 2, 3), 1: ("prev", 3, 3),
           2: ("prev", 0, 0), 3: ("prev", 1, 0), 4: ("prev", 0, 1), 5: ("prev", 1, 1), 6: ("prev", 0, 2), 7: ("prev", 1, 2), 8: ("prev", 0, 3), 9: ("prev", 1, 3)}
    # LDS reads behind a slot: fragment ks of the next step (into the other parity's registers) and, behind slot 9, the next
    # step's 16 start values (this step's were last read by slot 3)
    READS = {1: ("frag", 0), 5: ("frag", 1), 9: ("start", None), 11: ("frag", 2), 13: ("frag", 3)}
    # Waits in front of a slot: the fragment it reads (issued one step ago) must have landed.  Queue order per step:
    # F0 (slot 1) | F1 (slot 5) | N x 4 (slot 9) | F2 (slot 11) | F3 (slot 13).  Slot 0 needs F0 and the start values: the younger
    # F2, F3 may fly (F1 is older: landed as well, nothing to wait for at its first use, slot 4); slot 6 needs F2: younger are F3 and
    # this step's F0', F1'; slot 8 needs F3: younger are F0', F1'.
    WAITS = {0: 2, 6: 3, 8: 2}

    def step(par, nbuf, nstep, extra=None):
        extra = list(extra or [])                               # issued behind slots 4 .. 12
        for slot, (s, ks) in enumerate(ORDER):
            if slot in WAITS:
                e(f"s_waitcnt lgkmcnt({WAITS[slot]})")
            if slot == 10:
                # the step being folded from now on is this one
                e(f"s_lshl_b32 s41, s42, {CODE_BITS - STEP_BITS}")
                e("s_add_u32 s42, s42, 1")
                for g in range(NG):
                    e(f"s_add_u32 s{44 + g}, s41, {g}")
            a = accr(s, par)
            e(f"v_mfma_f32_32x32x64_f8f6f4 {a}, {fr(ks, par)}, {OP_B(s, ks)}, {'v[96:111]' if ks == 0 else a} cbsz:4 blgp:4")
            if slot >= 4 and extra:
                e.extend(extra.pop(0))
            which, fs, fq = GAP[slot]
            e.extend(fold_quarter(fs, fq, par if which == "cur" else par ^ 1))
            if slot in READS:
                kind, k = READS[slot]
                if kind == "start":
                    for g in range(4):
                        e(f"ds_read_b128 v[{96 + 4 * g}:{99 + 4 * g}], v{m.n_addr} offset:{(nbuf * TT + nstep * 32 + 8 * g) * 4}")
                else:
                    e(f"ds_read_b128 {fr(k, par ^ 1)}, v{m.a_addr + k} offset:{nbuf * TILE_BYTES + nstep * 32 * ROW_BYTES}")
        assert not extra

    emit_ring(e, m, step)
    # what the last step (parity 1) left unfolded: quarter 3 of its sets 2 and 3, all of its sets 0 and 1
    for fs, fq in [(2, 3), (3, 3)] + [(s_, q_) for s_ in (0, 1) for q_ in range(4)]:
        e.extend(fold_quarter(fs, fq, 1))
    emit_tail(e, m, KEY)
    return e


# ------------------------------------------------------------------------------------------------ the 16x16x32 schedule
NS16 = 8                              # sets of 16 queries per wave
M16 = reg_map(NS16, 2, "code", 2)


def gen16():
    e, m = Emit(), M16
    SCR, FTMP, CODE = m.scr, m.ftmp, m.code
    OP_B = lambda s, ks: f"%{2 * s + ks}"
    acc = lambda s, v: 8 * s + 4 * v
    accr = lambda s, v: f"v[{acc(s, v)}:{acc(s, v) + 3}]"
    fr = lambda v, ks, par: f"v[{64 + 16 * par + 8 * v + 4 * ks}:{64 + 16 * par + 8 * v + 4 * ks + 3}]"
    st = lambda v, par: f"v[{96 + 8 * par + 4 * v}:{96 + 8 * par + 4 * v + 3}]"

    def emit_swz(dst, row, tmp):
        e(f"v_bfe_u32 v{dst}, v{row}, 1, 2")
        e(f"v_bfe_u32 v{tmp}, v{row}, 4, 1")
        e(f"v_lshl_or_b32 v{dst}, v{tmp}, 2, v{dst}")
    for row in range(TT * RING):
        assert swz16(row) == (((row >> 1) & 3) | (((row >> 4) & 1) << 2)) and swz16(row) == swz16(row + 32) == swz16(row ^ 8)
    for lane in range(64):          # the set-up's arithmetic below, lane by lane
        n, c = lane & 15, lane >> 4
        row = (n & 3) | (((n >> 2) & 1) << 4) | (((n >> 3) & 1) << 2)
        for v in range(2):
            for ks in range(2):
                assert a_read(lane, v, ks) == (row + 8 * v, (4 * ks) | c)
    # ------------------------------------------------------------------ set-up
    emit_lane(e, m)
    e(f"v_and_b32 v{SCR + 1}, 15, v{SCR}")                   # n
    e(f"v_lshrrev_b32 v{SCR + 2}, 4, v{SCR}")                # c
    e(f"v_and_b32 v{FTMP}, 3, v{SCR + 1}")                   # i
    e(f"v_bfe_u32 v{FTMP + 1}, v{SCR + 1}, 2, 1")            # G of the row read
    e(f"v_lshl_or_b32 v{FTMP}, v{FTMP + 1}, 4, v{FTMP}")
    e(f"v_bfe_u32 v{FTMP + 1}, v{SCR + 1}, 3, 1")            # h of the row read
    e(f"v_lshl_or_b32 v{FTMP}, v{FTMP + 1}, 2, v{FTMP}")     # row 16 G + 4 h + i of virtual tile 0
    emit_swz(SCR + 3, FTMP, FTMP + 1)
    e(f"v_lshlrev_b32 v{m.nlds}, 7, v{FTMP}")
    e(f"v_add_u32 v{m.nlds}, {OP_LDS}, v{m.nlds}")           # the row in buffer 0, step 0
    for ks in range(2):
        e(f"v_or_b32 v{FTMP + 2}, {4 * ks}, v{SCR + 2}")      # logical slot 4 ks + c
        e(f"v_xor_b32 v{FTMP + 2}, v{FTMP + 2}, v{SCR + 3}")
        e(f"v_lshl_add_u32 v{m.a_addr + ks}, v{FTMP + 2}, 4, v{m.nlds}")
    e(f"v_and_b32 v{CODE}, 1, v{SCR + 2}")                   # G of the quarter: the code of step 0
    e(f"v_mov_b32 v{CODE + 1}, v{CODE}")                     # (the step before the first: placeholders)
    e(f"v_lshlrev_b32 v{FTMP}, 6, v{CODE}")
    e(f"v_lshrrev_b32 v{FTMP + 1}, 1, v{SCR + 2}")           # h of the quarter
    e(f"v_lshl_or_b32 v{FTMP}, v{FTMP + 1}, 4, v{FTMP}")
    e(f"v_add_u32 v{m.n_addr}, {OP_LDS}, v{FTMP}")
    e(f"v_add_u32 v{m.n_addr}, {NORM_BASE}, v{m.n_addr}")     # n_addr = lds_norm + 4 (16 G + 4 h)
    emit_dma_offsets(e, m, emit_swz, swz16)
    emit_norm_addrs(e, m)
    emit_constants(e, m, range(64))
    # tile 0 has landed for every wave (the caller's barrier).  Pipeline fill: the start values and the four fragments of step 0
    for v in range(2):
        e(f"ds_read_b128 {st(v, 0)}, v{m.n_addr} offset:{32 * v}")
    for v in range(2):
        for ks in range(2):
            e(f"ds_read_b128 {fr(v, ks, 0)}, v{m.a_addr + ks} offset:{8 * v * ROW_BYTES}")

    def fold(s, code):
        """The fold of set s' eight results of a step, in four chunks (one per MFMA slot it rides behind)."""
        b, t, key = acc(s, 0), FTMP + 2 * (s & 1), FTMP + 1 + 2 * (s & 1)
        med = insert_key(s, f"v{key}")
        return [[f"v_min3_f32 v{t}, v{b}, s52, v{b + 1}", f"v_min3_f32 v{t}, v{t}, v{b + 2}, v{b + 3}", f"v_min3_f32 v{t}, v{t}, v{b + 4}, v{b + 5}"],
                [f"v_min3_f32 v{t}, v{t}, v{b + 6}, v{b + 7}", f"v_and_or_b32 v{key}, v{t}, v{m.mask}, v{code}"],
                med[:KEEP // 2], med[KEEP // 2:]]

    READS = {1: (0, 0), 5: (1, 0), 9: (0, 1), 13: (1, 1), 17: (0, None), 21: (1, None)}      # slot -> (v, ks) fragment / (v, None) start values

    def step(par, nbuf, nstep, extra=None):
        extra = list(extra or [])                               # issued behind slots 4, 6, 8, ..
        e("s_waitcnt lgkmcnt(0)")                               # this step's fragments and start values (issued a step ago)
        for slot in range(32):
            p, idx = divmod(slot, 8)
            s, v, ks = 2 * p + ((idx >> 1) & 1), idx & 1, idx >> 2
            e(f"v_mfma_f32_16x16x32_bf16 {accr(s, v)}, {fr(v, ks, par)}, {OP_B(s, ks)}, {st(v, par) if ks == 0 else accr(s, v)}")
            if slot >= 4 and slot % 2 == 0 and extra:
                e.extend(extra.pop(0))
            # pair p - 1 of this step; behind octet 0: pair 3 of the previous step, under that step's code
            e.extend(fold(2 * ((p - 1) % 4) + (idx >> 2), CODE + (par if p else par ^ 1))[idx & 3])
            if slot == 7:
                e(f"v_add_u32 v{CODE + (par ^ 1)}, 2, v{CODE + par}")      # the next step's code
            if slot in READS:
                v_, k_ = READS[slot]
                if k_ is None:
                    e(f"ds_read_b128 {st(v_, par ^ 1)}, v{m.n_addr} offset:{(nbuf * TT + nstep * 32 + 8 * v_) * 4}")
                else:
                    e(f"ds_read_b128 {fr(v_, k_, par ^ 1)}, v{m.a_addr + k_} offset:{nbuf * TILE_BYTES + (nstep * 32 + 8 * v_) * ROW_BYTES}")
        assert not extra

    emit_ring(e, m, step)
    # what the last step (parity 1) left unfolded: its sets 6 and 7
    for s in (6, 7):
        for chunk in fold(s, CODE + 1):
            e.extend(chunk)
    # merge of the two quarters of a half: sets 2 s and 2 s + 1 trade rows of 16 lanes, so that a lane holds its own list and its
    # partner's of the set it answers for, in KEY(2 s, .) and KEY(2 s + 1, .); the second is inserted into the first
    e("s_nop 1")
    for s in range(NS):
        for i in range(KEEP):
            e(f"v_permlane16_swap_b32 {KEY(2 * s, i)}, {KEY(2 * s + 1, i)}")
    e("s_nop 1")
    for s in range(NS):
        for y in range(KEEP):
            e.extend(insert_key(2 * s, KEY(2 * s + 1, y)))
    emit_tail(e, m, lambda s, i: KEY(2 * s, i))
    return e


def render():
    """(text of the generated file, instruction lines)"""
    lines, m = (gen16(), M16) if SHAPE == "16x16x32" else (gen32(), M32)
    defines = [("KEEP", KEEP), ("SETS", NS), ("CODE_BITS", CODE_BITS), ("GRP", GRP), ("TT", TT), ("RING", RING)]
    if SHAPE == "16x16x32":
        defines.append(("QSETS", NS16))     # sets of 16 queries per wave: the B operands are [QSETS][2], slot 4 ks + (lane >> 4)
    return render_inc("gen_l2x1_segment_asm.py", PREFIX, defines, lines, m.end), lines


def main():
    text, lines = render()
    open(sys.argv[1] if len(sys.argv) > 1 else "l2x1_segment_gfx950.inc", "w").write(text)
    n_mfma = sum("v_mfma" in l for l in lines)
    print(f"{len(lines)} instructions, {n_mfma} MFMAs, KEEP = {KEEP}, GRP = {GRP}")


if __name__ == "__main__":
    main()
