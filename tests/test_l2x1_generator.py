"""The generators of the inline-asm main loops (easysfm_amd/csrc/gen_*.py), on the CPU: every committed .inc file is byte for byte what
its generator writes, whatever retired experiment switch the environment still carries; and the address maps of the one-product pass's
two schedules -- the LDS swizzle, the A-fragment reads, the LDS-DMA writer.  The maps are the generator's own pure functions (it
checks its set-up arithmetic against them when it runs)."""
import importlib.util
import os

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "easysfm_amd", "csrc")
_GEN_ENV = ["ESFM_GEN_MFMA", "ESFM_GEN_KEEP", "ESFM_GEN_STEP_BITS", "ESFM_GEN_PREFIX"]
_FP4_ENV = dict(ESFM_GEN_MFMA="fp4", ESFM_GEN_KEEP="2", ESFM_GEN_STEP_BITS="13", ESFM_GEN_PREFIX="ESFM_HMX1")     # the Makefile's, for hmx1_segment_gfx950.inc
# switches the generators had for timing experiments, with a value that changed the loop then (several: to wrong results by design)
_RETIRED_L2X1 = dict(ESFM_GEN_NOFOLD="1", ESFM_GEN_NOMFMA="1", ESFM_GEN_NOBAR="1", ESFM_GEN_NOVMWAIT="1", ESFM_GEN_NOLGKM="1", ESFM_GEN_NOLDSRD="1",
                     ESFM_GEN_GRP="4", ESFM_GEN_TT="128", ESFM_GEN_RING="4", ESFM_GEN_SHAPE="32x32")
_RETIRED_L2 = dict(ESFM_GEN_PRODUCTS="1", ESFM_GEN_KEEP="4", ESFM_GEN_DMA_SPREAD="0", ESFM_GEN_A_ORDER="hh")
_RETIRED_POTRF = dict(ESFM_GEN_POTRF_FMAC_DPP="0", ESFM_GEN_POTRF_B64DPP="0")


def _load(monkeypatch, name, filename="gen_l2x1_segment_asm.py", **env):
    """A generator as a fresh module, its switches (read from the environment at import) set to `env` and nothing else."""
    for k in _GEN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec = importlib.util.spec_from_file_location(name, os.path.join(CSRC, filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _committed(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture()
def gen(monkeypatch):
    return _load(monkeypatch, "gen_l2x1_default")


def test_default_is_the_16x16x32_schedule(gen):
    assert gen.SHAPE == "16x16x32" and gen.MFMA == "bf16" and gen.KEEP == 4 and gen.GRP == 8 and gen.CODE_BITS == 12
    text, lines = gen.render()
    with open(os.path.join(CSRC, "l2x1_segment_gfx950.inc")) as f:
        assert f.read() == text, "l2x1_segment_gfx950.inc is not what the generator writes"
    n16 = sum(l.startswith("v_mfma_f32_16x16x32_bf16") for l in lines)
    assert n16 == sum("v_mfma" in l for l in lines) == 32 * (gen.TT // 32) * gen.RING      # 32 per 32-train step, the ring unrolled


def test_every_a_fragment_read_covers_the_banks_once(gen):
    """A 16-lane group of a ds_read_b128 moves 256 bytes: conflict-free iff its 16 addresses fall into 16 different 16-byte columns
    of the 64 banks (address mod 256).  Every step of the ring (its rows start at a multiple of 32), both virtual tiles, both
    K-steps, all four lane groups."""
    for step_row0 in range(0, gen.TT * gen.RING, 32):
        for v in range(2):
            for ks in range(2):
                for c in range(4):
                    banks = set()
                    for n in range(16):
                        row, slot = gen.a_read(16 * c + n, v, ks)
                        addr = (step_row0 + row) * gen.ROW_BYTES + 16 * gen.lds_phys_slot(step_row0 + row, slot)
                        for w in range(4):
                            banks.add((addr // 4 + w) % 64)
                    assert len(banks) == 64, (step_row0, v, ks, c)


def test_rows_of_a_quarter_are_one_group_of_the_32x32_schedule(gen):
    """v_mfma_f32_16x16x32_bf16 delivers virtual row 4 c + i of a tile to lane group c (register i), and virtual row n is what
    A-fragment lane n read.  Quarter c = 2 h + G must receive rows 16 G + 4 h + (0..3) and 16 G + 8 + 4 h + (0..3) of the step: the
    group that finish_rerank_wave's row0_of decodes from code bit G and lane half h."""
    for c in range(4):
        h, G = c >> 1, c & 1
        got = set()
        for v in range(2):
            for i in range(4):
                rows = {gen.a_read(16 * cc + 4 * c + i, v, ks)[0] for cc in range(4) for ks in range(2)}
                assert len(rows) == 1          # every lane group and K-step reads the same row for virtual row 4 c + i
                got |= rows
        assert got == {16 * G + 4 * h + i for i in range(4)} | {16 * G + 8 + 4 * h + i for i in range(4)}, c
    for lane in range(64):                     # a lane's fragment of K-step ks is slot 4 ks + (lane >> 4): features 32 ks + 8 (lane >> 4) ..
        for v in range(2):
            for ks in range(2):
                assert gen.a_read(lane, v, ks)[1] == 4 * ks + (lane >> 4)


def test_dma_writer_and_reader_agree(gen):
    """Every (row, logical slot) of the 512 ring rows is written once, to the physical slot the reader computes for it."""
    pieces = gen.TT // 32
    for buf in range(gen.RING):
        seen = {}
        for wave in range(4):
            for piece in range(pieces):
                for lane in range(64):
                    row, phys, logical = gen.dma_write(wave, piece, lane)
                    assert 0 <= row < gen.TT and (row, logical) not in seen
                    seen[(row, logical)] = phys
                    # the piece lands as 1 KiB in lane order: lane l at byte 16 l behind the piece's first row
                    assert row * gen.ROW_BYTES + 16 * phys == (gen.WROWS * wave + 8 * piece) * gen.ROW_BYTES + 16 * lane
        assert len(seen) == gen.TT * 8
        for (row, logical), phys in seen.items():
            ring_row = buf * gen.TT + row
            assert gen.lds_phys_slot(ring_row, logical) == phys, (ring_row, logical)
    # pieces i and i + 4 share a source-offset register: rows 32 apart have one key; so have the two virtual tiles (rows 8 apart)
    for row in range(gen.TT * gen.RING - 32):
        assert gen.swz16(row) == gen.swz16(row + 32) and gen.swz16(row) == gen.swz16(row ^ 8)


def test_hamming_form_is_byte_identical(monkeypatch):
    """With the fp4 switch the generator writes the committed hmx1_segment_gfx950.inc: the Hamming matcher stays on the 32x32 schedule."""
    g = _load(monkeypatch, "gen_l2x1_fp4", **_FP4_ENV)
    assert g.SHAPE == "32x32"
    text, lines = g.render()
    with open(os.path.join(CSRC, "hmx1_segment_gfx950.inc")) as f:
        assert f.read() == text
    assert not any("16x16x32" in l for l in lines)


def test_three_product_loop_is_byte_identical(monkeypatch):
    """l2_segment_gfx950.inc is what gen_l2_segment_asm.py writes, with a clean environment and under each of its retired switches."""
    for env in [{}] + [{k: v} for k, v in _RETIRED_L2.items()]:
        g = _load(monkeypatch, "gen_l2_default", "gen_l2_segment_asm.py", **env)
        text, lines = g.render()
        assert text == _committed("l2_segment_gfx950.inc"), env
        assert (len(lines), sum("v_mfma" in l for l in lines)) == (1067, 192)
        monkeypatch.undo()


def test_potrf_block_is_byte_identical(monkeypatch, tmp_path):
    """potrf16_gfx950.inc is what gen_potrf16_asm.py writes (a fresh module each time: the generator keeps its program in module state)."""
    for n, env in enumerate([{}] + [{k: v} for k, v in _RETIRED_POTRF.items()]):
        g = _load(monkeypatch, f"gen_potrf16_{n}", "gen_potrf16_asm.py", **env)
        out = tmp_path / f"potrf16_{n}.inc"
        g.main(str(out))
        assert out.read_text() == _committed("potrf16_gfx950.inc"), env
        assert len(g.generate()[0]) == 489
        monkeypatch.undo()


@pytest.mark.parametrize("form", [{}, _FP4_ENV], ids=["bf16", "fp4"])
def test_retired_switches_change_nothing(monkeypatch, form):
    """A stray experiment variable on a build machine cannot produce another loop: render() reads the four kept switches only."""
    base = _load(monkeypatch, "gen_l2x1_base", **form).render()[0]
    assert base == _committed("hmx1_segment_gfx950.inc" if form else "l2x1_segment_gfx950.inc")
    for k, v in _RETIRED_L2X1.items():
        monkeypatch.undo()
        assert _load(monkeypatch, "gen_l2x1_retired", **form, **{k: v}).render()[0] == base, k


@pytest.fixture()
def gen_fp4(monkeypatch):
    return _load(monkeypatch, "gen_l2x1_fp4_maps", **_FP4_ENV)


def test_32x32_a_fragment_reads_cover_the_banks_once(gen_fp4):
    """The 32x32 schedule's reads, as for the 16x16x32 form above: every 16-lane group of a ds_read_b128 falls into 16 different 16-byte
    columns of the 64 banks -- within a group j >> 1 takes eight values twice, once per 128-byte half.  Every step of the ring, all
    four K-steps, all four lane groups."""
    gen = gen_fp4
    assert gen.SHAPE == "32x32" and gen.GRP == 8 and gen.CODE_BITS == 14
    for step_row0 in range(0, gen.TT * gen.RING, 32):
        for ks in range(4):
            for c in range(4):
                banks = set()
                for n in range(16):
                    row, slot = gen.a_read32(16 * c + n, ks)
                    assert 0 <= row < 32 and slot == 2 * ks + (c >> 1)
                    addr = (step_row0 + row) * gen.ROW_BYTES + 16 * gen.lds_phys_slot(step_row0 + row, slot, gen.swz32)
                    for w in range(4):
                        banks.add((addr // 4 + w) % 64)
                assert len(banks) == 64, (step_row0, ks, c)
    # a lane half reads all 32 rows of the step, each lane all eight slots of its row's half over the four K-steps
    for h in range(2):
        assert {gen.a_read32(32 * h + j, 0)[0] for j in range(32)} == set(range(32))
        assert {gen.a_read32(32 * h, ks)[1] for ks in range(4)} == {h, 2 + h, 4 + h, 6 + h}


def test_32x32_dma_writer_and_reader_agree(gen_fp4):
    """Every (row, logical slot) of the 512 ring rows is written once, to the physical slot the 32x32 reader computes for it."""
    gen = gen_fp4
    pieces = gen.TT // 32
    for buf in range(gen.RING):
        seen = {}
        for wave in range(4):
            for piece in range(pieces):
                for lane in range(64):
                    row, phys, logical = gen.dma_write(wave, piece, lane, gen.swz32)
                    assert 0 <= row < gen.TT and (row, logical) not in seen
                    seen[(row, logical)] = phys
                    assert row * gen.ROW_BYTES + 16 * phys == (gen.WROWS * wave + 8 * piece) * gen.ROW_BYTES + 16 * lane
        assert len(seen) == gen.TT * 8
        for (row, logical), phys in seen.items():
            ring_row = buf * gen.TT + row
            assert gen.lds_phys_slot(ring_row, logical, gen.swz32) == phys, (ring_row, logical)
    # pieces i and i + 4 share a source-offset register: the key repeats every 32 rows
    for row in range(gen.TT * gen.RING - 32):
        assert gen.swz32(row) == (row >> 1) & 7 == gen.swz32(row + 32)
