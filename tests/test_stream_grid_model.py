"""The streaming geometry of long frames, proven on the CPU (tests/_stream_grid.py;
measured on the GPU by bench/micro/mb16.hip): a unit grid anchored at
floor128(frame end) cuts a frame into a head read by ordinary loads, body
rounds of whole 128-B lines that LDS-DMA fetches with one request per line,
and a tail of at most 127 bytes fed after the merge. Also the wave's batch
image in LDS and the bank model of the rotated compact slice tables.
"""
import zlib

import numpy as np
import pytest

from tests import _stream_grid as sg

LENGTHS = list(range(8192 - 130, 8192 + 131)) + [16400, 49151, 49152, 65532]


def lanes_for(L: int) -> int:
    return 8 if L < 49152 else 16


def test_head_body_tail_partition_every_alignment():
    for L in LENGTHS:
        G = lanes_for(L)
        for a in range(128):
            fp = 4096 + a
            gr = sg.Grid(fp, L, G)
            h0, h1 = gr.head_range()
            t0, t1 = gr.tail_range()
            lines = gr.body_lines()
            # head | body | tail cover [fp, fp + L) once, in order
            assert h0 == fp and t1 == fp + L and h0 < h1, (L, a)
            assert h1 == (lines[0] if lines else t0), (L, a)
            assert lines == list(range(h1, t0, sg.LINE)), (L, a)   # consecutive, each once
            assert (h1 - h0) + sg.LINE * len(lines) + (t1 - t0) == L, (L, a)
            # no body line outside the frame, every one line-aligned; at most 127 tail bytes
            assert all(x % sg.LINE == 0 and fp <= x and x + sg.LINE <= fp + L for x in lines), (L, a)
            assert 0 <= t1 - t0 < sg.LINE and t0 % sg.LINE == 0, (L, a)
            # rounds: R - 1 body rounds of G / 2 lines; round 0 holds 1..G units and the padding
            assert len(lines) == (gr.R - 1) * G // 2, (L, a)
            assert 0 < h1 - h0 <= G * sg.UNIT and gr.pad < sg.UNIT, (L, a)
            # the rounds are the same lines, round by round
            assert [x for k in range(1, gr.R) for x in gr.round_lines(k)] == lines


def test_short_and_tiny_frames_have_no_body_outside_the_frame():
    for L in list(range(0, 300)) + [511, 512, 513, 640, 1023, 1100]:
        for a in (0, 1, 3, 4, 63, 64, 65, 125, 126, 127):
            for G in (8, 16):
                fp = 1024 + a
                gr = sg.Grid(fp, L, G)
                (h0, h1), (t0, t1), lines = gr.head_range(), gr.tail_range(), gr.body_lines()
                assert (h1 - h0) + sg.LINE * len(lines) + (t1 - t0) == L, (L, a, G)
                assert all(fp <= x and x + sg.LINE <= fp + L for x in lines), (L, a, G)
                if gr.tiny:
                    assert not lines and (h0, h1) == (fp, fp + L)


@pytest.mark.parametrize("L", [8192 - 130, 8191, 8192, 8193, 8319, 8192 + 130, 16400])
def test_model_crc_matches_zlib_g8(L):
    rng = np.random.default_rng(L)
    mem = rng.integers(0, 256, 4096 + 128 + L + 128, dtype=np.uint8).tobytes()
    for a in (0, 1, 2, 3, 4, 61, 63, 64, 65, 124, 125, 127):
        fp = 4096 + a
        assert sg.model_frame(mem, fp, L, 8) == zlib.crc32(mem[fp:fp + L]), (L, a)


@pytest.mark.parametrize("L", [49151, 49152, 65532])
def test_model_crc_matches_zlib_g16(L):
    rng = np.random.default_rng(L)
    mem = rng.integers(0, 256, 4096 + 128 + L + 128, dtype=np.uint8).tobytes()
    for a in (0, 3, 64, 127):
        fp = 4096 + a
        assert sg.model_frame(mem, fp, L, 16) == zlib.crc32(mem[fp:fp + L]), (L, a)


def test_model_crc_short_frames_and_seeds():
    rng = np.random.default_rng(5)
    mem = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    for L in (0, 1, 3, 4, 5, 63, 64, 127, 128, 129, 130, 131, 260, 700):
        for a in (0, 1, 125, 126, 127):
            fp = 1024 + a
            assert sg.model_frame(mem, fp, L, 8) == zlib.crc32(mem[fp:fp + L]), (L, a)
            for seed in (0, 0xDEADBEEF):
                assert sg.model_frame(mem, fp, L, 8, seed=seed, xorout=0) == sg.raw_update(seed, mem[fp:fp + L])


@pytest.mark.parametrize("G", [8, 16])
def test_batch_image_one_request_per_line_and_readback(G):
    # every 16-B piece of the wave's round is fetched by exactly one DMA lane, a
    # DMA instruction asks for whole lines only, and a line belongs to one instruction
    owner = {}
    for q in range(4):
        pieces = {}
        for l in range(64):
            fr, off = sg.dma_source(q, l, G)
            assert (fr, off) not in owner
            owner[(fr, off)] = (q, l)
            pieces.setdefault((fr, off // sg.LINE), set()).add(off % sg.LINE)
        assert all(p == set(range(0, sg.LINE, 16)) for p in pieces.values()), q
    assert len(owner) == 256 and {f for f, _ in owner} == set(range(64 // G))
    by_line = {}
    for (fr, off), (q, _) in owner.items():
        by_line.setdefault((fr, off // sg.LINE), set()).add(q)
    assert all(len(qs) == 1 for qs in by_line.values())
    # the read-back of hash lane m returns its unit's pieces in order
    for lane in range(64):
        for k in range(4):
            ro = sg.readback_offset(lane, k)
            q, l = ro // 1024, (ro % 1024) // 16
            assert sg.dma_source(q, l, G) == (lane // G, (lane % G) * sg.UNIT + 16 * k)
    # and each pass of a ds_read_b128 touches 16 different bank quads
    for k in range(4):
        for lanes in sg.B128_PASSES:
            assert len({(sg.readback_offset(x, k) // 16) % 16 for x in lanes}) == 16


@pytest.mark.parametrize("lookup,replicas", [(sg.lookup_64k, 16), (sg.lookup_32k, 8)])
def test_rotated_tables_are_conflict_free_for_any_data(lookup, replicas):
    # every lane reads each slot once, with the byte that slot's table consumes
    for lane in range(64):
        assert sorted(lookup(lane, i)[0] for i in range(4)) == [0, 1, 2, 3]
    # a ds_read_b32 serves lanes 0-31 and 32-63 in two passes over 32 banks: with
    # arbitrary byte values each pass must touch 32 different banks
    rng = np.random.default_rng(20260101)
    words = rng.integers(0, 256, (2000, 64, 4), dtype=np.uint32)
    for y in words:
        for i in range(4):
            for half in (range(0, 32), range(32, 64)):
                banks = set()
                for lane in half:
                    slot, addr = lookup(lane, i)
                    banks.add((addr(int(y[lane][slot])) // 4) % 32)
                assert len(banks) == 32
    # the bank does not depend on the byte value at all (rows are whole multiples of 32 banks)
    for lane in range(64):
        for i in range(4):
            _, addr = lookup(lane, i)
            assert len({(addr(b) // 4) % 32 for b in range(256)}) == 1
            assert addr(255) < replicas * 4 * 4 * 256
