"""The frame-launch policy (csrc/launch_plan.hpp) pinned without a GPU:
val_gpu_plan_frames() plans with plain numbers, so every threshold of the
policy (each a measured result, DESIGN.md / DESIGN_EXPERIMENTS.md) has a row
at each side here. A slip in a comparison leaves every CRC right and shows
only as a few percent on one workload; it shows here as a changed row.

EXPECTED holds what the planner returned when the arithmetic was moved
verbatim out of the launch functions; three rows (HAND) are also derived by
hand from that code below. A row is a launch as
(kernel, lanes, depth, grid, first, count, k0, qparts, static_rounds,
 tail_n, tail_k0, tail_units), kernel 0 ragged, 1 split, 2 k_frames,
3 k_frames with one-pass loads."""
import numpy as np
import pytest

import val_protocol_amd.crc as vc

KiB = 1024
CUS = 256
WAVES = CUS * 16  # persistent waves of a 256-CU device


def _rounds(lanes, r, extra=0):
    """Frames of r full group rounds at `lanes` lanes per frame, plus extra."""
    return WAVES * (64 // lanes) * r + extra


def _case(cid, n, typical, *, cus=CUS, desc=False, flen=None, last_len=None, pay=False, **knobs):
    flen = (0 if desc else typical) if flen is None else flen
    return cid, dict(cus=cus, n=n, typical_len=typical, descriptors=desc, flen=flen,
                     last_len=flen if last_len is None else last_len, want_payload=pay), knobs


def _cases():
    c = []
    # bench.py's configurations (cfg2/cfg3 strided, cfg4 descriptors with the hint, cfg5 ragged)
    c.append(_case("cfg3", 1 << 20, 16400))
    c.append(_case("cfg2", 1 << 16, 1040))
    c.append(_case("cfg4-strided", 131113, 65532))
    c.append(_case("cfg4-desc", 131113, 65532, desc=True))
    c.append(_case("cfg5", 262144, 0, desc=True))
    c.append(_case("cfg3-1Mi-x-16KiB", 1 << 20, 16 * KiB))
    c.append(_case("cfg3-desc", 1 << 20, 16400, desc=True))
    # the windows the split rule cites
    for n, L in ((256, 64 * KiB), (256, 8 * KiB), (512, 16 * KiB), (1024, 64 * KiB), (2048, 64 * KiB),
                 (257, 8 * KiB), (256, 8 * KiB - 1), (2048, 128 * KiB), (2049, 128 * KiB), (256, 16 * KiB)):
        c.append(_case(f"window-{n}x{L}", n, L))
    # short frames at 4, 8 and 12 group rounds (the dynamic-tail rules), strided and descriptor
    for L, lanes in ((600, 2), (1100, 4), (2000, 4), (4200, 8)):
        for r in (4, 8, 12):
            for desc in (False, True):
                c.append(_case(f"{'u' if desc else 's'}{L}{'d' if desc else ''}-r{r}", _rounds(lanes, r), L, desc=desc))
    c.append(_case("u600d-r7", _rounds(2, 7), 600, desc=True))
    for r in (6, 15, 16, 32):
        c.append(_case(f"u16400d-r{r}", _rounds(8, r), 16400, desc=True))
    # each side of the queue thresholds: bytes per wave, group bytes (one word / partitions)
    for r in (4, 5, 6, 7):
        c.append(_case(f"s65532-r{r}", _rounds(16, r), 65532))
    for r in (11, 12):
        c.append(_case(f"s16400-r{r}", _rounds(8, r), 16400))
    for L in (16 * KiB - 1, 16 * KiB):
        c.append(_case(f"s{L}-r16", _rounds(8, 16), L))
    for L in (24 * KiB - 1, 24 * KiB):
        c.append(_case(f"u{L}d-r12", _rounds(8, 12), L, desc=True))
    for L in (4 * KiB - 1, 4 * KiB):
        c.append(_case(f"s{L}-r47", _rounds(8, 47), L))
    for L in (511, 512):
        c.append(_case(f"u{L}d-r8", _rounds(2, 8), L, desc=True))
    # each side of the lane classes and of the 4-lane ring's length limit
    for L in (1023, 1024, 1599, 1600, 2047, 2048, 49151, 49152):
        c.append(_case(f"s{L}-4Mi", 1 << 22, L))
    # small windows: lanes doubled while half of the waves would idle
    for n, L in ((1, 64), (1, 100), (1, 8 * KiB), (64, 1100), (1024, 1100), (2048, 4200), (4096, 4200),
                 (4097, 4200), (300, 64 * KiB)):
        c.append(_case(f"small-{n}x{L}", n, L))
    # every parametrisation of tests/test_gpu_tail.py, the in-launch tail on and off
    for L, r, tail in ((65532, 1, 6), (65532, 1, 1024), (65532, 2, 41), (16400, 1, 100), (8192, 1, 3),
                       (24580, 4, 777), (32784, 1, 57), (8191, 1, 3)):
        lanes = 16 if L >= 49152 else 8
        c.append(_case(f"tail-s{L}-r{r}+{tail}", _rounds(lanes, r, tail), L))
        c.append(_case(f"tail-s{L}-r{r}+{tail}-off", _rounds(lanes, r, tail), L, tail_pieces=0))
    for L, r, tail in ((65532, 1, 6), (65532, 8, 41), (16400, 1, 33)):
        lanes = 16 if L >= 49152 else 8
        c.append(_case(f"tail-u{L}d-r{r}+{tail}", _rounds(lanes, r, tail), L, desc=True))
        c.append(_case(f"tail-u{L}d-r{r}+{tail}-off", _rounds(lanes, r, tail), L, desc=True, tail_pieces=0))
    for lanes in (8, 16, 32):
        c.append(_case(f"tail-forced{lanes}", _rounds(lanes, 1, 9), 65532, lanes=lanes))
        c.append(_case(f"tail-forced{lanes}-off", _rounds(lanes, 1, 9), 65532, lanes=lanes, tail_pieces=0))
    c.append(_case("tail-pay", _rounds(16, 1, 9), 65532, pay=True))
    c.append(_case("tail-short-frames", _rounds(4, 2, 100), 1100))           # re-cut second launch
    c.append(_case("tail-too-long", _rounds(16, 1, 3000), 65532))            # the tail does not fit more lanes
    # degenerate
    c.append(_case("n0", 0, 16400))
    c.append(_case("n1", 1, 16400))
    c.append(_case("n1-empty", 1, 0))
    c.append(_case("last-short", 131113, 65532, last_len=816))
    c.append(_case("last-short-window", 256, 64 * KiB, last_len=816))
    c.append(_case("last-longer-window", 256, 4 * KiB, flen=4 * KiB, last_len=64 * KiB))
    c.append(_case("last-short-tail-off", 131113, 65532, last_len=816, tail_pieces=0))
    c.append(_case("hint0-4095", 4095, 0, desc=True))
    c.append(_case("hint0-4096", 4096, 0, desc=True))
    c.append(_case("hint0-min1", 7, 0, desc=True, ragged_min=1))
    c.append(_case("hint0-forced-lanes", 262144, 0, desc=True, lanes=8))
    c.append(_case("hint0-strided", 262144, 0, flen=0))
    c.append(_case("ragged-depth0", 262144, 0, desc=True, prefetch=0))
    c.append(_case("ragged-ring", 262144, 0, desc=True, prefetch=-3))
    # payload states
    c.append(_case("pay-cfg3", 1 << 20, 16400, pay=True))
    c.append(_case("pay-window", 256, 64 * KiB, pay=True))
    c.append(_case("pay-ragged", 262144, 0, desc=True, pay=True))
    c.append(_case("pay-short", _rounds(2, 8), 600, desc=True, pay=True))
    c.append(_case("pay-forced-depth", 1 << 20, 16400, pay=True, prefetch=4))
    # forced lanes x forced depths, a multi-pass batch and a one-pass window
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        for depth in (0, 1, 2, 4, -2, -3):
            c.append(_case(f"forced-g{lanes}-d{depth}", 300000, 1100, lanes=lanes, prefetch=depth))
            c.append(_case(f"forced-g{lanes}-d{depth}-window", 64, 1100, lanes=lanes, prefetch=depth))
    for depth in (0, 1, 2, 4, -2, -3):
        c.append(_case(f"auto-lanes-d{depth}", _rounds(2, 8), 600, prefetch=depth))
        c.append(_case(f"auto-lanes-d{depth}-long", 131113, 65532, prefetch=depth))
    # a small device
    for cid, n, L, kw in (("cfg3", 1 << 20, 16400, {}), ("cfg4-desc", 131113, 65532, dict(desc=True)),
                          ("window-8x64KiB", 8, 64 * KiB, {}), ("window-64x64KiB", 64, 64 * KiB, {}),
                          ("window-65x64KiB", 65, 64 * KiB, {}), ("tail", 128 * 4 + 3, 65532, {}),
                          ("u600d-r8", 128 * 32 * 8, 600, dict(desc=True)), ("cfg5", 262144, 0, dict(desc=True)),
                          ("ragged-small", 100, 0, dict(desc=True, ragged_min=1))):
        c.append(_case(f"cus8-{cid}", n, L, cus=8, **kw))
    return c


CASES = _cases()

# Derived by hand from the launch functions this policy was moved out of:
#  cfg4-strided: 65,532 B -> 16 lanes, 4 frames per group: 32,779 groups on 4,096 waves = 8 full rounds
#    (131,072 frames) and 41 frames. 16 lanes, >= 8 KiB: in-launch pieces of 2^10 B (41 x 64 pieces = 656
#    groups of 4 <= 4,096 waves), 64 pieces per frame. Main part: grid 256, rounds 32,768 / 4,096 = 8,
#    8 x 262,128 B per wave >= 1,520,000 and groups >= 128 KiB: one-word queue, static_rounds 8 - 8 / 2 = 4;
#    more than one pass: plain k_frames<16, 1>.
#  window-256x65536: 2 x 256 <= 4,096 waves, 1,025 units -> 17 rounds at one wave per frame against
#    1 pass x 3: split; 16 << 12 = 65,536 >= the frame: k0 12; grid min(256, 256).
#  window-512x16384: (256 + 64) / 64 = 5 rounds at one wave per frame against 2 passes x 3: not split. 8 lanes
#    doubled while ceil(512 / (64 / G)) x 2 <= 4,096 and 2 G <= 256 units: 64 lanes, 512 groups in 32
#    workgroups of 16 waves, one pass: one-pass loads, static, no tail.
HAND = {
    "cfg4-strided": [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 41, 10, 64)],
    "window-256x65536": [(1, 0, 0, 256, 0, 256, 12, 0, 0, 0, 0, 0)],
    "window-512x16384": [(3, 64, 1, 32, 0, 512, 0, 0, 0, 0, 0, 0)],
}

EXPECTED = {
    'cfg3': [(2, 8, 1, 256, 0, 1048576, 0, 1, 16, 0, 0, 0)],
    'cfg2': [(3, 4, 1, 256, 0, 65536, 0, 0, 0, 0, 0, 0)],
    'cfg4-strided': [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 41, 10, 64)],
    'cfg4-desc': [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 41, 10, 64)],
    'cfg5': [(0, 0, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'cfg3-1Mi-x-16KiB': [(2, 8, 1, 256, 0, 1048576, 0, 1, 16, 0, 0, 0)],
    'cfg3-desc': [(2, 8, 1, 256, 0, 1048576, 0, 1, 16, 0, 0, 0)],
    'window-256x65536': [(1, 0, 0, 256, 0, 256, 12, 0, 0, 0, 0, 0)],
    'window-256x8192': [(1, 0, 0, 256, 0, 256, 10, 0, 0, 0, 0, 0)],
    'window-512x16384': [(3, 64, 1, 32, 0, 512, 0, 0, 0, 0, 0, 0)],
    'window-1024x65536': [(1, 0, 0, 256, 0, 1024, 12, 0, 0, 0, 0, 0)],
    'window-2048x65536': [(3, 64, 1, 128, 0, 2048, 0, 0, 0, 0, 0, 0)],
    'window-257x8192': [(3, 64, 1, 17, 0, 257, 0, 0, 0, 0, 0, 0)],
    'window-256x8191': [(3, 64, 1, 16, 0, 256, 0, 0, 0, 0, 0, 0)],
    'window-2048x131072': [(1, 0, 0, 256, 0, 2048, 13, 0, 0, 0, 0, 0)],
    'window-2049x131072': [(3, 64, 1, 129, 0, 2049, 0, 0, 0, 0, 0, 0)],
    'window-256x16384': [(1, 0, 0, 256, 0, 256, 10, 0, 0, 0, 0, 0)],
    's600-r4': [(2, 2, -3, 256, 0, 524288, 0, 0, 0, 0, 0, 0)],
    'u600d-r4': [(2, 2, -3, 256, 0, 524288, 0, 0, 0, 0, 0, 0)],
    's600-r8': [(2, 2, -3, 256, 0, 1048576, 0, 0, 0, 0, 0, 0)],
    'u600d-r8': [(2, 2, -3, 256, 0, 1048576, 0, 64, 4, 0, 0, 0)],
    's600-r12': [(2, 2, -3, 256, 0, 1572864, 0, 0, 0, 0, 0, 0)],
    'u600d-r12': [(2, 2, -3, 256, 0, 1572864, 0, 64, 6, 0, 0, 0)],
    's1100-r4': [(2, 4, -2, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'u1100d-r4': [(2, 4, -2, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    's1100-r8': [(2, 4, -2, 256, 0, 524288, 0, 0, 0, 0, 0, 0)],
    'u1100d-r8': [(2, 4, -2, 256, 0, 524288, 0, 64, 4, 0, 0, 0)],
    's1100-r12': [(2, 4, -2, 256, 0, 786432, 0, 0, 0, 0, 0, 0)],
    'u1100d-r12': [(2, 4, -2, 256, 0, 786432, 0, 64, 6, 0, 0, 0)],
    's2000-r4': [(2, 4, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'u2000d-r4': [(2, 4, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    's2000-r8': [(2, 4, 1, 256, 0, 524288, 0, 0, 0, 0, 0, 0)],
    'u2000d-r8': [(2, 4, 1, 256, 0, 524288, 0, 64, 4, 0, 0, 0)],
    's2000-r12': [(2, 4, 1, 256, 0, 786432, 0, 0, 0, 0, 0, 0)],
    'u2000d-r12': [(2, 4, 1, 256, 0, 786432, 0, 64, 6, 0, 0, 0)],
    's4200-r4': [(2, 8, 1, 256, 0, 131072, 0, 0, 0, 0, 0, 0)],
    'u4200d-r4': [(2, 8, 1, 256, 0, 131072, 0, 0, 0, 0, 0, 0)],
    's4200-r8': [(2, 8, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'u4200d-r8': [(2, 8, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    's4200-r12': [(2, 8, 1, 256, 0, 393216, 0, 0, 0, 0, 0, 0)],
    'u4200d-r12': [(2, 8, 1, 256, 0, 393216, 0, 0, 0, 0, 0, 0)],
    'u600d-r7': [(2, 2, -3, 256, 0, 917504, 0, 0, 0, 0, 0, 0)],
    'u16400d-r6': [(2, 8, 1, 256, 0, 196608, 0, 0, 0, 0, 0, 0)],
    'u16400d-r15': [(2, 8, 1, 256, 0, 491520, 0, 0, 0, 0, 0, 0)],
    'u16400d-r16': [(2, 8, 1, 256, 0, 524288, 0, 1, 8, 0, 0, 0)],
    'u16400d-r32': [(2, 8, 1, 256, 0, 1048576, 0, 1, 16, 0, 0, 0)],
    's65532-r4': [(2, 16, 1, 256, 0, 65536, 0, 0, 0, 0, 0, 0)],
    's65532-r5': [(2, 16, 1, 256, 0, 81920, 0, 0, 0, 0, 0, 0)],
    's65532-r6': [(2, 16, 1, 256, 0, 98304, 0, 1, 3, 0, 0, 0)],
    's65532-r7': [(2, 16, 1, 256, 0, 114688, 0, 1, 4, 0, 0, 0)],
    's16400-r11': [(2, 8, 1, 256, 0, 360448, 0, 0, 0, 0, 0, 0)],
    's16400-r12': [(2, 8, 1, 256, 0, 393216, 0, 1, 6, 0, 0, 0)],
    's16383-r16': [(2, 8, 1, 256, 0, 524288, 0, 64, 8, 0, 0, 0)],
    's16384-r16': [(2, 8, 1, 256, 0, 524288, 0, 1, 8, 0, 0, 0)],
    'u24575d-r12': [(2, 8, 1, 256, 0, 393216, 0, 0, 0, 0, 0, 0)],
    'u24576d-r12': [(2, 8, 1, 256, 0, 393216, 0, 1, 6, 0, 0, 0)],
    's4095-r47': [(2, 8, 1, 256, 0, 1540096, 0, 0, 0, 0, 0, 0)],
    's4096-r47': [(2, 8, 1, 256, 0, 1540096, 0, 64, 24, 0, 0, 0)],
    'u511d-r8': [(2, 2, -3, 256, 0, 1048576, 0, 0, 0, 0, 0, 0)],
    'u512d-r8': [(2, 2, -3, 256, 0, 1048576, 0, 64, 4, 0, 0, 0)],
    's1023-4Mi': [(2, 2, -3, 256, 0, 4194304, 0, 0, 0, 0, 0, 0)],
    's1024-4Mi': [(2, 4, -2, 256, 0, 4194304, 0, 0, 0, 0, 0, 0)],
    's1599-4Mi': [(2, 4, -2, 256, 0, 4194304, 0, 0, 0, 0, 0, 0)],
    's1600-4Mi': [(2, 4, 1, 256, 0, 4194304, 0, 0, 0, 0, 0, 0)],
    's2047-4Mi': [(2, 4, 1, 256, 0, 4194304, 0, 0, 0, 0, 0, 0)],
    's2048-4Mi': [(2, 8, 1, 256, 0, 4194304, 0, 0, 0, 0, 0, 0)],
    's49151-4Mi': [(2, 8, 1, 256, 0, 4194304, 0, 1, 64, 0, 0, 0)],
    's49152-4Mi': [(2, 16, 1, 256, 0, 4194304, 0, 1, 128, 0, 0, 0)],
    'small-1x64': [(3, 2, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0)],
    'small-1x100': [(3, 2, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0)],
    'small-1x8192': [(1, 0, 0, 1, 0, 1, 10, 0, 0, 0, 0, 0)],
    'small-64x1100': [(3, 16, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'small-1024x1100': [(3, 16, 1, 16, 0, 1024, 0, 0, 0, 0, 0, 0)],
    'small-2048x4200': [(3, 64, 1, 128, 0, 2048, 0, 0, 0, 0, 0, 0)],
    'small-4096x4200': [(3, 64, 1, 256, 0, 4096, 0, 0, 0, 0, 0, 0)],
    'small-4097x4200': [(3, 32, 1, 129, 0, 4097, 0, 0, 0, 0, 0, 0)],
    'small-300x65536': [(1, 0, 0, 256, 0, 300, 12, 0, 0, 0, 0, 0)],
    'tail-s65532-r1+6': [(3, 16, 1, 256, 0, 16384, 0, 0, 0, 6, 10, 64)],
    'tail-s65532-r1+6-off': [(3, 16, 1, 256, 0, 16384, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 6, 16384, 6, 12, 0, 0, 0, 0, 0)],
    'tail-s65532-r1+1024': [(3, 16, 1, 256, 0, 16384, 0, 0, 0, 1024, 12, 16)],
    'tail-s65532-r1+1024-off': [(3, 16, 1, 256, 0, 16384, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 256, 16384, 1024, 12, 0, 0, 0, 0, 0)],
    'tail-s65532-r2+41': [(2, 16, 1, 256, 0, 32768, 0, 0, 0, 41, 10, 64)],
    'tail-s65532-r2+41-off': [(2, 16, 1, 256, 0, 32768, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 41, 32768, 41, 12, 0, 0, 0, 0, 0)],
    'tail-s16400-r1+100': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 100, 10, 17)],
    'tail-s16400-r1+100-off': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 100, 32768, 100, 11, 0, 0, 0, 0, 0)],
    'tail-s8192-r1+3': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 3, 10, 8)],
    'tail-s8192-r1+3-off': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 3, 32768, 3, 10, 0, 0, 0, 0, 0)],
    'tail-s24580-r4+777': [(2, 8, 1, 256, 0, 131072, 0, 0, 0, 777, 10, 25)],
    'tail-s24580-r4+777-off': [(2, 8, 1, 256, 0, 131072, 0, 0, 0, 0, 0, 0),
        (3, 64, 1, 49, 131072, 777, 0, 0, 0, 0, 0, 0)],
    'tail-s32784-r1+57': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 57, 10, 33)],
    'tail-s32784-r1+57-off': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 57, 32768, 57, 12, 0, 0, 0, 0, 0)],
    'tail-s8191-r1+3': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 0, 0, 0),
        (3, 64, 1, 1, 32768, 3, 0, 0, 0, 0, 0, 0)],
    'tail-s8191-r1+3-off': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 0, 0, 0),
        (3, 64, 1, 1, 32768, 3, 0, 0, 0, 0, 0, 0)],
    'tail-u65532d-r1+6': [(3, 16, 1, 256, 0, 16384, 0, 0, 0, 6, 10, 64)],
    'tail-u65532d-r1+6-off': [(3, 16, 1, 256, 0, 16384, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 6, 16384, 6, 12, 0, 0, 0, 0, 0)],
    'tail-u65532d-r8+41': [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 41, 10, 64)],
    'tail-u65532d-r8+41-off': [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 0, 0, 0),
        (1, 0, 0, 41, 131072, 41, 12, 0, 0, 0, 0, 0)],
    'tail-u16400d-r1+33': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 33, 10, 17)],
    'tail-u16400d-r1+33-off': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 0, 0, 0),
        (1, 0, 0, 33, 32768, 33, 11, 0, 0, 0, 0, 0)],
    'tail-forced8': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 9, 10, 64)],
    'tail-forced8-off': [(3, 8, 1, 256, 0, 32768, 0, 0, 0, 0, 0, 0),
        (3, 64, 1, 1, 32768, 9, 0, 0, 0, 0, 0, 0)],
    'tail-forced16': [(3, 16, 1, 256, 0, 16384, 0, 0, 0, 9, 10, 64)],
    'tail-forced16-off': [(3, 16, 1, 256, 0, 16384, 0, 0, 0, 0, 0, 0),
        (3, 64, 1, 1, 16384, 9, 0, 0, 0, 0, 0, 0)],
    'tail-forced32': [(3, 32, 1, 256, 0, 8192, 0, 0, 0, 0, 0, 0),
        (3, 64, 1, 1, 8192, 9, 0, 0, 0, 0, 0, 0)],
    'tail-forced32-off': [(3, 32, 1, 256, 0, 8192, 0, 0, 0, 0, 0, 0),
        (3, 64, 1, 1, 8192, 9, 0, 0, 0, 0, 0, 0)],
    'tail-pay': [(2, 16, 1, 256, 0, 16384, 0, 0, 0, 0, 0, 0),
        (2, 64, 1, 1, 16384, 9, 0, 0, 0, 0, 0, 0)],
    'tail-short-frames': [(2, 4, -2, 256, 0, 131072, 0, 0, 0, 0, 0, 0),
        (3, 64, 1, 7, 131072, 100, 0, 0, 0, 0, 0, 0)],
    'tail-too-long': [(3, 16, 1, 256, 0, 16384, 0, 0, 0, 3000, 14, 4)],
    'n0': [],
    'n1': [(1, 0, 0, 1, 0, 1, 11, 0, 0, 0, 0, 0)],
    'n1-empty': [(3, 64, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0)],
    'last-short': [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 41, 10, 64)],
    'last-short-window': [(1, 0, 0, 256, 0, 256, 12, 0, 0, 0, 0, 0)],
    'last-longer-window': [(1, 0, 0, 256, 0, 256, 12, 0, 0, 0, 0, 0)],
    'last-short-tail-off': [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 0, 0, 0),
        (1, 0, 0, 41, 131072, 41, 12, 0, 0, 0, 0, 0)],
    'hint0-4095': [(3, 64, 1, 256, 0, 4095, 0, 0, 0, 0, 0, 0)],
    'hint0-4096': [(0, 0, 1, 65, 0, 4096, 0, 0, 0, 0, 0, 0)],
    'hint0-min1': [(0, 0, 1, 1, 0, 7, 0, 0, 0, 0, 0, 0)],
    'hint0-forced-lanes': [(2, 8, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'hint0-strided': [(2, 8, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'ragged-depth0': [(0, 0, 0, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'ragged-ring': [(0, 0, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'pay-cfg3': [(2, 8, 1, 256, 0, 1048576, 0, 1, 16, 0, 0, 0)],
    'pay-window': [(2, 64, 1, 16, 0, 256, 0, 0, 0, 0, 0, 0)],
    'pay-ragged': [(0, 0, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'pay-short': [(2, 2, 1, 256, 0, 1048576, 0, 64, 4, 0, 0, 0)],
    'pay-forced-depth': [(2, 8, 1, 256, 0, 1048576, 0, 1, 16, 0, 0, 0)],
    'forced-g1-d0': [(2, 1, 0, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, 0, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d0-window': [(2, 1, 0, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d1': [(3, 1, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (3, 4, 1, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d1-window': [(3, 1, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d2': [(2, 1, 2, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, 2, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d2-window': [(2, 1, 2, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d4': [(2, 1, 4, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, 4, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d4-window': [(2, 1, 4, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d-2': [(2, 1, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, -2, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d-2-window': [(2, 1, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d-3': [(2, 1, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, -3, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g1-d-3-window': [(2, 1, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d0': [(2, 2, 0, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, 0, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d0-window': [(2, 2, 0, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d1': [(2, 2, 1, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (3, 4, 1, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d1-window': [(3, 2, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d2': [(2, 2, 2, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, 2, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d2-window': [(2, 2, 2, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d4': [(2, 2, 4, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, 4, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d4-window': [(2, 2, 4, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d-2': [(2, 2, -2, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, -2, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d-2-window': [(2, 2, -2, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d-3': [(2, 2, -3, 256, 0, 262144, 0, 0, 0, 0, 0, 0),
        (2, 4, -3, 148, 262144, 37856, 0, 0, 0, 0, 0, 0)],
    'forced-g2-d-3-window': [(2, 2, -3, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d0': [(2, 4, 0, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d0-window': [(2, 4, 0, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d1': [(2, 4, 1, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d1-window': [(3, 4, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d2': [(2, 4, 2, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d2-window': [(2, 4, 2, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d4': [(2, 4, 4, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d4-window': [(2, 4, 4, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d-2': [(2, 4, -2, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d-2-window': [(2, 4, -2, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d-3': [(2, 4, -3, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g4-d-3-window': [(2, 4, -3, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d0': [(2, 8, 0, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 0, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d0-window': [(2, 8, 0, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d1': [(2, 8, 1, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (3, 32, 1, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d1-window': [(3, 8, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d2': [(2, 8, 2, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 2, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d2-window': [(2, 8, 2, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d4': [(2, 8, 4, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 4, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d4-window': [(2, 8, 4, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d-2': [(2, 8, 1, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 1, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d-2-window': [(2, 8, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d-3': [(2, 8, 1, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 1, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g8-d-3-window': [(2, 8, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d0': [(2, 16, 0, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 0, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d0-window': [(2, 16, 0, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d1': [(2, 16, 1, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (3, 32, 1, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d1-window': [(3, 16, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d2': [(2, 16, 2, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 2, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d2-window': [(2, 16, 2, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d4': [(2, 16, 4, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 4, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d4-window': [(2, 16, 4, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d-2': [(2, 16, 1, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 1, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d-2-window': [(2, 16, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d-3': [(2, 16, 1, 256, 0, 294912, 0, 0, 0, 0, 0, 0),
        (2, 32, 1, 159, 294912, 5088, 0, 0, 0, 0, 0, 0)],
    'forced-g16-d-3-window': [(2, 16, 1, 1, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d0': [(2, 32, 0, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d0-window': [(2, 32, 0, 2, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d1': [(2, 32, 1, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d1-window': [(3, 32, 1, 2, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d2': [(2, 32, 2, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d2-window': [(2, 32, 2, 2, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d4': [(2, 32, 4, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d4-window': [(2, 32, 4, 2, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d-2': [(2, 32, 1, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d-2-window': [(2, 32, 1, 2, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d-3': [(2, 32, 1, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g32-d-3-window': [(2, 32, 1, 2, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d0': [(2, 64, 0, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d0-window': [(2, 64, 0, 4, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d1': [(2, 64, 1, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d1-window': [(3, 64, 1, 4, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d2': [(2, 64, 2, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d2-window': [(2, 64, 2, 4, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d4': [(2, 64, 4, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d4-window': [(2, 64, 4, 4, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d-2': [(2, 64, 1, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d-2-window': [(2, 64, 1, 4, 0, 64, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d-3': [(2, 64, 1, 256, 0, 300000, 0, 0, 0, 0, 0, 0)],
    'forced-g64-d-3-window': [(2, 64, 1, 4, 0, 64, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d0': [(2, 2, 0, 256, 0, 1048576, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d0-long': [(2, 16, 0, 256, 0, 131072, 0, 1, 4, 0, 0, 0),
        (2, 64, 0, 3, 131072, 41, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d1': [(2, 2, 1, 256, 0, 1048576, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d1-long': [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 0, 0, 0),
        (3, 64, 1, 3, 131072, 41, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d2': [(2, 2, 2, 256, 0, 1048576, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d2-long': [(2, 16, 2, 256, 0, 131072, 0, 1, 4, 0, 0, 0),
        (2, 64, 2, 3, 131072, 41, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d4': [(2, 2, 4, 256, 0, 1048576, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d4-long': [(2, 16, 4, 256, 0, 131072, 0, 1, 4, 0, 0, 0),
        (2, 64, 4, 3, 131072, 41, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d-2': [(2, 2, -2, 256, 0, 1048576, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d-2-long': [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 0, 0, 0),
        (2, 64, 1, 3, 131072, 41, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d-3': [(2, 2, -3, 256, 0, 1048576, 0, 0, 0, 0, 0, 0)],
    'auto-lanes-d-3-long': [(2, 16, 1, 256, 0, 131072, 0, 1, 4, 0, 0, 0),
        (2, 64, 1, 3, 131072, 41, 0, 0, 0, 0, 0, 0)],
    'cus8-cfg3': [(2, 8, 1, 8, 0, 1048576, 0, 1, 512, 0, 0, 0)],
    'cus8-cfg4-desc': [(2, 16, 1, 8, 0, 131072, 0, 1, 128, 41, 13, 8)],
    'cus8-window-8x64KiB': [(1, 0, 0, 8, 0, 8, 12, 0, 0, 0, 0, 0)],
    'cus8-window-64x64KiB': [(3, 64, 1, 4, 0, 64, 0, 0, 0, 0, 0, 0)],
    'cus8-window-65x64KiB': [(3, 64, 1, 5, 0, 65, 0, 0, 0, 0, 0, 0)],
    'cus8-tail': [(3, 16, 1, 8, 0, 512, 0, 0, 0, 3, 10, 64)],
    'cus8-u600d-r8': [(2, 2, -3, 8, 0, 32768, 0, 64, 4, 0, 0, 0)],
    'cus8-cfg5': [(0, 0, 1, 8, 0, 262144, 0, 0, 0, 0, 0, 0)],
    'cus8-ragged-small': [(0, 0, 1, 2, 0, 100, 0, 0, 0, 0, 0, 0)],
}


@pytest.fixture()
def knobs():
    """Sets the process's knobs for one case and restores them, as the GPU tests' fixtures do."""
    lib = vc.lib()

    def set_(lanes=0, prefetch=-1, tail_pieces=-1, ragged_min=-1):
        vc.set_geometry(lanes, prefetch)
        lib.val_gpu_set_tail_pieces(tail_pieces)
        lib.val_gpu_set_ragged_min_frames(ragged_min)

    yield set_
    set_()


def _plan(args):
    return [l.astuple() for l in vc.plan_frames(args["cus"], args["n"], args["typical_len"],
                                                descriptors=args["descriptors"], flen=args["flen"],
                                                last_len=args["last_len"], want_payload=args["want_payload"])]


def test_table_is_complete():
    ids = [cid for cid, _, _ in CASES]
    assert len(set(ids)) == len(ids)
    assert set(ids) == set(EXPECTED)
    assert all(EXPECTED[k] == v for k, v in HAND.items())


@pytest.mark.parametrize("cid,args,kn", CASES, ids=[c[0] for c in CASES])
def test_plan(knobs, cid, args, kn):
    knobs(**kn)
    got = _plan(args)
    assert got == EXPECTED[cid], (args, kn)
    # a plan covers the batch exactly once
    assert sum(l[5] + l[9] for l in got) == args["n"]
    assert [l[4] for l in got] == [0, got[0][5] if got else 0][:len(got)]


@pytest.mark.parametrize("cus", [64, 128, 256, 304])
def test_gpu_queue_shapes_reach_the_queue(knobs, cus):
    """The shapes of tests/test_gpu_dyn_queue.py are functions of the CU count; each GPU case asserts
    from the plan that it reaches its branch (the 64 partitions with a round of the machine behind the
    static rounds, the second launch of a re-cut tail, more ragged items than waves). The same
    assertions here, for the device sizes the suite may meet."""
    from tests import test_gpu_dyn_queue as q

    knobs()
    n1, plan = q.plan_case1(vc, cus)
    assert (plan[0].qparts, plan[0].static_rounds, plan[0].depth, len(plan)) == (64, 4, -3, 2)
    n2, plan = q.plan_case2(vc, cus)
    assert n2 == n1 and (plan[0].qparts, plan[0].static_rounds, plan[0].depth) == (64, 4, 1)
    _, plans = q.plan_case3(vc, cus)
    assert [plans[k][0].depth for k in (-1, 1, 0, "pay")] == [-2, 1, 0, 1]
    assert all(p[0].qparts == 64 and p[0].static_rounds == 4 for p in plans.values())
    n4, plan = q.plan_case4(vc, cus)
    assert (plan[0].qparts, plan[0].static_rounds, plan[0].lanes) == (64, 24, 8) and n4 * 4100 < 8 << 30
    n4s, _ = q.plan_case4_stream(vc, cus)  # the same launches with the stream loads forced: [True, False]
    assert n4s == n4
    for G in (2, 4, 8, 16, 32):
        n5, plan = q.plan_case5(vc, cus, G)
        assert plan[0].qparts == 0 and plan[1].first == cus * 16 * (64 // G) * 2 and plan[1].count == 100
    q.plan_case6(vc, cus)
    _, plan = q.plan_case7(vc, cus)
    assert plan[0].lanes == 8 and plan[1].count == 77
    # and the knobs are back where the table assumes them
    assert vc.plan_frames(256, _rounds(2, 8), 600, descriptors=True)[0].astuple() == EXPECTED["u600d-r8"][0]


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_stream_loads_meet_the_partitioned_queue_by_the_rule(knobs, cus):
    """Shipped launches run k_frames_stream out of the 64-partition queue: a strided launch of 8,192-B
    frames over 24 group rounds and 13 frames is, by the rule and with nothing forced, one stream-load
    launch at 8 lanes with qparts 64, 12 static rounds and the 13 frames as in-launch tail pieces.
    tests/test_gpu_dyn_queue.py case 4 reaches that branch on the GPU by forcing the path onto its
    4,096-B frames; if the rule moves so that no such launch is planned, this fails."""
    knobs()
    n = 24 * cus * 128 + 13
    plan = vc.plan_frames(cus, n, 8192, flen=8192)
    assert len(plan) == 1, [l.astuple() for l in plan]
    m = plan[0]
    assert (m.kernel, m.lanes, m.depth, m.qparts, m.static_rounds, m.tail_n) == (2, 8, 1, 64, 12, 13), m.astuple()
    assert vc.plan_stream_loads(cus, n, 8192, flen=8192) == [True]


@pytest.mark.parametrize("cus", [64, 128, 256, 304])
def test_gpu_split_shapes_reach_split(knobs, cus):
    """The shapes of tests/test_gpu_split.py and tests/test_gpu_split_edges.py are functions of the CU
    count (tests/_split_shapes.py); each GPU case asserts from the plan that its call is a
    k_frames_split launch with the expected chunk size, grid and first frame. The same assertions
    here, with the properties the shape functions assert of their own batches (a bad frame in every
    trip, every length at every phase, what the fuzz rounds reached at the default seed), for the
    device sizes the suite may meet."""
    from tests import _split_shapes as s

    knobs()
    # the cases of tests/test_gpu_split.py
    for n, payload in ((1, 8192), (3, 16384), (17, 16384), (256, 65516), (64, 65520)):
        s.split_plan(vc, cus, n, 16 + payload, k0=s.STRIDED_K0[payload])
    for hint, k0 in ((8192, 10), (16400, 11), (65532, 12)):
        s.split_plan(vc, cus, min(200, cus), hint, descriptors=True, k0=k0)
    s.split_plan(vc, cus, 120, 32784, k0=12)
    s.split_plan(vc, cus, 1, 8192, k0=10)
    assert s.not_split_plan(vc, cus, 1, 8191)[0].kernel == vc.KERNEL_FRAMES_C0
    # 300 frames of 8,192 B: one trip of the grid or none
    assert s.rule_says_split(cus, 300, 8192) == (cus >= 300)
    if cus == 256:
        s.not_split_plan(vc, cus, 300, 8192)
    if cus == 304:
        s.split_plan(vc, cus, 300, 8192, k0=10)
    # 1. three trips
    for desc in (False, True):
        n, plan = s.trips_plan(vc, cus, desc)
        assert (n, plan[0].grid, plan[0].k0) == (2 * cus + 3, cus, 12)
    lens, offs, total = s.trips_descriptors(cus)
    assert lens.size == 2 * cus + 3 and total < 64 << 20
    bad = s.trips_bad(cus, lens)
    assert all(0 <= s.bad_position(k, int(lens[f]), s.TRIPS_K0) < int(lens[f]) + 4 for f, k in bad)
    assert all(s.bad_position(k, int(lens[f]), s.TRIPS_K0) < int(lens[f]) for f, k in bad if k in (0, 1, 6))
    # 2. the ladder, the edges, the long frame
    assert [s.ladder_plan(vc, cus, i)[0] for i in range(len(s.LADDER))] == [f for f, _ in s.LADDER]
    assert [k for _, k in s.LADDER] == [10, 11, 12, 13, 14, 16, 17, 20, 21] == [s.k0_for(f) for f, _ in s.LADDER]
    for hint, k0 in s.EDGE_HINTS:
        lens, offs, total = s.edge_descriptors(k0)
        W = 1 << k0
        assert lens.size == 288 and total < 64 << 20
        for m in s.EDGE_M:
            for r in (0, 1, 3, 4, 63, 64, 65, W - 1):
                assert set(int(o) % 4 for o, L in zip(offs, lens) if L == m * W + r) == {0, 1, 2, 3}, (m, r)
        assert set(int(c) for c in s.chunks(lens, k0)) >= {1, 15, 16, 17, 32, 33, 49}
        calls = s.edge_calls(vc, cus, hint, k0)
        assert calls[0][0] == 0 and calls[-1][1] == 288 and all(a[1] == b[0] for a, b in zip(calls, calls[1:]))
        assert len(calls) == (-(-288 // cus) if hint == 8192 else 1)
    s.big_plan(vc, cus)
    # 3. split as the second launch, with the tail pieces off
    with s.tail_pieces_off(vc):
        for tail in s.tail_counts(cus):
            for desc in (False, True):
                n, plan = s.tail_plan(vc, cus, tail, desc)
                assert (plan[1].first, plan[1].count, plan[1].k0) == (cus * 64, tail, 12)
                assert -(-tail // plan[1].grid) == (1 if tail == 6 else 2)
            lens, offs, total = s.tail_descriptors(cus, tail)
            assert lens.size == cus * 64 + tail and sorted(set(s.tail_bad(cus, tail))) == s.tail_bad(cus, tail)
    # with them on, the same batches are one launch with the tail inside it
    assert [l.tail_n for l in vc.plan_frames(cus, cus * 64 + 6, 65532, flen=65532)] == [6]
    # 4. the fuzz at its default seed and rounds: every round on split, and what the rounds must reach
    rounds = s.fuzz_rounds(vc, cus, s.FUZZ_DEFAULT_SEED, s.FUZZ_DEFAULT_ROUNDS)
    assert len(rounds) == 60
    for c in rounds:
        s.split_plan(vc, cus, c["n"], c["typical"], descriptors=c["descriptors"], k0=c["k0"])
        assert 1 <= c["n"] <= 3 * cus and 8192 <= c["typical"] <= 1 << 21 and c["total"] <= 64 << 20
        assert c["k0"] == s.k0_for(c["typical"]) and c["trips"] == -(-c["n"] // min(c["n"], cus))
    s.fuzz_coverage(rounds)
    # and the knobs are back where the table assumes them
    assert vc.plan_frames(256, 16384 + 6, 65532, flen=65532)[0].astuple() == EXPECTED["tail-s65532-r1+6"][0]


@pytest.fixture(scope="module")
def ragged_trips():
    """The 4.5 M lengths of the binning-trips case: no function of the CU count, built once."""
    from tests import _ragged_shapes as s

    return s.trips_batch()


def test_ragged_restatement_matches_the_header_table():
    """tests/_ragged_shapes.py restates length_bucket from the table in the comment above it: the
    ranges 0..7 | 8..36 | 37..117 | 118..134 and 135, the class limits, and each bucket's lowest
    and highest length, checked against each other over every length up to 70,000."""
    from tests import _ragged_shapes as s

    L = np.arange(0, 70001)
    b = s.bucket(L)
    assert np.array_equal(s.bucket_class(b), s.length_class(L)) and (np.diff(b) >= 0).all()
    assert [int(b[L == v][0]) for v in (0, 128, 129, 1023, 1024, 1025, 8191, 8192, 8193, 49151, 49152, 49153, 65536,
                                        65537)] == [0, 0, 1, 7, 8, 9, 36, 37, 38, 117, 118, 119, 134, 135]
    assert s.bucket(2**32 - 1) == 135 and s.bucket((1 << 24) + 5) == 135
    for k in range(s.BUCKETS):
        lo, hi = s.bucket_bounds(k)
        assert lo == int(L[b == k].min()) and (hi if hi is not None else 70000) == int(L[b == k].max()), k
    # rounds of the class: a bucket of class c spans LANES[c] * 64 bytes
    for c in range(4):
        for k in range(s.CLASS_FIRST_BUCKET[c] + 2, s.CLASS_FIRST_BUCKET[c + 1] - 1):
            lo, hi = s.bucket_bounds(k)
            assert hi is None or hi - lo + 1 == 64 * s.LANES[c], k
    assert s.bin_grid(1) == (1, 1, 1) and s.bin_grid(2048) == (1, 2048, 1) and s.bin_grid(2049) == (2, 1025, 1)
    assert s.bin_grid(262144) == (128, 2048, 1) and s.bin_grid(1 << 21) == (1024, 2048, 1)
    assert s.bin_grid((1 << 21) + 1) == (1024, 2049, 2)
    tab = s.class_table(np.array([5, 70000, 1024, 1023, 8192, 8192, 49152], np.uint32))
    assert (tab["count"], tab["start"], tab["items"], tab["first_item"], tab["total"], tab["one_bucket"]) == \
        ([2, 1, 2, 2], [5, 4, 2, 0], [1, 1, 1, 1], [3, 2, 1, 0], 4, False)
    assert [s.item_class(tab, it) for it in range(4)] == [3, 2, 1, 0]


@pytest.mark.parametrize("cus", [64, 128, 256, 304])
def test_gpu_ragged_shapes_reach_their_branches(knobs, cus, ragged_trips):
    """The shapes of tests/test_gpu_ragged_edges.py and tests/test_gpu_ragged_fuzz.py are functions of
    the CU count (tests/_ragged_shapes.py); each GPU case asserts from the restated plan and from
    val_gpu_plan_frames that it reaches its branch. The same assertions here for the device sizes
    the suite may meet, and ragged_grid against the planner around the point where the grid reaches
    the CU count."""
    from tests import _ragged_shapes as s

    knobs(ragged_min=1)
    for n in [1, 2, 3, 4, 5, 47, 48, 49, 60, 61, 64 * 63 - 16, 64 * 63 - 15, 64 * 64 - 16, 64 * 64 - 15, 5000] + \
            [64 * cus + d for d in (-80, -17, -16, -15, -13, -12, 0, 1, 64, 5000)] + [1 << 20, s.TRIPS_N]:
        for pay in (False, True):
            assert s.ragged_plan(vc, cus, n, want_payload=pay) == s.ragged_grid(cus, n)
    assert s.ragged_grid(cus, 64 * cus - 16) == cus and s.ragged_grid(cus, 64 * cus - 80) == cus - 1
    # 1. the binning loop's later trips
    lens, plants = ragged_trips
    assert s.ragged_plan(vc, cus, lens.size) == cus and len(plants) == 9
    assert all(int(lens[i]) == L for i, L in plants.items())
    # 2. every bucket
    lens, offs, total, bad = s.every_bucket_batch()
    assert s.ragged_plan(vc, cus, lens.size, want_payload=True) == 5 and s.class_table(lens)["total"] == 1 + 4 + 21 + 10
    # 3. class subsets and partial items
    seen = set()
    for si, classes in enumerate(s.SUBSETS):
        lens, offs, total, tab, bad = s.subset_batch(si)
        grid = s.ragged_plan(vc, cus, lens.size)
        assert s.parts(grid) == grid <= 4 and total < 2 << 20
        assert [tab["count"][c] for c in classes] == [s.count_of(c, s.subset_kind(si, j)) for j, c in enumerate(classes)]
        assert len(bad) == sum(1 + (tab["items"][c] > 1) for c in classes)
        seen |= {(c, s.subset_kind(si, j)) for j, c in enumerate(classes)}
    assert seen == {(c, k) for c in range(4) for k in range(s.COUNT_KINDS)}, "every class at every count"
    # 4. one bucket at a small grid and at the full grid
    grids = [s.identity_small_facts(cus, n, L) for n, L in s.IDENTITY_SMALL]
    assert [g for g, _ in grids] == [1, 1, 1, 3, 16, 18, 2] and [i for _, i in grids] == [1, 1, 2, 4, 32, 35, 7]
    n = s.identity_full_n(cus)
    assert s.ragged_plan(vc, cus, n) == cus
    assert [s.ragged_plan(vc, cus, k) for k in s.CHAIN_N] == [63, 15, 16] and s.CHAIN_N[1] * 4 < s.CHAIN_N[0]
    assert all(s.mixed_lens(k, i).size == k for i, k in enumerate(s.CHAIN_N[:2]))
    # 5. the deep queue, and its host chunks on the default threshold
    lens, offs, total, tab, bad, chunks = s.deep_batch(cus)
    assert s.ragged_plan(vc, cus, lens.size) == cus and tab["total"] >= 4 * 16 * cus
    knobs()
    for i, j in chunks:
        assert j - i >= 4096 and int(offs[j - 1]) + int(lens[j - 1]) - int(offs[i]) <= s.HOST_CHUNK
        assert s.ragged_plan(vc, cus, j - i) == s.ragged_grid(cus, j - i)
    assert chunks[0][0] == 0 and chunks[-1][1] == lens.size and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    knobs(ragged_min=1)
    # 6. both reservation paths
    assert s.slot_facts(8192) == (4, 2048, 1, 64) and s.slot_facts(8192 - 37) == (4, 2039, 1, 54)
    for n in (8192, 8192 - 37):
        lens, uniform = s.slot_batch(n)
        assert s.ragged_plan(vc, cus, n) == min(cus, 129 - (n < 8192)) and 40 <= sum(uniform) <= 44 and uniform[-1]
    # 7. the fuzz at its default seed and rounds
    rounds = s.fuzz_rounds(cus, s.FUZZ_DEFAULT_SEED, s.FUZZ_DEFAULT_ROUNDS)
    assert len(rounds) == 60
    for r in rounds:
        assert s.ragged_plan(vc, cus, r["n"], want_payload=r["mode"] == "ex") == r["grid"]
        assert 1 <= r["n"] <= s.FUZZ_MAX_N and int(r["lens"].astype(np.int64).sum()) <= s.FUZZ_CAP
    s.fuzz_coverage(rounds, cus)
    # and the knobs are back where the table assumes them
    knobs()
    assert vc.plan_frames(256, 262144, 0, descriptors=True)[0].astuple() == EXPECTED["cfg5"][0]


# ---- the window calls (val_gpu_plan_window) ----------------------------------
# The lanes and grids of the framer, both unpack calls, the scan and the fill,
# pinned the same way: W_EXPECTED holds what the launch functions computed
# before this arithmetic was moved out of them (their expressions, run as a
# host program over this table); three rows (W_HAND) are also derived by hand
# below. A row is a launch as (kernel, lanes, grid, count): kernel 4 k_pack,
# 5 k_unpack_parse, 6 k_unpack_order, 7 k_unpack_order_files, 8 k_unpack,
# 9 k_scan_streams (lanes per stream), 10 k_scan_first, 11 k_scan_compact,
# 12 k_fill_count, 13 k_fill_desc.
W_N = (1, 63, 64, 4096, 65535, 65536, 1 << 20)
W_HINTS = (0, 600, 1100, 16400, 65532)
W_STREAMS = (1, 256, 257, 100000)
W_MAX_FRAMES = (1, 513)


def _wcase(cid, call, cus, n, *, groups=0, max_frames=0, len_hint=0, **knobs):
    return cid, dict(call=call, cus=cus, n=n, groups=groups, max_frames=max_frames, len_hint=len_hint), knobs


def _window_cases():
    c = []
    for cus in (256, 8):
        for name, call in (("pack", vc.WINDOW_PACK), ("unpack", vc.WINDOW_UNPACK)):
            for n in W_N:
                for hint in W_HINTS:
                    c.append(_wcase(f"{name}-cus{cus}-n{n}-h{hint}", call, cus, n, len_hint=hint))
                for lanes in (1, 64):
                    c.append(_wcase(f"{name}-cus{cus}-n{n}-g{lanes}", call, cus, n, len_hint=1100, lanes=lanes))
        for groups in (1, 255, 256, 257):
            for n in (257, 65536):
                c.append(_wcase(f"unpack-files-cus{cus}-n{n}-f{groups}", vc.WINDOW_UNPACK_FILES, cus, n, groups=groups,
                                len_hint=1100))
        for n in W_STREAMS:
            for mf in W_MAX_FRAMES:
                for front in (0, 64, 1024):
                    c.append(_wcase(f"scan-cus{cus}-n{n}-m{mf}-front{front}", vc.WINDOW_SCAN, cus, n, max_frames=mf,
                                    front=front))
                for mtu in (21, 1024, 16396, 65547):
                    c.append(_wcase(f"fill-cus{cus}-n{n}-m{mf}-mtu{mtu}", vc.WINDOW_FILL, cus, n, max_frames=mf,
                                    len_hint=mtu))
        # each side of k_fill_desc's persistent grid: cus * kFillBlocksPerCU workgroups of kFillBlock slots
        full = cus * 8 * 256
        for slots in (full - 256, full, full + 1):
            c.append(_wcase(f"fill-cus{cus}-slots{slots}", vc.WINDOW_FILL, cus, 1, max_frames=slots, len_hint=1024))
    # what launches nothing, and what is no call
    c.append(_wcase("pack-n0", vc.WINDOW_PACK, 256, 0, len_hint=1100))
    c.append(_wcase("unpack-files-f0", vc.WINDOW_UNPACK_FILES, 256, 64, groups=0, len_hint=1100))
    c.append(_wcase("scan-m0", vc.WINDOW_SCAN, 256, 64, max_frames=0))
    c.append(_wcase("fill-n0", vc.WINDOW_FILL, 256, 0, max_frames=8, len_hint=1024))
    c.append(_wcase("fill-slots-overflow", vc.WINDOW_FILL, 256, 1 << 16, max_frames=1 << 16, len_hint=1024))
    c.append(_wcase("unknown-call", 5, 256, 64, max_frames=8, len_hint=1024))
    return c


W_CASES = _window_cases()

# Derived by hand from the launch functions this policy was moved out of:
#  pack-cus256-n65536-h600: 600 B -> 2 lanes; 65,536 x 2 x 2 = 262,144 <= 256 x 1,024 threads: 4 lanes;
#    65,536 x 4 x 2 is above: stays. 16 frames per wave: 4,096 groups in 256 workgroups of 16 waves, grid
#    min(256, 256).
#  scan-cus256-n257-m513-front0: 257 streams > 256 CUs: a wave per stream, 4 per workgroup: ceil(257 / 4) = 65
#    workgroups <= 256 x 8. k_scan_first is one workgroup. 257 x 513 = 131,841 slots in
#    ceil(131,841 / 256) = 516 workgroups <= 2,048.
#  fill-cus8-n256-m513-mtu1024: 256 transfers in one workgroup of 256; k_scan_first one workgroup; 131,328
#    slots are 513 workgroups, capped at 8 x 8 = 64. k_pack: content 1,020 B -> 2 lanes; 131,328 x 2 x 2 is
#    above 8 x 1,024 threads: stays. 32 frames per wave: 4,104 groups in ceil(4,104 / 16) = 257 workgroups,
#    capped at 8.
W_HAND = {
    "pack-cus256-n65536-h600": [(4, 4, 256, 65536)],
    "scan-cus256-n257-m513-front0": [(9, 64, 65, 257), (10, 0, 1, 257), (11, 0, 516, 131841)],
    "fill-cus8-n256-m513-mtu1024": [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 64, 131328), (4, 2, 8, 131328)],
}

W_EXPECTED = {
    'pack-cus256-n1-h0': [(4, 64, 1, 1)],
    'pack-cus256-n1-h600': [(4, 64, 1, 1)],
    'pack-cus256-n1-h1100': [(4, 64, 1, 1)],
    'pack-cus256-n1-h16400': [(4, 64, 1, 1)],
    'pack-cus256-n1-h65532': [(4, 64, 1, 1)],
    'pack-cus256-n1-g1': [(4, 1, 1, 1)],
    'pack-cus256-n1-g64': [(4, 64, 1, 1)],
    'pack-cus256-n63-h0': [(4, 64, 4, 63)],
    'pack-cus256-n63-h600': [(4, 64, 4, 63)],
    'pack-cus256-n63-h1100': [(4, 64, 4, 63)],
    'pack-cus256-n63-h16400': [(4, 64, 4, 63)],
    'pack-cus256-n63-h65532': [(4, 64, 4, 63)],
    'pack-cus256-n63-g1': [(4, 1, 1, 63)],
    'pack-cus256-n63-g64': [(4, 64, 4, 63)],
    'pack-cus256-n64-h0': [(4, 64, 4, 64)],
    'pack-cus256-n64-h600': [(4, 64, 4, 64)],
    'pack-cus256-n64-h1100': [(4, 64, 4, 64)],
    'pack-cus256-n64-h16400': [(4, 64, 4, 64)],
    'pack-cus256-n64-h65532': [(4, 64, 4, 64)],
    'pack-cus256-n64-g1': [(4, 1, 1, 64)],
    'pack-cus256-n64-g64': [(4, 64, 4, 64)],
    'pack-cus256-n4096-h0': [(4, 64, 256, 4096)],
    'pack-cus256-n4096-h600': [(4, 64, 256, 4096)],
    'pack-cus256-n4096-h1100': [(4, 64, 256, 4096)],
    'pack-cus256-n4096-h16400': [(4, 64, 256, 4096)],
    'pack-cus256-n4096-h65532': [(4, 64, 256, 4096)],
    'pack-cus256-n4096-g1': [(4, 1, 4, 4096)],
    'pack-cus256-n4096-g64': [(4, 64, 256, 4096)],
    'pack-cus256-n65535-h0': [(4, 4, 256, 65535)],
    'pack-cus256-n65535-h600': [(4, 4, 256, 65535)],
    'pack-cus256-n65535-h1100': [(4, 4, 256, 65535)],
    'pack-cus256-n65535-h16400': [(4, 8, 256, 65535)],
    'pack-cus256-n65535-h65532': [(4, 16, 256, 65535)],
    'pack-cus256-n65535-g1': [(4, 1, 64, 65535)],
    'pack-cus256-n65535-g64': [(4, 64, 256, 65535)],
    'pack-cus256-n65536-h0': [(4, 4, 256, 65536)],
    'pack-cus256-n65536-h600': [(4, 4, 256, 65536)],
    'pack-cus256-n65536-h1100': [(4, 4, 256, 65536)],
    'pack-cus256-n65536-h16400': [(4, 8, 256, 65536)],
    'pack-cus256-n65536-h65532': [(4, 16, 256, 65536)],
    'pack-cus256-n65536-g1': [(4, 1, 64, 65536)],
    'pack-cus256-n65536-g64': [(4, 64, 256, 65536)],
    'pack-cus256-n1048576-h0': [(4, 4, 256, 1048576)],
    'pack-cus256-n1048576-h600': [(4, 2, 256, 1048576)],
    'pack-cus256-n1048576-h1100': [(4, 4, 256, 1048576)],
    'pack-cus256-n1048576-h16400': [(4, 8, 256, 1048576)],
    'pack-cus256-n1048576-h65532': [(4, 16, 256, 1048576)],
    'pack-cus256-n1048576-g1': [(4, 1, 256, 1048576)],
    'pack-cus256-n1048576-g64': [(4, 64, 256, 1048576)],
    'unpack-cus256-n1-h0': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus256-n1-h600': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus256-n1-h1100': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus256-n1-h16400': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus256-n1-h65532': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus256-n1-g1': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 1, 1, 1)],
    'unpack-cus256-n1-g64': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus256-n63-h0': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus256-n63-h600': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus256-n63-h1100': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus256-n63-h16400': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus256-n63-h65532': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus256-n63-g1': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 1, 1, 63)],
    'unpack-cus256-n63-g64': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus256-n64-h0': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus256-n64-h600': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus256-n64-h1100': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus256-n64-h16400': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus256-n64-h65532': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus256-n64-g1': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 1, 1, 64)],
    'unpack-cus256-n64-g64': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus256-n4096-h0': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 64, 1024, 4096)],
    'unpack-cus256-n4096-h600': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 64, 1024, 4096)],
    'unpack-cus256-n4096-h1100': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 64, 1024, 4096)],
    'unpack-cus256-n4096-h16400': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 64, 1024, 4096)],
    'unpack-cus256-n4096-h65532': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 64, 1024, 4096)],
    'unpack-cus256-n4096-g1': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 1, 16, 4096)],
    'unpack-cus256-n4096-g64': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 64, 1024, 4096)],
    'unpack-cus256-n65535-h0': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 8, 2048, 65535)],
    'unpack-cus256-n65535-h600': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 8, 2048, 65535)],
    'unpack-cus256-n65535-h1100': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 8, 2048, 65535)],
    'unpack-cus256-n65535-h16400': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 8, 2048, 65535)],
    'unpack-cus256-n65535-h65532': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 16, 2048, 65535)],
    'unpack-cus256-n65535-g1': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 1, 256, 65535)],
    'unpack-cus256-n65535-g64': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 64, 2048, 65535)],
    'unpack-cus256-n65536-h0': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 8, 2048, 65536)],
    'unpack-cus256-n65536-h600': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 8, 2048, 65536)],
    'unpack-cus256-n65536-h1100': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 8, 2048, 65536)],
    'unpack-cus256-n65536-h16400': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 8, 2048, 65536)],
    'unpack-cus256-n65536-h65532': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 16, 2048, 65536)],
    'unpack-cus256-n65536-g1': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 1, 256, 65536)],
    'unpack-cus256-n65536-g64': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 64, 2048, 65536)],
    'unpack-cus256-n1048576-h0': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 4, 2048, 1048576)],
    'unpack-cus256-n1048576-h600': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 2, 2048, 1048576)],
    'unpack-cus256-n1048576-h1100': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 4, 2048, 1048576)],
    'unpack-cus256-n1048576-h16400': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 8, 2048, 1048576)],
    'unpack-cus256-n1048576-h65532': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 16, 2048, 1048576)],
    'unpack-cus256-n1048576-g1': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 1, 2048, 1048576)],
    'unpack-cus256-n1048576-g64': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 64, 2048, 1048576)],
    'unpack-files-cus256-n257-f1': [(5, 0, 2, 257), (7, 0, 1, 1), (8, 64, 65, 257)],
    'unpack-files-cus256-n65536-f1': [(5, 0, 256, 65536), (7, 0, 1, 1), (8, 8, 2048, 65536)],
    'unpack-files-cus256-n257-f255': [(5, 0, 2, 257), (7, 0, 255, 255), (8, 64, 65, 257)],
    'unpack-files-cus256-n65536-f255': [(5, 0, 256, 65536), (7, 0, 255, 255), (8, 8, 2048, 65536)],
    'unpack-files-cus256-n257-f256': [(5, 0, 2, 257), (7, 0, 256, 256), (8, 64, 65, 257)],
    'unpack-files-cus256-n65536-f256': [(5, 0, 256, 65536), (7, 0, 256, 256), (8, 8, 2048, 65536)],
    'unpack-files-cus256-n257-f257': [(5, 0, 2, 257), (7, 0, 256, 257), (8, 64, 65, 257)],
    'unpack-files-cus256-n65536-f257': [(5, 0, 256, 65536), (7, 0, 256, 257), (8, 8, 2048, 65536)],
    'scan-cus256-n1-m1-front0': [(9, 1024, 1, 1), (10, 0, 1, 1), (11, 0, 1, 1)],
    'scan-cus256-n1-m1-front64': [(9, 64, 1, 1), (10, 0, 1, 1), (11, 0, 1, 1)],
    'scan-cus256-n1-m1-front1024': [(9, 1024, 1, 1), (10, 0, 1, 1), (11, 0, 1, 1)],
    'fill-cus256-n1-m1-mtu21': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 1, 1), (4, 64, 1, 1)],
    'fill-cus256-n1-m1-mtu1024': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 1, 1), (4, 64, 1, 1)],
    'fill-cus256-n1-m1-mtu16396': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 1, 1), (4, 64, 1, 1)],
    'fill-cus256-n1-m1-mtu65547': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 1, 1), (4, 64, 1, 1)],
    'scan-cus256-n1-m513-front0': [(9, 1024, 1, 1), (10, 0, 1, 1), (11, 0, 3, 513)],
    'scan-cus256-n1-m513-front64': [(9, 64, 1, 1), (10, 0, 1, 1), (11, 0, 3, 513)],
    'scan-cus256-n1-m513-front1024': [(9, 1024, 1, 1), (10, 0, 1, 1), (11, 0, 3, 513)],
    'fill-cus256-n1-m513-mtu21': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 3, 513), (4, 64, 33, 513)],
    'fill-cus256-n1-m513-mtu1024': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 3, 513), (4, 64, 33, 513)],
    'fill-cus256-n1-m513-mtu16396': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 3, 513), (4, 64, 33, 513)],
    'fill-cus256-n1-m513-mtu65547': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 3, 513), (4, 64, 33, 513)],
    'scan-cus256-n256-m1-front0': [(9, 1024, 256, 256), (10, 0, 1, 256), (11, 0, 1, 256)],
    'scan-cus256-n256-m1-front64': [(9, 64, 64, 256), (10, 0, 1, 256), (11, 0, 1, 256)],
    'scan-cus256-n256-m1-front1024': [(9, 1024, 256, 256), (10, 0, 1, 256), (11, 0, 1, 256)],
    'fill-cus256-n256-m1-mtu21': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 1, 256), (4, 64, 16, 256)],
    'fill-cus256-n256-m1-mtu1024': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 1, 256), (4, 64, 16, 256)],
    'fill-cus256-n256-m1-mtu16396': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 1, 256), (4, 64, 16, 256)],
    'fill-cus256-n256-m1-mtu65547': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 1, 256), (4, 64, 16, 256)],
    'scan-cus256-n256-m513-front0': [(9, 1024, 256, 256), (10, 0, 1, 256), (11, 0, 513, 131328)],
    'scan-cus256-n256-m513-front64': [(9, 64, 64, 256), (10, 0, 1, 256), (11, 0, 513, 131328)],
    'scan-cus256-n256-m513-front1024': [(9, 1024, 256, 256), (10, 0, 1, 256), (11, 0, 513, 131328)],
    'fill-cus256-n256-m513-mtu21': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 513, 131328), (4, 2, 256, 131328)],
    'fill-cus256-n256-m513-mtu1024': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 513, 131328), (4, 2, 256, 131328)],
    'fill-cus256-n256-m513-mtu16396': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 513, 131328), (4, 8, 256, 131328)],
    'fill-cus256-n256-m513-mtu65547': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 513, 131328), (4, 16, 256, 131328)],
    'scan-cus256-n257-m1-front0': [(9, 64, 65, 257), (10, 0, 1, 257), (11, 0, 2, 257)],
    'scan-cus256-n257-m1-front64': [(9, 64, 65, 257), (10, 0, 1, 257), (11, 0, 2, 257)],
    'scan-cus256-n257-m1-front1024': [(9, 1024, 257, 257), (10, 0, 1, 257), (11, 0, 2, 257)],
    'fill-cus256-n257-m1-mtu21': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 2, 257), (4, 64, 17, 257)],
    'fill-cus256-n257-m1-mtu1024': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 2, 257), (4, 64, 17, 257)],
    'fill-cus256-n257-m1-mtu16396': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 2, 257), (4, 64, 17, 257)],
    'fill-cus256-n257-m1-mtu65547': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 2, 257), (4, 64, 17, 257)],
    'scan-cus256-n257-m513-front0': [(9, 64, 65, 257), (10, 0, 1, 257), (11, 0, 516, 131841)],
    'scan-cus256-n257-m513-front64': [(9, 64, 65, 257), (10, 0, 1, 257), (11, 0, 516, 131841)],
    'scan-cus256-n257-m513-front1024': [(9, 1024, 257, 257), (10, 0, 1, 257), (11, 0, 516, 131841)],
    'fill-cus256-n257-m513-mtu21': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 516, 131841), (4, 2, 256, 131841)],
    'fill-cus256-n257-m513-mtu1024': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 516, 131841), (4, 2, 256, 131841)],
    'fill-cus256-n257-m513-mtu16396': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 516, 131841), (4, 8, 256, 131841)],
    'fill-cus256-n257-m513-mtu65547': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 516, 131841), (4, 16, 256, 131841)],
    'scan-cus256-n100000-m1-front0': [(9, 64, 2048, 100000), (10, 0, 1, 100000), (11, 0, 391, 100000)],
    'scan-cus256-n100000-m1-front64': [(9, 64, 2048, 100000), (10, 0, 1, 100000), (11, 0, 391, 100000)],
    'scan-cus256-n100000-m1-front1024': [(9, 1024, 512, 100000), (10, 0, 1, 100000), (11, 0, 391, 100000)],
    'fill-cus256-n100000-m1-mtu21': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 391, 100000), (4, 2, 196, 100000)],
    'fill-cus256-n100000-m1-mtu1024': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 391, 100000), (4, 2, 196, 100000)],
    'fill-cus256-n100000-m1-mtu16396': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 391, 100000), (4, 8, 256, 100000)],
    'fill-cus256-n100000-m1-mtu65547': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 391, 100000), (4, 16, 256, 100000)],
    'scan-cus256-n100000-m513-front0': [(9, 64, 2048, 100000), (10, 0, 1, 100000), (11, 0, 2048, 51300000)],
    'scan-cus256-n100000-m513-front64': [(9, 64, 2048, 100000), (10, 0, 1, 100000), (11, 0, 2048, 51300000)],
    'scan-cus256-n100000-m513-front1024': [(9, 1024, 512, 100000), (10, 0, 1, 100000), (11, 0, 2048, 51300000)],
    'fill-cus256-n100000-m513-mtu21': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 2048, 51300000), (4, 2, 256, 51300000)],
    'fill-cus256-n100000-m513-mtu1024': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 2048, 51300000), (4, 2, 256, 51300000)],
    'fill-cus256-n100000-m513-mtu16396': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 2048, 51300000), (4, 8, 256, 51300000)],
    'fill-cus256-n100000-m513-mtu65547': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 2048, 51300000), (4, 16, 256, 51300000)],
    'fill-cus256-slots524032': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 2047, 524032), (4, 2, 256, 524032)],
    'fill-cus256-slots524288': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 2048, 524288), (4, 2, 256, 524288)],
    'fill-cus256-slots524289': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 2048, 524289), (4, 2, 256, 524289)],
    'pack-cus8-n1-h0': [(4, 64, 1, 1)],
    'pack-cus8-n1-h600': [(4, 64, 1, 1)],
    'pack-cus8-n1-h1100': [(4, 64, 1, 1)],
    'pack-cus8-n1-h16400': [(4, 64, 1, 1)],
    'pack-cus8-n1-h65532': [(4, 64, 1, 1)],
    'pack-cus8-n1-g1': [(4, 1, 1, 1)],
    'pack-cus8-n1-g64': [(4, 64, 1, 1)],
    'pack-cus8-n63-h0': [(4, 64, 4, 63)],
    'pack-cus8-n63-h600': [(4, 64, 4, 63)],
    'pack-cus8-n63-h1100': [(4, 64, 4, 63)],
    'pack-cus8-n63-h16400': [(4, 64, 4, 63)],
    'pack-cus8-n63-h65532': [(4, 64, 4, 63)],
    'pack-cus8-n63-g1': [(4, 1, 1, 63)],
    'pack-cus8-n63-g64': [(4, 64, 4, 63)],
    'pack-cus8-n64-h0': [(4, 64, 4, 64)],
    'pack-cus8-n64-h600': [(4, 64, 4, 64)],
    'pack-cus8-n64-h1100': [(4, 64, 4, 64)],
    'pack-cus8-n64-h16400': [(4, 64, 4, 64)],
    'pack-cus8-n64-h65532': [(4, 64, 4, 64)],
    'pack-cus8-n64-g1': [(4, 1, 1, 64)],
    'pack-cus8-n64-g64': [(4, 64, 4, 64)],
    'pack-cus8-n4096-h0': [(4, 4, 8, 4096)],
    'pack-cus8-n4096-h600': [(4, 2, 8, 4096)],
    'pack-cus8-n4096-h1100': [(4, 4, 8, 4096)],
    'pack-cus8-n4096-h16400': [(4, 8, 8, 4096)],
    'pack-cus8-n4096-h65532': [(4, 16, 8, 4096)],
    'pack-cus8-n4096-g1': [(4, 1, 4, 4096)],
    'pack-cus8-n4096-g64': [(4, 64, 8, 4096)],
    'pack-cus8-n65535-h0': [(4, 4, 8, 65535)],
    'pack-cus8-n65535-h600': [(4, 2, 8, 65535)],
    'pack-cus8-n65535-h1100': [(4, 4, 8, 65535)],
    'pack-cus8-n65535-h16400': [(4, 8, 8, 65535)],
    'pack-cus8-n65535-h65532': [(4, 16, 8, 65535)],
    'pack-cus8-n65535-g1': [(4, 1, 8, 65535)],
    'pack-cus8-n65535-g64': [(4, 64, 8, 65535)],
    'pack-cus8-n65536-h0': [(4, 4, 8, 65536)],
    'pack-cus8-n65536-h600': [(4, 2, 8, 65536)],
    'pack-cus8-n65536-h1100': [(4, 4, 8, 65536)],
    'pack-cus8-n65536-h16400': [(4, 8, 8, 65536)],
    'pack-cus8-n65536-h65532': [(4, 16, 8, 65536)],
    'pack-cus8-n65536-g1': [(4, 1, 8, 65536)],
    'pack-cus8-n65536-g64': [(4, 64, 8, 65536)],
    'pack-cus8-n1048576-h0': [(4, 4, 8, 1048576)],
    'pack-cus8-n1048576-h600': [(4, 2, 8, 1048576)],
    'pack-cus8-n1048576-h1100': [(4, 4, 8, 1048576)],
    'pack-cus8-n1048576-h16400': [(4, 8, 8, 1048576)],
    'pack-cus8-n1048576-h65532': [(4, 16, 8, 1048576)],
    'pack-cus8-n1048576-g1': [(4, 1, 8, 1048576)],
    'pack-cus8-n1048576-g64': [(4, 64, 8, 1048576)],
    'unpack-cus8-n1-h0': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus8-n1-h600': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus8-n1-h1100': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus8-n1-h16400': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus8-n1-h65532': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus8-n1-g1': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 1, 1, 1)],
    'unpack-cus8-n1-g64': [(5, 0, 1, 1), (6, 0, 1, 1), (8, 64, 1, 1)],
    'unpack-cus8-n63-h0': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus8-n63-h600': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus8-n63-h1100': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus8-n63-h16400': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus8-n63-h65532': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus8-n63-g1': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 1, 1, 63)],
    'unpack-cus8-n63-g64': [(5, 0, 1, 63), (6, 0, 1, 63), (8, 64, 16, 63)],
    'unpack-cus8-n64-h0': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus8-n64-h600': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus8-n64-h1100': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus8-n64-h16400': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus8-n64-h65532': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus8-n64-g1': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 1, 1, 64)],
    'unpack-cus8-n64-g64': [(5, 0, 1, 64), (6, 0, 1, 64), (8, 64, 16, 64)],
    'unpack-cus8-n4096-h0': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 4, 64, 4096)],
    'unpack-cus8-n4096-h600': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 4, 64, 4096)],
    'unpack-cus8-n4096-h1100': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 4, 64, 4096)],
    'unpack-cus8-n4096-h16400': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 8, 64, 4096)],
    'unpack-cus8-n4096-h65532': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 16, 64, 4096)],
    'unpack-cus8-n4096-g1': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 1, 16, 4096)],
    'unpack-cus8-n4096-g64': [(5, 0, 16, 4096), (6, 0, 1, 4096), (8, 64, 64, 4096)],
    'unpack-cus8-n65535-h0': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 4, 64, 65535)],
    'unpack-cus8-n65535-h600': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 2, 64, 65535)],
    'unpack-cus8-n65535-h1100': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 4, 64, 65535)],
    'unpack-cus8-n65535-h16400': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 8, 64, 65535)],
    'unpack-cus8-n65535-h65532': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 16, 64, 65535)],
    'unpack-cus8-n65535-g1': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 1, 64, 65535)],
    'unpack-cus8-n65535-g64': [(5, 0, 256, 65535), (6, 0, 1, 65535), (8, 64, 64, 65535)],
    'unpack-cus8-n65536-h0': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 4, 64, 65536)],
    'unpack-cus8-n65536-h600': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 2, 64, 65536)],
    'unpack-cus8-n65536-h1100': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 4, 64, 65536)],
    'unpack-cus8-n65536-h16400': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 8, 64, 65536)],
    'unpack-cus8-n65536-h65532': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 16, 64, 65536)],
    'unpack-cus8-n65536-g1': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 1, 64, 65536)],
    'unpack-cus8-n65536-g64': [(5, 0, 256, 65536), (6, 0, 1, 65536), (8, 64, 64, 65536)],
    'unpack-cus8-n1048576-h0': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 4, 64, 1048576)],
    'unpack-cus8-n1048576-h600': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 2, 64, 1048576)],
    'unpack-cus8-n1048576-h1100': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 4, 64, 1048576)],
    'unpack-cus8-n1048576-h16400': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 8, 64, 1048576)],
    'unpack-cus8-n1048576-h65532': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 16, 64, 1048576)],
    'unpack-cus8-n1048576-g1': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 1, 64, 1048576)],
    'unpack-cus8-n1048576-g64': [(5, 0, 4096, 1048576), (6, 0, 1, 1048576), (8, 64, 64, 1048576)],
    'unpack-files-cus8-n257-f1': [(5, 0, 2, 257), (7, 0, 1, 1), (8, 32, 33, 257)],
    'unpack-files-cus8-n65536-f1': [(5, 0, 256, 65536), (7, 0, 1, 1), (8, 4, 64, 65536)],
    'unpack-files-cus8-n257-f255': [(5, 0, 2, 257), (7, 0, 8, 255), (8, 32, 33, 257)],
    'unpack-files-cus8-n65536-f255': [(5, 0, 256, 65536), (7, 0, 8, 255), (8, 4, 64, 65536)],
    'unpack-files-cus8-n257-f256': [(5, 0, 2, 257), (7, 0, 8, 256), (8, 32, 33, 257)],
    'unpack-files-cus8-n65536-f256': [(5, 0, 256, 65536), (7, 0, 8, 256), (8, 4, 64, 65536)],
    'unpack-files-cus8-n257-f257': [(5, 0, 2, 257), (7, 0, 8, 257), (8, 32, 33, 257)],
    'unpack-files-cus8-n65536-f257': [(5, 0, 256, 65536), (7, 0, 8, 257), (8, 4, 64, 65536)],
    'scan-cus8-n1-m1-front0': [(9, 1024, 1, 1), (10, 0, 1, 1), (11, 0, 1, 1)],
    'scan-cus8-n1-m1-front64': [(9, 64, 1, 1), (10, 0, 1, 1), (11, 0, 1, 1)],
    'scan-cus8-n1-m1-front1024': [(9, 1024, 1, 1), (10, 0, 1, 1), (11, 0, 1, 1)],
    'fill-cus8-n1-m1-mtu21': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 1, 1), (4, 64, 1, 1)],
    'fill-cus8-n1-m1-mtu1024': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 1, 1), (4, 64, 1, 1)],
    'fill-cus8-n1-m1-mtu16396': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 1, 1), (4, 64, 1, 1)],
    'fill-cus8-n1-m1-mtu65547': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 1, 1), (4, 64, 1, 1)],
    'scan-cus8-n1-m513-front0': [(9, 1024, 1, 1), (10, 0, 1, 1), (11, 0, 3, 513)],
    'scan-cus8-n1-m513-front64': [(9, 64, 1, 1), (10, 0, 1, 1), (11, 0, 3, 513)],
    'scan-cus8-n1-m513-front1024': [(9, 1024, 1, 1), (10, 0, 1, 1), (11, 0, 3, 513)],
    'fill-cus8-n1-m513-mtu21': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 3, 513), (4, 8, 5, 513)],
    'fill-cus8-n1-m513-mtu1024': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 3, 513), (4, 8, 5, 513)],
    'fill-cus8-n1-m513-mtu16396': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 3, 513), (4, 8, 5, 513)],
    'fill-cus8-n1-m513-mtu65547': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 3, 513), (4, 16, 8, 513)],
    'scan-cus8-n256-m1-front0': [(9, 64, 64, 256), (10, 0, 1, 256), (11, 0, 1, 256)],
    'scan-cus8-n256-m1-front64': [(9, 64, 64, 256), (10, 0, 1, 256), (11, 0, 1, 256)],
    'scan-cus8-n256-m1-front1024': [(9, 1024, 16, 256), (10, 0, 1, 256), (11, 0, 1, 256)],
    'fill-cus8-n256-m1-mtu21': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 1, 256), (4, 32, 8, 256)],
    'fill-cus8-n256-m1-mtu1024': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 1, 256), (4, 32, 8, 256)],
    'fill-cus8-n256-m1-mtu16396': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 1, 256), (4, 32, 8, 256)],
    'fill-cus8-n256-m1-mtu65547': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 1, 256), (4, 32, 8, 256)],
    'scan-cus8-n256-m513-front0': [(9, 64, 64, 256), (10, 0, 1, 256), (11, 0, 64, 131328)],
    'scan-cus8-n256-m513-front64': [(9, 64, 64, 256), (10, 0, 1, 256), (11, 0, 64, 131328)],
    'scan-cus8-n256-m513-front1024': [(9, 1024, 16, 256), (10, 0, 1, 256), (11, 0, 64, 131328)],
    'fill-cus8-n256-m513-mtu21': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 64, 131328), (4, 2, 8, 131328)],
    'fill-cus8-n256-m513-mtu1024': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 64, 131328), (4, 2, 8, 131328)],
    'fill-cus8-n256-m513-mtu16396': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 64, 131328), (4, 8, 8, 131328)],
    'fill-cus8-n256-m513-mtu65547': [(12, 0, 1, 256), (10, 0, 1, 256), (13, 0, 64, 131328), (4, 16, 8, 131328)],
    'scan-cus8-n257-m1-front0': [(9, 64, 64, 257), (10, 0, 1, 257), (11, 0, 2, 257)],
    'scan-cus8-n257-m1-front64': [(9, 64, 64, 257), (10, 0, 1, 257), (11, 0, 2, 257)],
    'scan-cus8-n257-m1-front1024': [(9, 1024, 16, 257), (10, 0, 1, 257), (11, 0, 2, 257)],
    'fill-cus8-n257-m1-mtu21': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 2, 257), (4, 16, 5, 257)],
    'fill-cus8-n257-m1-mtu1024': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 2, 257), (4, 16, 5, 257)],
    'fill-cus8-n257-m1-mtu16396': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 2, 257), (4, 16, 5, 257)],
    'fill-cus8-n257-m1-mtu65547': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 2, 257), (4, 16, 5, 257)],
    'scan-cus8-n257-m513-front0': [(9, 64, 64, 257), (10, 0, 1, 257), (11, 0, 64, 131841)],
    'scan-cus8-n257-m513-front64': [(9, 64, 64, 257), (10, 0, 1, 257), (11, 0, 64, 131841)],
    'scan-cus8-n257-m513-front1024': [(9, 1024, 16, 257), (10, 0, 1, 257), (11, 0, 64, 131841)],
    'fill-cus8-n257-m513-mtu21': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 64, 131841), (4, 2, 8, 131841)],
    'fill-cus8-n257-m513-mtu1024': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 64, 131841), (4, 2, 8, 131841)],
    'fill-cus8-n257-m513-mtu16396': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 64, 131841), (4, 8, 8, 131841)],
    'fill-cus8-n257-m513-mtu65547': [(12, 0, 2, 257), (10, 0, 1, 257), (13, 0, 64, 131841), (4, 16, 8, 131841)],
    'scan-cus8-n100000-m1-front0': [(9, 64, 64, 100000), (10, 0, 1, 100000), (11, 0, 64, 100000)],
    'scan-cus8-n100000-m1-front64': [(9, 64, 64, 100000), (10, 0, 1, 100000), (11, 0, 64, 100000)],
    'scan-cus8-n100000-m1-front1024': [(9, 1024, 16, 100000), (10, 0, 1, 100000), (11, 0, 64, 100000)],
    'fill-cus8-n100000-m1-mtu21': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 64, 100000), (4, 2, 8, 100000)],
    'fill-cus8-n100000-m1-mtu1024': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 64, 100000), (4, 2, 8, 100000)],
    'fill-cus8-n100000-m1-mtu16396': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 64, 100000), (4, 8, 8, 100000)],
    'fill-cus8-n100000-m1-mtu65547': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 64, 100000), (4, 16, 8, 100000)],
    'scan-cus8-n100000-m513-front0': [(9, 64, 64, 100000), (10, 0, 1, 100000), (11, 0, 64, 51300000)],
    'scan-cus8-n100000-m513-front64': [(9, 64, 64, 100000), (10, 0, 1, 100000), (11, 0, 64, 51300000)],
    'scan-cus8-n100000-m513-front1024': [(9, 1024, 16, 100000), (10, 0, 1, 100000), (11, 0, 64, 51300000)],
    'fill-cus8-n100000-m513-mtu21': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 64, 51300000), (4, 2, 8, 51300000)],
    'fill-cus8-n100000-m513-mtu1024': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 64, 51300000), (4, 2, 8, 51300000)],
    'fill-cus8-n100000-m513-mtu16396': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 64, 51300000), (4, 8, 8, 51300000)],
    'fill-cus8-n100000-m513-mtu65547': [(12, 0, 391, 100000), (10, 0, 1, 100000), (13, 0, 64, 51300000), (4, 16, 8, 51300000)],
    'fill-cus8-slots16128': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 63, 16128), (4, 2, 8, 16128)],
    'fill-cus8-slots16384': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 64, 16384), (4, 2, 8, 16384)],
    'fill-cus8-slots16385': [(12, 0, 1, 1), (10, 0, 1, 1), (13, 0, 64, 16385), (4, 2, 8, 16385)],
    'pack-n0': [],
    'unpack-files-f0': [],
    'scan-m0': [],
    'fill-n0': [],
    'fill-slots-overflow': [],
    'unknown-call': [],
}


@pytest.fixture()
def window_knobs():
    """Sets the knobs the window plans honour for one case and restores them."""
    def set_(lanes=0, front=0):
        vc.set_lanes_per_frame(lanes)
        vc.set_scan_front(front)

    yield set_
    set_()


def test_window_table_is_complete():
    ids = [cid for cid, _, _ in W_CASES]
    assert len(set(ids)) == len(ids)
    assert set(ids) == set(W_EXPECTED)
    assert all(W_EXPECTED[k] == v for k, v in W_HAND.items())


@pytest.mark.parametrize("cid,args,kn", W_CASES, ids=[c[0] for c in W_CASES])
def test_window_plan(window_knobs, cid, args, kn):
    window_knobs(**kn)
    got = vc.plan_window(args["call"], args["cus"], args["n"], groups=args["groups"], max_frames=args["max_frames"],
                         len_hint=args["len_hint"])
    assert [(l.kernel, l.lanes, l.grid, l.count) for l in got] == W_EXPECTED[cid], (args, kn)
    # a window launch sets nothing else
    assert all((l.depth, l.first) + l.astuple()[6:] == (0,) * 8 for l in got)


def test_defaults_are_what_the_table_assumes():
    """The table is pinned with the dynamic tail and the split kernel enabled
    (VAL_GPU_DYNAMIC_TAIL / VAL_GPU_SPLIT unset) and the default ragged minimum."""
    assert vc.lib().val_gpu_ragged_min_frames() == 4096
    assert vc.lanes_per_frame(16400) == 8
