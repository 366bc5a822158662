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


def test_defaults_are_what_the_table_assumes():
    """The table is pinned with the dynamic tail and the split kernel enabled
    (VAL_GPU_DYNAMIC_TAIL / VAL_GPU_SPLIT unset) and the default ragged minimum."""
    assert vc.lib().val_gpu_ragged_min_frames() == 4096
    assert vc.lanes_per_frame(16400) == 8
