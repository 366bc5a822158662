"""Shapes of the k_frames_split tests (tests/test_gpu_split.py,
tests/test_gpu_split_edges.py) as plain functions of the CU count, with the
plan each of them must get (val_gpu_plan_frames through vc.plan_frames). No
GPU and no torch here: tests/test_launch_plan.py calls the same functions for
64, 128, 256 and 304 CUs, so a threshold that moves in launch_plan.hpp fails a
test there instead of moving a GPU case onto another kernel unnoticed.

A batch is (lens uint32, offs uint64, total bytes). Frame bytes come from the
GPU tests; nothing here depends on them."""
from __future__ import annotations

import contextlib
import os

import numpy as np

MiB = 1 << 20
LEAD = 5  # bytes in front of the first descriptor frame: any trailer position minus 4 stays inside the buffer


def k0_for(length: int) -> int:
    """log2 of the chunk bytes W: the least W >= 1 KiB with the frame in at most 16 chunks."""
    k0 = 10
    while (16 << k0) < length:
        k0 += 1
    return k0


def chunks(length, k0: int):
    """Chunks of W = 2^k0 bytes of a frame (an empty frame is one empty chunk), scalar or array."""
    return np.maximum(1, (np.asarray(length, dtype=np.int64) + (1 << k0) - 1) >> k0)


def groups(length, k0: int):
    return (chunks(length, k0) + 15) // 16


def rule_says_split(cus: int, n: int, length: int) -> bool:
    """DESIGN 4.4's rule restated (default knobs, no payload states): at most half a wave-round of
    frames of at least 8 KiB, and three round-times per pass of the grid against the rounds of one
    wave per frame."""
    if length < 8192 or 2 * n > 16 * cus:
        return False
    return -(-n // cus) * 3 <= (length // 64 + 1 + 63) // 64


def max_split_frames(cus: int, length: int) -> int:
    """The most frames of `length` bytes the rule sends to split in one call."""
    return min(8 * cus, ((length // 64 + 1 + 63) // 64 // 3) * cus)


@contextlib.contextmanager
def tail_pieces_off(vc):
    """The in-launch tail pieces off (the tail becomes a second launch), restored on the way out."""
    vc.lib().val_gpu_set_tail_pieces(0)
    try:
        yield
    finally:
        vc.lib().val_gpu_set_tail_pieces(-1)


# ---- 0. the plan assertion every case makes -------------------------------------------------
def split_plan(vc, cus: int, n: int, typical_len: int, *, descriptors: bool = False, k0: int):
    """The plan of one call that must be a single k_frames_split launch over all n frames."""
    plan = vc.plan_frames(cus, n, typical_len, descriptors=descriptors, flen=0 if descriptors else typical_len)
    rows = [l.astuple() for l in plan]
    assert len(plan) == 1, rows
    assert plan[0].kernel == vc.KERNEL_SPLIT, rows
    assert (plan[0].first, plan[0].count) == (0, n), rows
    assert plan[0].k0 == k0, rows
    assert plan[0].grid == min(n, cus), rows
    return plan


def not_split_plan(vc, cus: int, n: int, typical_len: int, *, descriptors: bool = False):
    plan = vc.plan_frames(cus, n, typical_len, descriptors=descriptors, flen=0 if descriptors else typical_len)
    assert plan and all(l.kernel != vc.KERNEL_SPLIT for l in plan), [l.astuple() for l in plan]
    return plan


def second_launch_plan(vc, cus: int, n_main: int, tail: int, typical_len: int, *, descriptors: bool = False, k0: int):
    """With the tail pieces off: the full rounds, then k_frames_split over the tail. The caller holds
    tail_pieces_off()."""
    plan = vc.plan_frames(cus, n_main + tail, typical_len, descriptors=descriptors,
                          flen=0 if descriptors else typical_len)
    rows = [l.astuple() for l in plan]
    assert len(plan) == 2, rows
    assert plan[0].kernel in (vc.KERNEL_FRAMES, vc.KERNEL_FRAMES_C0) and plan[0].tail_n == 0, rows
    assert (plan[0].first, plan[0].count) == (0, n_main), rows
    assert plan[1].kernel == vc.KERNEL_SPLIT, rows
    assert plan[1].first == plan[0].count and plan[1].count == tail, rows
    assert plan[1].k0 == k0 and plan[1].grid == min(tail, cus), rows
    return plan


def layout(lens, gaps, first: int = LEAD):
    """Frames one after the other: frame i's bytes, its 4 trailer bytes, gaps[i] - 4 spare bytes."""
    wire = np.asarray(lens, dtype=np.int64) + np.asarray(gaps, dtype=np.int64)
    offs = first + np.concatenate([[0], np.cumsum(wire)[:-1]])
    return offs.astype(np.uint64), int(offs[-1] + wire[-1]) + 8


# tests/test_gpu_split.py's strided cases, payload -> k0: flen = 16 + payload <= 16 << k0
STRIDED_K0 = {8192: 10, 16384: 11, 65516: 12, 8176: 10, 65520: 12}


# ---- 1. later trips of the grid loop --------------------------------------------------------
TRIPS_FLEN, TRIPS_K0 = 32784, 12  # 16 << 11 = 32,768 < 32,784; 9 rounds at one wave per frame = 3 passes x 3


def trips_n(cus: int) -> int:
    return 2 * cus + 3


def trips_plan(vc, cus: int, descriptors: bool):
    n = trips_n(cus)
    plan = split_plan(vc, cus, n, TRIPS_FLEN, descriptors=descriptors, k0=TRIPS_K0)
    assert plan[0].grid == cus < n and -(-n // plan[0].grid) == 3
    return n, plan


def trips_descriptors(cus: int):
    """2 CUs + 3 frames under the hint 32,784 (W = 4 KiB). In memory the lengths cycle through 0, 1,
    7, 16 W, 16 W + 1, 48 W + 3 and a random one up to 5 hints, at gaps of 4-7 bytes; the
    descriptors list them in a seeded permutation, so the frames a workgroup takes in its trips
    (f, f + CUs, f + 2 CUs) are unrelated, and workgroup 0 takes a four-group frame, a one-byte frame
    and a four-group frame again."""
    n, W = trips_n(cus), 1 << TRIPS_K0
    rng = np.random.default_rng(0x7B1B5 + cus)
    cycle = (0, 1, 7, 16 * W, 16 * W + 1, 48 * W + 3, None)
    mem_lens = np.array([cycle[i % 7] if cycle[i % 7] is not None else int(rng.integers(0, 5 * TRIPS_FLEN + 1))
                         for i in range(n)], dtype=np.uint32)
    mem_offs, total = layout(mem_lens, rng.integers(4, 8, n))
    perm = rng.permutation(n)
    for want_at, length in ((0, 48 * W + 3), (cus, 1), (2 * cus, 48 * W + 3)):
        have = int(np.nonzero((mem_lens[perm] == length) & (np.arange(n) % cus != 0))[0][0])
        perm[[want_at, have]] = perm[[have, want_at]]
    lens, offs = mem_lens[perm], mem_offs[perm]
    assert set(int(o) % 4 for o in offs) == {0, 1, 2, 3}
    g, c = groups(lens, TRIPS_K0), chunks(lens, TRIPS_K0)
    assert (g[0], c[cus], g[2 * cus]) == (4, 1, 4)  # one workgroup: four groups, one chunk, four groups
    assert not np.array_equal(np.sort(offs), offs)
    return lens, offs, total


BAD_FIRST, BAD_LAST_CHUNK, BAD_TRAILER0, BAD_FIRST_GROUP = 0, 1, 2, 6  # kinds 2..5: trailer byte kind - 2


def bad_position(kind: int, length: int, k0: int) -> int:
    """Byte of the frame (its trailer included) that a corruption of this kind flips."""
    if kind == BAD_FIRST:
        return 0
    if kind == BAD_LAST_CHUNK:
        return length - 1 - min(length - 1, 100)
    if kind == BAD_FIRST_GROUP:  # the bytes in front of the last (groups - 1) x 16 chunks
        return (length - (int(groups(length, k0)) - 1) * (16 << k0)) // 2
    return length + kind - BAD_TRAILER0


def trips_bad(cus: int, lens):
    """About 5% of the frames, (frame, kind): at least one in each trip of the grid, every kind of
    placement, kind 6 in the four-group frame of the third trip."""
    n = trips_n(cus)
    rng = np.random.default_rng(0xBAD + cus)
    want = max(9, round(0.05 * n))
    bad = [(2 * cus, BAD_FIRST_GROUP)]
    for f in rng.permutation(n):
        kind, L = len(bad) % 7, int(lens[f])
        if len(bad) == want:
            break
        if f == 2 * cus or (kind in (BAD_FIRST, BAD_LAST_CHUNK) and L == 0) or \
                (kind == BAD_FIRST_GROUP and L <= 16 << TRIPS_K0):
            continue
        bad.append((int(f), kind))
    assert len(bad) == want and len(set(f for f, _ in bad)) == want
    assert set(f // cus for f, _ in bad) == {0, 1, 2}, "a bad frame in every trip"
    assert set(k for _, k in bad) == set(range(7)), "every placement"
    return bad


# ---- 2. the k0 ladder and the chunk edges ---------------------------------------------------
# strided flen -> k0, each side of 16 << k0 < flen
LADDER = ((16384, 10), (16385, 11), (65536, 12), (65537, 13), (131072 + 5, 14), (1 << 20, 16), ((1 << 20) + 1, 17),
          ((1 << 24) - 1, 20), ((1 << 24) + 1, 21))
LADDER_N = 3


def ladder_plan(vc, cus: int, i: int):
    flen, k0 = LADDER[i]
    split_plan(vc, cus, LADDER_N, flen, k0=k0)
    return flen, flen + 4 + i % 4


EDGE_HINTS = ((8192, 10), (100_000, 13))
EDGE_M, EDGE_R = (0, 1, 15, 16, 17, 31, 32, 33, 48), (0, 1, 3, 4, 63, 64, 65, -1)  # -1: W - 1


def edge_descriptors(k0: int):
    """L = m W + r for every m and r above (m = 16, r = 1: a first group of one one-byte chunk and 15
    padded waves), each length starting at addresses 0..3 mod 4."""
    W = 1 << k0
    lens, offs, pos = [], [], LEAD
    for m in EDGE_M:
        for r in EDGE_R:
            for phase in range(4):
                L = m * W + (W - 1 if r < 0 else r)
                pos += (phase - pos) % 4
                lens.append(L)
                offs.append(pos)
                pos += L + 4
    assert (16 * W + 1) in lens
    return np.array(lens, np.uint32), np.array(offs, np.uint64), pos + 8


def edge_calls(vc, cus: int, hint: int, k0: int):
    """The 288 frames as calls that each plan as split: one where the rule admits them all, else
    (hint 8,192 admits one trip only) slices of at most a grid."""
    lens, _, _ = edge_descriptors(k0)
    per = min(lens.size, max_split_frames(cus, hint))
    calls = [(a, min(a + per, lens.size)) for a in range(0, lens.size, per)]
    for a, b in calls:
        split_plan(vc, cus, b - a, hint, descriptors=True, k0=k0)
    return calls


BIG_LEN, BIG_K0, BIG_OFF = (1 << 28) + 5, 24, 3  # hint 2^28: two groups, the first of one 5-byte chunk


def big_plan(vc, cus: int):
    split_plan(vc, cus, 1, 1 << 28, descriptors=True, k0=BIG_K0)
    assert int(groups(BIG_LEN, BIG_K0)) == 2 and int(chunks(BIG_LEN, BIG_K0)) == 17


# ---- 3. split as the second launch ----------------------------------------------------------
TAIL_FLEN, TAIL_K0 = 65532, 12


def tail_main(cus: int) -> int:
    return cus * 16 * 4  # one wave-round at 16 lanes: 4 frames per wave


def tail_counts(cus: int):
    return (6, cus + 5)  # one trip of the split grid, and two


def tail_plan(vc, cus: int, tail: int, descriptors: bool):
    """Call under tail_pieces_off()."""
    plan = second_launch_plan(vc, cus, tail_main(cus), tail, TAIL_FLEN, descriptors=descriptors, k0=TAIL_K0)
    assert rule_says_split(cus, tail, TAIL_FLEN)
    return tail_main(cus) + tail, plan


def tail_descriptors(cus: int, tail: int):
    """Full frames under the hint, with a 7-byte, an empty, a two-group and the file's 816-byte last
    frame among the tail frames."""
    n = tail_main(cus) + tail
    rng = np.random.default_rng(tail)
    lens = np.full(n, TAIL_FLEN, np.uint32)
    lens[n - tail], lens[-3], lens[-2], lens[-1] = 7, 0, TAIL_FLEN + 5000, 816
    offs, total = layout(lens, rng.integers(4, 8, n), first=LEAD + 2)
    return lens, offs, total


def tail_bad(cus: int, tail: int):
    """Two corrupted frames in the main part, three in the tail (its first and last frame among them)."""
    n_main = tail_main(cus)
    return [n_main // 3, n_main - 1, n_main, n_main + tail // 2, n_main + tail - 1]


# ---- 4. the seeded fuzz ---------------------------------------------------------------------
FUZZ_DEFAULT_SEED, FUZZ_DEFAULT_ROUNDS = 20261021, 60
FUZZ_CAP = 64 * MiB
FUZZ_MIN, FUZZ_MAX = 8192, 1 << 21


def fuzz_seed() -> int:
    return int(os.environ.get("FUZZ_SEED", str(FUZZ_DEFAULT_SEED)))


def fuzz_round_count() -> int:
    return int(os.environ.get("FUZZ_SPLIT_ROUNDS", str(FUZZ_DEFAULT_ROUNDS)))


def _fuzz_len(rng, lo_exp: int, hi_exp: int) -> int:
    """A hint or flen: a power of two 2^lo_exp..2^hi_exp minus one, itself or plus one (7 draws in 10),
    else log-uniform in that range; within 8,192 .. 2^21."""
    e = int(rng.integers(lo_exp, hi_exp + 1))
    u = rng.random()
    v = (1 << e) + (-1 if u < 0.25 else 0 if u < 0.45 else 1) if u < 0.7 else \
        int(2.0 ** rng.uniform(lo_exp, hi_exp))
    return min(max(v, FUZZ_MIN), FUZZ_MAX)


def fuzz_rounds(vc, cus: int, seed: int | None = None, rounds: int | None = None):
    """The rounds of the fuzz: dicts of descriptors (bool), n, typical (hint or flen), stride, lens,
    offs, total, verify (bool), bad [(frame, byte of the frame or its trailer, bit)], k0, trips. Every
    shape is drawn again until the planner says split, so every round runs on k_frames_split."""
    rng = np.random.default_rng(fuzz_seed() if seed is None else seed)
    out = []
    for _ in range(fuzz_round_count() if rounds is None else rounds):
        while True:
            descriptors = bool(rng.random() < 0.5)
            trips = int(rng.choice([1, 2, 3], p=[0.6, 0.2, 0.2]))
            # two trips need 6 rounds of one wave per frame (20 KiB), three need 9 (32 KiB); the byte cap
            # keeps the frames of two and three trips short
            typical = _fuzz_len(rng, *((13, 21), (15, 17), (15, 16))[trips - 1])
            n = int(rng.integers((trips - 1) * cus + 1, trips * cus + 1))
            if descriptors:
                lens = rng.integers(0, 4 * typical + 1, n).astype(np.uint32)
                if rng.random() < 0.5:
                    lens[int(rng.integers(0, n))] = 0
                gaps = rng.integers(4, 8, n)
                n = max(1, int(np.searchsorted(np.cumsum(lens.astype(np.int64) + gaps), FUZZ_CAP - 64)))
                lens, gaps = lens[:n], gaps[:n]
                offs, total = layout(lens, gaps, first=LEAD + int(rng.integers(0, 4)))
                stride = 0
            else:
                stride = typical + int(rng.integers(4, 8))
                n = max(1, min(n, (FUZZ_CAP - 64) // stride))
                lens = np.full(n, typical, np.uint32)
                offs, total = np.arange(n, dtype=np.uint64) * np.uint64(stride), n * stride + 8
            plan = vc.plan_frames(cus, n, typical, descriptors=descriptors, flen=0 if descriptors else typical)
            if len(plan) == 1 and plan[0].kernel == vc.KERNEL_SPLIT:
                break
        assert total <= FUZZ_CAP and plan[0].count == n and plan[0].k0 == k0_for(typical)
        verify = bool(rng.random() < 0.5)
        bad = []
        if verify and rng.random() < 0.7:
            for f in rng.choice(n, min(n, int(rng.integers(1, 5))), replace=False):
                bad.append((int(f), int(rng.integers(0, int(lens[f]) + 4)), int(rng.integers(0, 8))))
        out.append(dict(descriptors=descriptors, n=n, typical=typical, stride=stride, lens=lens, offs=offs, total=total,
                        verify=verify, bad=bad, k0=int(plan[0].k0), trips=-(-n // int(plan[0].grid))))
    return out


def fuzz_coverage(rounds) -> None:
    """What the default rounds must have included (asserted by the GPU test after its loop and, for
    64, 128, 256 and 304 CUs, by tests/test_launch_plan.py)."""
    assert set(range(10, 18)) <= set(r["k0"] for r in rounds), sorted(set(r["k0"] for r in rounds))
    assert set(r["trips"] for r in rounds) >= {1, 2, 3}
    assert any(r["descriptors"] and (r["lens"] == 0).any() for r in rounds), "a frame of 0 bytes"
    assert any((groups(r["lens"], r["k0"]) > 2).any() for r in rounds), "a frame of more than two groups"
    assert set(r["descriptors"] for r in rounds) == {False, True}
    assert any(r["verify"] and r["bad"] for r in rounds) and any(r["verify"] and not r["bad"] for r in rounds)
    assert any(not r["verify"] for r in rounds)
