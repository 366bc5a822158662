"""The ragged path's plan restated (csrc/crc_kernels.hpp
length_bucket, for_each_bucket, k_bin_scatter's class table, ragged_item,
k_frames_ragged; val_crc32_hip.hip launch_ragged; launch_plan.hpp ragged), and
the shapes of tests/test_gpu_ragged_edges.py and tests/test_gpu_ragged_fuzz.py
as plain functions of the CU count. No GPU and no torch here:
tests/test_launch_plan.py runs every shape function for 64, 128, 256 and 304
CUs, so a threshold that moves fails a test there instead of moving a GPU case
off its branch unnoticed.

A frame in the wrong bucket still gets the right CRC: every class's lanes hash
a frame of any length, a bucket only decides which frames share a wave. So the
bucket restatement here serves the reach assertions alone (which trip, which
wave, which item a frame is in). It is pinned to the table in the comment
above length_bucket, not to the device: the GPU tests compare CRCs with the
oracle and never with anything in this file."""
from __future__ import annotations

import contextlib
import itertools
import os

import numpy as np

MiB = 1 << 20
KERNEL_RAGGED = 0  # val_gpu_launch_t.kernel
LIMITS = (1024, 8192, 49152)  # class c holds LIMITS[c - 1] <= L < LIMITS[c]
LANES = (2, 4, 8, 16)
PER = tuple(64 // g for g in LANES)  # frames of one item
BUCKETS = 136
CLASS_FIRST_BUCKET = (0, 8, 37, 118, BUCKETS)
BIN_TRIP = 256 * 8  # kBinThreads x kBinBatch lengths per trip of for_each_bucket
QUEUE_PARTS, WAVES_PER_BLOCK = 64, 16
LEAD = 5  # bytes in front of the first packed frame


# ---- the restatement --------------------------------------------------------------------------
def bucket(L):
    """length_bucket: rounds of the frame's class, 0..7 | 8..36 | 37..117 | 118..134, longer 135."""
    L = np.asarray(L, dtype=np.int64)
    m = np.maximum(L - 1, 0)
    b = np.where(L < 1024, np.where(L <= 128, 0, m // 128),
                 np.where(L < 8192, 5 + m // 256,
                          np.where(L < 49152, 22 + m // 512, np.minimum(71 + m // 1024, BUCKETS - 1))))
    return int(b) if b.ndim == 0 else b


def bucket_class(b):
    c = np.searchsorted(np.array(CLASS_FIRST_BUCKET[1:4]), b, side="right")
    return int(c) if np.ndim(c) == 0 else c


def length_class(L):
    c = np.searchsorted(np.array(LIMITS), L, side="right")
    return int(c) if np.ndim(c) == 0 else c


def bucket_bounds(b: int):
    """The lowest and the highest length of bucket b (135: no highest, None)."""
    if b == 0:
        return 0, 128
    if b < 8:
        return 128 * b + 1, min(128 * (b + 1), 1023)
    if b == 8:
        return 1024, 1024
    if b < 37:
        return 256 * (b - 5) + 1, min(256 * (b - 4), 8191)
    if b == 37:
        return 8192, 8192
    if b < 118:
        return 512 * (b - 22) + 1, min(512 * (b - 21), 49151)
    if b == 118:
        return 49152, 49152
    if b < 135:
        return 1024 * (b - 71) + 1, 1024 * (b - 70)
    return 65537, None


def bin_grid(n: int):
    """launch_ragged: workgroups of the two binning kernels, lengths per workgroup, and the trips of
    for_each_bucket's loop in a workgroup with a full slice."""
    nbin = max(1, min(1024, -(-n // BIN_TRIP)))
    chunk = -(-n // nbin)
    return nbin, chunk, -(-chunk // BIN_TRIP)


def bin_slice(n: int, w: int):
    """Frames [lo, hi) of binning workgroup w."""
    _, chunk, _ = bin_grid(n)
    return w * chunk, min(n, (w + 1) * chunk)


def bin_waves(n: int):
    """Every (workgroup, first, end) for which one wave calls bucket_slot with a lane that holds a
    frame: 64 consecutive frames of a row of 256, cut at the slice's end."""
    nbin, _, _ = bin_grid(n)
    out = []
    for w in range(nbin):
        lo, hi = bin_slice(n, w)
        for s in range(lo, hi, 64):  # rows of 256 and trips of 2,048 are multiples of 64 from lo
            out.append((w, s, min(s + 64, hi)))
    return out


def class_table(lens):
    """ctab as k_bin_scatter's thread 0 writes it, from the lengths alone: per class its frame
    count, its start in sorted order (longest bucket first), its first item and its items; items
    are numbered longest class first. Also the bucket counts and starts, and the one-bucket flag."""
    lens = np.asarray(lens)
    n = lens.size
    cnt = np.bincount(bucket(lens), minlength=BUCKETS).astype(np.int64)
    after = np.concatenate([np.cumsum(cnt[::-1])[::-1][1:], [0]])  # frames in longer buckets
    count = [int(cnt[CLASS_FIRST_BUCKET[c]:CLASS_FIRST_BUCKET[c + 1]].sum()) for c in range(4)]
    start = [int(sum(count[c + 1:])) for c in range(4)]
    items = [-(-count[c] // PER[c]) for c in range(4)]
    first_item = [int(sum(items[c + 1:])) for c in range(4)]
    return dict(count=count, start=start, items=items, first_item=first_item, total=int(sum(items)),
                one_bucket=bool((cnt == n).any()), bucket_count=cnt, bucket_start=after)


def item_span(lens, tab=None):
    """Per frame the first and the last item that may hold it. The order within a bucket is not
    specified, so a frame of bucket b is somewhere in the bucket's sorted range; both are equal
    where that range lies in one item. A one-bucket batch keeps batch order: frame i is in item
    i // per."""
    lens = np.asarray(lens)
    tab = class_table(lens) if tab is None else tab
    b = bucket(lens)
    c = bucket_class(b)
    per, start, first = np.array(PER)[c], np.array(tab["start"])[c], np.array(tab["first_item"])[c]
    if tab["one_bucket"]:
        it = first + np.arange(lens.size) // per
        return it, it
    p0 = tab["bucket_start"][b]
    p1 = p0 + tab["bucket_count"][b] - 1
    return first + (p0 - start) // per, first + (p1 - start) // per


def ragged_grid(cus: int, n: int) -> int:
    return max(1, min(cus, -(-(-(-n // 4) + 4) // WAVES_PER_BLOCK)))


def parts(grid: int) -> int:
    return min(QUEUE_PARTS, grid)


def waves(grid: int) -> int:
    return WAVES_PER_BLOCK * grid


def part_items(tab, grid: int, part: int):
    """The items of one queue partition in the order its waves take them: item = part + P k, or in
    a one-bucket batch runs of four consecutive items, run = part + P k."""
    P, run = parts(grid), 4 if tab["one_bucket"] else 1
    out = []
    for base in range(part * run, tab["total"], P * run):
        out += [it for it in range(base, base + run) if it < tab["total"]]
    return out


def item_class(tab, it):
    return int(3 - np.searchsorted(np.array(tab["first_item"][::-1][1:]), it, side="right"))


@contextlib.contextmanager
def binned(vc):
    """The binned path for every descriptor batch without a hint, and the automatic geometry; both
    restored on the way out."""
    vc.set_geometry()
    vc.set_ragged_min_frames(1)
    try:
        yield
    finally:
        vc.set_ragged_min_frames(-1)
        vc.set_geometry()


def ragged_plan(vc, cus: int, n: int, want_payload: bool = False) -> int:
    """The plan of one call that must be a single ragged launch over all n frames; returns its grid."""
    plan = vc.plan_frames(cus, n, 0, descriptors=True, want_payload=want_payload)
    rows = [l.astuple() for l in plan]
    assert len(plan) == 1 and plan[0].kernel == KERNEL_RAGGED, rows
    assert (plan[0].first, plan[0].count) == (0, n), rows
    assert plan[0].grid == ragged_grid(cus, n), (rows, ragged_grid(cus, n))
    return int(plan[0].grid)


# ---- layouts ----------------------------------------------------------------------------------
def packed(lens, rng, gap_hi: int = 8):
    """Frames one after the other in the order given: a gap of 0..gap_hi-1 bytes, the frame, room
    for its trailer. Returns the offsets and the buffer's size."""
    lens = np.asarray(lens, dtype=np.int64)
    step = rng.integers(0, gap_hi, lens.size) + lens + 4
    offs = LEAD + np.cumsum(step) - (lens + 4)
    return offs.astype(np.uint64), int(offs[-1] + lens[-1]) + 4 + 8


def views(lens, rng, pool: int):
    """Frames as overlapping views anywhere in a pool of `pool` bytes (no room for trailers)."""
    lens = np.asarray(lens, dtype=np.int64)
    assert int(lens.max()) + 8 <= pool
    return (rng.random(lens.size) * (pool - 8 - lens)).astype(np.uint64)


# ---- 1. later trips of the binning loop ---------------------------------------------------------
TRIPS_N = 2 * (1 << 21) + 300 * 1024 + 77
TRIPS_POOL = 4 * MiB


def trips_batch():
    """4,501,581 lengths: 1,024 binning workgroups of 4,397 (the last of 3,450), so three trips, the
    third of 301 lengths: a full row of 256, a row of 45, then the workgroup-uniform break. The
    last workgroup has two trips, its second of 1,402: five rows and one of 122. About 99.5% of the
    frames are 0..96 B; the rest are of classes 1, 2 and 3, twenty of them of 100,000 B. A frame of
    each longer class is planted in the third trip of workgroup 0 and of workgroup 1,022 and in the
    last trip of the last workgroup. Returns the lengths and the planted {index: length}."""
    n = TRIPS_N
    nbin, chunk, trips = bin_grid(n)
    assert (n, nbin, chunk, trips) == (4_501_581, 1024, 4397, 3)
    assert chunk - 2 * BIN_TRIP == 301 == 256 + 45
    lo_last, hi_last = bin_slice(n, nbin - 1)
    assert hi_last == n and hi_last - lo_last == 3450 and 3450 - BIN_TRIP == 5 * 256 + 122
    rng = np.random.default_rng(0x7219)
    u = rng.random(n)
    lens = rng.integers(0, 97, n)
    for lo_p, hi_p, lo_l, hi_l in ((0, .003, 1024, 3001), (.003, .0045, 8192, 12001), (.0045, .0048, 49152, 70001)):
        m = (u >= lo_p) & (u < hi_p)
        lens[m] = rng.integers(lo_l, hi_l, int(m.sum()))
    lens[rng.choice(n, 20, replace=False)] = 100_000
    plants = {}
    for w in (0, nbin - 2):
        lo, hi = bin_slice(n, w)
        assert hi - lo == chunk
        t = lo + 2 * BIN_TRIP  # the third trip: [t, hi)
        plants.update({t + 3: 2000, t + 256 + 7: 9000, hi - 1: 65537})  # row 0, row 1, the trip's last length
        assert t + 256 + 7 < hi - 1 and (hi - 1 - t) // 256 == 1
    t = lo_last + BIN_TRIP  # the last workgroup's last trip: [t, n)
    plants.update({t + 1: 1024, t + 5 * 256 + 100: 8192, n - 1: 49152})
    assert (n - 1 - t) // 256 == 5
    for i, L in plants.items():
        lens[i] = L
    assert sorted(set(length_class(np.array(list(plants.values()))))) == [1, 2, 3]
    lens = lens.astype(np.uint32)
    assert set(np.unique(length_class(lens))) == {0, 1, 2, 3} and (bucket(lens) == BUCKETS - 1).sum() >= 20
    assert (lens <= 96).mean() > 0.994 and int(lens.astype(np.int64).sum()) < 512 * MiB
    return lens, plants


# ---- 2. every bucket ----------------------------------------------------------------------------
BUCKET_LONG = ((1 << 20) + 3, (1 << 24) + 5)


def every_bucket_batch():
    """Two frames in each of the 136 buckets, at its lowest and highest length (bucket 135: 65,537
    and 2^20 + 3), and one of 2^24 + 5, in a seeded permutation, packed with gaps of 0..7 bytes.
    Returns lens, offs, total and the frames to corrupt: one of every eighth bucket and the longest."""
    lens = []
    for b in range(BUCKETS):
        lo, hi = bucket_bounds(b)
        lens += [lo, hi if hi is not None else BUCKET_LONG[0]]
    lens.append(BUCKET_LONG[1])
    rng = np.random.default_rng(0xB0C)
    lens = np.array(lens, dtype=np.uint32)[rng.permutation(len(lens))]
    assert lens.size == 2 * BUCKETS + 1 and (0 in lens) and (128 in lens)
    cnt = np.bincount(bucket(lens), minlength=BUCKETS)
    assert cnt[:BUCKETS - 1].tolist() == [2] * (BUCKETS - 1) and cnt[BUCKETS - 1] == 3
    offs, total = packed(lens, rng)
    b = bucket(lens)
    bad = [int(np.flatnonzero(b == k)[-1]) for k in range(0, BUCKETS, 8)] + [int(np.argmax(lens))]
    assert len(set(bad)) == 18 and total < 32 * MiB
    return lens, offs, total, bad


# ---- 3. class subsets and partial items ---------------------------------------------------------
SUBSETS = tuple(s for k in range(1, 5) for s in itertools.combinations(range(4), k))  # 15
EDGE_LENS = ((0, 1, 1023), (1024, 1025, 8191), (8192, 8193, 49151), (49152, 65536, 65537))
COUNT_KINDS = 5


def count_of(c: int, kind: int) -> int:
    return (1, PER[c] - 1, PER[c], PER[c] + 1, 3 * PER[c] + 1)[kind]


def subset_kind(si: int, j: int) -> int:
    """The count kind of the j-th class of subset si: a class is in eight subsets and cycles through
    the five kinds over them, each class from another start."""
    c = SUBSETS[si][j]
    return (sum(c in s for s in SUBSETS[:si]) + c) % COUNT_KINDS


def subset_batch(si: int):
    """Subset si of the classes, each with 1, per - 1, per, per + 1 or 3 per + 1 frames at its edge
    lengths. A class of more than one item has exactly `per` frames of its longest length, which
    are its first item, and (classes 1..3) exactly a last item's worth of its shortest, which are
    its partial last item. Class 0's edge lengths have two buckets only (0 and 1 share bucket 0):
    at 3 per + 1 frames its shortest bucket spans the three items behind the first.
    Returns lens, offs, total, the class table and the frames to corrupt."""
    classes = SUBSETS[si]
    rng = np.random.default_rng(0x5B5 + si)
    lens = []
    for j, c in enumerate(classes):
        k, per = count_of(c, subset_kind(si, j)), PER[c]
        short, mid, long_ = EDGE_LENS[c]
        if k <= per:
            lens += [EDGE_LENS[c][i % 3] for i in range(k)]
        elif c == 0:
            lens += [long_] * per + [(short, mid)[i % 2] for i in range(k - per)]
        else:
            last = (k - 1) % per + 1
            lens += [long_] * per + [mid] * (k - per - last) + [short] * last
    lens = np.array(lens, dtype=np.uint32)[rng.permutation(len(lens))]
    offs, total = packed(lens, rng)
    tab = class_table(lens)
    assert [c for c in range(4) if tab["count"][c]] == list(classes)
    lo, hi = item_span(lens, tab)
    cls = length_class(lens)
    bad = []
    for c in classes:
        first, last = tab["first_item"][c], tab["first_item"][c] + tab["items"][c] - 1
        bad.append(int(np.flatnonzero((cls == c) & (lo == first) & (hi == first))[0]))
        if last > first:
            sure = np.flatnonzero((cls == c) & (lo == last) & (hi == last))
            if c == 0 and tab["items"][c] > 2:
                assert sure.size == 0
                sure = np.flatnonzero((cls == c) & (lo > first) & (hi == last))
            bad.append(int(sure[0]))
    assert len(set(bad)) == len(bad)
    return lens, offs, total, tab, bad


# ---- 4. one bucket at a small grid and at the full grid ------------------------------------------
IDENTITY_SMALL = ((1, 600), (3, 600), (33, 600), (127, 600), (1000, 600), (1100, 600), (50, 16400))


def identity_batch(n: int, L: int, seed: int):
    """n frames of L bytes packed with gaps, listed in a seeded permutation of their memory order."""
    rng = np.random.default_rng(seed)
    lens = np.full(n, L, np.uint32)
    offs, total = packed(lens, rng)
    return lens, offs[rng.permutation(n)].copy(), total


def identity_small_facts(cus: int, n: int, L: int):
    """One bucket, P = the grid < 64; returns the grid and the items."""
    tab = class_table(np.full(n, L, np.uint32))
    grid = ragged_grid(cus, n)
    assert tab["one_bucket"] and parts(grid) == grid < QUEUE_PARTS
    return grid, tab["total"]


IDENTITY_FULL_LEN = 100


def identity_full_n(cus: int) -> int:
    """Frames of 100 B (32 per item) with 3 items per wave of the full grid and a partial last item."""
    n = 32 * 3 * waves(cus) + 37
    tab = class_table(np.full(n, IDENTITY_FULL_LEN, np.uint32))
    grid = ragged_grid(cus, n)
    assert tab["one_bucket"] and grid == cus and parts(grid) == QUEUE_PARTS
    assert tab["total"] >= 3 * waves(grid) and tab["total"] % 4 != 0
    return n


CHAIN_N = (4000, 900, 1000)  # a mixed batch, a mixed batch of less than a quarter, an identity batch of 600-B frames


def mixed_lens(n: int, seed: int):
    """Log-uniform 40..66,000 B: every class."""
    rng = np.random.default_rng(seed)
    lens = np.exp(rng.uniform(np.log(40), np.log(66000), n)).astype(np.uint32)
    assert set(np.unique(length_class(lens))) == {0, 1, 2, 3} and not class_table(lens)["one_bucket"]
    return lens


# ---- 5. a deep queue across class boundaries ------------------------------------------------------
HOST_CHUNK = 1 << 20
RAGGED_MIN_DEFAULT = 4096


def host_chunks(offs, lens, cap: int, tail: int = 0):
    """frames_host's chunks of whole frames [i0, i1) over non-decreasing offsets: a chunk takes frames
    while its wire span stays within cap (at least one)."""
    offs = np.asarray(offs).astype(np.int64)
    ends = offs + np.asarray(lens).astype(np.int64) + tail
    assert (np.diff(offs) >= 0).all() and (np.diff(ends) >= 0).all()
    out, i = [], 0
    while i < offs.size:
        j = max(i + 1, int(np.searchsorted(ends, offs[i] + cap, side="right")))
        out.append((i, j))
        i = j
    return out


def _spread(parts_):
    """Lists merged so that each is spread evenly over the result."""
    key = np.concatenate([(np.arange(len(p)) + 0.5) / len(p) for p in parts_])
    return np.concatenate(parts_)[np.argsort(key, kind="stable")]


def deep_batch(cus: int):
    """Items >= 4 x the waves of the full grid, every class non-empty, no class's item count a
    multiple of P = 64; most frames 129..160 B at 32 per item, some 1,100, 550 and 80 of classes 1,
    2 and 3, spread evenly in memory order. Every class has exactly one item's worth of frames in
    its longest bucket (its first item) and exactly its partial last item's worth in its shortest
    (its last item). Partitions 0..19 take an item of class 3, of class 2, of class 1 and then of
    class 0. Packed in memory order, so that the host call cuts it into chunks of whole frames;
    the gaps are 0..g-1 bytes, g the first from 8 on for which every chunk of 1 MiB (the last one
    too) holds 4,096 frames or more.
    Returns lens, offs, total, the class table, the frames to corrupt (1%) and the host chunks."""
    rng = np.random.default_rng(0xDEE9 + cus)
    w = waves(cus)
    items0 = max(4 * w, 16384) + 1
    n0 = 32 * (items0 - 1) + 5
    c0 = np.concatenate([rng.integers(129, 161, n0 - 37), rng.integers(900, 1024, 32), [0, 128, 1, 64, 127]])
    c1 = np.concatenate([rng.integers(1025, 2001, 16 * 68), rng.integers(7937, 8192, 16), np.full(7, 1024)])
    c2 = np.concatenate([rng.integers(8193, 12001, 8 * 68), rng.integers(48641, 49152, 8), np.full(3, 8192)])
    c3 = np.concatenate([rng.integers(49153, 52001, 4 * 18), rng.integers(65537, 70001, 4), np.full(1, 49152)])
    lens = _spread([rng.permutation(c) for c in (c0, c1, c2, c3)]).astype(np.uint32)
    n = lens.size
    tab = class_table(lens)
    grid = ragged_grid(cus, n)
    P = parts(grid)
    assert grid == cus and P == QUEUE_PARTS and tab["total"] >= 4 * waves(grid)
    assert tab["items"] == [items0, 70, 70, 20] and all(k % P for k in tab["items"]) and all(tab["count"])
    for part in range(20):
        seq = [item_class(tab, it) for it in part_items(tab, grid, part)]
        assert seq[:4] == [3, 2, 1, 0] and len(seq) >= 4 * WAVES_PER_BLOCK * (grid // P), (part, seq[:6])
    # corrupted frames: 1% at random, and every frame of each class's first and last item
    lo, hi = item_span(lens, tab)
    cls = length_class(lens)
    bad = set(rng.choice(n, n // 100, replace=False).tolist())
    for c in range(4):
        first, last = tab["first_item"][c], tab["first_item"][c] + tab["items"][c] - 1
        in_first = np.flatnonzero((cls == c) & (lo == first) & (hi == first))
        in_last = np.flatnonzero((cls == c) & (lo == last) & (hi == last))
        assert in_first.size == PER[c] and in_last.size == (tab["count"][c] - 1) % PER[c] + 1 < PER[c]
        bad |= set(in_first[:2].tolist()) | set(in_last[:1].tolist())
    bad = np.array(sorted(bad))
    for c in range(4):
        first, last = tab["first_item"][c], tab["first_item"][c] + tab["items"][c] - 1
        assert ((cls[bad] == c) & (hi[bad] == first)).any() and ((cls[bad] == c) & (lo[bad] == last)).any()
    for gap_hi in range(8, 48):
        offs, total = packed(lens, np.random.default_rng(cus), gap_hi)
        chunks = host_chunks(offs, lens, HOST_CHUNK)
        if min(j - i for i, j in chunks) >= RAGGED_MIN_DEFAULT:
            break
    else:
        raise AssertionError(("no gap width leaves 4,096 frames in every host chunk", [j - i for i, j in chunks]))
    assert len(chunks) >= 8 and total < 200 * MiB
    return lens, offs, total, tab, bad, chunks


# ---- 6. both reservation paths into one bucket -----------------------------------------------------
SLOT_BUCKET = 10  # 1,281..1,536 B


def slot_batch(n: int):
    """Per binning workgroup, waves of three kinds in turn: all 64 frames in bucket 10; all but one
    or two; fully mixed lengths with at least one frame of bucket 10. The last wave of the last
    workgroup is wholly in bucket 10. Returns the lengths and, per wave of bin_waves(n), whether
    bucket_slot takes the one-atomic path."""
    rng = np.random.default_rng(0x5107 + n)
    lo_b, hi_b = bucket_bounds(SLOT_BUCKET)
    lens = np.zeros(n, dtype=np.int64)
    wv = bin_waves(n)
    kinds = []
    for j, (w, s, e) in enumerate(wv):
        kind = 0 if j == len(wv) - 1 else j % 3
        m = e - s
        if kind == 2:
            row = np.exp(rng.uniform(0, np.log(70000), m)).astype(np.int64)
            row[0] = lo_b
            row[m - 1] = 0
        else:
            row = rng.integers(lo_b, hi_b + 1, m)
            if kind == 1:
                row[int(rng.integers(0, m))] = 600
                if j % 2:
                    row[int(rng.integers(0, m))] = 20000
        lens[s:e] = row
        kinds.append(kind)
    b = bucket(lens)
    uniform = [bool((b[s:e] == b[s]).all()) for _, s, e in wv]
    assert uniform == [k == 0 for k in kinds]
    nbin = bin_grid(n)[0]
    for w in range(nbin):
        mine = [(k, s, e) for k, (ww, s, e) in zip(kinds, wv) if ww == w]
        assert set(k for k, _, _ in mine) == {0, 1, 2}
        assert all((b[s:e] == SLOT_BUCKET).any() for _, s, e in mine)
    return lens.astype(np.uint32), uniform


def slot_facts(n: int):
    nbin, chunk, trips = bin_grid(n)
    last = bin_waves(n)[-1]
    return nbin, chunk, trips, last[2] - last[1]


# ---- 7. the seeded fuzz ----------------------------------------------------------------------------
FUZZ_DEFAULT_SEED, FUZZ_DEFAULT_ROUNDS = 20261021, 60
FUZZ_CAP = 32 * MiB
FUZZ_MAX_N = 40000
FUZZ_POOL = 4 * MiB
CLASS_RANGE = ((0, 1023), (1024, 8191), (8192, 49151), (49152, 70000))


def _edges(c: int):
    """Bucket and class edges of class c, and their neighbours."""
    lo_c, hi_c = CLASS_RANGE[c]
    out = set()
    for b in range(CLASS_FIRST_BUCKET[c], CLASS_FIRST_BUCKET[c + 1]):
        lo, hi = bucket_bounds(b)
        out |= {lo - 1, lo, lo + 1, hi_c if hi is None else hi, hi_c if hi is None else hi + 1}
    return np.array(sorted(v for v in out if lo_c <= v <= hi_c))


EDGES = tuple(_edges(c) for c in range(4))


def fuzz_seed() -> int:
    return int(os.environ.get("FUZZ_SEED", str(FUZZ_DEFAULT_SEED)))


def fuzz_round_count() -> int:
    return int(os.environ.get("FUZZ_RAGGED_ROUNDS", str(FUZZ_DEFAULT_ROUNDS)))


def fuzz_rounds(cus: int, seed: int | None = None, rounds: int | None = None):
    """The rounds of the fuzz: dicts of n, lens, offs, total, layout ('packed', 'views', 'perm'),
    mode ('crc', 'verify', 'ex'), bad [(frame, byte of the frame or its trailer, bit)], and the
    facts of the plan: grid, P, items, waves, nbin, classes, one_bucket. A round hashes at most
    32 MiB: the batch is cut where its bytes reach that."""
    rng = np.random.default_rng(fuzz_seed() if seed is None else seed)
    out = []
    for _ in range(fuzz_round_count() if rounds is None else rounds):
        n = max(1, min(FUZZ_MAX_N, int(2.0 ** rng.uniform(0, np.log2(FUZZ_MAX_N)))))
        weights = rng.random(4) * (rng.random(4) < 0.55)
        if not weights.any():
            weights[int(rng.integers(0, 4))] = 1.0
        kind = rng.random()
        if kind < 0.08:  # many items: short class-1 frames, as many as the bytes allow
            n, weights = int(rng.integers(36000, FUZZ_MAX_N + 1)), np.array([0.0, 1.0, 0.0, 0.0])
        one_length = 0.08 <= kind < 0.2
        weights /= weights.sum()
        lens = np.zeros(n, dtype=np.int64)
        i = 0
        while i < n:
            run = min(n - i, int(2.0 ** rng.uniform(0, np.log2(300))))
            c = int(rng.choice(4, p=weights))
            if kind < 0.08:
                L = int(rng.integers(1024, 1030))
            elif rng.random() < 0.6:
                L = int(rng.choice(EDGES[c]))
            else:
                L = int(rng.integers(CLASS_RANGE[c][0], CLASS_RANGE[c][1] + 1))
            lens[i:i + run] = L
            i += run
        if one_length:
            lens[:] = lens[0]
        if rng.random() < 0.1:
            for f in rng.choice(n, min(n, int(rng.integers(1, 4))), replace=False):
                lens[f] = int(rng.integers(70001, 2 * MiB + 1))
        mode = ("crc", "verify", "ex")[int(rng.integers(0, 3))]
        layout = ("packed", "perm", "views")[int(rng.integers(0, 3 if mode == "crc" else 2))]
        n = max(1, int(np.searchsorted(np.cumsum(lens + 12), FUZZ_CAP - 64, side="right")))
        lens = lens[:n]
        if layout == "views":
            pool = max(FUZZ_POOL, int(lens.max()) + 64)
            offs, total = views(lens, rng, pool), pool
        else:
            offs, total = packed(lens, rng)
            if layout == "perm":
                perm = rng.permutation(n)
                offs, lens = offs[perm].copy(), lens[perm].copy()
        bad = []
        if mode != "crc" and rng.random() < 0.6:
            for f in rng.choice(n, min(n, int(rng.integers(1, 5))), replace=False):
                bad.append((int(f), int(rng.integers(0, int(lens[f]) + 4)), int(rng.integers(0, 8))))
        lens = lens.astype(np.uint32)
        tab = class_table(lens)
        grid = ragged_grid(cus, n)
        assert int(lens.astype(np.int64).sum()) <= FUZZ_CAP and total <= FUZZ_CAP + 2 * MiB + 64
        out.append(dict(n=n, lens=lens, offs=offs, total=total, layout=layout, mode=mode, bad=bad, grid=grid,
                        P=parts(grid), items=tab["total"], waves=waves(grid), nbin=bin_grid(n)[0],
                        classes=tuple(c for c in range(4) if tab["count"][c]), one_bucket=tab["one_bucket"],
                        long=bool((bucket(lens) == BUCKETS - 1).any())))
    return out


def fuzz_items_can_outnumber_waves(cus: int) -> bool:
    """At most 32 MiB in at most 40,000 frames: the most items are 2,048 of 16 class-1 frames of
    1,024 B (class 0 packs 32 frames per item: 1,250 at most), so only a device of fewer than 128
    CUs (2,048 waves) can have more items than waves in a round. The edge cases reach that at any
    size (identity_full_n, deep_batch)."""
    return waves(cus) < FUZZ_MANY_ITEMS


FUZZ_MANY_ITEMS = 2000  # what a many-items round reaches: 32 MiB / (16 x (1,024..1,029 + 12) B)


def fuzz_coverage(rounds, cus: int) -> None:
    """What the default rounds must have included (asserted by the GPU test after its loop and, for
    64, 128, 256 and 304 CUs, by tests/test_launch_plan.py)."""
    assert any(r["one_bucket"] for r in rounds), "a one-bucket round"
    assert any(r["one_bucket"] and r["n"] > 64 for r in rounds), "a one-bucket round of several items"
    assert set(len(r["classes"]) for r in rounds) == {1, 2, 3, 4}, "class subsets of every size"
    assert any(r["P"] < QUEUE_PARTS for r in rounds) and any(r["P"] == QUEUE_PARTS for r in rounds)
    if fuzz_items_can_outnumber_waves(cus):
        assert any(r["items"] > r["waves"] for r in rounds), "items > waves"
    assert max(r["items"] for r in rounds) >= FUZZ_MANY_ITEMS, "a many-items round"
    assert any(r["nbin"] > 1 for r in rounds), "nbin > 1"
    assert any(r["long"] for r in rounds), "a frame in bucket 135"
    assert any(r["mode"] == "crc" for r in rounds)
    for mode in ("verify", "ex"):
        assert any(r["mode"] == mode and r["bad"] for r in rounds), mode + " with a bad frame"
        assert any(r["mode"] == mode and not r["bad"] for r in rounds), mode + " without a bad frame"
    assert set(r["layout"] for r in rounds) == {"packed", "perm", "views"}
