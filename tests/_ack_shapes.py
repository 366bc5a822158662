"""Shapes of the ACK calls' edge tests (tests/test_gpu_acks_edges.py) as plain
functions of the CU count, with the plan each of them must get
(val_gpu_plan_ack_calls through vc.plan_ack_calls). No GPU and no torch here:
tests/test_ack_shapes.py calls the same functions for 64, 128, 256 and 304
CUs, so a threshold that moves in launch_plan.hpp fails a test there instead of
moving a GPU case onto the other workgroup size, or onto a grid in which no
workgroup takes a second file, unnoticed.

A shape is (counts, n_pad, grid, longs): frames per file, the unowned (0, 0)
padding entries behind the frames, the grid of the per-file launch and
{file index: frames} of the files that are not tiny. What the frames hold
comes from the GPU tests; nothing here depends on it."""
from __future__ import annotations

import numpy as np

# val_gpu_plan_ack_calls' kernels and calls (val_protocol_amd.crc names them too; restated so that a
# renumbering fails here)
RESPOND, APPLY = 0, 1
CHUNK = {1024: 1024, 256: 256}  # frames per chunk = threads per workgroup
SMALL_FRAMES = 256  # calls whose files own this many frames or fewer on average run in workgroups of 256

SHARED_LONG = {1024: (2049, 1025, 5121, 1024), 256: (257, 600, 1025, 1281)}
SHARED_APPLY_LONG = (1025, 2049, 4097)
PASS1_COUNTS = {1024: (3073, 5120, 5121, 9217), 256: (1281, 2305)}


def respond_plan(vc, cus: int, n: int, n_files: int, lanes: int):
    """The respond call's three launches; -> the grid of k_ack_respond_files, which must run in
    workgroups of `lanes` threads."""
    plan = vc.plan_ack_calls(vc.ACK_RESPOND, cus, n, n_files)
    rows = [l.astuple() for l in plan]
    assert [l.kernel for l in plan] == [vc.KERNEL_UNPACK_PARSE, vc.KERNEL_ACK_RESPOND_FILES, vc.KERNEL_ACK_EMIT], rows
    assert plan[1].lanes == lanes and plan[1].count == n_files, rows
    want = min(n_files, cus * (8 if lanes == 256 else 1))
    assert plan[1].grid == want, rows
    return int(plan[1].grid)


def apply_plan(vc, cus: int, n: int, n_files: int):
    plan = vc.plan_ack_calls(vc.ACK_APPLY, cus, n, n_files)
    rows = [l.astuple() for l in plan]
    assert [l.kernel for l in plan] == [vc.KERNEL_ACK_APPLY_FILES], rows
    assert plan[0].grid == min(n_files, cus) and plan[0].count == n_files, rows
    return int(plan[0].grid)


def order_grid(vc, cus: int, n: int, n_files: int) -> int:
    """The grid of k_unpack_order_files for the same window (vc.plan_window)."""
    plan = vc.plan_window(vc.WINDOW_UNPACK_FILES, cus, n, groups=n_files)
    rows = [l.astuple() for l in plan]
    order = [l for l in plan if l.kernel == vc.KERNEL_UNPACK_ORDER_FILES]
    assert len(order) == 1 and order[0].grid == min(n_files, cus), rows
    return int(order[0].grid)


def chunks(count: int, block: int) -> int:
    return -(-count // block)


def _place(counts, grid: int, longs):
    """The long files into workgroups 0, 1 and 2 of a grid-stride loop over 2 grid + 3 files:
    workgroup 0 takes long, tiny, long; workgroup 1 tiny, long, empty; workgroup 2 empty, long,
    tiny (and workgroups 0..2 are the ones that take a third file at all when S = 2 grid + 3)."""
    a, b, c, d = longs
    at = {0: a, grid: 2, 2 * grid: c, 1: 3, 1 + grid: b, 1 + 2 * grid: 0, 2: 0, 2 + grid: d, 2 + 2 * grid: 1}
    for s, v in at.items():
        counts[s] = v
    return {s: v for s, v in at.items() if v > 3}


def shared_respond(vc, cus: int, lanes: int, seed: int = 1):
    """S = 2 grid + 3 files of 0..3 frames with SHARED_LONG[lanes] placed by _place. In workgroups
    of 1,024 threads the grid is the CUs and padding raises n until n // S > 256; in workgroups
    of 256 the grid is 8 per CU. -> (counts, n_pad, grid, longs)."""
    grid = cus * (8 if lanes == 256 else 1)
    S = 2 * grid + 3
    rng = np.random.default_rng(0xACC5 + 7 * cus + lanes + seed)
    counts = rng.integers(0, 4, S)
    longs = _place(counts, grid, SHARED_LONG[lanes])
    n = int(counts.sum())
    n_pad = max(0, (SMALL_FRAMES + 1) * S - n) if lanes == 1024 else 0
    assert respond_plan(vc, cus, n + n_pad, S, lanes) == grid
    if lanes == 1024:  # one entry fewer and the call would run in workgroups of 256
        assert vc.plan_ack_calls(vc.ACK_RESPOND, cus, n + n_pad - 1, S)[1].lanes == 256
    return counts, n_pad, grid, longs


def shared_apply(vc, cus: int, seed: int = 2):
    """S = 2 grid + 3 transfers of 0..3 responses with 2049, 1025 and 4097 placed by _place (and a
    fourth of 1,024). -> (counts, grid, longs)."""
    grid = cus
    S = 2 * grid + 3
    rng = np.random.default_rng(0xACC6 + 7 * cus + seed)
    counts = rng.integers(0, 4, S)
    longs = _place(counts, grid, (2049, 1025, 4097, 1024))
    assert apply_plan(vc, cus, int(counts.sum()), S) == grid
    return counts, grid, longs


def shares(S: int, grid: int):
    """The files each workgroup of a grid-stride loop takes, in the order it takes them."""
    return [list(range(g, S, grid)) for g in range(grid)]


def check_shared(counts, grid: int, longs, block: int, want_long) -> None:
    """What the GPU tests rely on: more than two files per workgroup somewhere, the long files where
    _place says, and workgroups that take a multi-chunk file before and after another file."""
    S = len(counts)
    assert S > 2 * grid and S == 2 * grid + 3
    sh = shares(S, grid)
    assert sh[0] == [0, grid, 2 * grid] and sh[1] == [1, 1 + grid, 1 + 2 * grid] and sh[2] == [2, 2 + grid, 2 + 2 * grid]
    assert all(len(x) == 2 for x in sh[3:])
    assert sorted(longs.values()) == sorted(want_long)
    c = [int(x) for x in counts]
    multi = lambda s: chunks(c[s], block) > 1  # noqa: E731
    # long, tiny, long: a multi-chunk file first, a file of a few frames behind it, a multi-chunk file behind that
    assert multi(sh[0][0]) and 0 < c[sh[0][1]] <= 3 and multi(sh[0][2])
    # tiny, long, empty
    assert 0 < c[sh[1][0]] <= 3 and multi(sh[1][1]) and c[sh[1][2]] == 0
    # empty, long (a whole number of chunks in 1,024 mode), tiny
    assert c[sh[2][0]] == 0 and c[sh[2][1]] >= block and 0 < c[sh[2][2]] <= 3
    tiny = [x for s, x in enumerate(c) if s not in longs]
    assert set(tiny) == {0, 1, 2, 3}


# ---- pass 1 of k_ack_respond_files ----------------------------------------------------------
def pass1_slot(i: int, block: int):
    """Where pass 1 reads frame i of a file: None for the first chunk (kept in registers), else
    (step of the loop, slot u of that step)."""
    if i < block:
        return None
    return (i - block) // (4 * block), (i - block) % (4 * block) // block


def pass1_places(count: int, block: int):
    """{name: index of the file's last accepted frame}: the first chunk, each slot of pass 1's
    first step, the second step, the file's very last frame; only those the file has."""
    at = {"chunk0": 5, "u0": block + 7, "u1": 2 * block + 7, "u2": 3 * block + 7, "u3": 4 * block + 7,
          "step2": 5 * block, "last": count - 1}
    return {k: i for k, i in at.items() if i < count}


def pass1_files(lanes: int):
    """The files of the pass-1 test -> [(frames, what, index or None)]: every place of every count,
    then (for the largest count) a file in which nothing is accepted, one in which only the last
    frame is, and one that completes inside the second step."""
    block = CHUNK[lanes]
    out = []
    for count in PASS1_COUNTS[lanes]:
        out += [(count, name, i) for name, i in pass1_places(count, block).items()]
    big = PASS1_COUNTS[lanes][-1]
    out += [(big, "none", None), (big, "only-last", big - 1), (big, "completes", 5 * block + block // 2)]
    return out


def pass1_shape(vc, cus: int, lanes: int):
    """-> (files as pass1_files, fill): `fill` one-frame files behind them bring the average to 256
    frames or fewer where the 256-thread instance is wanted. The grid must hold every file, so no
    workgroup's state from another file can mask what pass 1 leaves."""
    files = pass1_files(lanes)
    n = sum(f[0] for f in files)
    fill = 0
    if lanes == 256:
        while (n + fill) // (len(files) + fill) > SMALL_FRAMES:
            fill += 1
    respond_plan(vc, cus, n + fill, len(files) + fill, lanes)
    return files, fill


def check_pass1(lanes: int) -> None:
    block = CHUNK[lanes]
    files = pass1_files(lanes)
    names = {}
    for count, name, i in files:
        names.setdefault(name, []).append((count, i))
    # every slot of the first step and the second step hold a file's last accepted frame
    for u in range(4):
        assert any(pass1_slot(i, block) == (0, u) for _, i in names[f"u{u}"])
    assert all(pass1_slot(i, block)[0] == 1 for _, i in names["step2"]) and names["step2"]
    assert all(pass1_slot(i, block) is None for _, i in names["chunk0"])
    assert {c for c, _ in names["last"]} == set(PASS1_COUNTS[lanes])
    big = PASS1_COUNTS[lanes][-1]
    # the long files: pass 1 takes its second step, and its first step has a frame in all four slots
    assert big > 5 * block and pass1_slot(big - 1, block)[0] >= 1
    assert sum(c > 5 * block for c in PASS1_COUNTS[lanes]) >= 2 - (lanes == 256)
    assert {pass1_slot(i, block) for i in range(block, 5 * block)} == {(0, u) for u in range(4)}
    (count, i), = names["completes"]
    assert pass1_slot(i, block)[0] == 1 and i < count - 1
    if lanes == 1024:  # the four counts: 3 chunks + 1, 5 chunks, 5 chunks + 1, 9 chunks + 1
        assert [c - (c // block) * block for c in PASS1_COUNTS[lanes]] == [1, 0, 1, 1]
        assert pass1_slot(5120 - 1, block) == (0, 3) and pass1_slot(5121 - 1, block) == (1, 0)
