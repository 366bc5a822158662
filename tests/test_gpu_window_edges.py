"""Directed tests for branches of the window calls' kernels that only a shape
beyond the other tests' reaches: a round of the 1,024-lane scan front in which
every lane matches, more streams than fronts, more slots than one pass of the
compacting grids, the largest frames, the chunk edges of k_scan_first.

Expected values never come from a device path: every call goes through
test_gpu_scan._scan or test_gpu_fill._fill, which compare with wire.scan_frames
and wire.fill_window (the rules in plain C). Every test that depends on a grid
size takes the grid from vc.plan_window for the device it runs on and asserts
that its shape exceeds it."""
import numpy as np
import pytest

from tests.test_gpu_fill import MTU, T, _bytes, _fill
from tests.test_gpu_scan import _cat, _decoy, _f, _scan
from tests.test_gpu_unpack import vc, wire  # noqa: F401 - fixtures

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WIDE_EDGES = (65, 321, 1345, 2369)  # frames a uniform run has given when a round of the wide front ends


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 1. rounds of the wide front ----------------------------------------------------------------
@pytest.mark.parametrize("d", [-1, 0, 1])
@pytest.mark.parametrize("E", WIDE_EDGES)
def test_wide_front_round_edges(vc, wire, E, d):
    """scan_kernel.hpp, k_scan_streams<16>: `m = has ? ... : kFront` with has == 0 (all 1,024
    lanes match: a run of 1,345 or more), `act = all ? min(act * 4u, kFront) : 64u` in both
    directions, and `e = min(m, p.max_frames - k)` with the limit on a round's edge. The run
    ends one frame before, at and one frame behind the round that ends at frame E; a frame of
    another size follows, then 70 frames of the run's size (a round of 64 and part of one of 256).
    Once more with max_frames = the run, and with len 1 and 9 bytes into the frame behind the
    run (no header; a header and no frame)."""
    run = E + d
    content = run % 5  # wire 12 .. 16
    other = (content + 2) % 5
    a, b = _f(wire, content), _f(wire, other)
    s = _cat([a] * run + [b] + [a] * 70)
    head = run * a.size
    want = _scan(vc, wire, [s, (s, head + 1), (s, head + 9)], 1024, run + 100)
    assert (want[0][0], want[0][1].size, want[0][3]) == (0, run + 71, s.size) and want[0][2][run] == 8 + other
    for st, off, ln, used in want[1:]:
        assert (st, off.size, used) == (0, run, head)
    (st, off, ln, used), = _scan(vc, wire, [s], 1024, run)
    assert (st, off.size, used) == (0, run, head)


def test_wide_front_decoys_in_later_waves(vc, wire):
    """scan_kernel.hpp, k_scan_streams<16>: `fw = has ? __builtin_ctz(has) : 0u` when the waves
    behind the first mismatch report a full match. A frame of 2P or 3P whose payload reads as
    headers of P stands right behind frame 321 (lane 0 of the first 1,024-lane round) and right
    behind frame 1,345 (lane 0 of the second), and once in the sixth wave of a 1,024-lane round;
    every other lane of those rounds holds a complete frame of size P."""
    P = 40
    a = _f(wire, P - 12)
    b = _f(wire, 2 * P - 12, _decoy(P, 2))
    c = _f(wire, 3 * P - 12, _decoy(P, 3))
    streams = [_cat([a] * 321 + [b] + [a] * 1100),
               _cat([a] * 1345 + [c] + [a] * 1100),
               _cat([a] * 321 + [b] + [a] * 1023 + [c] + [a] * 80),  # frame 1,345 is the decoy of 3P
               _cat([a] * (321 + 5 * 64 + 7) + [c] + [a] * 800)]
    want = _scan(vc, wire, streams, 1024, 3000)
    assert [(w[0], w[1].size) for w in want] == [(0, 1422), (0, 2446), (0, 1426), (0, 1449)]
    assert want[0][2][321] == 2 * P - 4 and want[1][2][1345] == 3 * P - 4
    assert want[2][2][321] == 2 * P - 4 and want[2][2][1345] == 3 * P - 4 and want[3][2][648] == 3 * P - 4


# ---- 2. more streams than fronts, more slots than the compacting grid ------------------------------
def _tiny_streams(wire, S, seed):
    """S streams of 0 to 8 frames with content 0..8 from a pool (mtu 20 admits them all): empty
    ones, runs, mixed sizes, some cut inside their last frame, some that stop on a frame over the
    MTU. Neighbours differ in their counts and so in the rounds their walks take."""
    rng = np.random.default_rng(seed)
    pool = [_f(wire, c) for c in range(0, 9)]
    over = _f(wire, 9)
    streams = []
    for s in range(S):
        kind = int(rng.integers(0, 6))
        n = int(rng.integers(0, 9))
        if kind == 0:
            streams.append((pool[4], 0) if s % 2 else np.zeros(0, np.uint8))  # empty
        elif kind == 1:
            streams.append(_cat([pool[int(c)] for c in rng.integers(0, 9, n)]))
        elif kind == 2:
            streams.append(_cat([pool[int(rng.integers(0, 9))]] * n))
        elif kind == 3:
            full = _cat([pool[8]] * n + [pool[5]])
            streams.append((full, full.size - int(rng.integers(1, 17))))
        elif kind == 4:
            at = int(rng.integers(0, 8))
            streams.append(_cat([pool[3]] * at + [over] + [pool[3]] * (7 - at)))  # protocol error at `at`
        else:
            streams.append(_cat([pool[0]] * (n // 2) + [pool[7]] * (n - n // 2)))
    return streams


@pytest.mark.parametrize("front", [64, 1024])
def test_more_streams_than_fronts(vc, wire, front):
    """scan_kernel.hpp: the second and later iterations of `for (s = front; s < p.n_streams;
    s += nfronts)` in k_scan_streams (the wide front's `flip` and LDS slots go from one stream
    into the next; streams with even and odd numbers of rounds follow each other), with a
    partial last pass; and of `for (e = ...; e < slots; e += stride)` in k_scan_compact, with
    `(uint32_t)e / p.max_frames` beyond the grid."""
    cus, max_frames = _cus(), 64
    S = 32 * cus + 108
    vc.set_scan_front(front)
    try:
        plan = vc.plan_window(vc.WINDOW_SCAN, cus, S, max_frames=max_frames)
    finally:
        vc.set_scan_front(0)
    assert [p.kernel for p in plan] == [vc.KERNEL_SCAN_STREAMS, vc.KERNEL_SCAN_FIRST, vc.KERNEL_SCAN_COMPACT]
    assert plan[0].lanes == front
    nfronts = plan[0].grid * (4 if front == 64 else 1)
    assert nfronts < S and S % nfronts, (nfronts, S)  # a second pass, and a partial last one
    assert S * max_frames > plan[2].grid * 256, (S, plan[2].grid)  # k_scan_compact takes a second pass
    streams = _tiny_streams(wire, S, seed=front)
    want = _scan(vc, wire, streams, 20, max_frames, phases=(0,), fronts=(front,))
    cnt = np.array([w[1].size for w in want])
    status = np.array([w[0] for w in want])
    assert set(cnt.tolist()) == set(range(9)) and (status == vc.VAL_ERR_PROTOCOL).sum() > S // 10
    # streams that share a front differ: what one leaves behind would show in the next
    assert (cnt[:S - nfronts] != cnt[nfronts:]).sum() > (S - nfronts) // 2


def test_more_fill_slots_than_the_grid(vc, wire):
    """fill_kernel.hpp, k_fill_desc: the second iteration of `for (e = ...; e < slots;
    e += stride)`, `(uint32_t)e / p.max_frames` and `first[s] + j` beyond one pass of the grid,
    and the padding entries behind the total there. Most transfers are finished or one to three
    frames long; ten run to the full 256 frames."""
    cus, max_frames = _cus(), 256
    S = 8 * cus + 52
    plan = vc.plan_window(vc.WINDOW_FILL, cus, S, max_frames=max_frames, len_hint=MTU)
    assert plan[2].kernel == vc.KERNEL_FILL_DESC and S * max_frames > plan[2].grid * 256, (S, plan[2].grid)
    M = MTU - 12
    rng = np.random.default_rng(256)
    pool = _bytes(256, 1 << 16)
    full = set(rng.choice(S, 10, replace=False).tolist()) | {S - 1}
    specs = []
    for s in range(S):
        at, nxt = int(rng.integers(0, 4096)), int(rng.integers(0, 300))
        if s in full:
            specs.append(T(pool[at:at + nxt + 257 * M], next=nxt, la=nxt if s % 2 else 0))
        elif s % 4 == 0:
            specs.append(T(pool[at:at + nxt], next=nxt))  # finished
        else:
            size = nxt + int(rng.integers(1, 3 * M - 8))
            specs.append(T(pool[at:at + size], next=nxt, la=nxt if s % 3 else nxt // 2))
    want = _fill(vc, wire, specs, MTU, max_frames, phases=(0,), lanes=(0,))
    cnt = np.array([w[1].size for w in want])
    assert (cnt == max_frames).sum() == len(full) and set(cnt.tolist()) == {0, 1, 2, 3, max_frames}
    assert cnt[S - 1] == max_frames  # the last slots of the last pass are frames, not padding


# ---- 3. the largest frames ------------------------------------------------------------------------
def test_largest_scan_frames(vc, wire):
    """scan_kernel.hpp, k_scan_streams: `q = pos + (uint64_t)j * P` and `wire == P` with
    P = 65,547 and content_len 65,535, the most a header can say; 330 frames reach a 1,024-lane
    round whose lanes look up to 67 MB ahead of the stream's end. One stream ends inside a frame;
    against mtu 65,546 the same frame is a protocol error."""
    mtu = 65547
    big = _f(wire, 65535)
    less = _f(wire, 65534)
    assert big.size == mtu
    s70, s330 = np.tile(big, 70), np.tile(big, 330)
    cut = _cat([s70[:20 * mtu], less, big])
    streams = [s70, s330, (cut, cut.size - 1), _cat([less] * 3 + [big] + [less])]
    want = _scan(vc, wire, streams, mtu, 400, phases=(0,))
    assert [(w[0], w[1].size, w[3]) for w in want] == [(0, 70, 70 * mtu), (0, 330, 330 * mtu),
                                                      (0, 21, 21 * mtu - 1), (0, 5, 5 * mtu - 4)]
    want = _scan(vc, wire, [streams[3], _cat([less] * 70 + [big])], mtu - 1, 400, phases=(0,))
    assert [(w[0], w[1].size, w[3]) for w in want] == [(vc.VAL_ERR_PROTOCOL, 3, 3 * (mtu - 1)),
                                                      (vc.VAL_ERR_PROTOCOL, 70, 70 * (mtu - 1))]


# ---- 4. k_scan_first's chunks -----------------------------------------------------------------------
@pytest.mark.parametrize("S", [1023, 1024, 1025, 2048, 2049])
def test_scan_first_chunk_edges(vc, wire, S):
    """scan_kernel.hpp, k_scan_first: `for (c0 = 0; c0 < p.n_streams; c0 += kScanFirstBlock)`
    with the last count of a chunk, the first of the next (`carry += total`) and
    `p.first[p.n_streams]` on either side of 1,024 and 2,048 streams; 0 to 3 empty frames each."""
    rng = np.random.default_rng(S)
    empty = _f(wire, 0)
    cnt = rng.integers(0, 4, S)
    cnt[[0, 1022, S - 1]] = [1, 2, 3]
    streams = [np.tile(empty, int(c)) for c in cnt]
    want = _scan(vc, wire, streams, 1024, 4, phases=(0,), fronts=(0,))
    assert [w[1].size for w in want] == cnt.tolist()
