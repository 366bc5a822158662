"""Seeded differential tests of val_frame_respond_files_dev and
val_frame_apply_acks_files_dev against the host's statements of their rules
(val_frame_respond_window with val_frame_put_response and val_frame_accept;
val_frame_apply_acks with val_frame_ack_offsets), in the manner of
tests/test_gpu_file_windows_fuzz.py.

Expected values never come from a device path: every round goes through
tests/test_gpu_acks.py's Receiver (the whole response canvas, the lengths, the
counts, since, and with delivery the unpack call's verdicts and positions) or
its _apply_case, and tests/test_gpu_acks_edges.py's _apply for strided slots.
The generators only shape the inputs. Each function asserts, from the
reference side and the planner alone, that its rounds reached the cases it is
there for.

Seeded: every assertion message names the seed, the round and its shape.
FUZZ_SEED reseeds; FUZZ_WINDOW_ROUNDS scales the rounds (at the default of 20
each function runs its *_SHARE rounds). The shares, RESPOND_SHARE = 36 and
APPLY_SHARE = 48, keep a function's host model plus device time at a second or
two on an MI355X."""
import numpy as np
import pytest

from tests.test_ack_rules import ACK, NAK
from tests.test_gpu_acks import U64, Receiver, _apply_case, _cus
from tests.test_gpu_acks_edges import _apply, _laid, _resp
from tests.test_gpu_unpack import vc, wire  # noqa: F401 - fixtures
from tests.test_gpu_window_fuzz import SEED, _case, _covered, _rounds

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BIG = 1 << 40
RESPOND_SHARE = 36
APPLY_SHARE = 48
STRIDES = (0, 1, 2, 7, 64, 1000)
CAPS = ("fit", "short", 0, 11, "big")


def fuzz_frames(rng, count, w0, *, fixed=None, implied=0.0):
    """count frames of one transfer whose receiver stands at w0, drawn with numpy: in order (a share
    of them without an offset), duplicates, gaps, corrupt and control frames, against a notional
    position that ignores the capacity. fixed: every payload that long (strided slots)."""
    ln = rng.integers(0, 24, count) if fixed is None else np.full(count, fixed)
    kind = rng.choice(5, count, p=[0.6, 0.1, 0.1, 0.1, 0.1])  # in order, duplicate, gap, corrupt, control
    moves = kind == 0
    before = w0 + np.cumsum(np.where(moves, ln, 0)) - np.where(moves, ln, 0)
    d = rng.integers(1, 50, count)
    fo = np.where(kind == 1, np.maximum(0, before - d), np.where(kind == 2, before + d, before))
    fl = np.where(kind == 3, "x", np.where(kind == 4, "c", "d"))
    if implied:
        fl = np.where(moves & (rng.random(count) < implied), "i", fl)
    return fo.tolist(), ln.tolist(), fl.tolist()


def _counts(rng, S, grid, long_ok=True):
    """Frames per file: empty, tiny, around 256, around 1,024, and in most rounds one long file. Calls
    of more files than workgroups are tiny files with one or two multi-chunk files whose workgroup
    takes another file with frames."""
    if S > grid:
        c = rng.integers(0, 4, S)
        extra = S - grid
        for s in rng.choice(extra, min(extra, 2), replace=False):
            c[s] = int(rng.choice([1025, 1030, 2049, 300]))
            c[s + grid] = max(int(c[s + grid]), 1)
        return c
    pick = (lambda: 0, lambda: int(rng.integers(1, 4)), lambda: int(rng.integers(250, 263)),
            lambda: int(rng.integers(1020, 1031)))
    c = np.array([pick[int(rng.choice(4, p=[0.15, 0.45, 0.25, 0.15]))]() for _ in range(S)])
    if long_ok and rng.random() < 0.6:
        c[int(rng.integers(0, S))] = int(rng.integers(1100, 5300))
    return c


def _shares_a_long_file(counts, grid, block):
    """A workgroup of a grid-stride loop takes two files with frames, one of them of several chunks."""
    c = np.asarray(counts)
    if c.size <= grid:
        return False
    a, b = c[:c.size - grid], c[grid:]
    return bool((((a > block) & (b > 0)) | ((b > block) & (a > 0))).any())


def test_fuzz_respond(vc, wire):
    """RESPOND_SHARE = 36 rounds of one or two chained windows: 1, a few or more files than workgroups;
    counts as _counts draws them; unowned padding; descriptors or strided slots; with delivery or on
    the host rule's accepted set (then some receivers stand around 2^32); strides 0, 1, 2, 7, 64 and
    1,000 with a random since; totals near the files' positions; capacities fit, short, 0, 11, big."""
    cus = _cus()
    rng = np.random.default_rng(SEED + 40)
    lanes_seen, sizes_seen, shared, dropped, silent, completed = set(), set(), 0, 0, 0, 0
    for r in range(_rounds(RESPOND_SHARE)):
        many = r % 8 == 3  # every eighth round: more files than workgroups, in either workgroup size in turn
        want_small = bool((r // 8) % 2) if many else bool(rng.integers(0, 2))
        grid_of = cus * (8 if want_small else 1)
        u = 0.9 if many else 0.8 * rng.random()
        S = 1 if u < 0.15 else int(rng.integers(2, 13)) if u < 0.8 else grid_of + int(rng.integers(1, 40))
        strided = 0 if S > 12 or rng.random() < 0.7 else int(rng.integers(0, 24))
        deliver = bool(rng.random() < 0.6)
        counts = _counts(rng, S, grid_of)
        if not counts.any():
            counts[0] = 5
        n = int(counts.sum())
        n_pad = 0
        if strided == 0:
            n_pad = int(rng.integers(0, 50))
            if not want_small and n // S <= 256 and S > 12:
                n_pad = 257 * S - n
        plan = vc.plan_ack_calls(vc.ACK_RESPOND, cus, n + n_pad, S)[1]
        lanes, grid = int(plan.lanes), int(plan.grid)
        stride = int(rng.choice(STRIDES))
        since = [int(rng.choice([0, 1, max(stride - 1, 0), stride, stride + 5, (1 << 32) - 1])) for _ in range(S)]
        high = (not deliver) and rng.random() < 0.6
        w0 = [int((1 << 32) - rng.integers(0, 300)) if high and rng.random() < 0.5 else int(rng.integers(0, 2000))
              for _ in range(S)]
        windows = int(rng.integers(1, 3))
        fixed = int(rng.integers(0, 24)) if strided else None
        room = [w + (fixed if strided else 12) * int(c) * windows for w, c in zip(w0, counts)]  # about twice the bytes
        total = [int(rng.integers(w, t + 1)) if rng.random() < 0.4 else BIG for w, t in zip(w0, room)]
        if deliver:
            cap = [int(rng.integers(w, t + 1)) if rng.random() < 0.3 else t + 8 for w, t in zip(w0, room)]
        else:
            cap = [int(rng.integers(w, t + 1)) if rng.random() < 0.3 else U64 for w, t in zip(w0, room)]
        case = (f"seed {SEED + 40} round {r} files={S} counts={counts[:8].tolist()} n_pad={n_pad} lanes={lanes} "
                f"grid={grid} strided={strided and 12 + 8 + fixed + strided} deliver={deliver} stride={stride} "
                f"since={since[:6]} windows={windows}")
        rx = Receiver(wire, w0, total, cap, stride, since, deliver=deliver)
        for k in range(windows):
            per_file = [fuzz_frames(rng, int(c), rx.w[s], fixed=fixed, implied=0.0 if strided else 0.3)
                        for s, c in enumerate(counts)]
            caps = [CAPS[int(rng.choice(5, p=[0.2, 0.2, 0.1, 0.1, 0.4]))] for _ in range(S)]
            with _case(f"{case} window {k}"):
                want, _ = rx.window(per_file, 2000 + 10 * r + k, caps, n_pad=n_pad,
                                    strided=strided and 12 + 8 + fixed + strided)
                if deliver:
                    assert np.array_equal(rx.lay.nacc.cpu().numpy().view(np.uint32), rx.nacc)
                    assert np.array_equal(rx.lay.novf.cpu().numpy().view(np.uint32), rx.novf)
            sizes_seen |= {len(x) for rs in want for x in rs}
        lanes_seen.add(lanes)
        shared += _shares_a_long_file(counts, grid, lanes)
        dropped += int(rx.dropped.sum())
        silent += int(rx.novf.sum())
        completed += sum(1 for s in range(S) if rx.nacc[s] and rx.w[s] >= total[s])
    print(f"respond: {_rounds(RESPOND_SHARE)} rounds, workgroup sizes {sorted(lanes_seen)}, {shared} rounds in which a "
          f"workgroup takes a multi-chunk file and another, response sizes {sorted(sizes_seen)}, {dropped} responses "
          f"dropped, {silent} silent refusals, {completed} files completed", flush=True)
    if _covered(RESPOND_SHARE):
        what = f"seed {SEED + 40}"
        assert lanes_seen == {256, 1024}, (what, "both workgroup sizes planned", lanes_seen)
        assert shared >= 2, (what, "rounds in which a workgroup takes two files, one of several chunks", shared)
        assert sizes_seen >= {12, 16, 24}, (what, "response sizes", sizes_seen)
        assert dropped > 0 and silent > 0 and completed > 0, (what, "dropped, silent, completed", dropped, silent,
                                                              completed)


def _strided_apply_round(rng, wire, case):
    """Equal slots: 12-byte ACKs (flen 8), or 16- and 24-byte frames with a high half (flen 12, 20)."""
    flen = int(rng.choice([8, 12, 20]))
    slot = flen + 4 + 4 * int(rng.integers(0, 3))
    S = int(rng.integers(1, 6))
    counts = rng.choice([0, 2, 40, 300, 1100], S)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(first[-1]) + int(rng.integers(0, 5))
    if n == 0:
        return 0, 0
    sizes = [int(rng.integers(0, 1 << 20)) if flen == 8 or rng.random() < 0.3 else int(rng.integers(1 << 32, 1 << 34))
             for _ in range(S)]
    la0 = [int(rng.integers(0, sz + 1)) for sz in sizes]
    nx0 = [la + int(rng.integers(0, sz - la + 1)) for la, sz in zip(la0, sizes)]
    frames = []
    owner = np.searchsorted(first, np.arange(n), side="right") - 1
    for i in range(n):
        sz = sizes[min(int(owner[i]), S - 1)]
        o = int(rng.integers(0, sz + 1 + sz // 8))
        kind = NAK if flen == 20 and rng.random() < 0.2 else ACK
        f = _resp(wire, kind, o if flen > 8 else o & 0xFFFFFFFF, flen - 8, bad=rng.random() < 0.03)
        frames.append(f + bytes(slot - len(f)))
    base, off, _ = _laid(frames, lead=0)
    segs = [(int(a), int(b)) for a, b in zip(first[:-1], first[1:])]
    with _case(f"{case} strided slot={slot} flen={flen} counts={counts.tolist()} n={n}"):
        want = _apply(wire, base, segs, sizes, la0, nx0, first=first.tolist(), n=n, stride=slot, flen=flen,
                      len_hint=flen, nbad0=int(rng.integers(0, 100)))
    return sum(w[2] for w in want), sum(w[3] for w in want)


def test_fuzz_apply(vc, wire):
    """APPLY_SHARE = 48 rounds: 1, a few or more transfers than workgroups with counts as _counts
    draws them, descriptors with padding through _apply_case (file sizes on both sides of 2^32) or
    strided slots of 12, 16 and 24 bytes and more through _apply."""
    cus = _cus()
    rng = np.random.default_rng(SEED + 41)
    shared, retr, bad, idle, high, strided = 0, 0, 0, 0, 0, 0
    for r in range(_rounds(APPLY_SHARE)):
        case = f"seed {SEED + 41} round {r}"
        if rng.random() < 0.3:
            a, b = _strided_apply_round(rng, wire, case)
            retr, bad, strided = retr + a, bad + b, strided + 1
            continue
        u = 0.9 if r % 8 == 3 else 0.8 * rng.random()  # every eighth round: more transfers than workgroups
        S = 1 if u < 0.15 else int(rng.integers(2, 13)) if u < 0.8 else cus + int(rng.integers(1, 40))
        counts = _counts(rng, S, cus).tolist()
        if not any(counts):
            counts[0] = 5
        grid = int(vc.plan_ack_calls(vc.ACK_APPLY, cus, sum(counts), S)[0].grid)
        sizes = [int(rng.integers(0, 50000)) if rng.random() < 0.7 else int(rng.integers(1 << 32, 1 << 33))
                 for _ in range(S)]
        start = {s: (1 << 32) - int(rng.integers(0, 20000)) for s, sz in enumerate(sizes) if sz > 1 << 32}
        n_pad = int(rng.integers(0, 40))
        with _case(f"{case} transfers={S} counts={counts[:8]} n_pad={n_pad} grid={grid} sizes={sizes[:6]}"):
            la0, nx0, la, nx, w_retr, w_bad = _apply_case(wire, counts, sizes, SEED + 1000 + r, n_pad=n_pad, start=start)
        shared += _shares_a_long_file(counts, grid, 1024)
        retr, bad = retr + sum(w_retr), bad + sum(w_bad)
        idle += sum(1 for c, a, b, x, y in zip(counts, la0, nx0, la, nx) if c == 0 and (a, b) == (x, y))
        high += sum(1 for s in start if la[s] > 1 << 32)
    print(f"apply: {_rounds(APPLY_SHARE)} rounds ({strided} strided), {shared} in which a workgroup takes a multi-chunk "
          f"transfer and another, {retr} retransmits, {bad} bad frames, {idle} transfers without frames, {high} "
          f"acknowledged past 2^32", flush=True)
    if _covered(APPLY_SHARE):
        what = f"seed {SEED + 41}"
        assert shared >= 2, (what, "rounds in which a workgroup takes two transfers, one of several chunks", shared)
        assert strided >= 3 and retr > bad > 0 and idle > 0 and high > 0, (what, strided, retr, bad, idle, high)
