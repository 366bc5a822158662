"""Seeded differential tests of the device window calls against the host's
statements of their rules: val_frame_unpack_batch_dev and
val_frame_unpack_files_dev against wire.frame_accept with
vc.fold_payload_states_at, val_frame_scan_streams_dev against wire.scan_frames,
val_frame_fill_files_dev against wire.fill_window, val_frame_data_batch_dev
against wire.build_data_batch, and a chain of fill, scan and unpack against the
files it started from.

Expected values never come from a device path. The generators only shape the
inputs (they keep a notional file position, no more); what a call must leave
is computed by the helpers of the directed test modules, from the host rules
and the oracle. Each function also asserts, from the reference results alone,
that its rounds reached the cases it is there for, so a generator that drifts
into windows where nothing happens fails the test.

Seeded: every assertion message names the seed, the round and its shape.
FUZZ_SEED reseeds; FUZZ_WINDOW_ROUNDS scales the rounds of every function (at
the default of 20 each runs its *_SHARE rounds, at 40 twice as many). The
shares are set so that a function takes a second or two on an MI355X."""
import contextlib
import os

import numpy as np
import pytest

from tests import _oracle, _prng
from tests.test_gpu_fill import LANES, T, _fill
from tests.test_gpu_pack import Batch, _expected, _spread
from tests.test_gpu_pack import _run as _pack
from tests.test_gpu_scan import _cat, _decoy, _f, _scan
from tests.test_gpu_unpack import (ALL_LANES, CANARY, CTRL, File, Window, _d8, _d32, _d64, _expect, _frame, _same,
                                   vc, wire)  # noqa: F401 - vc and wire are fixtures
from tests.test_gpu_unpack_files import Files

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("FUZZ_SEED", "20261020"))
DEFAULT_ROUNDS = 20
ROUNDS = int(os.environ.get("FUZZ_WINDOW_ROUNDS", str(DEFAULT_ROUNDS)))
U64 = (1 << 64) - 1


def _rounds(share):
    """A function's rounds: `share` at the default FUZZ_WINDOW_ROUNDS, in proportion otherwise."""
    return max(1, ROUNDS * share // DEFAULT_ROUNDS)


def _covered(share):
    """The coverage conditions are stated for the default rounds (or more)."""
    return _rounds(share) >= share


@contextlib.contextmanager
def _case(what):
    """Every assertion of the helpers, with the round's seed and shape in front."""
    try:
        yield
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from e


# ---- the receiver's frames --------------------------------------------------------------------------
_POOL = _prng.prng_bytes(0xF022, 8192)


def _bytes_at(p, n, other=False):
    """The file's bytes [p, p + n) (`other`: bytes that differ from them)."""
    at = (p + (1777 if other else 0)) % 4096
    return _POOL[at:at + n]


KINDS = ("explicit", "implied", "gap", "stale", "duplicate", "corrupt", "control", "short", "empty", "goback", "loss")
WEIGHTS = np.array([28, 24, 6, 5, 4, 4, 4, 3, 5, 4, 4], dtype=np.float64)
CLEAN = ("explicit", "implied", "empty", "control")  # kinds that never make a DATA frame that is not accepted


def _order_frames(rng, wire, n, w0, clean_until=None):
    """n frames of one transfer whose receiver stands at w0 -> (frames, the notional end). With
    clean_until, frames before that index are in order and the frame at it announces a gap."""
    frames, hist, pos = [], [], w0

    def size():
        return int(rng.integers(0, 25)) if rng.random() < 0.93 else int(rng.integers(25, 301))

    def in_order(explicit, L):
        nonlocal pos
        f = _frame(wire, _bytes_at(pos, L), pos if explicit else None)
        hist.append((pos, L, f))
        frames.append(f)
        pos += L

    while len(frames) < n:
        if clean_until is not None and len(frames) <= clean_until:
            kind = "gap" if len(frames) == clean_until else CLEAN[int(rng.integers(0, len(CLEAN)))]
        else:
            kind = KINDS[int(rng.choice(len(KINDS), p=WEIGHTS / WEIGHTS.sum()))]
        L = size()
        if kind in ("explicit", "implied"):
            in_order(kind == "explicit", L)
        elif kind == "empty":
            in_order(bool(rng.integers(0, 2)), 0)
        elif kind == "gap":
            frames.append(_frame(wire, _bytes_at(pos, L), pos + int(rng.integers(1, 2000))))
        elif kind == "stale":  # an offset below the position, a valid trailer, other bytes
            if pos:
                at = int(rng.integers(max(0, pos - 300), pos))
                frames.append(_frame(wire, _bytes_at(at, L, other=True), at))
        elif kind == "duplicate":  # a frame that was sent before, byte for byte
            if hist:
                _, Lh, f = hist[int(rng.integers(0, len(hist)))]
                frames.append(f)
                if not f[1] & 1:  # an implied frame lands wherever the receiver stands
                    pos += Lh
        elif kind == "corrupt":
            frames.append(_frame(wire, _bytes_at(pos, L), pos if rng.integers(0, 2) else None, corrupt=True))
        elif kind == "control":
            frames.append(_frame(wire, _bytes_at(pos, L), pos if rng.integers(0, 2) else None, ptype=CTRL))
        elif kind == "short":  # DATA that announces an offset and has no room for it
            frames.append(_frame(wire, _bytes_at(pos, int(rng.integers(0, 8))), flags=1))
        elif kind == "goback":  # the last k frames again, the first of them with its offset
            k = int(rng.integers(1, 7))
            for i, (at, Lh, f) in enumerate(hist[-k:]):
                if i == 0:
                    frames.append(_frame(wire, _bytes_at(at, Lh), at))
                else:
                    frames.append(f)
                    if not f[1] & 1:  # an implied frame lands wherever the receiver stands
                        pos += Lh
        else:  # a lost frame, what the sender sent behind it, then all of it again from the lost one
            g = [size() for _ in range(int(rng.integers(0, 6)))]
            L = max(L, 1)  # (an empty lost frame would leave the frame behind it in order)
            frames.append(_frame(wire, _bytes_at(pos, L), pos, corrupt=True))
            at = pos + L
            for Lg in g:
                frames.append(_frame(wire, _bytes_at(at, Lg), at))
                at += Lg
            in_order(True, L)
            for Lg in g:
                in_order(bool(rng.integers(0, 3) == 0), Lg)
    return frames[:n], pos


def _window_n(rng):
    r = rng.random()
    if r < 0.25:
        return int(rng.integers(1020, 1031))
    if r < 0.45:
        return int(rng.integers(2040, 2061))
    return int(rng.integers(1, 2301))


def _order_round(rng, vc, wire):
    """One window and what the host's rule makes of it -> (win, size, w0, state, cap, want, stats)."""
    n = _window_n(rng)
    w0 = int(rng.integers(0, 4))
    state = int(rng.integers(0, 1 << 32))
    clean_until = int(rng.choice([1023, 1024])) if n > 1030 and rng.random() < 0.3 else None
    frames, end = _order_frames(rng, wire, n, w0, clean_until)
    size = end + 40
    cap = None
    if clean_until is None and end > w0 and rng.random() < 0.6:
        cap = int(rng.integers(w0, end + 1))  # a cut inside the delivered range
    win = Window(frames, phase=rng.integers(0, 4, n))
    want = _expect(vc, wire, win.stream, win.off, win.len, size, w0, state, cap)
    # what this window reached, from the reference's results alone
    fo = wire.data_offsets(win.stream, win.off, win.len)
    pl = wire.payload_lens(win.stream, win.off, win.len)
    acc = want["accept"].astype(bool)
    cand = (want["ok"] != 0) & (fo != wire.OFFSET_NOT_DATA)
    miss = np.flatnonzero(cand & ~acc)
    # the first overflow: replay the accepted prefix to find where `written` stood at each frame
    w_at = w0 + np.concatenate([[0], np.cumsum(np.where(acc, pl, 0).astype(np.uint64))[:-1]]).astype(np.uint64)
    limit = size if cap is None else cap
    ovf = cand & ~acc & ((fo == wire.OFFSET_IMPLIED) | (fo == w_at)) & (w_at + pl > limit)
    first_ovf = int(np.flatnonzero(ovf)[0]) if ovf.any() else None
    assert int(ovf.sum()) == want["novf"]
    stats = dict(rate=float(acc.mean()), novf=want["novf"],
                 after=first_ovf is not None and bool(acc[first_ovf:].any()),
                 first_break=int(miss[0]) if miss.size else None)
    return win, size, w0, state, cap, want, stats


def _order_coverage(stats, what):
    n = len(stats)
    mid = sum(0.1 <= s["rate"] <= 0.9 for s in stats)
    assert 2 * mid >= n, (what, "rounds that accept 10% to 90% of their frames", mid, n)
    ovf = sum(s["novf"] > 0 and s["after"] for s in stats)
    assert 5 * ovf >= n, (what, "rounds with an overflow and an accept behind it", ovf, n)
    edge = sum(s["first_break"] in (1023, 1024) for s in stats)
    assert edge >= 1, (what, "rounds whose first break is at frame 1,023 or 1,024", edge)


ORDER_SHARE = 160


def test_fuzz_ordering(vc, wire):
    """unpack_data_batch_dev against _expect: windows of 1 to 2,300 frames of every kind a
    receiver may see, with and without a capacity inside the delivered range."""
    rng = np.random.default_rng(SEED)
    stats = []
    for r in range(_rounds(ORDER_SHARE)):
        win, size, w0, state, cap, want, st = _order_round(rng, vc, wire)
        stats.append(st)
        base, off, length = _d8(win.stream), _d64(win.off), _d32(win.len)
        for lanes in (0, int(rng.choice(ALL_LANES))):
            hint = int(rng.choice([0, 24]))
            case = f"seed {SEED} round {r} n={win.n} written={w0} cap={cap} lanes={lanes} len_hint={hint}"
            f = File(size, w0, state)
            vc.set_lanes_per_frame(lanes)
            try:
                f.unpack(wire, base, off, length, cap=cap, len_hint=hint)
                got = f.result()
            finally:
                vc.set_lanes_per_frame(0)
            with _case(case):
                _same(got, want)
    print(f"ordering: {len(stats)} rounds, {sum(s['novf'] > 0 for s in stats)} with overflows, first breaks at "
          f"1,023 / 1,024 in {sum(s['first_break'] in (1023, 1024) for s in stats)}", flush=True)
    if _covered(ORDER_SHARE):
        _order_coverage(stats, f"seed {SEED}")


# ---- the same windows, many files in one call ---------------------------------------------------------
FILES_SHARE = 96


def _files_round(rng, vc, wire, r):
    """1 to 40 files, some of them empty; in one round of four one file has more than 1,024
    frames -> (win, first, lay arguments, per-file expectations)."""
    S = int(rng.integers(1, 41))
    counts = [0 if rng.random() < 0.15 else int(rng.integers(1, 120)) for _ in range(S)]
    if r % 4 == 0:
        counts[int(rng.integers(0, S))] = int(rng.integers(1025, 1400))
    frames, first, per = [], [0], []
    for s in range(S):
        w0 = int(rng.integers(0, 4))
        f, end = _order_frames(rng, wire, counts[s], w0) if counts[s] else ([], w0)
        cap = int(rng.integers(w0, end + 1)) if end > w0 and rng.random() < 0.5 else end + 7
        per.append(dict(w0=w0, state=int(rng.integers(0, 1 << 32)), size=end + 7 + int(rng.integers(0, 30)), cap=cap))
        frames += f
        first.append(len(frames))
    loose, _ = _order_frames(rng, wire, int(rng.integers(0, 4)), 0)  # frames behind the last file: nobody's
    win = Window(frames + loose, phase=rng.integers(0, 4, len(frames) + len(loose))) if frames or loose else None
    return S, win, first, per


def test_fuzz_ordering_files(vc, wire):
    """unpack_data_files_dev: every file's result is _expect on its frames alone, and no byte
    outside the files changes."""
    rng = np.random.default_rng(SEED + 1)
    big = 0
    for r in range(_rounds(FILES_SHARE)):
        S, win, first, per = _files_round(rng, vc, wire, r)
        if win is None:
            continue
        big += max(b - a for a, b in zip(first[:-1], first[1:])) > 1024
        lay = Files([p["size"] for p in per], written=[p["w0"] for p in per], state=[p["state"] for p in per],
                    caps=[p["cap"] for p in per], phase=rng.integers(0, 4, S), guard=int(rng.integers(5, 30)))
        hint = int(rng.choice([0, 24]))
        case = f"seed {SEED + 1} round {r} files={S} n={win.n} first={first[:6]} len_hint={hint}"
        lay.unpack(wire, _d8(win.stream), first, _d64(win.off), _d32(win.len), len_hint=hint)
        got = lay.result()
        ok, nbad = _oracle.verify_frames(win.stream, win.off, win.len, nthreads=8)
        with _case(case):
            assert got["nbad"] == nbad and np.array_equal(got["ok"], ok)
            blank = np.ones(lay.total, dtype=bool)
            for s, p in enumerate(per):
                lo, hi, at = first[s], first[s + 1], int(lay.pos[s])
                blank[at:at + p["size"]] = False
                mine = dict(file=got["canvas"][at:at + p["size"]], written=int(got["written"][s]),
                            state=int(got["state"][s]), ok=got["ok"][lo:hi], accept=got["accept"][lo:hi],
                            nbad=int(got["fnbad"][s]), nacc=int(got["nacc"][s]), novf=int(got["novf"][s]))
                if lo == hi:
                    assert (mine["file"] == CANARY).all(), s
                    assert (mine["written"], mine["state"], mine["nbad"], mine["nacc"], mine["novf"]) == \
                        (p["w0"], p["state"], 0, 0, 0), s
                    continue
                want = _expect(vc, wire, win.stream, win.off[lo:hi], win.len[lo:hi], p["size"], p["w0"], p["state"],
                               p["cap"])
                with _case(f"file {s} frames {lo}..{hi}"):
                    _same(mine, want)
            assert (got["canvas"][blank] == CANARY).all() and not got["accept"][first[-1]:].any()
    print(f"ordering, files: {_rounds(FILES_SHARE)} rounds, {big} with a file of more than 1,024 frames", flush=True)
    if _covered(FILES_SHARE):
        assert 4 * big >= _rounds(FILES_SHARE), ("rounds with a file of more than 1,024 frames", big)


# ---- scan -----------------------------------------------------------------------------------------
SCAN_SHARE = 400
RUNS = ((1, 6), (60, 71), (250, 261), (315, 326))


def _scan_round(rng, wire, r, pool):
    """1 to 12 streams of runs -> (streams, mtu, max_frames)."""
    def frame(c):
        if c not in pool:
            pool[c] = _f(wire, c)
        return pool[c]

    mtu = int(rng.choice([1024, 3100]))
    streams, counts = [], []
    S = int(rng.integers(1, 13))
    long_at = int(rng.integers(0, S)) if r % 3 == 0 else None  # once per few rounds: a run of 1,340 to 1,350
    for s in range(S):
        parts, stopped = [], False
        for k in range(int(rng.integers(1, 6))):
            c = int(rng.integers(0, 41)) if rng.random() < 0.7 else int(rng.integers(1000, 1013))
            lo, hi = RUNS[int(rng.integers(0, len(RUNS) if c < 1000 else 2))]  # long runs of small frames only
            run = int(rng.integers(lo, hi))
            if s == long_at and k == 0:
                run, c = int(rng.integers(1340, 1351)), int(rng.integers(0, 41))
            parts += [frame(c)] * run
            P = 12 + c
            if rng.random() < 0.3:  # a frame of 2P or 3P whose payload reads as headers of P where the lanes look
                mult = int(rng.integers(2, 4))
                parts.append(_f(wire, mult * P - 12, _decoy(P, mult)))
            if rng.random() < 0.08:  # a frame over the MTU, and frames behind it that nobody may see
                parts += [frame(mtu - 11), frame(c)]
        full = _cat(parts)
        ln = full.size
        if rng.random() < 0.3:  # a cut at a random byte of the last frame
            ln -= int(rng.integers(1, parts[-1].size + 1))
        streams.append((full, ln))
        counts.append(len(parts))
    max_frames = max(counts) + 5
    if rng.random() < 0.3:
        max_frames = int(rng.integers(1, max(counts) + 1))
    return streams, mtu, max_frames


def _scan_stats(vc, want, streams, max_frames):
    """Which ends the host's results hold, and its longest run of equal sizes."""
    out = dict(clean=0, cut=0, protocol=0, longest=0)
    for (st, off, ln, used), (full, slen) in zip(want, streams):
        if st == vc.VAL_ERR_PROTOCOL:
            out["protocol"] += 1
        elif used == slen:
            out["clean"] += 1
        elif off.size < max_frames:
            out["cut"] += 1  # bytes of a frame that has not arrived in full
        if ln.size:
            edges = np.flatnonzero(np.diff(ln) != 0)
            runs = np.diff(np.concatenate([[-1], edges, [ln.size - 1]]))
            out["longest"] = max(out["longest"], int(runs.max()))
    return out


def _scan_coverage(stats, what):
    for k in ("clean", "cut", "protocol"):
        assert sum(s[k] for s in stats) >= 1, (what, "streams that end with", k)
    full = sum(s["longest"] >= 1345 for s in stats)
    assert full >= 1, (what, "rounds with a run of 1,345 frames or more: a full 1,024-lane match", full)


def test_fuzz_scan(vc, wire):
    """scan_streams_dev against wire.scan_frames through _scan (the three fronts, the four
    phases): runs on either side of the fronts' widths, decoys, frames over the MTU, cuts,
    frame limits below the count."""
    rng = np.random.default_rng(SEED + 2)
    stats, pool = [], {}
    for r in range(_rounds(SCAN_SHARE)):
        streams, mtu, max_frames = _scan_round(rng, wire, r, pool)
        case = (f"seed {SEED + 2} round {r} streams={len(streams)} mtu={mtu} max_frames={max_frames} "
                f"len={[ln for _, ln in streams][:6]}")
        with _case(case):
            want = _scan(vc, wire, streams, mtu, max_frames)
        stats.append(_scan_stats(vc, want, streams, max_frames))
    print(f"scan: {len(stats)} rounds, streams that end clean / cut / on a protocol error: "
          f"{[sum(s[k] for s in stats) for k in ('clean', 'cut', 'protocol')]}, "
          f"{sum(s['longest'] >= 1345 for s in stats)} rounds with a full 1,024-lane match", flush=True)
    if _covered(SCAN_SHARE):
        _scan_coverage(stats, f"seed {SEED + 2}")


# ---- fill -----------------------------------------------------------------------------------------
FILL_SHARE = 400
FILL_MTUS = (21, 29, 112, 1024, 4096, 65547)


def _fill_round(rng, wire):
    """1 to 200 transfers in random states -> (specs, mtu, max_frames)."""
    mtu = int(rng.choice(FILL_MTUS))
    M = mtu - 12
    if mtu >= 4096:  # file data stays small: at most three frames per transfer, and few transfers
        max_frames, S = int(rng.integers(1, 4)), int(rng.integers(1, 40 if mtu == 4096 else 7))
    else:
        max_frames, S = int(rng.integers(1, 13)), int(rng.integers(1, 201))
    pool = _prng.prng_bytes(int(rng.integers(1 << 30)), 1 << 16)
    specs = []
    for s in range(S):
        virt = (1 << 33) if rng.random() < 0.15 else 0
        pre = int(rng.integers(0, 60))
        left = int(rng.integers(0, (max_frames + 2) * M)) if rng.random() < 0.8 else int(rng.integers(0, M + 2))
        if mtu >= 4096:
            left = min(left, 3 * M)
        at = int(rng.integers(0, 4096)) if pre + left < 60000 else 0
        data = np.resize(pool[at:], pre + left) if pre + left > pool.size - at else pool[at:at + pre + left]
        nxt = virt + pre
        r = rng.random()
        if r < 0.08:
            nxt = virt + pre + left + int(rng.integers(0, 3))  # at or beyond the size
        r = rng.random()
        j = int(rng.integers(0, 7))
        if r < 0.2:
            la = nxt - int(rng.integers(1, pre + 1)) if pre else nxt
        elif r < 0.5:
            la = nxt
        elif r < 0.8:
            la = nxt + j * M
        else:
            la = max(0, nxt + j * M + int(rng.choice([-1, 1])))
        budget = int(rng.integers(0, max_frames + 3))
        r = rng.random()
        cap = U64
        if r < 0.35:
            cap = max(0, int(rng.integers(0, max_frames + 2)) * mtu + int(rng.choice([0, -1, 11, 12, 20])))
        elif r < 0.55:  # the exact size of what the rule makes without a limit, a byte less, a byte more
            used = wire.fill_window(nxt, la, virt + data.size, mtu, min(budget, max_frames))[5]
            cap = max(0, used + int(rng.choice([-1, 0, 1])))
        specs.append(T(data, next=nxt, la=la, budget=budget, cap=cap, virt=virt))
    return specs, mtu, max_frames


def _fill_stats(wire, specs, mtu, max_frames):
    out = dict(capacity=0, budget=0, ends=0, je=0)
    for t in specs:
        eff = min(t["budget"], max_frames)
        fo, pl, inc, off, cl, used, nxt = wire.fill_window(t["next"], t["la"], t["size"], mtu, eff, t["cap"])
        if t["next"] >= t["size"] or eff == 0:
            continue
        free = wire.fill_window(t["next"], t["la"], t["size"], mtu, eff)[0].size  # without the capacity
        out["capacity"] += fo.size < free
        out["budget"] += fo.size == eff and nxt < t["size"]
        out["ends"] += fo.size > 0 and nxt == t["size"]
        out["je"] += bool(inc[1:].any())
    return out


def _fill_coverage(stats, what):
    for k, name in (("capacity", "cut by the capacity"), ("budget", "cut by the budget"),
                    ("ends", "a file that ends in the window"), ("je", "an explicit frame behind the first")):
        assert sum(s[k] for s in stats) >= 1, (what, "transfers with", name)


def test_fuzz_fill(vc, wire):
    """fill_files_dev against wire.fill_window and the host framer through _fill: every MTU
    class, last_acked behind, at and ahead of next (on a frame start and a byte off it),
    budgets and capacities around the frame ends."""
    rng = np.random.default_rng(SEED + 3)
    stats = []
    for r in range(_rounds(FILL_SHARE)):
        specs, mtu, max_frames = _fill_round(rng, wire)
        stats.append(_fill_stats(wire, specs, mtu, max_frames))
        case = f"seed {SEED + 3} round {r} transfers={len(specs)} mtu={mtu} max_frames={max_frames}"
        with _case(case):
            _fill(vc, wire, specs, mtu, max_frames, phases=(0, 1, 2, 3) if len(specs) < 4 else (0,), lanes=LANES)
    print(f"fill: {len(stats)} rounds, transfers cut by the capacity / by the budget / ending / explicit behind "
          f"the first: {[sum(s[k] for s in stats) for k in ('capacity', 'budget', 'ends', 'je')]}", flush=True)
    if _covered(FILL_SHARE):
        _fill_coverage(stats, f"seed {SEED + 3}")


# ---- the framer -------------------------------------------------------------------------------------
PACK_SHARE = 400


def _pack_round(rng):
    """A batch for val_frame_data_batch_dev -> (payload, pay_off, pay_len, file_off, inc, stride or 0)."""
    n = int(rng.integers(1, 400))
    slot = rng.random() < 0.4
    stride = int(rng.choice([12, 33, 112, 1024, 1031])) if slot else 0
    most = stride - 12 if slot else 65535  # the largest content that fits
    inc = rng.integers(0, 2, n).astype(np.uint8)
    pay_len = rng.integers(0, min(most, 300) + 1, n).astype(np.int64)
    edge = rng.random(n)
    room = most - 8 * inc.astype(np.int64)  # the largest payload the call takes
    pay_len = np.where(edge < 0.05, 0, pay_len)
    if slot or rng.random() < 0.5:  # (without slots: two of these are 128 KiB of payload)
        few = rng.choice(n, min(n, 8 if slot else 2), replace=False)
        pay_len[few] = room[few]
        few = rng.choice(n, min(n, 8 if slot else 2), replace=False)
        pay_len[few] = room[few] + rng.integers(1, 3, few.size)  # one and two bytes too many: rejected
    pay_len = np.maximum(pay_len, 0).astype(np.uint32)
    gaps = rng.integers(0, 5, n)
    pay_off = (np.cumsum(pay_len.astype(np.int64) + gaps) - pay_len).astype(np.uint64)
    payload = _prng.prng_bytes(int(rng.integers(1 << 30)), int(pay_off[-1]) + int(pay_len[-1]) + 8)
    file_off = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    return payload, pay_off, pay_len, file_off, inc, stride


def test_fuzz_framer(vc, wire):
    """build_data_batch_dev against the host framer with the oracle's CRCs on a whole 0xA5
    canvas, in descriptor and slot mode: payloads of 0 bytes, of the most a frame or a slot
    holds, and of a byte or two more, which the call must reject and count."""
    rng = np.random.default_rng(SEED + 4)
    modes, rejected, largest = set(), 0, 0
    for r in range(_rounds(PACK_SHARE)):
        payload, pay_off, pay_len, file_off, inc, stride = _pack_round(rng)
        n = pay_len.size
        content = pay_len.astype(np.int64) + 8 * inc
        good = np.flatnonzero(content <= (stride - 12 if stride else 65535))
        if stride:
            frame_off, size = np.arange(n, dtype=np.uint64) * np.uint64(stride), n * stride
        else:
            frame_off, size = _spread(pay_len, inc, rng.integers(0, 4, n))
        lanes = int(rng.choice((0, 0) + ALL_LANES))
        hint = int(rng.choice([0, 0, 1020, 8 + 65535]))
        case = (f"seed {SEED + 4} round {r} n={n} stride={stride} lanes={lanes} len_hint={hint} "
                f"pay_len {int(pay_len.min())}..{int(pay_len.max())} rejected={n - good.size}")
        modes.add(bool(stride))
        rejected += n - good.size
        largest = max(largest, int(content[good].max()) if good.size else 0)
        if good.size:
            want, w_cl, w_crc, w_hdr = _expected(wire, payload, pay_off[good], pay_len[good], file_off[good],
                                                 inc[good], frame_off[good], size)
        else:
            want, w_cl, w_crc, w_hdr = np.full(size, CANARY, np.uint8), *(np.zeros(0, np.uint32),) * 3
        b = Batch(payload, pay_off, pay_len, file_off, inc)
        vc.set_lanes_per_frame(lanes)
        try:
            got, cl, crc, hdr, nrej = _pack(wire, b, size, None if stride else frame_off, out_stride=stride,
                                           len_hint=hint)
        finally:
            vc.set_lanes_per_frame(0)
        with _case(case):
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, ("first differing byte", int(bad[0]))
            assert nrej == n - good.size
            for name, out, w in (("crc_len", cl, w_cl), ("crc", crc, w_crc), ("hdr", hdr, w_hdr)):
                full = np.zeros(n, np.uint32)
                full[good] = w
                assert np.array_equal(out, full), name
    print(f"framer: {_rounds(PACK_SHARE)} rounds, {rejected} frames rejected, largest content {largest}", flush=True)
    if _covered(PACK_SHARE):
        assert modes == {False, True} and rejected > 0 and largest == 65535, (modes, rejected, largest)


# ---- fill -> scan -> unpack, window after window, nothing read back ----------------------------------
CHAIN_SHARE = 120
LOSSY = 3  # windows of which only a prefix arrives


def test_fuzz_chain(vc, wire):
    """Random files go from one device buffer into another through fill, scan and unpack,
    window after window on a side stream, as in test_gpu_fill's round trip. Loss is a prefix:
    in the first LOSSY windows the scan sees torch.minimum(stream_len, cut) bytes of every
    stream, with cuts uploaded before the loop, so frames that did not arrive are not scanned
    and nothing is misplaced. After every window last_acked and next are device copies of
    `written` (every window begins with an explicit frame). A clean window moves every
    unfinished transfer by max_frames * M - 8 bytes or to its end, so the clean windows needed
    when the lossy ones delivered nothing are known from constants."""
    rng = np.random.default_rng(SEED + 5)
    for r in range(_rounds(CHAIN_SHARE)):
        S, mtu, max_frames = int(rng.integers(2, 9)), int(rng.choice([112, 1024])), int(rng.integers(2, 10))
        Mx = mtu - 12
        sizes = [int(rng.integers(0, 60 * Mx)) if rng.random() < 0.85 else int(rng.integers(0, 3)) for _ in range(S)]
        case = f"seed {SEED + 5} round {r} files={S} mtu={mtu} max_frames={max_frames} sizes={sizes}"
        data = [_prng.prng_bytes(1000 * r + s, n) for s, n in enumerate(sizes)]
        fpos = np.cumsum([2] + [n + 3 for n in sizes[:-1]])
        files = _prng.prng_bytes(59 + r, int(fpos[-1]) + sizes[-1] + 8)
        for o, d in zip(fpos, data):
            files[o:o + d.size] = d
        d_files, d_fpos, d_size = _d8(files), _d64(fpos), _d64(sizes)
        room = max_frames * mtu
        soff = [1 + s * (room + 1) for s in range(S)]
        out = torch.zeros(soff[-1] + room + 8, dtype=torch.uint8, device="cuda:0")
        d_soff, d_cap = _d64(soff), _d64([room] * S)
        d_next, d_la = _d64([0] * S), _d64([0] * S)
        cuts = [_d64(rng.integers(0, room + 1, S)) for _ in range(LOSSY)]
        lay = Files(sizes, phase=rng.integers(0, 4, S))
        per_window = max_frames * Mx - 8
        windows = LOSSY + max(-(-n // per_window) for n in sizes)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for w in range(windows):
                f = wire.fill_files_dev(d_files, d_fpos, d_size, d_next, d_la, mtu, max_frames, out=out,
                                        stream_off=d_soff, stream_cap=d_cap, stream=side)
                arrived = torch.minimum(f[5], cuts[w]) if w < LOSSY else f[5]
                foff, clen, first, *_ = wire.scan_streams_dev(out, d_soff, arrived, mtu, max_frames, stream=side)
                wire.unpack_data_files_dev(out, first=first, file_ptr=lay.ptr, file_cap=lay.cap, written=lay.written,
                                           off=foff, length=clen, n=S * max_frames, len_hint=mtu - 4,
                                           file_state=lay.state, naccepted=lay.nacc, noverflow=lay.novf,
                                           file_nbad=lay.fnbad, nbad=None, stream=side)
                d_la.copy_(lay.written)  # the ACK
                d_next.copy_(lay.written)  # and the sender goes on from it
        side.synchronize()
        canvas = lay.canvas.cpu().numpy()
        written = lay.written.cpu().numpy().view(np.uint64)
        state = lay.state.cpu().numpy().view(np.uint32)
        with _case(case):
            blank = np.ones(lay.total, dtype=bool)
            for s in range(S):
                at = int(lay.pos[s])
                assert np.array_equal(canvas[at:at + sizes[s]], data[s]), s
                blank[at:at + sizes[s]] = False
            assert (canvas[blank] == CANARY).all()
            assert written.tolist() == sizes
            assert state.tolist() == [_oracle.update_state(0xFFFFFFFF, d) for d in data]
            assert not lay.fnbad.cpu().numpy().any() and not lay.novf.cpu().numpy().any()
            assert np.array_equal(d_next.cpu().numpy().view(np.uint64), sizes)
