"""val_frame_respond_files_dev and val_frame_apply_acks_files_dev where
tests/test_gpu_acks.py does not reach: workgroups that
take a file after a multi-chunk file and a multi-chunk file after another file,
pass 1 of k_ack_respond_files in all four slots and in its second step, ACK
strides above a chunk, a window and near 2^32, implied offsets among corrupt,
control, gap and capacity-refused neighbours, the clauses of the two contracts
that no device test ran, and NAKs through respond -> scan -> apply with nothing
read back.

Expected values never come from a device path: the plain-C rules through
val_protocol_amd.wire (respond_window, put_response, frame_accept, apply_acks,
ack_offsets, scan_frames) over the oracle's trailer verdicts, as in
tests/test_gpu_acks.py, whose Receiver, mixed_frames, _apply_case and
response_stream run here. The shapes, with the plans they must get, are in
tests/_ack_shapes.py; tests/test_ack_shapes.py holds them to 64..304 CUs
without a GPU."""
import numpy as np
import pytest

from tests import _ack_shapes as shp
from tests import _oracle
from tests.test_ack_rules import ACK, NAK
from tests.test_gpu_acks import (U64, Receiver, _apply_case, _cus, _in_order, _u32, _u64,  # noqa: F401
                                 mixed_frames)
from tests.test_gpu_unpack import DEV, _d8, _d32, _d64, vc, wire  # noqa: F401 - vc and wire are fixtures
from tests.test_gpu_unpack_files import _segments

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BIG = 1 << 40
SAT = (1 << 32) - 1


def tiny_files(rng, counts, w0, cap):
    """mixed_frames' flavours for many files of a few frames each, drawn with numpy for all files at
    once (one step per frame index) -> a list of (file_off, pay_len, flavour)."""
    counts = np.asarray(counts, np.int64)
    S, m = counts.size, int(counts.max()) if counts.size else 0
    w, cap = np.array(w0, np.int64), np.asarray(cap, np.int64)
    r, ln, d = rng.random((S, m)), rng.integers(0, 24, (S, m)), rng.integers(1, 50, (S, m))
    fo, fl = np.zeros((S, m), np.int64), np.full((S, m), "d", dtype="<U1")
    for j in range(m):
        rj = r[:, j]
        dup, gap = (rj >= 0.6) & (rj < 0.7), (rj >= 0.7) & (rj < 0.8)
        off = np.where(dup, np.maximum(0, w - d[:, j]), np.where(gap, w + d[:, j], w))
        fl[(rj >= 0.8) & (rj < 0.9), j] = "x"
        fl[rj >= 0.9, j] = "c"
        moves = (j < counts) & ((rj < 0.6) | (dup & (off == w))) & (w + ln[:, j] <= cap)
        fo[:, j] = off
        w = np.where(moves, w + ln[:, j], w)
    return [(fo[s, :c].tolist(), ln[s, :c].tolist(), fl[s, :c].tolist()) for s, c in enumerate(counts.tolist())]


def _counts_match(rx):
    """k_unpack_order_files' per-file counters against val_frame_accept's, over all windows so far."""
    assert np.array_equal(_u32(rx.lay.nacc), rx.nacc) and np.array_equal(_u32(rx.lay.novf), rx.novf)


# ---- 1. workgroups that take several files, long ones among them ------------------------------
@pytest.mark.parametrize("stride", (0, 3))
@pytest.mark.parametrize("lanes", (1024, 256), ids=("workgroups of 1024", "workgroups of 256"))
def test_shared_workgroups_respond(vc, wire, lanes, stride):
    """2 x grid + 3 files of 0..3 frames with long mixed files placed so that one workgroup takes long,
    tiny, long, another tiny, long, empty and a third empty, long, tiny (tests/_ack_shapes.py); two
    chained windows with delivery. In 1,024-thread mode padding entries raise n / n_files above 256.
    k_unpack_order_files runs the same windows in one workgroup per CU, its counters are compared too."""
    cus = _cus()
    counts, n_pad, grid, longs = shp.shared_respond(vc, cus, lanes)
    shp.check_shared(counts, grid, longs, shp.CHUNK[lanes], shp.SHARED_LONG[lanes])
    S = len(counts)
    assert shp.respond_plan(vc, cus, int(counts.sum()) + n_pad, S, lanes) == grid and S == 2 * grid + 3
    rng = np.random.default_rng(300 + stride + lanes)
    w0 = rng.integers(1, 1000, S)
    cap, total = w0 + 50, w0 + rng.integers(0, 60, S)  # tiny files: some fill up, some complete
    order = sorted(longs)
    for s in order:
        cap[s], total[s] = w0[s] + 24 * 2 * longs[s], BIG
    cap[order[1]] = w0[order[1]] + 6 * longs[order[1]]  # one long file runs into its capacity,
    total[order[2]] = w0[order[2]] + 5 * longs[order[2]]  # one completes inside the first window
    rx = Receiver(wire, w0, total, cap, stride, rng.integers(0, 4, S))
    for rnd in range(2):
        per_file = tiny_files(rng, counts, rx.w, cap)
        for s in order:
            per_file[s] = mixed_frames(rng, longs[s], rx.w[s], int(cap[s]))
        rx.window(per_file, 400 + rnd, ["big"] * S, n_pad=n_pad)
        _counts_match(rx)
    assert rx.novf[order[1]] > 100 and rx.w[order[2]] >= total[order[2]]
    assert rx.novf.sum() > rx.novf[order[1]] and 0 < rx.nacc.sum()


def test_shared_workgroups_apply(vc, wire):
    """2 x CUs + 3 transfers of 0..3 responses with 2,049, 1,025, 4,097 and 1,024 placed the same way,
    through _apply_case (nretrans and file_nbad start at canary values and are incremented)."""
    counts, grid, longs = shp.shared_apply(vc, _cus())
    shp.check_shared(counts, grid, longs, 1024, (2049, 1025, 4097, 1024))
    rng = np.random.default_rng(31)
    sizes = rng.integers(0, 50000, len(counts)).tolist()
    order = sorted(longs)
    for s in order:
        sizes[s] = 10 ** 7
    sizes[order[0]] = (1 << 32) + 10 ** 6
    la0, nx0, la, nx, retr, bad = _apply_case(wire, counts.tolist(), sizes, 32, start={order[0]: (1 << 32) - 5000})
    assert la[order[0]] > 1 << 32 and all(bad[s] > 50 and retr[s] > bad[s] for s in order)
    none = [s for s, c in enumerate(counts) if c == 0]
    assert none and all((la[s], nx[s]) == (la0[s], nx0[s]) for s in none)


# ---- 2. pass 1 of k_ack_respond_files ---------------------------------------------------------
def placed_frames(rng, count, w0, last, completes=None):
    """count frames for a receiver at w0 >= 1 whose last accepted frame is frame `last` (None: no frame
    is accepted): up to it in-order frames of 1..23 bytes with duplicates, gaps and corrupt frames
    among them ("only": nothing but those in front of it), behind it only duplicates, gaps and
    corrupt frames. completes: the frame whose bytes reach the returned total.
    -> (file_off, pay_len, flavour), total."""
    ln = rng.integers(1, 24, count)
    kind = rng.choice(4, count, p=[0.7, 0.1, 0.1, 0.1])  # in order, duplicate, gap, corrupt
    other = rng.integers(1, 4, count)
    if last is None:
        kind = other
    else:
        if last == "only":
            last, kind = count - 1, other.copy()
        kind[last] = 0
        kind[last + 1:] = np.where(kind[last + 1:] == 0, other[last + 1:], kind[last + 1:])
    moves = kind == 0
    after = w0 + np.cumsum(np.where(moves, ln, 0))
    before = after - np.where(moves, ln, 0)
    fo = np.where(kind == 1, w0 - 1, np.where(kind == 2, before + 1 + ln, before))
    fl = np.where(kind == 3, "x", "d")
    total = int(after[completes]) if completes is not None else BIG
    return (fo.tolist(), ln.tolist(), fl.tolist()), total


@pytest.mark.parametrize("lanes", (1024, 256), ids=("workgroups of 1024", "workgroups of 256"))
def test_last_accepted_frame_in_every_slot_of_pass_one(vc, wire, lanes):
    """ack_stride == 0: the window's ACK rides on the file's last accepted frame, which pass 1 finds
    in the first chunk, in each of the four slots of its first step, in its second step or at the
    file's very last frame; files of 3,073, 5,120, 5,121 and 9,217 frames (1,281 and 2,305 in
    workgroups of 256). Also a long file without an accepted frame, one whose only accepted frame is
    the last, and one that completes inside the second step, so every accepted frame from there on
    answers."""
    files, fill = shp.pass1_shape(vc, _cus(), lanes)
    shp.check_pass1(lanes)
    rng = np.random.default_rng(500 + lanes)
    per_file, total, w0 = [], [], []
    for count, what, i in files:
        w = int(rng.integers(1, 100))
        last = {"none": None, "only-last": "only", "completes": count - 1}.get(what, i)
        f, t = placed_frames(rng, count, w, last, completes=i if what == "completes" else None)
        per_file.append(f), total.append(t), w0.append(w)
    for _ in range(fill):
        per_file.append(_in_order(1, 3)), total.append(BIG), w0.append(3)
    S = len(per_file)
    rx = Receiver(wire, w0, total, [w + 24 * len(f[0]) + 8 for w, f in zip(w0, per_file)], 0, [0] * S)
    want, _ = rx.window(per_file, 510, ["big"] * S)
    _counts_match(rx)
    for s, (count, what, i) in enumerate(files):
        acks = [r for r in want[s] if len(r) == 12]
        if what == "none":
            assert rx.nacc[s] == 0 and acks  # duplicates and gaps alone answer, every ACK for w0
            assert {r for r in acks} == {wire.put_response(ACK, w0[s])}
        elif what == "only-last":
            assert rx.nacc[s] == 1 and want[s][-1] == wire.put_response(ACK, rx.w[s])
        elif what == "completes":
            assert rx.w[s] > total[s] and rx.nacc[s] > i - (i // 2)
        else:
            assert rx.nacc[s] > 0 and wire.put_response(ACK, rx.w[s]) in want[s]


# ---- 3. strides above a chunk, above a window and near 2^32 -----------------------------------
STRIDE_COUNTS = (1, 63, 1023, 2049)


@pytest.mark.parametrize("k", (64, 1000, 1025, SAT))
def test_large_strides(vc, wire, k):
    """since on entry at 0, k - 1, k, k + 5 and 2^32 - 1 (where it fits 32 bits), files of 1, 63, 1,023
    and 2,049 mixed frames, three chained windows: since accumulates over windows until the stride
    fires, and saturates as the host rule's does. At k = 64 and 1,025 one-frame files bring the call
    into workgroups of 256."""
    sinces = [s for s in (0, k - 1, k, k + 5, SAT) if s <= SAT]
    files = [(c, s) for s in dict.fromkeys(sinces) for c in STRIDE_COUNTS]
    small = k in (64, 1025)
    n = sum(c for c, _ in files)
    fill = 0
    while small and (n + fill) // (len(files) + fill) > 256:
        fill += 1
    S = len(files) + fill
    shp.respond_plan(vc, _cus(), n + fill, S, 256 if small else 1024)
    counts = [c for c, _ in files] + [1] * fill
    rng = np.random.default_rng(600 + k % 1000)
    w0 = rng.integers(0, 1000, S).tolist()
    cap = [w + 24 * 3 * c + 8 for w, c in zip(w0, counts)]
    rx = Receiver(wire, w0, [BIG] * S, cap, k, [s for _, s in files] + [0] * fill)
    fired_in = {}
    for rnd in range(3):
        since0, nacc0 = list(rx.since), rx.nacc.copy()
        rx.window([mixed_frames(rng, c, rx.w[s], cap[s]) for s, c in enumerate(counts)], 610 + rnd, ["big"] * S)
        for s in range(len(files)):  # the host rule's since was reset: a stride ACK went out in this window
            if rx.since[s] != min(since0[s] + int(rx.nacc[s] - nacc0[s]), SAT) and s not in fired_in:
                fired_in[s] = rnd
    _counts_match(rx)
    if k < SAT:
        assert any(r > 0 for r in fired_in.values()), fired_in  # a first stride ACK in the second or third window
        assert any(files[s][1] == 0 and r > 0 for s, r in fired_in.items())
    assert any(r == 0 for r in fired_in.values())  # since at k - 1 or above fires with the first accepted frame
    never = [s for s in range(len(files)) if s not in fired_in and files[s][1] == 0]
    assert never and all(rx.since[s] < k for s in never)


# ---- 4. implied offsets among frames that are not accepted ------------------------------------
@pytest.mark.parametrize("stride", (0, 2))
@pytest.mark.parametrize("lanes", (1024, 256), ids=("workgroups of 1024", "workgroups of 256"))
def test_implied_offsets_in_mixed_windows(vc, wire, lanes, stride):
    """Half of the in-order frames carry no offset: they land behind corrupt and control frames, behind
    a gap, and where the capacity refuses them (silent: no response)."""
    rng = np.random.default_rng(700 + lanes + stride)
    counts = [12, 60, 60, 40, 300, 1025, 2049]
    fill = 0
    while lanes == 256 and (sum(counts) + fill) // (len(counts) + fill) > 256:
        fill += 1
    counts += [2] * fill
    S = len(counts)
    shp.respond_plan(vc, _cus(), sum(counts), S, lanes)
    w0 = rng.integers(0, 500, S).tolist()
    cap = [w + 24 * 2 * c + 8 for w, c in zip(w0, counts)]
    cap[1] = w0[1] + 12  # file 1: two 5-byte frames fit, every later implied frame is refused
    cap[4], cap[5] = w0[4] + 1500, w0[5] + 9000  # run full in the first window
    rx = Receiver(wire, w0, [BIG] * S, cap, stride, [0] * S)
    for rnd in range(2):
        per_file = [mixed_frames(rng, c, rx.w[s], cap[s], implied=0.5) for s, c in enumerate(counts)]
        w = rx.w[0]  # file 0, literally: implied frames behind a gap, a corrupt and a control frame
        per_file[0] = ([w, w + 100, w + 5, w + 9, w + 9, w + 12, w + 12, w + 20, w + 20, w + 20, w + 27, w + 27],
                       [5, 7, 4, 6, 3, 6, 8, 8, 0, 7, 9, 1],
                       ["d", "d", "i", "x", "i", "c", "i", "x", "i", "i", "d", "i"])
        per_file[1] = ([rx.w[1] + 5 * i for i in range(counts[1])], [5] * counts[1], ["i"] * counts[1])
        want, _ = rx.window(per_file, 710 + rnd, ["big"] * S)
        _counts_match(rx)
        assert not rx.dropped.any()
        if rnd == 0:
            assert rx.w[0] == w + 5 + 4 + 3 + 8 + 0 + 7 + 9 + 1 and rx.w[1] == w0[1] + 10
            assert len(want[1]) == (2 // stride if stride else 1) and rx.novf[1] == counts[1] - 2
            assert any(len(r) == 24 for r in want[0])
        else:  # nothing fits any more: no accepted frame, no response
            assert want[1] == [] and rx.novf[1] == 2 * counts[1] - 2
    assert rx.novf[4] > 50 and rx.novf[5] > 50


# ---- 5. clauses of the contracts --------------------------------------------------------------
def _six_files(rng, rx):
    return [mixed_frames(rng, c, rx.w[s], rx.file_cap[s]) for s, c in enumerate((30, 25, 0, 40, 35, 1100))]


def test_response_offsets_no_buffer_has(vc, wire):
    """d_resp_off[s] of 2^60 and of 2^63 + 5 among normal files, with a large capacity: nothing is
    written for them, d_resp_len and d_nresp are 0, every response counts as dropped, and the canvas
    around the other files' streams is intact. Twice, so d_ndropped accumulates."""
    rng = np.random.default_rng(801)
    rx = Receiver(wire, [0, 7, 3, 0, 5, 9], [BIG] * 6, [1 << 20] * 6, 1, [0] * 6)
    dead = {1: 1 << 60, 4: (1 << 63) + 5}
    for rnd in range(2):
        before = rx.dropped.copy()
        want, _ = rx.window(_six_files(rng, rx), 810 + rnd, ["big", "big", "big", "short", "big", "big"], dead=dead)
        assert [int(x) for x in rx.dropped - before] == [0, len(want[1]), 0, 1, len(want[4]), 0]
        assert len(want[1]) > 10 and len(want[4]) > 10
        assert _u64(rx.last["resp_len"])[[1, 4]].tolist() == [0, 0] and _u32(rx.ndropped)[1] == rx.dropped[1]


def test_respond_without_a_dropped_count(vc, wire):
    """d_ndropped == NULL through the raw call: short capacities drop responses, nobody counts them,
    and every other output is as with the count."""
    rng = np.random.default_rng(802)
    rx = Receiver(wire, [0, 7, 3, 0, 5, 9], [BIG] * 6, [1 << 20] * 6, 2, [0, 1, 0, 1, 0, 1])
    want, full = rx.window(_six_files(rng, rx), 820, ["short", 11, "big", 0, "fit", 37], null_ndropped=True)
    assert all(f > 37 for s, f in enumerate(full) if s != 2) and not rx.dropped.any()
    rx.window(_six_files(rng, rx), 821, ["short", 11, "big", 0, "fit", 37])  # and the next window counts
    assert rx.dropped[[0, 1, 3, 5]].all() and not rx.dropped[[2, 4]].any()


@pytest.mark.parametrize("case", ("n below first[n_files]", "a descending step"))
def test_respond_first_is_clamped(vc, wire, case):
    """d_first as val_frame_unpack_files_dev clamps it (tests/test_gpu_unpack_files.py's _segments): a
    file's frames end at n, and a bound below its predecessor leaves the file empty. Frames that no
    file owns get no response, are not accepted and change no file."""
    rng = np.random.default_rng(803)
    if case == "n below first[n_files]":
        first, n, counts = [0, 5, 12, 14, 14], 10, (5, 5, 0, 0)
    else:
        first, n, counts = [0, 5, 10, 7, 7], 12, (5, 5, 0, 0)
    assert _segments(first, n)[:2] == [(0, 5), (5, 10)] and all(a == b for a, b in _segments(first, n)[2:])
    rx = Receiver(wire, [0, 4, 0, 0], [BIG] * 4, [1 << 16] * 4, 1, [0] * 4)
    for rnd in range(2):
        per_file = [_in_order(c, rx.w[s]) if s == 0 else mixed_frames(rng, c, rx.w[s]) for s, c in enumerate(counts)]
        loose = _in_order(4, 0)  # in order for the empty files at 0: nobody's
        want, _ = rx.window(per_file, 830 + rnd, ["big"] * 4, loose=loose, first_dev=first, n_dev=n)
        assert len(want[0]) == 5 and want[2] == want[3] == [] and rx.w[2:] == [0, 0]
    _counts_match(rx)


class ShortEntries(Receiver):
    """Receiver whose flavours 's0', 's4', 's7' (and 's4!' ...: with a bad trailer) are owned entries of
    crc_len 0, 4 and 7: the first bytes of a DATA frame in order, with the trailer of those bytes."""

    def build(self, per_file, seed, strided=0):
        flav = [x for f in per_file for x in f[2]]
        plain = [(f[0], f[1], ["d" if x[0] == "s" else x for x in f[2]]) for f in per_file]
        stream, f_off, c_len = super().build(plain, seed, strided)
        c_len = c_len.copy()
        for i, x in enumerate(flav):
            if x[0] == "s":
                at, L = int(f_off[i]), int(x[1])
                crc = _oracle.crc32(stream[at:at + L]) ^ (0x100 if x.endswith("!") else 0)
                stream[at + L:at + L + 4] = np.frombuffer(crc.to_bytes(4, "little"), np.uint8)
                c_len[i] = L
        return stream, f_off, c_len


@pytest.mark.parametrize("deliver", (True, False), ids=("delivered", "respond alone"))
def test_respond_entries_shorter_than_a_header(vc, wire, deliver):
    """Owned entries of crc_len 0, 4 and 7 among DATA frames: not DATA whatever their trailer says, so
    no response, no accepted byte, and the frames around them answer as if they were not there."""
    w = 40
    a = ([w, w, w + 5, w + 5, w + 5, w + 11, w + 300, w + 11, w + 15],
         [5, 9, 6, 9, 9, 4, 7, 9, 3],
         ["d", "s0", "d", "s4", "s7!", "d", "d", "s7", "d"])
    b = ([0, 0, 0], [8, 8, 8], ["s4!", "s0!", "s7"])
    c = _in_order(6, 9)
    rx = ShortEntries(wire, [w, 0, 9], [BIG] * 3, [1 << 12] * 3, 1, [0] * 3, deliver=deliver)
    want, _ = rx.window([a, b, c], 840, ["big"] * 3)
    assert rx.w == [w + 18, 0, 9 + 42] and rx.nacc.tolist() == [4, 0, 6]
    assert [len(r) for r in want[0]] == [12, 12, 12, 24, 12, 12] and want[1] == []
    if deliver:
        assert _u32(rx.lay.fnbad).tolist() == [1, 2, 0]
        _counts_match(rx)


def _resp(wire, kind, off, clen, bad=False):
    """A response frame with `clen` content bytes whatever the offset needs (0: the low half alone)."""
    body = wire.serialize_header(kind, 0, clen, off & SAT)
    body += ((off >> 32).to_bytes(4, "little") + (1).to_bytes(4, "little") + bytes(4))[:clen]
    crc = _oracle.crc32(body) ^ (0x10 if bad else 0)
    return body + crc.to_bytes(4, "little")


def _apply(wire, base, segs, sizes, la0, nx0, *, first, n, off=None, length=None, stride=0, flen=0, len_hint=12,
           null=(), nbad0=None):
    """The raw apply call against val_frame_apply_acks per segment (the segments `first` and n must
    clamp to). null: outputs passed as NULL. -> the host rule's (last_acked, next, retransmits, bad)."""
    S = len(sizes)
    assert _segments(first, n) == segs
    f_off = np.arange(n, dtype=np.uint64) * np.uint64(stride) if off is None else np.asarray(off, np.uint64)
    c_len = np.full(n, flen, np.uint32) if length is None else np.asarray(length, np.uint32)
    ok_all = _oracle.verify_frames(base, f_off[:n], c_len[:n])[0]
    kind, aoff = wire.ack_offsets(base, f_off[:n], c_len[:n])
    want = []
    for s, (lo, hi) in enumerate(segs):
        want.append(wire.apply_acks(kind[lo:hi], aoff[lo:hi], sizes[s], la0[s], nx0[s], ok_all[lo:hi]) if hi > lo
                    else (la0[s], nx0[s], 0, 0))
    d_la, d_nx = _d64(la0), _d64(nx0)
    out = dict(nretrans=torch.full((S,), 3, dtype=torch.int32, device=DEV),
               file_nbad=torch.full((S,), 5, dtype=torch.int32, device=DEV),
               ok=torch.full((n,), 7, dtype=torch.uint8, device=DEV),
               nbad=None if nbad0 is None else torch.full((1,), nbad0, dtype=torch.int32, device=DEV))
    work = torch.empty(max(wire.apply_acks_work_bytes(n), 16), dtype=torch.uint8, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    d_base, d_first, d_size = _d8(base), _d32(first), _d64(sizes)
    d_off = None if off is None else _d64(off)
    d_len = None if length is None else _d32(length)
    args = [None if k in null else ptr(out[k]) for k in ("nretrans", "file_nbad", "ok", "nbad")]
    st = wire.lib().val_frame_apply_acks_files_dev(ptr(d_base), ptr(d_off), ptr(d_len), stride, flen, n, len_hint, S,
                                                   ptr(d_first), ptr(d_size), ptr(d_la), ptr(d_nx), *args, ptr(work),
                                                   work.numel(), torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert _u64(d_la).tolist() == [w[0] for w in want] and _u64(d_nx).tolist() == [w[1] for w in want]
    # a NULL output's tensor was not passed: it must hold its canary
    assert (_u32(out["nretrans"]) - 3).tolist() == [0 if "nretrans" in null else w[2] for w in want]
    assert (_u32(out["file_nbad"]) - 5).tolist() == [0 if "file_nbad" in null else w[3] for w in want]
    if "ok" in null:
        assert (out["ok"].cpu().numpy() == 7).all()
    else:
        assert np.array_equal(out["ok"].cpu().numpy(), ok_all)
    if nbad0 is not None:  # incremented by every bad frame of the call, owned or not
        assert int(out["nbad"].item()) == nbad0 + int((ok_all == 0).sum())
    return want


def _responses(wire, rng, n, size, la):
    """n responses as tests/test_gpu_acks.py's response_stream mixes them -> frames, one by one."""
    from tests.test_gpu_acks import response_stream

    st = np.frombuffer(response_stream(rng, n, size, la), np.uint8)
    _, f_off, c_len, _ = wire.scan_frames(st, 64)
    return [st[int(o):int(o) + int(c) + 4].tobytes() for o, c in zip(f_off, c_len)]


def _laid(frames, lead=3):
    base = np.frombuffer(b"\x5a" * lead + b"".join(frames) + b"\x5a" * 8, np.uint8).copy()
    size = np.array([len(f) for f in frames], np.int64)
    off = lead + np.cumsum(size) - size
    return base, off.astype(np.uint64), (size - 4).astype(np.uint32)


@pytest.mark.parametrize("null", ((), ("nretrans",), ("file_nbad",), ("nretrans", "file_nbad", "ok")),
                         ids=lambda x: "+".join(x) or "all outputs")
def test_apply_outputs_that_may_be_null(vc, wire, null):
    """d_nretrans, d_file_nbad and d_ok NULL through the raw call, d_nbad given with a nonzero start:
    the states and the outputs that remain are the host rule's."""
    rng = np.random.default_rng(804)
    sizes, la0 = [10 ** 6, 0, 5000, 10 ** 7], [100, 0, 7, 0]
    frames = [f for s, c in enumerate((300, 0, 80, 1100)) for f in _responses(wire, rng, c, sizes[s], la0[s])]
    base, off, length = _laid(frames + _responses(wire, rng, 9, 1000, 0))  # nine frames that no transfer owns
    first = [0, 300, 300, 380, 1480]
    want = _apply(wire, base, _segments(first, off.size), sizes, la0, [200, 0, 9, 50], first=first, n=off.size, off=off,
                  length=length, null=null, nbad0=1000)
    assert all(w[3] > 0 and w[2] > w[3] for s, w in enumerate(want) if s != 1)


@pytest.mark.parametrize("case", ("n below first[n_files]", "a descending step"))
def test_apply_first_is_clamped(vc, wire, case):
    rng = np.random.default_rng(805)
    if case == "n below first[n_files]":
        first, n, segs = [0, 5, 12, 14, 14], 10, [(0, 5), (5, 10), (10, 10), (10, 10)]
    else:
        first, n, segs = [0, 5, 10, 7, 7], 12, [(0, 5), (5, 10), (10, 10), (7, 7)]
    acks = [wire.put_response(ACK if i % 4 else NAK, 100 * (i + 1)) for i in range(14)]
    acks[8] = _resp(wire, ACK, 900, 0, bad=True)
    base, off, length = _laid(acks)
    want = _apply(wire, base, segs, [5000] * 4, [0, 50, 60, 70], [80] * 4, first=first, n=n, off=off, length=length,
                  nbad0=0)
    # transfer 1 ends at frame 9 (ACK 1000), not at frame 11 or 13; the empty transfers keep their entries
    assert [w[:2] for w in want] == [(500, 500), (1000, 1000), (60, 80), (70, 80)] and want[1][2:] == (1, 1)


@pytest.mark.parametrize("slot,flen", ((16, 12), (24, 20)))
def test_apply_strided_slots_with_a_high_half(vc, wire, slot, flen):
    """Strided mode with flen >= 12: the offset's high half at +8 counts. 16-byte slots hold ACKs with
    four content bytes, 24-byte slots NAKs and ACKs with twelve; offsets on both sides of 2^32 and
    beyond the file, a few bad trailers."""
    rng = np.random.default_rng(806 + slot)
    n, cut = 1300, 200
    sizes = [(1 << 32) + 10 ** 6, (3 << 32) + 77]
    top = [(1 << 32) + 2 * 10 ** 6, 4 << 32]
    frames = []
    for i in range(n):
        s = int(i >= cut)
        r = rng.random()
        o = int(rng.integers(0, 1 << 32)) if r < 0.4 else int(rng.integers(1 << 32, top[s])) if r < 0.9 else sizes[s]
        kind = NAK if flen == 20 and rng.random() < 0.3 else ACK
        frames.append(_resp(wire, kind, o, flen - 8, bad=rng.random() < 0.05))
    base, off, _ = _laid(frames, lead=0)
    assert np.array_equal(off, np.arange(n, dtype=np.uint64) * np.uint64(slot))
    la0, nx0 = [5, (1 << 32) + 9], [5000, (2 << 32)]
    want = _apply(wire, base, [(0, cut), (cut, n)], sizes, la0, nx0, first=[0, cut, n], n=n, stride=slot, flen=flen,
                  len_hint=flen, nbad0=7)
    assert la0[0] < 1 << 32 < want[0][0] <= sizes[0] and 2 << 32 < want[1][0] <= sizes[1]
    assert all(w[3] > 0 for w in want) and (flen == 12 or all(w[2] > w[3] for w in want))
    kind, aoff = wire.ack_offsets(base, off, np.full(n, flen, np.uint32))
    assert (aoff[cut:] > sizes[1]).any() and (aoff[:cut] > sizes[0]).any() and (aoff < 1 << 32).any()


def test_apply_entries_shorter_than_a_header(vc, wire):
    """Owned entries of crc_len 0, 4 and 7: with a good trailer they are ignored (whatever their first
    byte says), with a bad one they count as corrupt and restart the transfer."""
    def short(L, bad=False, first_byte=6):
        body = bytes([first_byte] + [0x40 + i for i in range(L)][1:]) if L else b""
        crc = _oracle.crc32(body) ^ (1 if bad else 0)
        return body + crc.to_bytes(4, "little")

    a = [wire.put_response(ACK, 100), short(0), short(4), short(7), wire.put_response(ACK, 300), short(7, first_byte=13)]
    b = [wire.put_response(ACK, 100), short(4, bad=True), wire.put_response(ACK, 300)]
    c = [short(0, bad=True)]
    d = [short(0), short(4), short(7)]
    base, off, length = _laid(a + b + c + d)
    assert set(length.tolist()) == {0, 4, 7, 8}
    want = _apply(wire, base, [(0, 6), (6, 9), (9, 10), (10, 13)], [1000] * 4, [0, 0, 40, 40], [900, 900, 900, 900],
                  first=[0, 6, 9, 10, 13], n=13, off=off, length=length, len_hint=0, nbad0=0)
    assert want == [(300, 900, 0, 0), (300, 300, 1, 1), (40, 40, 1, 1), (40, 900, 0, 0)]


# ---- 6. respond -> scan -> apply, NAKs included, nothing read back -----------------------------
@pytest.mark.parametrize("flip", (False, True), ids=("as written", "one offset bit flipped on the device"))
def test_respond_scan_apply_with_nothing_read_back(vc, wire, flip):
    """A mixed window's response streams, as the device wrote them (12-, 16- and 24-byte responses, one
    receiver past 2^32, one stream cut short by its capacity), scanned and applied on a side stream;
    the sender's states are val_frame_apply_acks over the host rule's kept responses. With a bit of
    one kept response's offset flipped by a torch op, that response counts as corrupt."""
    rng = np.random.default_rng(900)
    w0 = [0, 50, (1 << 32) - 200, (1 << 32) + 7, 9, 3]
    S = len(w0)
    rx = Receiver(wire, w0, [BIG] * S, [U64] * S, 1, [0] * S, deliver=False)
    per_file = [mixed_frames(rng, c, w) for c, w in zip((60, 1100, 40, 50, 0, 30), w0)]
    want, _ = rx.window(per_file, 910, ["big", "big", "big", "fit", "big", 250])
    kept = rx.last["kept"]
    assert {len(r) for rs in kept for r in rs} == {12, 16, 24} and rx.dropped[5] > 0 and len(kept[5]) > 5
    assert {len(r) for r in kept[2]} >= {12, 16} and any(len(r) == 24 for r in kept[1])
    out, r_off, r_len = rx.last["out"], rx.last["resp_off"], rx.last["resp_len"]
    ok = [np.ones(len(rs), np.uint8) for rs in kept]
    if flip:  # file 1's 20th kept response: bit 5 of its third offset byte
        at = int(_u64(r_off)[1]) + sum(len(r) for r in kept[1][:20]) + 6
        ok[1][20] = 0
    max_frames = max(len(rs) for rs in kept) + 3
    sizes = [BIG] * S
    la0 = list(w0)
    nx0 = [w + 5000 for w in w0]
    w_la, w_nx, w_retr, w_bad = [], [], [], []
    for s, rs in enumerate(kept):
        st = np.frombuffer(b"".join(rs), np.uint8)
        code, f_off, c_len, used = wire.scan_frames(st, 1024) if st.size else (0, np.zeros(0, np.uint64),
                                                                                np.zeros(0, np.uint32), 0)
        assert code == 0 and used == st.size and f_off.size == len(rs)
        kind, aoff = wire.ack_offsets(st, f_off, c_len)
        la, nx, retr, ncrc = wire.apply_acks(kind, aoff, sizes[s], la0[s], nx0[s], ok[s])
        w_la.append(la), w_nx.append(nx), w_retr.append(retr), w_bad.append(ncrc)
    d_la, d_nx, d_size = _d64(la0), _d64(nx0), _d64(sizes)
    retr = torch.zeros(S, dtype=torch.int32, device=DEV)
    fbad = torch.zeros(S, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        if flip:
            out[at:at + 1].bitwise_xor_(0x20)
        f_off, c_len, first, nframes, consumed, status = wire.scan_streams_dev(out, r_off, r_len, 1024, max_frames,
                                                                               stream=side)
        wire.apply_acks_files_dev(out, first=first, file_size=d_size, last_acked=d_la, next=d_nx, off=f_off,
                                  length=c_len, n=S * max_frames, len_hint=12, nretrans=retr, file_nbad=fbad,
                                  stream=side)
    side.synchronize()
    assert _u32(nframes).tolist() == [len(rs) for rs in kept] and not _u32(status).any()
    assert _u64(d_la).tolist() == w_la and _u64(d_nx).tolist() == w_nx
    assert _u32(retr).tolist() == w_retr and _u32(fbad).tolist() == w_bad
    assert sum(w_retr) > 50 and w_bad == [0, int(flip), 0, 0, 0, 0]
    assert w_la[2] > 1 << 32 and (w_la[4], w_nx[4]) == (la0[4], nx0[4])
