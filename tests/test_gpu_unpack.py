"""val_frame_unpack_batch_dev: a window of received frames in HBM delivered
into a GPU-resident file (include/val_crc32_gpu.h; the device form of the
reference's receive loop, src/val_core.c:963-993 and src/val_receiver.c:
871-895, for a whole window).

Every test fills the device file with 0xA5 first and compares the WHOLE canvas
afterwards: the call may write the accepted payloads at their offsets and
nothing else. Expected bytes are val_frame_accept (the rule in plain C) plus a
numpy scatter; expected `written` and CRC state come from
val_crc32_fold_payload_states_at over the oracle's payload states, and again
from the oracle's CRC of the delivered bytes themselves."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import _oracle, _prng

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
DEV = "cuda:0"
ALL_LANES = (1, 2, 4, 8, 16, 32, 64)  # every k_unpack instantiation
U64 = (1 << 64) - 1
CTRL = 3  # a packet type that is not VAL_PKT_DATA


@pytest.fixture(scope="module")
def vc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import val_protocol_amd.crc as m

    m.init(0)
    m.set_geometry()
    yield m
    m.set_geometry()
    m.set_ragged_min_frames(-1)


@pytest.fixture(scope="module")
def wire(vc):
    import val_protocol_amd.wire as w

    return w


def _d64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _d32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _d8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)


def _le(v, nbytes):
    return np.frombuffer(int(v).to_bytes(nbytes, "little"), np.uint8)


def _frame(wire, payload, off=None, *, ptype=5, flags=None, corrupt=False):
    """One wire frame by hand: header, the LE64 offset when `off` is given,
    payload, LE32 trailer. content_len is what 16 bits can say of it."""
    body = np.asarray(payload, dtype=np.uint8)
    if flags is None:
        flags = 1 if off is not None else 0
    if off is not None:
        body = np.concatenate([_le(off, 8), body])
    hdr = np.frombuffer(wire.serialize_header(ptype, flags, min(body.size, 0xFFFF), 0), np.uint8)
    f = np.concatenate([hdr, body])
    f = np.concatenate([f, _le(_oracle.crc32(f), 4)])
    if corrupt:
        f[f.size // 2] ^= 0x10
    return f


class Window:
    """Wire frames (trailers included) laid into one stream: frame i starts
    1..4 filler bytes after frame i-1, at an address with phase[i] mod 4."""

    def __init__(self, frames, phase=None, front=5):
        n = len(frames)
        off, pos = [], front
        for i, f in enumerate(frames):
            pos += 1
            if phase is not None:
                pos += (int(phase[i]) - pos) % 4
            off.append(pos)
            pos += f.size
        self.stream = _prng.prng_bytes(99, pos + 9)
        for o, f in zip(off, frames):
            self.stream[o:o + f.size] = f
        self.off = np.array(off, dtype=np.uint64)
        self.len = np.array([f.size - 4 for f in frames], dtype=np.uint32)
        self.n = n


def _built(wire, pay_len, file_off, inc, seed=7):
    """Frames from the host framer with the oracle's trailers -> list of wire frames, payload bytes."""
    pay_len = np.asarray(pay_len, dtype=np.uint32)
    payload = np.random.default_rng(seed).integers(0, 256, max(int(pay_len.sum()), 1), dtype=np.uint8)
    pay_off = (np.cumsum(pay_len, dtype=np.uint64) - pay_len).astype(np.uint64)
    stream, fo, cl = wire.build_data_batch(payload, pay_off, pay_len, np.asarray(file_off, dtype=np.uint64),
                                           np.asarray(inc, dtype=np.uint8))
    wire.put_trailers(stream, fo, cl, _oracle.frames(stream, fo, cl, nthreads=8))
    return [stream[int(o):int(o) + int(c) + 4] for o, c in zip(fo, cl)], payload


def _in_order(pay_len, start=0):
    pay_len = np.asarray(pay_len, dtype=np.uint64)
    return start + np.cumsum(pay_len) - pay_len


class File:
    """The device side of a transfer: the 0xA5 canvas, `written`, the CRC state, the counters."""

    def __init__(self, size, written=0, state=0xFFFFFFFF):
        self.file = torch.full((size,), CANARY, dtype=torch.uint8, device=DEV)
        self.written = _d64([written])
        self.state = _d32([state])
        self.nbad, self.nacc, self.novf = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(3))
        self.ok, self.accept = [], []

    def unpack(self, wire, base, off, length, *, cap=None, **kw):
        ok, acc, _, _, _ = wire.unpack_data_batch_dev(base, file=self.file, written=self.written, off=off, length=length,
                                                      file_cap=cap, file_state=self.state, nbad=self.nbad,
                                                      naccepted=self.nacc, noverflow=self.novf, **kw)
        self.ok.append(ok)
        self.accept.append(acc)

    def result(self):
        torch.cuda.synchronize()
        return dict(file=self.file.cpu().numpy(), written=int(self.written.cpu().numpy().view(np.uint64)[0]),
                    state=int(self.state.cpu().numpy().view(np.uint32)[0]),
                    ok=np.concatenate([t.cpu().numpy() for t in self.ok]),
                    accept=np.concatenate([t.cpu().numpy() for t in self.accept]),
                    nbad=int(self.nbad.item()), nacc=int(self.nacc.item()), novf=int(self.novf.item()))


def _expect(vc, wire, stream, off, length, size, written=0, state=0xFFFFFFFF, cap=None):
    """What the receiver's loop leaves: the oracle's verdicts, val_frame_accept, a scatter, the fold."""
    cap = size if cap is None else cap
    off, length = np.asarray(off, dtype=np.uint64), np.asarray(length, dtype=np.uint32)
    ok, nbad = _oracle.verify_frames(stream, off, length, nthreads=8)
    fo = wire.data_offsets(stream, off, length)
    pl = wire.payload_lens(stream, off, length)
    dst, w, nacc, novf = wire.frame_accept(fo, pl, written, cap, ok)
    acc = dst != wire.NOT_ACCEPTED
    canvas = np.full(size, CANARY, dtype=np.uint8)
    pay = np.zeros(off.size, dtype=np.uint32)
    src = off + (length - pl)
    for i in np.flatnonzero(acc):
        p = stream[int(src[i]):int(src[i]) + int(pl[i])]
        canvas[int(dst[i]):int(dst[i]) + int(pl[i])] = p
        pay[i] = _oracle.update_state(0, p)
    st, w2, nf = vc.fold_payload_states_at(state, pay, pl, fo, written, (ok != 0) & acc)
    assert (w2, nf) == (w, nacc)
    if written <= w <= size:  # the accepted payloads are the file bytes [written, w), in order
        assert st == _oracle.update_state(state, canvas[written:w])
    return dict(file=canvas, written=w, state=st, ok=ok, accept=acc.astype(np.uint8), nbad=nbad, nacc=nacc, novf=novf)


def _same(got, want):
    for k in ("written", "state", "nbad", "nacc", "novf"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("ok", "accept"):
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:8])
    bad = np.flatnonzero(got["file"] != want["file"])
    assert bad.size == 0, (bad.size, bad[:8])


def _roundtrip(vc, wire, win, size, *, written=0, state=0xFFFFFFFF, cap=None, len_hint=0):
    f = File(size, written, state)
    f.unpack(wire, _d8(win.stream), _d64(win.off), _d32(win.len), cap=cap, len_hint=len_hint)
    got = f.result()
    want = _expect(vc, wire, win.stream, win.off, win.len, size, written, state, cap)
    _same(got, want)
    return got


# ---- 1. the reference's own transfer ----------------------------------------------------
def test_reference_loopback_transfer(vc, wire):
    """The 1 MiB / MTU 1024 transfer the reference recorded: its 1,045 DATA
    frames in, the file, its length and its CRC out."""
    with open(os.path.join(ROOT, "tests", "golden", "dropin_vectors.json")) as f:
        lb = json.load(f)["loopback"]
    file = _prng.prng_bytes(lb["file_seed"], lb["bytes"])
    parts, off, lens, pos = [], [], [], 0
    for ptype, wire_len, trailer, foff, prefix in lb["tx_frames"]:
        if ptype != 5:
            continue
        head = np.frombuffer(bytes.fromhex(prefix), np.uint8)
        body = np.concatenate([head, file[foff:foff + wire_len - 4 - head.size]])
        parts += [body, _le(trailer, 4)]
        off.append(pos)
        lens.append(body.size)
        pos += wire_len
    stream = np.concatenate(parts)
    off, lens = np.array(off, np.uint64), np.array(lens, np.uint32)
    size = lb["bytes"] + 77
    f = File(size)
    f.unpack(wire, _d8(stream), _d64(off), _d32(lens), cap=lb["bytes"], len_hint=int(lens.max()))
    got = f.result()
    assert np.array_equal(got["file"][:lb["bytes"]], file)
    assert (got["file"][lb["bytes"]:] == CANARY).all()
    assert got["written"] == lb["bytes"] and got["state"] ^ 0xFFFFFFFF == lb["file_crc"]
    assert (got["nbad"], got["nacc"], got["novf"]) == (0, 1045, 0) and got["ok"].all() and got["accept"].all()
    _same(got, _expect(vc, wire, stream, off, lens, size, cap=lb["bytes"]))


# ---- 2. alignment and length sweep ------------------------------------------------------
@pytest.mark.parametrize("lanes", ALL_LANES)
def test_alignment_and_length_sweep(vc, wire, lanes):
    """Every source phase x destination phase for payloads of 0..140 bytes and
    of 64k - 1, 64k, 64k + 1 bytes up to k = 2 * lanes + 1, explicit and
    implied prefixes alternating. The destination phase of a frame is that of
    `written` when it arrives: a 0..3-byte frame in front of it sets it."""
    lengths = list(range(141)) + [64 * k + d for k in range(1, 2 * lanes + 2) for d in (-1, 0, 1)]
    start = lanes.bit_length() % 4
    pay_len, phase, w = [], [], start
    for L in lengths:
        for combo in range(16):
            sp, dp = combo & 3, combo >> 2
            fill = (dp - w) % 4
            if fill:
                pay_len.append(fill)
                phase.append((sp + 1) % 4)
                w += fill
            pay_len.append(L)
            phase.append(sp)
            w += L
    inc = (np.arange(len(pay_len)) % 3 == 0).astype(np.uint8)
    frames, _ = _built(wire, pay_len, _in_order(pay_len, start), inc, seed=lanes)
    win = Window(frames, phase)
    vc.set_lanes_per_frame(lanes)
    try:
        got = _roundtrip(vc, wire, win, w + 67, written=start, len_hint=0)
    finally:
        vc.set_lanes_per_frame(0)
    assert got["accept"].all() and got["written"] == w


# ---- 3. ordering ------------------------------------------------------------------------
def test_ordering_in_one_batch(vc, wire):
    """A go-back-N window with everything a receiver may see in it."""
    rng = np.random.default_rng(31)
    lens = [1012, 1012, 1012, 777, 1012, 1012, 1012, 333, 1012, 0, 1012, 500]
    pos = _in_order(lens, 3)
    data = [rng.integers(0, 256, L, dtype=np.uint8) for L in lens]
    A = lambda i, **kw: _frame(wire, data[i], int(pos[i]), **kw)  # noqa: E731
    other = rng.integers(0, 256, lens[2], dtype=np.uint8)
    frames = [A(0), A(1), A(2), A(3), A(4),
              A(5, corrupt=True),                       # lost
              A(6), A(7), A(8),                         # gaps behind it
              _frame(wire, data[1], ptype=CTRL),        # a control frame
              A(5), A(6), A(7), A(8),                   # the retransmission and what follows it, again
              A(7),                                     # an exact duplicate
              _frame(wire, other, int(pos[2])),         # a stale duplicate: valid CRC, other bytes
              _frame(wire, data[9 + 1], int(pos[9]), ptype=CTRL),  # looks like DATA at the right place, is not
              _frame(wire, data[3][:5], flags=1),       # DATA, too short for the offset it announces
              _frame(wire, data[9]),                    # implied, empty, after the skips
              _frame(wire, data[10]),                   # implied
              _frame(wire, data[11][:100], int(pos[11]) + 1),  # a gap of one byte
              _frame(wire, data[11])]                   # implied after a skip
    win = Window(frames)
    size = int(pos[-1]) + lens[-1] + 50
    got = _roundtrip(vc, wire, win, size, written=3)
    want_acc = [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1]
    assert got["accept"].tolist() == want_acc and got["nbad"] == 1 and got["ok"].tolist() == [1] * 5 + [0] + [1] * 16
    assert got["written"] == int(pos[-1]) + lens[-1] and got["nacc"] == sum(want_acc) and got["novf"] == 0
    assert np.array_equal(got["file"][3:got["written"]], np.concatenate(data))  # not `other`


# ---- 4. chunk edges of the order pass ---------------------------------------------------
def _small_window(wire, n, gap_at=(), corrupt_at=(), seed=5):
    """n small explicit / implied frames in order; frames in gap_at announce an
    offset 1000 bytes ahead (and are skipped), frames in corrupt_at fail their CRC."""
    rng = np.random.default_rng(seed)
    pay_len = rng.integers(0, 24, n).astype(np.uint32)
    inc = (rng.integers(0, 3, n) > 0).astype(np.uint8)
    skip = np.zeros(n, dtype=bool)
    skip[list(gap_at)] = True
    skip[list(corrupt_at)] = True
    inc[list(gap_at)] = 1
    eff = np.where(skip, 0, pay_len).astype(np.uint64)
    file_off = 2 + np.cumsum(eff) - eff
    file_off[list(gap_at)] += 1000
    frames, _ = _built(wire, pay_len, file_off, inc, seed)
    for i in corrupt_at:
        frames[i] = frames[i].copy()
        frames[i][9] ^= 0x01
    return Window(frames), 2 + int(eff.sum())


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
@pytest.mark.parametrize("brk", [1023, 1024])
def test_order_chunk_edges(vc, wire, n, brk):
    """The only break of the batch on either side of the first chunk boundary."""
    win, end = _small_window(wire, n, gap_at=[brk] if brk < n else [])
    got = _roundtrip(vc, wire, win, end + 40, written=2, len_hint=24)
    assert got["written"] == end and got["nacc"] == n - (1 if brk < n else 0)


def test_order_alternating_accept_and_gap(vc, wire):
    win, end = _small_window(wire, 3000, gap_at=range(1, 3000, 2))
    got = _roundtrip(vc, wire, win, end + 40, written=2, len_hint=24)
    assert got["nacc"] == 1500 and got["accept"].tolist() == [1, 0] * 1500


def test_order_all_gaps_after_a_lost_frame(vc, wire):
    """Frame 1 is lost; every later frame of the go-back-N window is a gap."""
    n = 3000
    rng = np.random.default_rng(8)
    pay_len = rng.integers(1, 24, n).astype(np.uint32)
    frames, _ = _built(wire, pay_len, _in_order(pay_len), np.ones(n, np.uint8))
    frames[1] = frames[1].copy()
    frames[1][-1] ^= 0x80
    win = Window(frames)
    got = _roundtrip(vc, wire, win, int(pay_len.sum()) + 40, len_hint=24)
    assert got["nacc"] == 1 and got["written"] == int(pay_len[0]) and got["nbad"] == 1


# ---- 5. capacity ------------------------------------------------------------------------
@pytest.mark.parametrize("cut", ["inside", "at_end", "one_short"])
def test_capacity(vc, wire, cut):
    pay_len = [100] * 6 + [100, 100, 10, 100]
    inc = [1, 0, 1, 0, 1, 0, 1, 0, 0, 1]
    frames, _ = _built(wire, pay_len, _in_order(pay_len, 1), inc)
    win = Window(frames)
    cap = {"inside": 1 + 650, "at_end": 1 + 700, "one_short": 1 + 699}[cut]
    got = _roundtrip(vc, wire, win, 1200, written=1, cap=cap)
    if cut == "at_end":  # frame 6 ends exactly at the capacity; 7 and 8 are implied and do not fit, 9 is a gap
        assert got["accept"].tolist() == [1] * 7 + [0, 0, 0] and got["novf"] == 2 and got["written"] == 701
    elif cut == "inside":  # 6 and 7 do not fit, the 10-byte frame 8 does, 9 is a gap then
        assert got["accept"].tolist() == [1] * 6 + [0, 0, 1, 0] and got["novf"] == 2 and got["written"] == 611
    else:
        assert got["accept"].tolist() == [1] * 6 + [0, 0, 1, 0] and got["novf"] == 2 and got["written"] == 611
    assert (got["file"][got["written"]:] == CANARY).all()


# ---- 6. lengths beyond the wire's -------------------------------------------------------
@pytest.mark.parametrize("len_hint", [0, 8 + 65535])
def test_lengths_beyond_content_len(vc, wire, len_hint):
    """Descriptor lengths are the caller's: 65,535 content bytes, 300,000 and
    1 MiB + 3 bytes of CRC input."""
    rng = np.random.default_rng(77)
    pls = [65535, 65527, 300000 - 16, (1 << 20) + 3 - 8, 65535, 9]
    expl = [0, 1, 1, 0, 0, 1]
    pos = _in_order(pls, 2)
    frames = [_frame(wire, rng.integers(0, 256, L, dtype=np.uint8), int(p) if e else None)
              for L, e, p in zip(pls, expl, pos)]
    win = Window(frames, phase=[1, 2, 3, 0, 1, 2])
    assert win.len.tolist()[:4] == [8 + 65535, 8 + 65535, 300000, (1 << 20) + 3]
    got = _roundtrip(vc, wire, win, 2 + sum(pls) + 33, written=2, len_hint=len_hint)
    assert got["accept"].all() and got["written"] == 2 + sum(pls)


# ---- 7. strided mode and the ragged verify path -----------------------------------------
def test_strided_mode(vc, wire):
    n, pl, stride = 300, 1004, 1031  # an odd stride: every source phase
    frames, _ = _built(wire, [pl] * n, _in_order([pl] * n), np.ones(n, np.uint8))
    frames[57] = frames[57].copy()
    frames[57][500] ^= 0x04
    flen = 16 + pl
    stream = _prng.prng_bytes(3, n * stride + 8)
    for i, f in enumerate(frames):
        stream[i * stride:i * stride + f.size] = f
    size = n * pl + 19
    f = File(size)
    f.unpack(wire, _d8(stream), None, None, stride=stride, flen=flen, n=n)
    got = f.result()
    off = np.arange(n, dtype=np.uint64) * stride
    _same(got, _expect(vc, wire, stream, off, np.full(n, flen, np.uint32), size))
    assert got["nacc"] == 57 and got["nbad"] == 1


def test_ragged_verify_path(vc, wire):
    """len_hint = 0 with the device-binned verify path pinned on."""
    n = 700
    rng = np.random.default_rng(12)
    pay_len = rng.choice([0, 1, 9, 64, 100, 700, 1012, 4000, 16376], n).astype(np.uint32)
    inc = rng.integers(0, 2, n).astype(np.uint8)
    frames, _ = _built(wire, pay_len, _in_order(pay_len), inc)
    frames[333] = frames[333].copy()
    frames[333][3] ^= 0x40
    win = Window(frames)
    vc.set_ragged_min_frames(1)
    try:
        got = _roundtrip(vc, wire, win, int(pay_len.sum()) + 40, len_hint=0)
    finally:
        vc.set_ragged_min_frames(-1)
    assert got["nbad"] == 1 and got["accept"][:333].all() and not got["accept"][333]


# ---- 8. streams and chaining ------------------------------------------------------------
def test_two_calls_on_a_side_stream_chain(vc, wire):
    """Two calls back to back on a side stream, nothing between them: the
    second continues from the first's written and state; counters accumulate."""
    win, end = _small_window(wire, 700, gap_at=[100, 500], corrupt_at=[250, 600], seed=21)
    base, off, length = _d8(win.stream), _d64(win.off), _d32(win.len)
    size, cut = end + 30, 400
    f = File(size, written=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    f.unpack(wire, base, off[:cut], length[:cut], len_hint=24, stream=side)
    f.unpack(wire, base, off[cut:], length[cut:], len_hint=24, stream=side)
    side.synchronize()
    got = f.result()
    _same(got, _expect(vc, wire, win.stream, win.off, win.len, size, 2))
    assert got["nbad"] == 2 and got["nacc"] == 696 and got["written"] == end


# ---- 9. arguments -----------------------------------------------------------------------
def test_invalid_arguments_and_empty_batch(vc, wire):
    win, end = _small_window(wire, 10)
    base, off, length = _d8(win.stream), _d64(win.off), _d32(win.len)
    f = File(end + 20, written=2)
    work = torch.zeros(wire.unpack_work_bytes(10), dtype=torch.uint8, device=DEV)
    assert wire.unpack_work_bytes(10) >= 10 * 25 and wire.unpack_work_bytes(0) == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(base=base, off=off, length=length, n=10, file=f.file, written=f.written, work=work, wb=None):
        return vc.lib().val_frame_unpack_batch_dev(p(base), p(off), p(length), 0, 0, n, 0, p(file), f.file.numel(),
                                                   p(written), p(f.state), None, p(f.nbad), None, p(f.nacc), p(f.novf),
                                                   p(work), work.numel() if wb is None and work is not None else (wb or 0), s)

    for what, kw in (("file", dict(file=None)), ("written", dict(written=None)), ("work", dict(work=None)),
                     ("work_bytes", dict(wb=wire.unpack_work_bytes(10) - 1)), ("off/len", dict(off=None)),
                     ("off/len", dict(length=None))):
        assert call(**kw) == vc.VAL_ERR_INVALID_ARG, what
        assert what.split("/")[0] in vc.last_error(), (what, vc.last_error())
    assert call(n=0) == vc.VAL_OK
    torch.cuda.synchronize()
    assert (f.file.cpu().numpy() == CANARY).all() and int(f.written.item()) == 2
    assert int(f.state.cpu().numpy().view(np.uint32)[0]) == 0xFFFFFFFF
    assert (int(f.nbad.item()), int(f.nacc.item()), int(f.novf.item())) == (0, 0, 0)
    assert call() == vc.VAL_OK  # and the same arguments, complete, deliver
    torch.cuda.synchronize()
    assert int(f.written.item()) == end and int(f.nacc.item()) == 10
