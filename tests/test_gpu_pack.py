"""val_frame_data_batch_dev: DATA frames built in HBM from GPU-resident file
bytes, trailers included, in one launch (include/val_crc32_gpu.h; the device
form of reference src/val_core.c:733-834 for a whole window).

Every test fills the output with 0xA5 first and compares the WHOLE buffer
afterwards: the kernel may write the 12 + content wire bytes of each accepted
frame and nothing else. Expected bytes are the reference's own recorded wire
bytes (tests/golden), or the host framer's layout with the oracle's CRCs
(tests/_oracle.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import _oracle, _prng, _sessions

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
ALL_LANES = (1, 2, 4, 8, 16, 32, 64)  # every k_pack instantiation
MAX_HINT = 8 + 65535


@pytest.fixture(scope="module")
def vc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import val_protocol_amd.crc as m

    m.init(0)
    m.set_geometry()
    yield m
    m.set_geometry()


@pytest.fixture(scope="module")
def wire(vc):
    import val_protocol_amd.wire as w

    return w


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "dropin_vectors.json")) as f:
        return json.load(f)


DEV = "cuda:0"


def _d64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _d32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _d8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


class Batch:
    """One batch's device inputs, uploaded once."""

    def __init__(self, payload, pay_off, pay_len, file_off, inc):
        self.n = len(pay_len)
        self.payload = _d8(payload) if payload is not None else None
        self.pay_off = _d64(pay_off) if pay_off is not None else None
        self.pay_len = _d32(pay_len)
        self.file_off = _d64(file_off)
        self.inc = _d8(inc) if inc is not None else None


def _run(wire, b: Batch, size, frame_off=None, *, out_stride=0, len_hint=0, stream=None, nrejected=None):
    """Build on the device into a 0xA5 canvas of `size` bytes ->
    (bytes, crc_len, crc, hdr, nrejected) as numpy."""
    out = torch.full((size,), CANARY, dtype=torch.uint8, device=DEV)
    hdr = torch.full((b.n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    fo = _d64(frame_off) if frame_off is not None else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    cl, crc, nrej = wire.build_data_batch_dev(b.payload, b.pay_off, b.pay_len, b.file_off, b.inc, out=out, frame_off=fo,
                                              out_stride=out_stride, len_hint=len_hint, out_hdr=hdr, stream=stream,
                                              nrejected=nrejected)
    torch.cuda.synchronize()
    return out.cpu().numpy(), _u32(cl), _u32(crc), _u32(hdr), int(_u32(nrej)[0])


def _scatter(canvas, stream, src_off, dst_off, lens):
    """canvas[dst_off[i] : +lens[i]] = stream[src_off[i] : +lens[i]] for every i."""
    lens = np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    if total == 0:
        return
    start = np.cumsum(lens) - lens
    within = np.arange(total, dtype=np.int64) - np.repeat(start, lens)
    canvas[np.repeat(np.asarray(dst_off, dtype=np.int64), lens) + within] = \
        stream[np.repeat(np.asarray(src_off, dtype=np.int64), lens) + within]


def _expected(wire, payload, pay_off, pay_len, file_off, inc, frame_off, size):
    """Host framer + oracle CRCs, frames moved to frame_off on a 0xA5 canvas ->
    (bytes, crc_len, crc, hdr)."""
    stream, fo, cl = wire.build_data_batch(payload, pay_off, pay_len, file_off, inc)
    crc, hdr = _oracle.frames(stream, fo, cl, header=True, nthreads=8)
    tr = (fo + cl)[:, None].astype(np.int64) + np.arange(4)
    stream[tr] = (crc[:, None] >> (8 * np.arange(4, dtype=np.uint32))).astype(np.uint8)
    canvas = np.full(size, CANARY, dtype=np.uint8)
    shift = np.asarray(frame_off, dtype=np.int64) - fo.astype(np.int64)
    if shift.size and (shift == shift[0]).all():  # back to back: the framer's stream, moved as a whole
        canvas[int(shift[0]):int(shift[0]) + stream.size] = stream
    else:
        _scatter(canvas, stream, fo, frame_off, cl.astype(np.int64) + 4)
    return canvas, cl, crc, hdr


def _spread(pay_len, inc, dst_align, front=67):
    """Frame offsets 1..4 canary bytes apart with frame_off % 4 == dst_align[i]."""
    pos, off = front, []
    for pl, ex, al in zip(pay_len, inc, dst_align):
        pos += 1
        pos += (int(al) - pos) % 4
        off.append(pos)
        pos += 12 + int(pl) + (8 if ex else 0)
    return np.array(off, dtype=np.uint64), pos + 61


# ---- 1. the reference's own wire bytes ------------------------------------------------
def test_reference_tx_frames(vc, wire, fx):
    recs = [r for r in fx["tx"] if r["payload_len"] + (8 if r["include_offset"] else 0) <= 0xFFFF]
    assert len(recs) >= 20
    pays = [_prng.prng_bytes(r["seed"], r["payload_len"]) for r in recs]
    pay_len = np.array([p.size for p in pays], dtype=np.uint32)
    pay_off = (np.cumsum(pay_len) - pay_len).astype(np.uint64)
    inc = np.array([r["include_offset"] for r in recs], dtype=np.uint8)
    file_off = np.array([r["offset"] for r in recs], dtype=np.uint64)
    frame_off, size = _spread(pay_len, inc, np.arange(len(recs)) % 4)
    want = np.full(size, CANARY, dtype=np.uint8)
    for r, p, o in zip(recs, pays, frame_off):
        # "prefix" is the frame's first min(16, CRC input) bytes as the reference sent them: the header, the
        # offset when present, and for an implied frame its first payload bytes
        head = bytes.fromhex(r["prefix"])
        hs = 16 if r["include_offset"] else 8
        assert head[hs:] == p.tobytes()[:len(head) - hs]
        f = head[:hs] + p.tobytes() + int(r["trailer"]).to_bytes(4, "little")
        assert len(f) == r["wire_len"]
        want[int(o):int(o) + len(f)] = np.frombuffer(f, dtype=np.uint8)
    b = Batch(np.concatenate(pays), pay_off, pay_len, file_off, inc)
    got, cl, crc, _, nrej = _run(wire, b, size, frame_off)
    assert np.array_equal(got, want)
    assert crc.tolist() == [r["trailer"] for r in recs] and cl.tolist() == [r["wire_len"] - 4 for r in recs]
    assert nrej == 0


@pytest.mark.parametrize("k", range(5))
def test_reference_windows(vc, wire, fx, k):
    w = fx["windows"][k]
    file = _prng.prng_bytes(w["file_seed"], w["file_size"])
    fr = np.array(w["frames"], dtype=np.uint64)
    b = Batch(file, fr[:, 0], fr[:, 1].astype(np.uint32), fr[:, 0], fr[:, 2].astype(np.uint8))
    fo, cl, total = wire.data_layout(fr[:, 1].astype(np.uint32), fr[:, 2].astype(np.uint8))
    assert total == w["wire_bytes"]
    front = 37
    got, cl_d, crc, _, nrej = _run(wire, b, total + front + 50, fo + np.uint64(front), len_hint=w["mtu"] - 4)
    stream = got[front:front + total]
    assert (got[:front] == CANARY).all() and (got[front + total:] == CANARY).all()
    assert vc.val_crc32(stream.tobytes()) == w["wire_crc"]
    assert crc.tolist() == w["trailers"] and np.array_equal(cl_d, cl) and nrej == 0


@pytest.mark.parametrize("name", ["window64_mtu1024", "window64_mtu16404", "resume_tail_cap8m", "resume_tail_cap1k"])
def test_reference_sessions(vc, wire, name):
    s = _sessions.load()[name]
    file = _sessions.input_file(s)
    d_file = _d8(file)
    data_recs = [r for r in s["tx_frames"] if r[0] == _sessions.PKT_DATA]
    k = 0
    for pay_off, pay_len, inc, trailers in _sessions.windows(s):
        b = Batch(None, pay_off, pay_len, pay_off, inc)
        b.payload = d_file
        fo, cl, total = wire.data_layout(pay_len, inc)
        front = 5 + k % 4
        got, _, crc, _, nrej = _run(wire, b, total + front + 9, fo + np.uint64(front))
        want = np.full(got.size, CANARY, dtype=np.uint8)
        want[front:front + total] = _sessions.wire_stream(data_recs[k:k + len(trailers)], file)
        assert np.array_equal(got, want), (name, k)
        assert np.array_equal(crc, trailers) and nrej == 0
        k += len(trailers)
    assert k == len(data_recs)


# ---- 2. edges ---------------------------------------------------------------------------
EDGE_LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 39, 40, 41, 47, 48, 49, 55, 56, 57, 63, 64, 65, 111, 112, 113, 119, 120, 121,
             127, 128, 129, 1003, 1004, 1005, 1011, 1012, 1013, 2047, 2048, 2049, 16375, 16376, 16377, 65519, 65527]


@pytest.fixture(scope="module")
def edges(wire):
    cases = [(pl, ex, sa, da, None) for pl in EDGE_LENS for ex in (1, 0) for sa in range(4) for da in range(4)]
    cases += [(65535, 0, sa, da, None) for sa in range(4) for da in range(4)]
    # payloads that start s bytes before a 128-byte line boundary and end e bytes after one
    i = 0
    for s in (1, 2, 3):
        for e in (1, 2, 3):
            for lines in (0, 1, 8):
                cases.append((128 * lines + s + e, i & 1, None, i % 4, s))
                i += 1
    pay_off, pos = [], 256
    for pl, ex, sa, da, before in cases:
        pos = (pos + 127) // 128 * 128 + 128  # a fresh line: no payload shares one with its neighbour
        start = pos - before if before is not None else pos + 4 + sa
        pay_off.append(start)
        pos = start + pl
    payload = np.random.default_rng(2024).integers(0, 256, pos + 256, dtype=np.uint8)
    pay_len = np.array([c[0] for c in cases], dtype=np.uint32)
    inc = np.array([c[1] for c in cases], dtype=np.uint8)
    pay_off = np.array(pay_off, dtype=np.uint64)
    file_off = np.random.default_rng(7).integers(0, 1 << 63, len(cases), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    frame_off, size = _spread(pay_len, inc, [c[3] for c in cases])
    assert 1400 <= len(cases) <= 1700
    want = _expected(wire, payload, pay_off, pay_len, file_off, inc, frame_off, size)
    return Batch(payload, pay_off, pay_len, file_off, inc), frame_off, size, want


@pytest.mark.parametrize("lanes,len_hint", [(0, 0), (0, MAX_HINT)] + [(g, 0) for g in ALL_LANES])
def test_edges(vc, wire, edges, lanes, len_hint):
    b, frame_off, size, (want, want_cl, want_crc, want_hdr) = edges
    vc.set_lanes_per_frame(lanes)
    try:
        got, cl, crc, hdr, nrej = _run(wire, b, size, frame_off, len_hint=len_hint)
    finally:
        vc.set_lanes_per_frame(0)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (lanes, "first differing byte", int(bad[0]), "frame",
                           int(np.searchsorted(frame_off, bad[0], side="right")) - 1)
    assert np.array_equal(cl, want_cl) and np.array_equal(crc, want_crc) and np.array_equal(hdr, want_hdr)
    assert nrej == 0


# ---- 3. slot mode -----------------------------------------------------------------------
def _window_shape(last):
    pay_len = np.array([1004] + [1012] * 298 + [last], dtype=np.uint32)
    inc = np.array([1] + [0] * 299, dtype=np.uint8)
    pay_off = (np.cumsum(pay_len) - pay_len).astype(np.uint64)
    payload = np.random.default_rng(last).integers(0, 256, int(pay_len.sum()), dtype=np.uint8)
    return payload, pay_off, pay_len, inc


@pytest.mark.parametrize("stride", [1024, 1031])
@pytest.mark.parametrize("last", [1, 517, 1011])
def test_slot_mode(vc, wire, stride, last):
    payload, pay_off, pay_len, inc = _window_shape(last)
    n = pay_len.size
    slots = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    size = n * stride
    want, want_cl, want_crc, want_hdr = _expected(wire, payload, pay_off, pay_len, pay_off, inc, slots, size)
    b = Batch(payload, pay_off, pay_len, pay_off, inc)
    got, cl, crc, hdr, nrej = _run(wire, b, size, None, out_stride=stride, len_hint=1020)
    assert np.array_equal(got, want)
    tail = got.reshape(n, stride)[-1, 12 + last:]
    assert tail.size and (tail == CANARY).all()  # the short last slot's unused tail
    assert np.array_equal(cl, want_cl) and np.array_equal(crc, want_crc) and np.array_equal(hdr, want_hdr)
    assert nrej == 0


def test_slot_too_small_rejects_full_frames(vc, wire):
    payload, pay_off, pay_len, inc = _window_shape(1011)  # 12 + 1011 = 1023 still fits
    n, stride = pay_len.size, 1023
    b = Batch(payload, pay_off, pay_len, pay_off, inc)
    got, cl, crc, hdr, nrej = _run(wire, b, n * stride, None, out_stride=stride)
    assert nrej == n - 1
    assert (got[:(n - 1) * stride] == CANARY).all()
    assert not cl[:-1].any() and not crc[:-1].any() and not hdr[:-1].any()
    want, want_cl, want_crc, want_hdr = _expected(wire, payload, pay_off[-1:], pay_len[-1:], pay_off[-1:], inc[-1:],
                                                  [(n - 1) * stride], n * stride)
    assert np.array_equal(got, want)
    assert cl[-1] == want_cl[0] and crc[-1] == want_crc[0] and hdr[-1] == want_hdr[0]


# ---- 4. more frames than one pass of the grid ------------------------------------------
def test_more_frames_than_one_grid_pass(vc, wire):
    n = 300_000  # one pass: at most 256 CUs x 16 waves x 64 single-lane frames = 262,144
    rng = np.random.default_rng(4)
    pay_len = rng.integers(40, 121, n).astype(np.uint32)
    inc = (rng.integers(0, 4, n) == 0).astype(np.uint8)
    pay_off = (np.cumsum(pay_len) - pay_len).astype(np.uint64)
    payload = rng.integers(0, 256, int(pay_len.sum()), dtype=np.uint8)
    fo, _, total = wire.data_layout(pay_len, inc)
    front = 131
    frame_off = fo + np.uint64(front)
    want, want_cl, want_crc, want_hdr = _expected(wire, payload, pay_off, pay_len, pay_off, inc, frame_off,
                                                  total + front + 77)
    b = Batch(payload, pay_off, pay_len, pay_off, inc)
    vc.set_lanes_per_frame(1)
    try:
        got, cl, crc, hdr, nrej = _run(wire, b, want.size, frame_off)
    finally:
        vc.set_lanes_per_frame(0)
    assert np.array_equal(got, want)
    assert np.array_equal(cl, want_cl) and np.array_equal(crc, want_crc) and np.array_equal(hdr, want_hdr)
    assert nrej == 0


# ---- 5. rejects inside a batch -----------------------------------------------------------
@pytest.mark.parametrize("lanes", [0, 1, 16])
def test_rejects_inside_a_batch(vc, wire, lanes):
    pay_len = np.array([700, 65528, 33, 65536, 1012, 5], dtype=np.uint32)
    inc = np.array([1, 1, 0, 0, 0, 1], dtype=np.uint8)
    pay_off = (np.cumsum(pay_len) - pay_len + 3).astype(np.uint64)
    payload = np.random.default_rng(5).integers(0, 256, int(pay_len.sum()) + 8, dtype=np.uint8)
    frame_off, size = _spread(pay_len, inc, [1, 2, 3, 0, 1, 2])  # the rejected frames keep their reserved bytes
    good = np.array([0, 2, 4, 5])
    want, want_cl, want_crc, want_hdr = _expected(wire, payload, pay_off[good], pay_len[good], pay_off[good], inc[good],
                                                  frame_off[good], size)
    b = Batch(payload, pay_off, pay_len, pay_off, inc)
    start = torch.full((1,), 40, dtype=torch.int32, device=DEV)
    vc.set_lanes_per_frame(lanes)
    try:
        got, cl, crc, hdr, nrej = _run(wire, b, size, frame_off, nrejected=start)
    finally:
        vc.set_lanes_per_frame(0)
    assert nrej == 42
    assert np.array_equal(got, want)
    for out, w in ((cl, want_cl), (crc, want_crc), (hdr, want_hdr)):
        assert np.array_equal(out[good], w) and out[1] == 0 and out[3] == 0


# ---- 6. round trip and reuse --------------------------------------------------------------
def test_round_trip_and_reuse(vc, wire):
    n = 257
    pay_len = np.array([4088] + [4096 - 12] * (n - 2) + [1234], dtype=np.uint32)
    inc = np.array([1] + [0] * (n - 1), dtype=np.uint8)
    pay_off = (np.cumsum(pay_len) - pay_len).astype(np.uint64)
    file = np.random.default_rng(6).integers(0, 256, int(pay_len.sum()), dtype=np.uint8)
    fo, cl, total = wire.data_layout(pay_len, inc)
    b = Batch(file, pay_off, pay_len, pay_off, inc)
    d_fo, d_cl = _d64(fo), _d32(cl)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()

    def build(stream):
        out = torch.full((total,), CANARY, dtype=torch.uint8, device=DEV)
        stream.wait_stream(torch.cuda.current_stream())
        cl_d, crc, nrej = wire.build_data_batch_dev(b.payload, b.pay_off, b.pay_len, b.file_off, b.inc, out=out,
                                                    frame_off=d_fo, len_hint=4096, stream=stream)
        return out, cl_d, crc, nrej

    out, cl_d, crc, nrej = build(s1)
    with torch.cuda.stream(s1):
        ok, nbad, pay = vc.verify_frames_ex(out, off=d_fo, length=cl_d, len_hint=4096, stream=s1)
    torch.cuda.synchronize()
    entries = vc.scratch_entries(0)[0]
    assert ok.cpu().numpy().all() and int(nbad.item()) == 0 and int(nrej.item()) == 0
    assert np.array_equal(_u32(cl_d), cl)
    state, folded = vc.fold_payload_states(0xFFFFFFFF, _u32(pay), pay_len)
    assert folded == n and state == vc.val_crc32_update_state(0xFFFFFFFF, file)
    first = out.cpu().numpy(), _u32(crc)
    again = build(s1)
    torch.cuda.synchronize()
    assert vc.scratch_entries(0)[0] == entries  # the same stream: nothing new
    other = build(s2)
    torch.cuda.synchronize()
    assert vc.scratch_entries(0)[0] <= entries + 1  # at most one entry per stream
    for o, _, c, r in (again, other):
        assert np.array_equal(o.cpu().numpy(), first[0]) and np.array_equal(_u32(c), first[1]) and int(r.item()) == 0


# ---- 7. argument checks (refused on the host, before any launch) ---------------------------
def test_argument_checks(vc, wire):
    lib = vc.lib()
    t = torch.zeros(64, dtype=torch.uint8, device=DEV)
    p, z = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(0)

    def call(payload=p, pay_off=p, pay_len=p, file_off=p, inc=z, n=1, out=p, frame_off=p, stride=0):
        return lib.val_frame_data_batch_dev(payload, pay_off, pay_len, file_off, inc, n, out, frame_off, stride, 0,
                                            z, z, z, z, z)

    assert call(n=0) == vc.VAL_OK
    assert call(n=0, out=z, pay_len=z, file_off=z, frame_off=z) == vc.VAL_OK
    for bad in ({"out": z}, {"pay_len": z}, {"file_off": z}, {"frame_off": z, "stride": 11},
                {"frame_off": z, "stride": 0}):
        assert call(**bad) == vc.VAL_ERR_INVALID_ARG, bad
        assert vc.last_error(), bad
    torch.cuda.synchronize()
    assert not t.cpu().numpy().any()
