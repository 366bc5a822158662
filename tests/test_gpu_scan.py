"""val_frame_scan_streams_dev: byte streams in HBM walked into frame
descriptors on the device (include/val_crc32_gpu.h).

Expected values never come from the device path: wire.scan_frames (the host's
val_frame_scan) runs per stream on the same bytes, and the layout rules of the
header (compaction in stream order, d_first, absolute offsets, (0, 0) padding)
are applied to its results in numpy.

Every call goes through _scan: the streams sit in one larger device buffer of
pseudo-random bytes, their starts cover all four phases of d_stream_off % 4,
and each stream is followed by the rest of a frame it was cut in (when it was)
and then by two whole frames, so a walk that did not honour `len` would find
more frames than the host. The outputs are over-allocated and filled with a
canary that must survive past n_streams * max_frames and past
d_first[n_streams]."""
import numpy as np
import pytest

from tests import _prng
from tests.test_gpu_unpack import DEV, _d8, _d32, _d64, _frame, vc, wire  # noqa: F401 - vc and wire are fixtures
from tests.test_gpu_unpack_files import Files, _small_frames

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAD = 5  # canary entries behind every output
C64, C32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
OUTS = ("nframes", "consumed", "status")
FRONTS = (0, 64, 1024)  # val_gpu_set_scan_front


def _f(wire, content, fill=None):
    """A control-free DATA frame of 12 + content wire bytes (implied offset)."""
    pay = np.full(content, 0xEE, np.uint8) if fill is None else np.asarray(fill, dtype=np.uint8)
    assert pay.size == content
    return _frame(wire, pay)


def _cat(frames):
    return np.concatenate(frames) if len(frames) else np.zeros(0, np.uint8)


def _host(wire, stream, mtu, max_frames):
    if max_frames == 0:  # the host's loop does not start: nothing scanned, nothing consumed
        return 0, np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0
    return wire.scan_frames(stream, mtu, max_frames)


def _scan(vc, wire, streams, mtu, max_frames, *, phases=(0, 1, 2, 3), null=(), fronts=FRONTS):
    """streams: list of (bytes, len) or plain byte arrays; the stream is bytes[:len] and bytes[len:]
    follows it in the buffer. The whole list is laid out once per phase shift, so every stream starts
    at every phase of phases. -> the per-stream host results of the first copy."""
    streams = [(s, s.size) if isinstance(s, np.ndarray) else s for s in streams]
    n0 = len(streams)
    laid = [(full, ln, (i + c) % 4) for c in phases for i, (full, ln) in enumerate(streams)]
    S = len(laid)
    after = _cat([_f(wire, 0), _f(wire, 3)])
    pos, soff = 9, []
    for full, ln, ph in laid:
        pos += (ph - pos) % 4
        soff.append(pos)
        pos += full.size + after.size + 1
    buf = _prng.prng_bytes(1234, pos + 8)
    for o, (full, ln, ph) in zip(soff, laid):
        buf[o:o + full.size] = full
        buf[o + full.size:o + full.size + after.size] = after
    soff = np.array(soff, dtype=np.uint64)
    slen = np.array([ln for _, ln, _ in laid], dtype=np.uint64)
    assert S < 4 or sorted(set((soff % 4).tolist())) == [0, 1, 2, 3]
    slots = S * max_frames
    base = _d8(buf)
    assert base.data_ptr() % 4 == 0
    d_soff, d_slen = _d64(soff), _d64(slen)
    want = [_host(wire, full[:ln], mtu, max_frames) for full, ln, _ in laid]
    cnt = np.array([w[1].size for w in want], dtype=np.uint64)
    total = int(cnt.sum())
    w_first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    w_off = np.concatenate([w[1] + soff[s] for s, w in enumerate(want)] + [np.zeros(slots - total, np.uint64)])
    w_len = np.concatenate([w[2] for w in want] + [np.zeros(slots - total, np.uint32)])
    for front in fronts:  # automatic, then each instantiation of the walk: the results are the same
        foff = torch.full((slots + PAD,), C64, dtype=torch.int64, device=DEV)
        clen = torch.full((slots + PAD,), C32, dtype=torch.int32, device=DEV)
        first = torch.full((S + 1 + PAD,), C32, dtype=torch.int32, device=DEV)
        out = dict(nframes=torch.full((S + PAD,), C32, dtype=torch.int32, device=DEV),
                   consumed=torch.full((S + PAD,), C64, dtype=torch.int64, device=DEV),
                   status=torch.full((S + PAD,), C32, dtype=torch.int32, device=DEV))
        work = torch.empty(max(wire.scan_work_bytes(S, max_frames), 16), dtype=torch.uint8, device=DEV)
        ptr = lambda t: t.data_ptr()  # noqa: E731
        args = [None if k in null else ptr(out[k]) for k in OUTS]
        vc.set_scan_front(front)
        try:
            st = vc.lib().val_frame_scan_streams_dev(ptr(base), ptr(d_soff), ptr(d_slen), S, mtu, max_frames,
                                                     ptr(foff), ptr(clen), ptr(first), *args, ptr(work), work.numel(),
                                                     torch.cuda.current_stream().cuda_stream)
        finally:
            vc.set_scan_front(0)
        assert st == vc.VAL_OK, vc.last_error()
        torch.cuda.synchronize()
        g_off = foff.cpu().numpy().view(np.uint64)
        g_len = clen.cpu().numpy().view(np.uint32)
        g_first = first.cpu().numpy().view(np.uint32)
        assert np.array_equal(g_first[:S + 1], w_first), (g_first[:S + 1][:12], w_first[:12])
        bad = np.flatnonzero((g_off[:slots] != w_off) | (g_len[:slots] != w_len))
        assert bad.size == 0, (bad[:8], g_off[bad[:8]], w_off[bad[:8]], g_len[bad[:8]], w_len[bad[:8]])
        assert (g_off[slots:] == C64).all() and (g_len[slots:] == C32).all() and (g_first[S + 1:] == C32).all()
        w_out = dict(nframes=cnt.astype(np.uint32), consumed=np.array([w[3] for w in want], dtype=np.uint64),
                     status=np.array([w[0] for w in want], dtype=np.int32))
        for k in OUTS:
            g = out[k].cpu().numpy()
            g = g.view(np.uint64) if k == "consumed" else g.view(w_out[k].dtype)
            canary = C64 if k == "consumed" else np.array(C32, np.uint32).astype(w_out[k].dtype)
            if k in null:
                assert (g == canary).all(), k
                continue
            bad = np.flatnonzero(g[:S] != w_out[k])
            assert bad.size == 0, (k, bad[:8], g[bad[:8]], w_out[k][bad[:8]])
            assert (g[S:] == canary).all(), k
    return want[:n0]


# ---- 1. runs ----------------------------------------------------------------------------------
def test_uniform_runs(vc, wire):
    """300 frames of 40 wire bytes and a shorter last one: several full-match rounds."""
    s = _cat([_f(wire, 28)] * 300 + [_f(wire, 5)])
    (st, off, ln, used), = _scan(vc, wire, [s], 1024, 1000)
    assert (st, off.size, used) == (0, 301, s.size) and ln[-1] == 13


def test_no_runs(vc, wire):
    """500 frames with random content 0..100: a prediction rarely holds."""
    content = np.random.default_rng(8).integers(0, 101, 500)
    content[[0, 7, 8, 499]] = 0
    s = _cat([_f(wire, int(c)) for c in content])
    (st, off, ln, used), = _scan(vc, wire, [s], 1024, 600)
    assert (st, off.size, used) == (0, 500, s.size) and (ln == content + 8).all()


@pytest.mark.parametrize("run", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_front_width_boundaries(vc, wire, run):
    """A run of 64 k - 1, 64 k and 64 k + 1 frames (k = 1, 4, 16), then a frame of another size,
    then the run's size again. For the one-wave walk, whose rounds end at frames 1 + 64 k, the
    runs of 64 k + 1 end on a round and the others one and two frames before it. The wide front
    looks with 64, 256 and 1,024 lanes in turn, so its rounds end at frames 1, 65, 321 and 1,345:
    of these only 65 is a run here, and no run is long enough for a round in which all 1,024
    lanes match. Those edges are in test_gpu_window_edges.py."""
    content = run % 5  # wire 12 .. 16
    other = (content + 2) % 5
    s = _cat([_f(wire, content)] * run + [_f(wire, other)] + [_f(wire, content)] * 3)
    (st, off, ln, used), = _scan(vc, wire, [s], 1024, 2000)
    assert (st, off.size, used) == (0, run + 4, s.size) and ln[run] == 8 + other


# ---- 2. decoys --------------------------------------------------------------------------------
def _decoy(P, mult):
    """Payload of a frame of mult * P wire bytes that reads, at every predicted position
    (multiples of P into the frame), as the header of a frame of P wire bytes."""
    pay = np.full(mult * P - 12, 0xEE, np.uint8)
    for j in range(1, mult):
        at = j * P - 8  # payload byte of frame byte j * P
        pay[at:at + 8] = [5, 0, (P - 12) & 0xFF, (P - 12) >> 8, 0, 0, 0, 0]
    return pay


def test_decoy_headers_behind_a_mismatch(vc, wire):
    """Frames of P, then of 2P and 3P whose payload holds matching headers where the lanes look;
    real frames of P follow, so lanes behind the decoys match too. Only the leading run counts."""
    P = 40
    a = _f(wire, P - 12)
    b = _f(wire, 2 * P - 12, _decoy(P, 2))
    c = _f(wire, 3 * P - 12, _decoy(P, 3))
    s = _cat([a] * 3 + [b] + [a] * 2 + [c] + [a] * 70 + [b, c, b])
    (st, off, ln, used), = _scan(vc, wire, [s], 1024, 200)
    assert (st, off.size, used) == (0, 80, s.size)
    assert ln[3] == 2 * P - 4 and ln[6] == 3 * P - 4


def test_decoy_that_alone_is_complete(vc, wire):
    """The stream ends inside the frame of 3P; the decoys in it are whole frames of P that fit.
    The host stops in front of the long frame."""
    P = 40
    a = _f(wire, P - 12)
    c = _f(wire, 3 * P - 12, _decoy(P, 3))
    full = _cat([a] * 3 + [c])
    for cut in (3 * P - 1, 2 * P, 2 * P + 1):
        (st, off, ln, used), = _scan(vc, wire, [(full, 3 * P + cut)], 1024, 200)
        assert (st, off.size, used) == (0, 3, 3 * P)
    # and one whose own content is beyond the MTU: a protocol error, whatever its payload reads as
    (st, off, ln, used), = _scan(vc, wire, [_cat([a] * 3 + [c] + [a] * 4)], 3 * P - 1, 200)
    assert (st, off.size, used) == (vc.VAL_ERR_PROTOCOL, 3, 3 * P)


# ---- 3. stops ---------------------------------------------------------------------------------
def test_tails_and_cut_frames(vc, wire):
    """1..7 bytes behind the last frame; the last frame cut to 8, 9, 11 and wire - 1 bytes. What
    follows the cut in the buffer is the rest of that frame."""
    run = [_f(wire, 20)] * 70
    last = _f(wire, 33)
    full = _cat(run + [last])
    head = 70 * 32
    streams = [(full, head + t) for t in list(range(1, 8)) + [8, 9, 11, last.size - 1]]
    for st, off, ln, used in _scan(vc, wire, streams, 1024, 100):
        assert (st, off.size, used) == (0, 70, head)
    (st, off, ln, used), = _scan(vc, wire, [(full, head + last.size)], 1024, 100)
    assert (off.size, used) == (71, full.size)


@pytest.mark.parametrize("at", [0, 1, 63, 64, 65])
def test_content_beyond_the_mtu(vc, wire, at):
    """content_len == max_content is a frame; max_content + 1 at frame `at` of a uniform run of
    full-size frames stops the stream there with VAL_ERR_PROTOCOL and keeps the frames before it."""
    mtu = 52
    ok, over = _f(wire, mtu - 12), _f(wire, mtu - 11)
    frames = [ok] * 70
    (st, off, ln, used), = _scan(vc, wire, [_cat(frames)], mtu, 100)
    assert (st, off.size, used) == (0, 70, 70 * mtu)
    frames[at] = over
    (st, off, ln, used), = _scan(vc, wire, [_cat(frames)], mtu, 100)
    assert (st, off.size, used) == (vc.VAL_ERR_PROTOCOL, at, at * mtu)
    # at the frame limit the offending header is not looked at
    if at:
        (st, off, ln, used), = _scan(vc, wire, [_cat(frames)], mtu, at)
        assert (st, off.size, used) == (0, at, at * mtu)


def test_smallest_mtu_and_shortest_streams(vc, wire):
    """mtu = 12 admits empty frames only; streams of 0 and of 5 bytes hold no header."""
    empty = _f(wire, 0)
    s = _cat([empty] * 70 + [_f(wire, 1)] + [empty])
    (st, off, ln, used), = _scan(vc, wire, [s], 12, 100)
    assert (st, off.size, used) == (vc.VAL_ERR_PROTOCOL, 70, 840) and (ln == 8).all()
    full = _cat([empty] * 3)
    for st, off, ln, used in _scan(vc, wire, [(full, 0), (full, 5)], 12, 100):
        assert (st, off.size, used) == (0, 0, 0)


@pytest.mark.parametrize("max_frames", [0, 1, 63, 64, 65])
def test_frame_limit(vc, wire, max_frames):
    """A run of 200 against max_frames: consumed is the end of the last frame emitted."""
    s = _cat([_f(wire, 9)] * 200)
    (st, off, ln, used), = _scan(vc, wire, [s], 1024, max_frames)
    assert (st, off.size, used) == (0, max_frames, 21 * max_frames)
    # the limit inside a run that follows a frame of another size
    t = _cat([_f(wire, 2)] + [_f(wire, 9)] * 200)
    (st, off, ln, used), = _scan(vc, wire, [t], 1024, max_frames)
    assert (st, off.size) == (0, max_frames) and used == (14 + 21 * (max_frames - 1) if max_frames else 0)


# ---- 4. many streams --------------------------------------------------------------------------
def _mixed_streams(wire, S, seed):
    """S streams with mixed counts: empty ones, runs, random sizes, one cut by the frame limit of 32,
    one that stops on a protocol error (mtu 112), some cut inside their last frame."""
    rng = np.random.default_rng(seed)
    pool = [_f(wire, c) for c in range(0, 101)]
    streams = []
    for s in range(S):
        kind = s % 6 if S > 1 else 1
        if kind == 0:
            streams.append((pool[4], 0) if s % 12 else np.zeros(0, np.uint8))  # empty
        elif kind == 1:
            streams.append(_cat([pool[int(c)] for c in rng.integers(0, 101, int(rng.integers(1, 30)))]))
        elif kind == 2:
            streams.append(_cat([pool[60]] * 40 + [pool[1]]))  # cut by max_frames = 32
        elif kind == 3:
            streams.append(_cat([pool[7]] * 5 + [_f(wire, 101)] + [pool[7]] * 2))  # protocol error at 5
        elif kind == 4:
            full = _cat([pool[100]] * int(rng.integers(1, 32)) + [pool[50]])
            streams.append((full, full.size - int(rng.integers(1, 62))))
        else:
            streams.append(_cat([pool[int(rng.integers(0, 20))]] * int(rng.integers(1, 32))))
    return streams


@pytest.mark.parametrize("S", [1, 3, 300])
def test_many_streams(vc, wire, S):
    streams = _mixed_streams(wire, S, seed=S)
    phases = (0, 1, 2, 3) if S < 300 else (0,)  # 300 streams in a row cover every phase by themselves
    want = _scan(vc, wire, streams, 112, 32, phases=phases)
    if S >= 3:
        assert want[2][1].size == 32 and want[2][3] == 32 * 72  # cut by the limit
    if S == 300:
        assert want[3][0] == vc.VAL_ERR_PROTOCOL and want[3][1].size == 5
        assert want[0][1].size == 0 and want[6][1].size == 0
        assert len({w[1].size for w in want}) > 20
    # every nullable per-stream output left out, one by one and all together
    for null in [("nframes",), ("consumed",), ("status",), OUTS]:
        _scan(vc, wire, streams, 112, 32, phases=phases[:1], null=null)


# ---- 5. scan, then unpack, nothing read in between ----------------------------------------------
def test_scan_then_unpack_without_a_read_back(vc, wire):
    """Five transfers, one stream each (a stream has to be contiguous, so the frames are laid back
    to back here, not through Window's fillers): one has a corrupt trailer, one a gap, one ends
    inside a frame, one is empty. scan_streams_dev and unpack_data_files_dev with
    n = S * max_frames and the device's `first` run back to back on a side stream; the expected
    files come from the same unpack call driven with the host's descriptors and the exact n."""
    S, max_frames, mtu = 5, 64, 1024
    spec = [(40, [], [17]), (25, [9], []), (50, [], []), (0, [], []), (30, [], [])]
    frames, ends = [], []
    for s, (nf, gaps, bad) in enumerate(spec):
        f, end = _small_frames(wire, nf, 3 * s, gap_at=gaps, corrupt_at=bad, seed=40 + s) if nf else ([], 3 * s)
        frames.append(f)
        ends.append(end)
    streams = [_cat(f) for f in frames]
    cut = frames[4][-1].size - 2  # the last frame of stream 4 has not arrived in full
    lens = [s.size for s in streams]
    lens[4] -= cut
    pos, soff = 6, []
    for s in range(S):
        pos += (s - pos) % 4
        soff.append(pos)
        pos += streams[s].size + 3
    buf = _prng.prng_bytes(77, pos + 8)
    for o, s in zip(soff, streams):
        buf[o:o + s.size] = s
    base, d_soff, d_slen = _d8(buf), _d64(soff), _d64(lens)
    w0 = [3 * s for s in range(S)]
    sizes = [e + 40 for e in ends]
    state = [0xFFFFFFFF, 11, 22, 33, 44]

    def unpack(lay, first, off, length, n, stream=None):
        r = wire.unpack_data_files_dev(base, first=first, file_ptr=lay.ptr, file_cap=lay.cap, written=lay.written,
                                       off=off, length=length, n=n, len_hint=24, file_state=lay.state,
                                       naccepted=lay.nacc, noverflow=lay.novf, file_nbad=lay.fnbad, nbad=None,
                                       stream=stream)
        lay.ok.append(r[0])
        lay.accept.append(r[1])
        return r

    # the device route
    lay = Files(sizes, written=w0, state=state)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        foff, clen, first, nfr, cons, stat = wire.scan_streams_dev(base, d_soff, d_slen, mtu, max_frames, stream=side)
        ok, accept, *_ = unpack(lay, first, foff, clen, S * max_frames, stream=side)
    side.synchronize()
    got = lay.result()
    # the host route: val_frame_scan per stream, the exact n
    h = [wire.scan_frames(buf[o:o + n], mtu, max_frames) for o, n in zip(soff, lens)]
    cnt = [x[1].size for x in h]
    assert cnt == [40, 25, 50, 0, 29] and [x[3] for x in h][4] == lens[4] - (frames[4][-1].size - cut)
    h_first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    h_off = np.concatenate([x[1] + np.uint64(o) for x, o in zip(h, soff)])
    h_len = np.concatenate([x[2] for x in h])
    ref = Files(sizes, written=w0, state=state)
    r_ok, r_accept, *_ = unpack(ref, _d32(h_first), _d64(h_off), _d32(h_len), int(h_first[-1]))
    want = ref.result()
    total = int(h_first[-1])
    for k in ("canvas", "written", "state", "nacc", "novf", "fnbad"):
        assert np.array_equal(got[k], want[k]), (k, got[k][:8], want[k][:8])
    accept = accept.cpu().numpy()
    assert np.array_equal(accept[:total], r_accept.cpu().numpy()) and not accept[total:].any()
    assert accept.size == S * max_frames
    assert np.array_equal(nfr.cpu().numpy(), cnt) and np.array_equal(first.cpu().numpy(), h_first)
    assert np.array_equal(cons.cpu().numpy(), [x[3] for x in h]) and not stat.cpu().numpy().any()
    # the transfers did what their frames say: the corrupt frame and the gap are the two that were not delivered
    assert want["fnbad"].tolist() == [1, 0, 0, 0, 0] and want["nacc"].tolist() == [39, 24, 50, 0, 29]
    assert want["written"][2] == ends[2]
