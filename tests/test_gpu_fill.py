"""val_frame_fill_files_dev: the send windows of many transfers filled on the
device, from file bytes in HBM to wire bytes with trailers
(include/val_crc32_gpu.h).

Expected values never come from the device path: wire.fill_window (the rule in
plain C) runs per transfer, wire.build_data_batch frames its result from the
same file bytes, the oracle supplies the trailers and header CRCs, and the
layout rules of the header (compaction in transfer order, d_first, absolute
offsets, zeros behind the total) are applied in numpy.

Every call goes through _fill: the files sit in one device buffer and the
streams in another, both of pseudo-random bytes, at all four phases of address
mod 4, with a few guard bytes between neighbours. The output canvas is compared
WHOLE against the expected one, so a byte written outside the frames made (in a
gap, behind a stream cut by its capacity) fails the test. The per-frame and
per-transfer outputs are over-allocated and filled with a canary that must
survive past n_files * max_frames and past d_first[n_files]. Every case runs
with the lanes per frame left to the library and forced to 1 and to 64."""
import numpy as np
import pytest

from tests import _oracle, _prng, _sessions
from tests.test_fill_rule import segments
from tests.test_gpu_unpack import DEV, _d8, _d32, _d64, vc, wire  # noqa: F401 - vc and wire are fixtures
from tests.test_gpu_unpack_files import Files

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAD = 5  # canary entries behind every output
C64, C32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
U64 = (1 << 64) - 1
LANES = (0, 1, 64)
PER_FRAME = ("crc_len", "crc", "hdr")
PER_FILE = ("stream_len", "nframes")
MTU = 112  # M = 100: small frames, so that many transfers stay a few megabytes


def T(data, next=0, la=None, budget=0xFFFFFFFF, cap=U64, virt=0):
    """One transfer: the file's bytes `data` stand for file offsets [virt, virt + len(data));
    la None = next (the first frame is explicit)."""
    data = np.asarray(data, dtype=np.uint8)
    return dict(data=data, virt=virt, size=virt + data.size, next=next, la=next if la is None else la,
                budget=budget, cap=cap)


def _bytes(seed, n):
    return _prng.prng_bytes(seed, n)


def _expect(wire, t, mtu, max_frames):
    """The host route for one transfer -> (wire bytes, frame_off rel, crc_len, crc, hdr, used, next)."""
    fo, pl, inc, off, cl, used, nxt = wire.fill_window(t["next"], t["la"], t["size"], mtu, min(t["budget"], max_frames),
                                                       t["cap"])
    if fo.size == 0:
        z32 = np.zeros(0, np.uint32)
        return np.zeros(0, np.uint8), np.zeros(0, np.uint64), z32, z32, z32, 0, nxt
    stream, b_off, b_len = wire.build_data_batch(t["data"], fo - np.uint64(t["virt"]), pl, fo, inc)
    assert stream.size == used and np.array_equal(b_off, off) and np.array_equal(b_len, cl)
    crc, hdr = _oracle.frames(stream, off, cl, header=True)
    wire.put_trailers(stream, off, cl, crc)
    return stream, off, cl, crc, hdr, used, nxt


def _fill(vc, wire, specs, mtu, max_frames, *, phases=(0, 1, 2, 3), null=(), lanes=LANES):
    """specs: list of T(...). The list is laid out once per phase shift, so every file and stream
    starts at every phase. -> the host results of the first copy, one per transfer."""
    n0 = len(specs)
    laid = [(t, (i + c) % 4, (i + 3 * c + 1) % 4) for c in phases for i, t in enumerate(specs)]
    S = len(laid)
    want = {}
    for i, t in enumerate(specs):
        want[i] = _expect(wire, t, mtu, max_frames)
    want = [want[i % n0] for i in range(S)]
    # the files
    pos, fpos = 13, []
    for t, ph, _ in laid:
        pos += (ph - pos) % 4
        fpos.append(pos)
        pos += t["data"].size + 5
    files = _bytes(4321, pos + 8)
    for o, (t, _, _) in zip(fpos, laid):
        files[o:o + t["data"].size] = t["data"]
    # the streams: what the host made and a gap; a capacity beyond that is room the call must not touch
    pos, soff = 7, []
    for (t, _, ph), w in zip(laid, want):
        pos += (ph - pos) % 4
        soff.append(pos)
        pos += w[5] + 3
    canvas0 = _bytes(8765, pos + 8)
    canvas = canvas0.copy()
    for o, w in zip(soff, want):
        canvas[o:o + w[5]] = w[0]
    if len(phases) == 4 or n0 >= 4:
        assert sorted(set(np.array(fpos) % 4)) == sorted(set(np.array(soff) % 4)) == [0, 1, 2, 3]
    soff = np.array(soff, dtype=np.uint64)
    slots = S * max_frames
    cnt = np.array([w[1].size for w in want], dtype=np.uint64)
    total = int(cnt.sum())
    w_first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    z = slots - total
    w_off = np.concatenate([w[1] + soff[s] for s, w in enumerate(want)] + [np.zeros(z, np.uint64)])
    w_frame = {k: np.concatenate([w[i] for w in want] + [np.zeros(z, np.uint32)])
               for k, i in (("crc_len", 2), ("crc", 3), ("hdr", 4))}
    w_file = dict(stream_len=np.array([w[5] for w in want], dtype=np.uint64), nframes=cnt.astype(np.uint32))
    w_next = np.array([w[6] for w in want], dtype=np.uint64)

    d_files = _d8(files)
    assert d_files.data_ptr() % 4 == 0
    d_fpos = _d64([(o - t["virt"]) & U64 for o, (t, _, _) in zip(fpos, laid)])
    d_size = _d64([t["size"] for t, _, _ in laid])
    d_la = _d64([t["la"] for t, _, _ in laid])
    d_budget = _d32([t["budget"] for t, _, _ in laid])
    d_soff = _d64(soff)
    d_cap = _d64([t["cap"] for t, _, _ in laid])
    ptr = lambda t: t.data_ptr()  # noqa: E731
    for ln in lanes:
        out = _d8(canvas0)
        assert out.data_ptr() % 4 == 0
        d_next = _d64([t["next"] for t, _, _ in laid] + [C64] * PAD)
        foff = torch.full((slots + PAD,), C64, dtype=torch.int64, device=DEV)
        first = torch.full((S + 1 + PAD,), C32, dtype=torch.int32, device=DEV)
        frame = {k: torch.full((slots + PAD,), C32, dtype=torch.int32, device=DEV) for k in PER_FRAME}
        per = dict(stream_len=torch.full((S + PAD,), C64, dtype=torch.int64, device=DEV),
                   nframes=torch.full((S + PAD,), C32, dtype=torch.int32, device=DEV))
        work = torch.empty(max(wire.fill_work_bytes(S, max_frames), 16), dtype=torch.uint8, device=DEV)
        arg = lambda k, t: None if k in null else ptr(t)  # noqa: E731
        vc.set_lanes_per_frame(ln)
        try:
            st = vc.lib().val_frame_fill_files_dev(
                ptr(d_files), ptr(d_fpos), ptr(d_size), ptr(d_next), ptr(d_la), arg("budget", d_budget), S, mtu,
                max_frames, ptr(out), ptr(d_soff), ptr(d_cap), arg("stream_len", per["stream_len"]),
                arg("nframes", per["nframes"]), ptr(first), ptr(foff), arg("crc_len", frame["crc_len"]),
                arg("crc", frame["crc"]), arg("hdr", frame["hdr"]), ptr(work), work.numel(),
                torch.cuda.current_stream().cuda_stream)
        finally:
            vc.set_lanes_per_frame(0)
        assert st == vc.VAL_OK, vc.last_error()
        torch.cuda.synchronize()
        g_canvas = out.cpu().numpy()
        bad = np.flatnonzero(g_canvas != canvas)
        assert bad.size == 0, (ln, bad[:8], g_canvas[bad[:8]], canvas[bad[:8]], soff[:4])
        g_first = first.cpu().numpy().view(np.uint32)
        assert np.array_equal(g_first[:S + 1], w_first), (ln, g_first[:S + 1][:12], w_first[:12])
        assert (g_first[S + 1:] == C32).all()
        g_off = foff.cpu().numpy().view(np.uint64)
        bad = np.flatnonzero(g_off[:slots] != w_off)
        assert bad.size == 0 and (g_off[slots:] == C64).all(), (ln, bad[:8], g_off[bad[:8]], w_off[bad[:8]])
        for k in PER_FRAME:
            g = frame[k].cpu().numpy().view(np.uint32)
            if k in null:
                assert (g == C32).all(), k
                continue
            bad = np.flatnonzero(g[:slots] != w_frame[k])
            assert bad.size == 0 and (g[slots:] == C32).all(), (ln, k, bad[:8], g[bad[:8]], w_frame[k][bad[:8]])
        for k in PER_FILE:
            g = per[k].cpu().numpy()
            g, canary = (g.view(np.uint64), C64) if k == "stream_len" else (g.view(np.uint32), C32)
            if k in null:
                assert (g == canary).all(), k
                continue
            bad = np.flatnonzero(g[:S] != w_file[k])
            assert bad.size == 0 and (g[S:] == canary).all(), (ln, k, bad[:8], g[bad[:8]], w_file[k][bad[:8]])
        g_next = d_next.cpu().numpy().view(np.uint64)
        bad = np.flatnonzero(g_next[:S] != w_next)
        assert bad.size == 0 and (g_next[S:] == C64).all(), (ln, bad[:8], g_next[bad[:8]], w_next[bad[:8]])
    return want[:n0]


# ---- 1. the rule's edges, one transfer each ----------------------------------------------------
M = MTU - 12
EDGES = {
    "remainder M - 8, explicit": (T(_bytes(1, M - 8 + 40), next=40), 1),
    "remainder M - 7, explicit": (T(_bytes(2, M - 7 + 40), next=40), 2),
    "remainder M, explicit": (T(_bytes(3, M), next=0), 2),
    "remainder M, implied": (T(_bytes(3, M + 9), next=9, la=0), 1),
    "remainder M + 1, implied": (T(_bytes(4, M + 10), next=9, la=0), 2),
    "remainder 1, explicit": (T(_bytes(5, 500), next=499), 1),
    "remainder 1, implied": (T(_bytes(5, 500), next=499, la=3), 1),
    "remainder 0": (T(_bytes(6, 500), next=500), 0),
    "empty file": (T(np.zeros(0, np.uint8)), 0),
    "next beyond the size": (T(_bytes(7, 500), next=501), 0),
    "next != last_acked": (T(_bytes(8, 1000), next=300, la=200), 7),
    "last_acked ahead, on a frame start": (T(_bytes(8, 1000), next=300, la=500), 8),
    "budget 0": (T(_bytes(9, 1000), budget=0), 0),
    "budget 1": (T(_bytes(10, 1000), budget=1), 1),
    "budget 1, implied": (T(_bytes(10, 1000), next=1, la=0, budget=1), 1),
    "capacity at a frame end": (T(_bytes(11, 1000), cap=3 * MTU), 3),
    "capacity one byte less": (T(_bytes(11, 1000), cap=3 * MTU - 1), 2),
    "capacity at the last frame's end": (T(_bytes(12, 250), cap=2 * MTU + 12 + 58), 3),
    "capacity a byte below the last frame's end": (T(_bytes(12, 250), cap=2 * MTU + 12 + 57), 2),
    "capacity 11": (T(_bytes(13, 1000), cap=11), 0),
    "capacity 0": (T(_bytes(13, 1000), cap=0), 0),
    "capacity a byte below one short frame": (T(_bytes(14, 3), cap=22), 0),
    "capacity of one short frame": (T(_bytes(14, 3), cap=23), 1),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges_one_transfer_each(vc, wire, name):
    t, frames = EDGES[name]
    for max_frames in (12, 1):
        (_, off, *_), = _fill(vc, wire, [t], MTU, max_frames)
        assert off.size == min(frames, max_frames, t["budget"])


def test_smallest_mtu(vc, wire):
    """mtu 21: the explicit frame carries one byte, implied ones nine."""
    want = _fill(vc, wire, [T(_bytes(20, 200)), T(_bytes(21, 200), next=5, la=4), T(_bytes(22, 12), next=11)], 21, 70)
    assert want[0][2].tolist() == [17] * 23 + [9] and want[0][6] == 200  # 1 + 22 * 9 + 1
    assert want[1][2].tolist() == [17] * 21 + [14] and want[2][2].tolist() == [17]


def test_largest_mtu(vc, wire):
    """mtu 65547: content 65,535, the most a header can say; one byte more in the file is one frame more."""
    a = T(_bytes(23, 65527 + 65535 + 1))
    b = T(_bytes(24, 2 * 65535), next=0, la=7, cap=2 * 65547)
    want = _fill(vc, wire, [a, b], 65547, 4, phases=(0, 1))
    assert want[0][2].tolist() == [65543, 65543, 9] and want[1][2].tolist() == [65543, 65543]


# ---- 2. many transfers ---------------------------------------------------------------------------
def _mixed(S, max_frames, seed):
    """S transfers in mixed states: finished files, next beyond the size, budget 0, cuts by the
    capacity (at a frame end and inside a frame), by max_frames and by a smaller budget, files that
    end inside the window, explicit and implied starts."""
    rng = np.random.default_rng(seed)
    pool = _bytes(seed, 1 << 16)
    out = []
    for s in range(S):
        kind = s % 8 if S >= 8 else (5, 3, 6, 0, 4, 7, 1, 2)[s]  # a few transfers: the ones that make frames
        nxt = int(rng.integers(0, 300))
        at = int(rng.integers(0, 4096))
        if kind == 0:
            out.append(T(pool[at:at + nxt], next=nxt))  # finished
        elif kind == 1:
            out.append(T(pool[at:at + nxt], next=nxt + 1 + s % 3))  # beyond the size
        elif kind == 2:
            out.append(T(pool[at:at + nxt + 700], next=nxt, budget=0))
        elif kind == 3:  # cut by the capacity
            k = int(rng.integers(0, max(max_frames, 1) + 1))
            out.append(T(pool[at:at + nxt + (max_frames + 2) * M], next=nxt, la=nxt if s % 16 < 8 else 0,
                         cap=k * MTU + int(rng.integers(0, MTU))))
        elif kind == 4:  # cut by max_frames
            out.append(T(pool[at:at + nxt + (max_frames + 1) * M + 1], next=nxt, budget=max_frames + 1 + s % 2))
        elif kind == 5:  # ends inside the window, explicit
            out.append(T(pool[at:at + nxt + int(rng.integers(1, max(max_frames, 1) * M - 8 + 1))], next=nxt))
        elif kind == 6:  # implied start
            out.append(T(pool[at:at + nxt + 1 + int(rng.integers(0, (max_frames + 3) * M))], next=nxt + 1,
                         la=int(rng.integers(0, nxt + 1))))
        else:  # a budget below max_frames
            out.append(T(pool[at:at + nxt + (max_frames + 2) * M], next=nxt, budget=int(rng.integers(0, max_frames + 1)),
                         cap=U64 if s % 16 < 8 else max_frames * MTU // 2))
    return out


@pytest.mark.parametrize("max_frames", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("S", [1, 3, 300, 1100])
def test_many_transfers(vc, wire, S, max_frames):
    specs = _mixed(S, max_frames, seed=1000 * S + max_frames)
    phases = (0, 1, 2, 3) if S < 300 else (0,)  # hundreds of transfers in a row cover every phase by themselves
    want = _fill(vc, wire, specs, MTU, max_frames, phases=phases)
    cnt = [w[1].size for w in want]
    if S >= 300 and max_frames >= 63:
        assert cnt[0] == cnt[1] == cnt[2] == 0 and cnt[4] == max_frames and len(set(cnt)) > 20
        assert any(0 < c < max_frames for c in cnt[3::8]) and any(0 < c < max_frames for c in cnt[7::8])
    if max_frames == 0:
        assert not any(cnt) and [w[6] for w in want] == [t["next"] for t in specs]


@pytest.mark.parametrize("S", [3, 300])
def test_nullable_outputs_left_out_in_turn(vc, wire, S):
    specs = _mixed(S, 64, seed=77 + S)
    phases = (0, 1) if S < 300 else (0,)
    for null in [("budget",), ("stream_len",), ("nframes",), ("crc_len",), ("crc",), ("hdr",),
                 ("budget",) + PER_FILE + PER_FRAME]:
        sp = [dict(t, budget=0xFFFFFFFF) for t in specs] if "budget" in null else specs
        _fill(vc, wire, sp, MTU, 64, phases=phases, null=null, lanes=(0,))


# ---- 3. positions beyond 32 bits -----------------------------------------------------------------
def test_file_offsets_beyond_32_bits(vc, wire):
    """No 4 GiB allocation: d_file_pos is the file's real place minus 2^33, wrapping, and next is
    2^33 + k. The LE64 offsets on the wire (inside the compared canvas) and d_next carry the large
    values."""
    V = 1 << 33
    specs = [T(_bytes(30, 900), next=V + 17, virt=V),
             T(_bytes(31, 900), next=V + 100, la=V, virt=V),
             T(_bytes(32, 300), next=(1 << 63) + 5, virt=1 << 63),
             T(_bytes(33, 2000), next=V + 1, virt=V, cap=5 * MTU)]
    want = _fill(vc, wire, specs, MTU, 12)
    assert [w[6] for w in want] == [V + 900, V + 900, (1 << 63) + 300, V + 1 + 92 + 400]
    stream = want[0][0]
    assert stream[1] == 1 and int.from_bytes(stream[8:16].tobytes(), "little") == V + 17


# ---- 4. two calls chain ----------------------------------------------------------------------------
def test_two_calls_on_a_side_stream_chain(vc, wire):
    """Two calls of budget B, the second placed behind the first by stream_off + stream_len computed
    on the device, equal one host fill of budget 2 B: only the first call's first frame is explicit."""
    B, mtu = 5, 1024
    specs = [T(_bytes(40, 20_000), next=100), T(_bytes(41, 7000), next=0, la=0), T(_bytes(42, 3000), next=50, la=9)]
    S = len(specs)
    want = [_expect(wire, t, mtu, 2 * B) for t in specs]
    assert [w[1].size for w in want] == [10, 7, 3]
    room = 2 * B * mtu + 7
    soff = np.array([3 + s * room + s for s in range(S)], dtype=np.uint64)
    canvas0 = _bytes(50, int(soff[-1]) + room + 8)
    canvas = canvas0.copy()
    for o, w in zip(soff, want):
        canvas[int(o):int(o) + w[5]] = w[0]
    fpos = np.cumsum([5] + [t["data"].size + 6 for t in specs[:-1]])
    files = _bytes(51, int(fpos[-1]) + specs[-1]["data"].size + 8)
    for o, t in zip(fpos, specs):
        files[o:o + t["data"].size] = t["data"]
    d_files, out = _d8(files), _d8(canvas0)
    d_fpos, d_size = _d64(fpos), _d64([t["size"] for t in specs])
    d_next, d_la = _d64([t["next"] for t in specs]), _d64([t["la"] for t in specs])
    d_soff, d_cap = _d64(soff), _d64([B * mtu] * S)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        a = wire.fill_files_dev(d_files, d_fpos, d_size, d_next, d_la, mtu, B, out=out, stream_off=d_soff,
                                stream_cap=d_cap, stream=side)
        d_soff2 = d_soff + a[5]
        b = wire.fill_files_dev(d_files, d_fpos, d_size, d_next, d_la, mtu, B, out=out, stream_off=d_soff2,
                                stream_cap=d_cap, stream=side)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), canvas)
    assert np.array_equal(d_next.cpu().numpy().view(np.uint64), [w[6] for w in want])
    na, nb = a[4].cpu().numpy(), b[4].cpu().numpy()
    assert na.tolist() == [5, 5, 3] and nb.tolist() == [5, 2, 0]
    crc_a, crc_b = a[2].cpu().numpy().view(np.uint32), b[2].cpu().numpy().view(np.uint32)
    fa, fb = a[3].cpu().numpy(), b[3].cpu().numpy()
    for s, w in enumerate(want):
        got = np.concatenate([crc_a[fa[s]:fa[s + 1]], crc_b[fb[s]:fb[s + 1]]])
        assert np.array_equal(got, w[3])
    assert not crc_b[fb[S]:].any() and fa[S] == 13 and fb[S] == 7


# ---- 5. the reference's own trailers ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["window64_mtu1024", "resume_tail_cap1k"])
def test_reference_sessions_trailers(vc, wire, name):
    """One call whose transfers are the recorded sender's window fills (its DATA frames split in
    front of every explicit one), all reading the same file: every trailer the reference put on the
    wire comes back in d_crc, and the wire lengths are its."""
    s = _sessions.load()[name]
    file = _sessions.input_file(s)
    segs = segments(s)
    S, max_frames = len(segs), max(len(g) for g in segs)
    recorded = [rec for rec in s["tx_frames"] if rec[0] == _sessions.PKT_DATA]
    assert sum(len(g) for g in segs) == len(recorded) and S > 5
    d_file = _d8(file)
    start = [g[0][0] for g in segs]
    room = max_frames * s["mtu"]
    out = torch.zeros(S * room + 8, dtype=torch.uint8, device=DEV)
    d_next = _d64(start)
    r = wire.fill_files_dev(d_file, _d64([0] * S), _d64([file.size] * S), d_next, _d64(start), s["mtu"], max_frames,
                            out=out, stream_off=_d64([i * room for i in range(S)]), stream_cap=_d64([room] * S),
                            budget=_d32([len(g) for g in segs]))
    torch.cuda.synchronize()
    frame_off, crc_len, crc, first, nframes, stream_len = (x.cpu().numpy() for x in r)
    n = len(recorded)
    assert first[-1] == n and nframes.tolist() == [len(g) for g in segs]
    assert np.array_equal(crc.view(np.uint32)[:n], np.array([rec[2] for rec in recorded], dtype=np.uint32))
    assert np.array_equal(crc_len[:n] + 4, [rec[1] for rec in recorded])
    assert stream_len.tolist() == [sum(w for _, w, _ in g) for g in segs]
    # and the bytes in front of the trailers are the recorded prefixes and the file's bytes
    host = out.cpu().numpy()
    for i in (0, 1, n // 2, n - 1):
        o = int(frame_off[i])
        assert np.array_equal(host[o:o + crc_len[i]], _sessions.frame_bytes(recorded[i], file)), i
    assert np.array_equal(d_next.cpu().numpy().view(np.uint64)[:-1], start[1:])


# ---- 6. file -> frames -> streams -> scan -> unpack -> file, nothing read back -----------------------
def test_round_trip_with_a_restart_and_nothing_read_back(vc, wire):
    """Five files of unequal sizes go from one device buffer into another through fill, scan and
    unpack, window after window on a side stream; the only things the host ever passes are
    constants. After every window the ACK is a device copy (last_acked = the receiver's written).
    In the third window one byte of the LAST frame of transfer 3 is flipped in HBM (a corrupt frame
    in front of implied ones would let those land at its place, in this protocol as in the
    reference: the restart is what a sender does after the NAK), then every sender goes back to
    next = last_acked = written, and the windows run until the files must be complete."""
    S, mtu, max_frames = 5, 1024, 8
    Mx = mtu - 12
    sizes = [30_000, 1, 8 * Mx - 8 + 5, 50_001, 17_000]
    data = [_bytes(60 + s, n) for s, n in enumerate(sizes)]
    fpos = np.cumsum([2] + [n + 3 for n in sizes[:-1]])
    files = _bytes(59, int(fpos[-1]) + sizes[-1] + 8)
    for o, d in zip(fpos, data):
        files[o:o + d.size] = d
    d_files, d_fpos, d_size = _d8(files), _d64(fpos), _d64(sizes)
    room = max_frames * mtu
    soff = [1 + s * (room + 1) for s in range(S)]  # phases 1, 2, 3, 0, 1
    out = torch.zeros(soff[-1] + room + 8, dtype=torch.uint8, device=DEV)
    d_soff, d_cap = _d64(soff), _d64([room] * S)
    d_next, d_la = _d64([0] * S), _d64([0] * S)
    lay = Files(sizes, phase=[3, 2, 1, 0, 3])
    # the host's own account of the session, from constants: where window 3 of transfer 3 starts
    per_window = max_frames * Mx - 8
    flip_at = soff[3] + (max_frames - 1) * mtu + 500
    restart_from = 2 * per_window + (max_frames - 1) * Mx - 8
    windows = 3 + max(-(-(n - (restart_from if s == 3 else 3 * per_window)) // per_window) for s, n in enumerate(sizes))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    kept = []
    with torch.cuda.stream(side):
        for w in range(windows):
            f = wire.fill_files_dev(d_files, d_fpos, d_size, d_next, d_la, mtu, max_frames, out=out,
                                    stream_off=d_soff, stream_cap=d_cap, stream=side)
            if w == 2:
                out[flip_at] ^= 0x40
            if w == 3:
                kept = [out.clone(), f[4].clone()]
            foff, clen, first, *_ = wire.scan_streams_dev(out, d_soff, f[5], mtu, max_frames, stream=side)
            r = wire.unpack_data_files_dev(out, first=first, file_ptr=lay.ptr, file_cap=lay.cap,
                                           written=lay.written,
                                           off=foff, length=clen, n=S * max_frames, len_hint=mtu - 4,
                                           file_state=lay.state, naccepted=lay.nacc, noverflow=lay.novf,
                                           file_nbad=lay.fnbad, nbad=None, stream=side)
            lay.ok.append(r[0])
            lay.accept.append(r[1])
            d_la.copy_(lay.written)  # the ACK
            if w == 2:
                d_next.copy_(lay.written)  # go-back-N
    side.synchronize()
    got = lay.result()
    for s in range(S):
        at = int(lay.pos[s])
        assert np.array_equal(got["canvas"][at:at + sizes[s]], data[s]), s
    blank = np.ones(lay.total, dtype=bool)
    for s in range(S):
        blank[int(lay.pos[s]):int(lay.pos[s]) + sizes[s]] = False
    assert (got["canvas"][blank] == 0xA5).all()
    assert got["written"].tolist() == sizes
    assert got["state"].tolist() == [_oracle.update_state(0xFFFFFFFF, d) for d in data]
    assert got["fnbad"].tolist() == [0, 0, 0, 1, 0] and got["novf"].tolist() == [0] * S
    assert np.array_equal(d_next.cpu().numpy().view(np.uint64), sizes)
    # the restart's first frame carries the explicit offset of the frame that was lost
    again = kept[0].cpu().numpy()
    head = again[soff[3]:soff[3] + 16]
    assert head[0] == 5 and head[1] & 1 and int.from_bytes(head[8:16].tobytes(), "little") == restart_from
    assert int(kept[1][3]) == max_frames
