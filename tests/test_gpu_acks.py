"""val_frame_respond_files_dev and val_frame_apply_acks_files_dev: a delivered
window answered with DATA_ACK / DATA_NAK frames, and such answers applied to
the send state, on the device (include/val_crc32_gpu.h; DESIGN.md section
4.13).

Expected values never come from the device path. The recorded reference
sessions (tests/golden/session_vectors.json) hold the receiver's ACK frames
byte for byte; everywhere else the plain-C rules of val_wire.h
(val_frame_respond_window, val_frame_put_response, val_frame_apply_acks), which
tests/test_ack_rules.py pins against those sessions, run per file over the
oracle's trailer verdicts. Response streams lie in one canvas of pseudo-random
bytes at all four phases of address mod 4 and the WHOLE canvas is compared, so
a byte written outside a kept response fails the test."""
import numpy as np
import pytest

from tests import _oracle, _prng, _sessions
from tests.test_ack_rules import ACK, NAK, SESSIONS, recorded_acks, session_windows
from tests.test_gpu_unpack import DEV, _d8, _d32, _d64, vc, wire  # noqa: F401 - vc and wire are fixtures
from tests.test_gpu_unpack_files import Files

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CTRL = 3  # a packet type that is neither DATA nor a response


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 1. the recorded sessions ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_recorded_sessions_on_the_device(vc, wire, name):
    s = _sessions.load()[name]
    file = _sessions.input_file(s)
    want = np.frombuffer(recorded_acks(s), np.uint8)
    wins = session_windows(s)
    start = int(wins[0][2][0])
    lay = Files([s["bytes"]], written=[start])
    total = _d64([s["bytes"]])
    since = _d32([0])
    rx0 = _prng.prng_bytes(31, want.size + 64)
    rx = _d8(rx0)
    w, sn, at = start, 0, 16
    for fo, plen, foff in wins:
        inc = (fo != np.uint64(wire.OFFSET_IMPLIED)).astype(np.uint8)
        stream, f_off, c_len = wire.build_data_batch(file, foff, plen, foff, inc)
        wire.put_trailers(stream, f_off, c_len, _oracle.frames(stream, f_off, c_len, nthreads=8))
        base, first, d_off, d_len = _d8(stream), _d32([0, plen.size]), _d64(f_off), _d32(c_len)
        lay.unpack(wire, base, [0, plen.size], d_off, d_len, with_state=False)
        rlen, nresp, ndrop = wire.respond_files_dev(base, first=first, ok=lay.ok[-1], accept=lay.accept[-1],
                                                    written=lay.written, total=total, out=rx, resp_off=_d64([at]),
                                                    resp_cap=_d64([want.size + 16 - at]), ack_stride=1, since=since,
                                                    off=d_off, length=d_len)
        _, kind, _, w, sn = wire.respond_window(fo, plen, w, s["bytes"], 1, sn)  # where the next window's answers go
        assert int(rlen.item()) == 12 * kind.size and int(nresp.item()) == kind.size and int(ndrop.item()) == 0
        at += 12 * kind.size
    got = rx.cpu().numpy()
    assert np.array_equal(got[16:16 + want.size], want)
    assert np.array_equal(got[:16], rx0[:16]) and np.array_equal(got[16 + want.size:], rx0[16 + want.size:])
    assert int(_u64(lay.written)[0]) == s["bytes"] and int(since.item()) == 0
    # the sender's side: scan what was written, then apply
    n_ack = SESSIONS[name]
    f_off, c_len, first, nframes, consumed, status = wire.scan_streams_dev(rx, _d64([16]), _d64([want.size]), 1024,
                                                                           n_ack + 3)
    la, nx = _d64([start]), _d64([start])
    retr, fbad = wire.apply_acks_files_dev(rx, first=first, file_size=total, last_acked=la, next=nx, off=f_off,
                                           length=c_len, n=n_ack + 3)
    assert int(nframes.item()) == n_ack and int(consumed.item()) == want.size
    assert (int(_u64(la)[0]), int(_u64(nx)[0])) == (s["bytes"], s["bytes"])
    assert int(retr.item()) == 0 and int(fbad.item()) == 0


# ---- 2. constructed windows against the host rule ---------------------------------------------
def mixed_frames(rng, n, w0, cap=U64, big=False, implied=0.0):
    """n frames for a receiver at w0 -> (file_off, pay_len, flavour): in order, duplicate, gap, corrupt
    ('x'), control ('c'); frames that would pass `cap` are refused and do not move the model. Every
    frame is explicit unless `implied` is given: the share of the in-order frames that carry no offset
    ('i': such a frame lands wherever the receiver stands, behind a gap or a corrupt frame as well)."""
    fo, pl, fl = [], [], []
    w = w0
    for _ in range(n):
        r = rng.random()
        ln = int(rng.integers(0, 1500 if big else 24))
        flavour = "d"
        if r < 0.6:
            off = w
            if implied and rng.random() < implied:
                flavour = "i"
            if w + ln <= cap:
                w += ln
        elif r < 0.7:
            off = max(0, w - int(rng.integers(1, 50)))
            if off == w and w + ln <= cap:
                w += ln
        elif r < 0.8:
            off = w + int(rng.integers(1, 50))
        elif r < 0.9:
            off, flavour = w, "x"
        else:
            off, flavour = w, "c"
        fo.append(off), pl.append(ln), fl.append(flavour)
    return fo, pl, fl


class Receiver:
    """S receivers on the device and their host mirror. window() builds one window on the device with
    val_frame_data_batch_dev (frames of flavour 'i' without an offset, every other frame explicit),
    delivers it, answers it, and compares everything with the host rules; state carries over to the
    next window. nacc and novf count what val_frame_accept accepted and refused by capacity."""

    def __init__(self, wire, w0, total, file_cap, stride, since, deliver=True):
        self.wire, self.S, self.stride, self.deliver = wire, len(w0), stride, deliver
        self.w, self.since = [int(x) for x in w0], [int(x) for x in since]
        self.total, self.file_cap = [int(x) for x in total], [int(x) for x in file_cap]
        if deliver:
            self.lay = Files(self.file_cap, written=self.w)
        self.d_written = self.lay.written if deliver else _d64(self.w)
        self.d_total = _d64(self.total)
        self.d_since = _d32(self.since) if stride else None
        self.ndropped = torch.zeros(self.S, dtype=torch.int32, device=DEV)
        self.dropped = np.zeros(self.S, np.uint32)
        self.nacc, self.novf = np.zeros(self.S, np.uint32), np.zeros(self.S, np.uint32)

    def build(self, per_file, seed, strided=0):
        """-> host copy of the stream, frame_off, crc_len (descriptor or strided slots)."""
        fo = np.array([o for f in per_file for o in f[0]], np.uint64)
        pl = np.array([p for f in per_file for p in f[1]], np.uint32)
        fl = [x for f in per_file for x in f[2]]
        n = pl.size
        payload = _prng.prng_bytes(seed, max(int(pl.sum()), 1))
        pay_off = (np.cumsum(pl, dtype=np.uint64) - pl).astype(np.uint64)
        inc = np.array([x != "i" for x in fl], np.uint8) if "i" in fl else None
        if strided:
            f_off, size = np.arange(n, dtype=np.uint64) * np.uint64(strided), n * strided
        else:
            f_off, _, size = self.wire.data_layout(pl, inc)
        out = _d8(_prng.prng_bytes(seed + 1, size + 8))
        c_len, _, nrej = self.wire.build_data_batch_dev(_d8(payload), _d64(pay_off), _d32(pl), _d64(fo),
                                                        None if inc is None else _d8(inc), out=out,
                                                        frame_off=None if strided else _d64(f_off), out_stride=strided)
        assert int(nrej.item()) == 0
        stream, c_len = out.cpu().numpy(), _u32(c_len)
        for i, x in enumerate(fl):
            at = int(f_off[i])
            if x == "x":
                stream[at + 9] ^= 0x04
            elif x == "c":  # a good frame of another type
                stream[at] = CTRL
                end = at + int(c_len[i])
                stream[end:end + 4] = np.frombuffer(_oracle.crc32(stream[at:end]).to_bytes(4, "little"), np.uint8)
        return stream, f_off, c_len

    def window(self, per_file, seed, resp_caps, n_pad=0, strided=0, *, loose=None, first_dev=None, n_dev=None,
               dead=None, null_ndropped=False):
        """per_file: S tuples (file_off, pay_len, flavour); resp_caps: per file 'fit', 'short', 11, 0 or 'big';
        n_pad: unowned padding entries (0, 0) behind the frames (descriptor mode).
        loose: one more such tuple, frames behind the files' that no file owns. first_dev, n_dev: the
        d_first and n the device gets instead of the files' own bounds; clamped as the contract says
        they must give the segments of per_file. dead: {file: d_resp_off[s] of 2^60 or more}, nothing
        is written for these files and all their responses are dropped. null_ndropped: the call gets
        d_ndropped == NULL and the counts stay where they were."""
        wire = self.wire
        stream, f_off, c_len = self.build(list(per_file) + ([loose] if loose else []), seed, strided)
        cnt = np.array([len(f[0]) for f in per_file])
        first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        n = int(first[-1])
        n_call = (int(f_off.size) + n_pad) if n_dev is None else int(n_dev)  # the device's n
        if first_dev is None:
            first_dev = first
        owned = [(min(int(a), n_call), min(max(int(a), int(b)), n_call)) for a, b in zip(first_dev[:-1], first_dev[1:])]
        model = [(int(a), int(b)) for a, b in zip(first[:-1], first[1:])]
        assert [x for x in owned if x[0] < x[1]] == [x for x in model if x[0] < x[1]] and n <= n_call
        assert [x[0] < x[1] for x in owned] == [x[0] < x[1] for x in model]
        ok, _ = _oracle.verify_frames(stream, f_off[:n], c_len[:n], nthreads=8) if n else (np.zeros(0, np.uint8), 0)
        fo = wire.data_offsets(stream, f_off[:n], c_len[:n])
        pl = wire.payload_lens(stream, f_off[:n], c_len[:n])
        want, accept = [], np.zeros(n_call, np.uint8)
        for s in range(self.S):
            lo, hi = int(first[s]), int(first[s + 1])
            dst, w_acc, nacc, novf = wire.frame_accept(fo[lo:hi], pl[lo:hi], self.w[s], self.file_cap[s], ok[lo:hi])
            _, kind, off, w_new, since = wire.respond_window(fo[lo:hi], pl[lo:hi], self.w[s], self.total[s], self.stride,
                                                             self.since[s], self.file_cap[s], ok[lo:hi])
            assert w_new == w_acc
            accept[lo:hi] = dst != U64
            self.nacc[s] += nacc
            self.novf[s] += novf
            self.w[s] = w_new
            if self.stride and hi > lo:
                self.since[s] = since
            want.append([wire.put_response(int(k), int(o)) for k, o in zip(kind, off)])
        # capacities and places: every stream at its own phase, guard bytes between neighbours
        full = [sum(len(r) for r in rs) for rs in want]
        caps = []
        for s, c in enumerate(resp_caps):
            caps.append({"fit": full[s], "short": max(full[s] - 1, 0), "big": full[s] + 1000}.get(c, c))
        pos, r_off = 9, []
        for s in range(self.S):
            pos += (s - pos) % 4
            r_off.append(pos)
            pos += full[s] + 3
        canvas0 = _prng.prng_bytes(seed + 2, pos + 8)
        canvas = canvas0.copy()
        w_len, w_n = np.zeros(self.S, np.uint64), np.zeros(self.S, np.uint32)
        dead = dead or {}
        dropped0 = self.dropped.copy()
        for s, rs in enumerate(want):
            at = 0
            for k, r in enumerate(rs):
                if at + len(r) > caps[s] or s in dead:
                    self.dropped[s] += len(rs) - k
                    break
                canvas[r_off[s] + at:r_off[s] + at + len(r)] = np.frombuffer(r, np.uint8)
                at += len(r)
                w_n[s] += 1
            w_len[s] = at
        # the device
        base = _d8(stream)
        if strided:
            desc = dict(stride=strided, flen=int(c_len[0]), n=n_call)
        else:
            desc = dict(off=_d64(np.concatenate([f_off, np.zeros(n_pad, np.uint64)])),
                        length=_d32(np.concatenate([c_len, np.zeros(n_pad, np.uint32)])), n=n_call)
        d_first = _d32(first_dev)
        if self.deliver:
            self.lay.unpack(wire, base, first_dev, desc.get("off"), desc.get("length"), with_state=False,
                            **{k: v for k, v in desc.items() if k in ("stride", "flen", "n")})
            d_ok, d_acc = self.lay.ok[-1], self.lay.accept[-1]
        else:  # respond alone: the verdicts and the accepted set of the host rule, the position after them
            d_ok, d_acc = _d8(np.concatenate([ok, np.ones(n_call - n, np.uint8)])), _d8(accept)
            self.d_written.copy_(_d64(self.w))
        out = _d8(canvas0)
        # a dead stream's capacity is large: the offset alone must keep every byte of it unwritten
        d_roff = _d64([dead.get(s, o) for s, o in enumerate(r_off)])
        d_caps = _d64([(1 << 40) if s in dead else c for s, c in enumerate(caps)])
        if null_ndropped:  # the raw call: the wrapper would allocate the counts
            rlen = torch.full((self.S,), -1, dtype=torch.int64, device=DEV)
            nresp = torch.full((self.S,), -1, dtype=torch.int32, device=DEV)
            work = torch.empty(max(wire.respond_work_bytes(n_call), 16), dtype=torch.uint8, device=DEV)
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            st = wire.lib().val_frame_respond_files_dev(
                ptr(base), ptr(desc.get("off")), ptr(desc.get("length")), strided, desc.get("flen", 0), n_call, self.S,
                ptr(d_first), ptr(d_ok), ptr(d_acc), ptr(self.d_written), ptr(self.d_total), self.stride,
                ptr(self.d_since), ptr(out), ptr(d_roff), ptr(d_caps), ptr(rlen), ptr(nresp), None, ptr(work),
                work.numel(), torch.cuda.current_stream().cuda_stream)
            assert st == 0
            self.dropped = dropped0
        else:
            rlen, nresp, _ = wire.respond_files_dev(base, first=d_first, ok=d_ok, accept=d_acc, written=self.d_written,
                                                    total=self.d_total, out=out, resp_off=d_roff, resp_cap=d_caps,
                                                    ack_stride=self.stride, since=self.d_since, ndropped=self.ndropped,
                                                    **desc)
        torch.cuda.synchronize()
        assert np.array_equal(d_ok.cpu().numpy()[:n], ok) and np.array_equal(d_acc.cpu().numpy(), accept)
        assert _u64(self.d_written).tolist() == self.w
        got = out.cpu().numpy()
        bad = np.flatnonzero(got != canvas)
        assert bad.size == 0, (bad.size, bad[:8], r_off)
        assert np.array_equal(_u64(rlen), w_len) and np.array_equal(_u32(nresp), w_n)
        assert np.array_equal(_u32(self.ndropped), self.dropped)
        if self.stride:
            assert _u32(self.d_since).tolist() == self.since
        # what a sender's scan and apply go on from: the device's streams, and the host rule's kept responses
        self.last = dict(out=out, resp_off=d_roff, resp_len=rlen, kept=[rs[:int(k)] for rs, k in zip(want, w_n)])
        return want, full


def _in_order(n, w0, ln=7):
    return [w0 + ln * i for i in range(n)], [ln] * n, ["d"] * n


@pytest.mark.parametrize("extra", (0, 60), ids=("workgroups of 1024", "workgroups of 256"))
@pytest.mark.parametrize("stride", (0, 1, 3))
def test_file_sizes_around_the_chunk(vc, wire, stride, extra):
    """Files of 0, 1, 1023, 1024, 1025 and 2049 frames in one call, mixed frames, two chained windows. With
    60 more files of 2 frames the call's files are small on average and the rule runs in workgroups of 256
    threads, whose chunks the same files cross at other places."""
    rng = np.random.default_rng(100 + stride)
    counts = (0, 1, 1023, 1024, 1025, 2049) + (2,) * extra
    lanes = vc.plan_ack_calls(vc.ACK_RESPOND, _cus(), sum(counts), len(counts))[1].lanes
    assert lanes == (256 if extra else 1024)
    w0 = [5, 0, 100, 7, 0, 3] + [9] * extra
    # 1025 frames: refused by capacity from the first window's middle on
    cap = [10, 40, 20000, 20000, 3000, 60000] + [200] * extra
    total = [10, 1 << 40, 6000, 1 << 40, 1 << 40, 20000] + [30] * extra  # two files complete inside a window
    rx = Receiver(wire, w0, total, cap, stride, [0, 2, 5, 1, 0, 70] + [1] * extra)
    seen = set()
    for rnd in range(2):
        per_file = [mixed_frames(rng, c, rx.w[s], cap[s]) for s, c in enumerate(counts)]
        want, _ = rx.window(per_file, 40 + rnd, ["big"] * len(counts))
        seen |= {len(r) for rs in want for r in rs}
    assert seen == {12, 24}
    assert int(rx.lay.novf.sum().item()) > 100  # capacity refusals happened, silently
    assert rx.w[2] >= total[2] and rx.w[5] >= total[5]


def test_more_files_than_workgroups(vc, wire):
    """3 x the planned grid + 1 files of 0-3 frames each: every workgroup takes several files."""
    grid = vc.plan_ack_calls(vc.ACK_RESPOND, _cus(), 10 ** 6, 10 ** 6)[1].grid
    S = 3 * grid + 1
    rng = np.random.default_rng(9)
    w0 = rng.integers(0, 1000, S)
    rx = Receiver(wire, w0, w0 + rng.integers(0, 60, S), w0 + 50, 2, rng.integers(0, 4, S))
    per_file = [mixed_frames(rng, int(rng.integers(0, 4)), rx.w[s], rx.file_cap[s]) for s in range(S)]
    assert {len(f[0]) for f in per_file} == {0, 1, 2, 3}
    rx.window(per_file, 50, ["big"] * S, n_pad=17)


def test_response_capacity_and_unowned_padding(vc, wire):
    """d_resp_cap at the exact fit, one byte short, 11 and 0; padding entries behind the frames."""
    rng = np.random.default_rng(11)
    S = 8
    rx = Receiver(wire, [0] * S, [1 << 40] * S, [1 << 20] * S, 1, [0] * S)
    per_file = [mixed_frames(rng, 40, 0) for _ in range(S)]
    want, full = rx.window(per_file, 60, ["fit", "short", 11, 0, 12, 35, "big", 24], n_pad=S * 64 - 40 * S)
    assert all(f > 36 for f in full)
    assert rx.dropped[0] == 0 and rx.dropped[1] == 1 and rx.dropped[3] == sum(len(r) > 0 for r in want[3])
    assert any(len(r) == 24 for rs in want for r in rs)


@pytest.mark.parametrize("stride", (0, 1))
def test_ack_size_changes_inside_the_window(vc, wire, stride):
    """A receiver at 2^32 - 3000: ACKs of 12 and of 16 bytes, NAKs with a high half. Respond alone, with
    the accepted set of the host rule: nothing has to be delivered 4 GiB into a file."""
    rng = np.random.default_rng(12)
    w0 = [(1 << 32) - 3000, (1 << 32) - 1, 1 << 32, (5 << 32) + 9]
    rx = Receiver(wire, w0, [1 << 40, (1 << 32) + 2000, 1 << 40, 1 << 40], [U64] * 4, stride, [0] * 4, deliver=False)
    per_file = [mixed_frames(rng, 30, w, big=True) for w in w0]
    want, _ = rx.window(per_file, 70, ["big", "fit", "short", "big"])
    sizes = {len(r) for r in want[0]}
    assert sizes >= {16, 24} and (stride == 0 or 12 in sizes)  # one ACK per window: the only one is past 2^32
    want, _ = rx.window([mixed_frames(rng, 5, w) for w in rx.w], 71, ["big"] * 4)
    assert {len(r) for rs in want for r in rs} <= {16, 24}


def test_strided_mode(vc, wire):
    """Slots of equal frames: duplicates, a gap and a corrupt frame among in-order frames, three files."""
    ln, slot = 20, 48
    a = _in_order(30, 0, ln)
    b = ([0, 0, ln, 5 * ln, 2 * ln, ln] + [3 * ln + ln * i for i in range(20)], [ln] * 26, ["d"] * 5 + ["x"] + ["d"] * 20)
    c = _in_order(10, 40, ln)
    rx = Receiver(wire, [0, 0, 40], [1 << 30, 1 << 30, 40 + 10 * ln], [1 << 16] * 3, 3, [1, 0, 0])
    want, _ = rx.window([a, b, c], 80, ["big", "big", "fit"], strided=slot)
    assert any(len(r) == 24 for r in want[1]) and len(want[2]) >= 4


# ---- 3. apply against the host rule -----------------------------------------------------------
def response_stream(rng, n, size, la):
    """n response frames for a transfer of `size` bytes acknowledged up to la -> wire bytes."""
    out, hi = [], la
    for _ in range(n):
        r = rng.random()
        if r < 0.55:
            hi = min(size, hi + int(rng.integers(0, 3000)))
            f = wire_put(ACK, hi)
        elif r < 0.65:
            f = wire_put(NAK, min(size, hi + int(rng.integers(0, 100))))  # NAK, then higher ACKs may follow
        elif r < 0.72:
            f = wire_put(ACK, size + 1 + int(rng.integers(0, 5)))  # beyond the file
        elif r < 0.8:
            f = wire_put(ACK, max(0, hi - int(rng.integers(0, 5000))))  # stale
        elif r < 0.9:
            head = bytes([12, 2, 0, 0]) + int(rng.integers(0, 1 << 31)).to_bytes(4, "little")  # DONE_ACK
            f = head + _oracle.crc32(head).to_bytes(4, "little")
        else:
            f = bytearray(wire_put(ACK if rng.random() < 0.5 else NAK, hi + 77))
            at = int(rng.integers(2, len(f)))  # a flipped bit, anywhere but in content_len: the scan stays in step
            f[at if at >= 4 else at - 2] ^= 1 << int(rng.integers(0, 8))
            f = bytes(f)
        out.append(f)
    return b"".join(out)


def wire_put(kind, off):
    import val_protocol_amd.wire as w

    return w.put_response(kind, off)


def _apply_case(wire, counts, sizes, seed, n_pad=0, start=None):
    rng = np.random.default_rng(seed)
    S = len(counts)
    la0 = [int(rng.integers(0, sz + 1)) for sz in sizes]
    for s, la in (start or {}).items():
        la0[s] = la
    nx0 = [la + int(rng.integers(0, sz - la + 1)) for la, sz in zip(la0, sizes)]
    streams = [response_stream(rng, c, sz, la) for c, sz, la in zip(counts, sizes, la0)]
    base = np.frombuffer(b"\x5a\x5a\x5a" + b"".join(streams) + b"\x5a" * 8, np.uint8).copy()
    off, length, first, at = [], [], [0], 3
    w_la, w_nx, w_retr, w_bad, w_ok = [], [], [], [], []
    for s, st in enumerate(streams):
        arr = np.frombuffer(st, np.uint8)
        code, f_off, c_len, used = wire.scan_frames(arr, 64) if arr.size else (0, np.zeros(0, np.uint64),
                                                                               np.zeros(0, np.uint32), 0)
        assert code == 0 and used == arr.size and f_off.size == counts[s]
        ok = _oracle.verify_frames(arr, f_off, c_len)[0] if arr.size else np.zeros(0, np.uint8)
        kind, aoff = wire.ack_offsets(arr, f_off, c_len)
        la, nx, retr, ncrc = wire.apply_acks(kind, aoff, sizes[s], la0[s], nx0[s], ok)
        w_la.append(la), w_nx.append(nx), w_retr.append(retr), w_bad.append(ncrc), w_ok.append(ok)
        off.append(f_off + np.uint64(at)), length.append(c_len), first.append(first[-1] + f_off.size)
        at += arr.size
    n = first[-1] + n_pad
    off = np.concatenate(off + [np.zeros(n_pad, np.uint64)])
    length = np.concatenate(length + [np.zeros(n_pad, np.uint32)])
    d_la, d_nx = _d64(la0), _d64(nx0)
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    retr = torch.full((S,), 3, dtype=torch.int32, device=DEV)  # incremented, not set
    fbad = torch.full((S,), 5, dtype=torch.int32, device=DEV)
    wire.apply_acks_files_dev(_d8(base), first=_d32(first), file_size=_d64(sizes), last_acked=d_la, next=d_nx,
                              off=_d64(off), length=_d32(length), n=n, len_hint=12, nretrans=retr, file_nbad=fbad,
                              out_ok=d_ok)
    torch.cuda.synchronize()
    assert _u64(d_la).tolist() == w_la and _u64(d_nx).tolist() == w_nx
    assert (_u32(retr) - 3).tolist() == w_retr and (_u32(fbad) - 5).tolist() == w_bad
    assert np.array_equal(d_ok.cpu().numpy()[:first[-1]], np.concatenate(w_ok))
    return la0, nx0, w_la, w_nx, w_retr, w_bad


def test_apply_transfer_sizes_around_the_chunk(vc, wire):
    counts = (0, 1, 1023, 1024, 1025, 2049, 0, 30)
    sizes = [1000, 5, 10 ** 6, (1 << 32) + 10 ** 6, 10 ** 6, 1 << 40, 0, 4000]
    la0, nx0, la, nx, retr, bad = _apply_case(wire, counts, sizes, 21, n_pad=40, start={3: (1 << 32) - 5000})
    assert (la[0], nx[0], la[6], nx[6]) == (la0[0], nx0[0], la0[6], nx0[6])  # no frames: untouched
    assert sum(bad) > 100 and sum(retr) > sum(bad) and all(a <= s for a, s in zip(la, sizes))
    assert la[3] > 1 << 32


def test_apply_more_transfers_than_workgroups(vc, wire):
    grid = vc.plan_ack_calls(vc.ACK_APPLY, _cus(), 10 ** 6, 10 ** 6)[0].grid
    S = 3 * grid + 1
    rng = np.random.default_rng(22)
    counts = rng.integers(0, 4, S).tolist()
    _apply_case(wire, counts, rng.integers(0, 50000, S).tolist(), 23)


def test_apply_literal_orders(vc, wire):
    """NAK then a higher ACK; an ACK beyond the file; a DONE_ACK in between; strided 12-byte frames."""
    done = bytes([12, 2, 0, 0, 9, 0, 0, 0])
    done += _oracle.crc32(done).to_bytes(4, "little")
    a = wire.put_response(ACK, 100) + wire.put_response(NAK, 200) + done + wire.put_response(ACK, 300)
    b = wire.put_response(ACK, 100) + done + wire.put_response(ACK, 1001)
    base = np.frombuffer(a + b, np.uint8).copy()
    oa, la_, _ = wire.scan_frames(np.frombuffer(a, np.uint8), 64)[1:]
    ob, lb_, _ = wire.scan_frames(np.frombuffer(b, np.uint8), 64)[1:]
    d_la, d_nx = _d64([0, 0]), _d64([800, 800])
    retr, fbad = wire.apply_acks_files_dev(_d8(base), first=_d32([0, 4, 7]), file_size=_d64([1000, 1000]),
                                           last_acked=d_la, next=d_nx, off=_d64(np.concatenate([oa, ob + np.uint64(len(a))])),
                                           length=_d32(np.concatenate([la_, lb_])))
    assert _u64(d_la).tolist() == [300, 100] and _u64(d_nx).tolist() == [300, 800]
    assert _u32(retr).tolist() == [1, 0] and _u32(fbad).tolist() == [0, 0]
    acks = b"".join(wire.put_response(ACK, 50 * (i + 1)) for i in range(20))
    d_la, d_nx = _d64([7, 0]), _d64([9, 0])
    wire.apply_acks_files_dev(_d8(np.frombuffer(acks, np.uint8).copy()), first=_d32([0, 15, 15]), file_size=_d64([600, 600]),
                              last_acked=d_la, next=d_nx, stride=12, flen=8, n=20)
    assert _u64(d_la).tolist() == [600, 0] and _u64(d_nx).tolist() == [600, 0]  # ACKs 650 .. 750 pass the file


# ---- 4. the closed loop -----------------------------------------------------------------------
MTU, WIN = 1024, 8
LOOP_SIZES = (0, 1, 1003, 1004, 5000, 70001, 300000)
WITHHELD = (2, 5)  # in round 2, transfer 5's window does not arrive


def loop_model(wire, stride):
    """The same loop on the host, rule by rule -> the states after every round."""
    S = len(LOOP_SIZES)
    la, nx, w, since = [0] * S, [0] * S, [0] * S, [0] * S
    rounds = []
    while any(a < sz for a, sz in zip(la, LOOP_SIZES)):
        rnd = len(rounds)
        for s, size in enumerate(LOOP_SIZES):
            fo, pl, inc, _, _, _, nxt = wire.fill_window(nx[s], la[s], size, MTU, WIN)
            nx[s] = nxt
            if (rnd, s) == WITHHELD:
                nx[s] = la[s]
                continue
            fo = np.where(inc != 0, fo, np.uint64(wire.OFFSET_IMPLIED)).astype(np.uint64)
            _, kind, off, w[s], sn = wire.respond_window(fo, pl, w[s], size, stride, since[s], size)
            if stride and fo.size:
                since[s] = sn
            la[s], nx[s], retr, ncrc = wire.apply_acks(kind, off, size, la[s], nx[s])
            assert retr == 0 and ncrc == 0
        rounds.append((list(la), list(nx), list(w)))
        assert len(rounds) < 100
    return rounds


@pytest.mark.parametrize("stride", (1, 0))
def test_closed_loop_with_nothing_read_back(vc, wire, stride):
    rounds = loop_model(wire, stride)
    assert len(rounds) > 300000 // (WIN * (MTU - 12))
    S = len(LOOP_SIZES)
    sizes = np.array(LOOP_SIZES, np.uint64)
    fpos = np.concatenate([[0], np.cumsum(sizes + np.uint64(3))])[:S].astype(np.uint64)
    src = _prng.prng_bytes(77, int(fpos[-1] + sizes[-1]) + 8)
    d_src, d_fpos, d_size = _d8(src), _d64(fpos), _d64(sizes)
    d_la, d_nx = _d64([0] * S), _d64([0] * S)
    lay = Files(list(LOOP_SIZES))
    tx = torch.zeros(S * (WIN * MTU + 8) + 8, dtype=torch.uint8, device=DEV)
    tx_off, tx_cap = _d64(np.arange(S, dtype=np.uint64) * np.uint64(WIN * MTU + 8) + np.uint64(4)), _d64([WIN * MTU] * S)
    r_cap = int(vc.lib().val_frame_respond_bytes_max(WIN))
    rx = torch.zeros(S * r_cap + 8, dtype=torch.uint8, device=DEV)
    rx_off, rx_cap = _d64(np.arange(S, dtype=np.uint64) * np.uint64(r_cap) + np.uint64(4)), _d64([r_cap] * S)
    since = _d32([0] * S) if stride else None
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    states = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for rnd in range(len(rounds)):
            _, _, _, _, _, tx_len = wire.fill_files_dev(d_src, d_fpos, d_size, d_nx, d_la, MTU, WIN, out=tx,
                                                        stream_off=tx_off, stream_cap=tx_cap)
            if rnd == WITHHELD[0]:
                tx_len[WITHHELD[1]:WITHHELD[1] + 1].copy_(zero)  # the window is lost on the way
            f_off, c_len, first, _, _, _ = wire.scan_streams_dev(tx, tx_off, tx_len, MTU, WIN)
            ok, acc, *_ = wire.unpack_data_files_dev(tx, first=first, file_ptr=lay.ptr, file_cap=lay.cap,
                                                     written=lay.written, off=f_off, length=c_len, n=S * WIN)
            r_len, _, ndrop = wire.respond_files_dev(tx, first=first, ok=ok, accept=acc, written=lay.written,
                                                     total=d_size, out=rx, resp_off=rx_off, resp_cap=rx_cap,
                                                     ack_stride=stride, since=since, off=f_off, length=c_len,
                                                     n=S * WIN)
            a_off, a_len, a_first, _, _, _ = wire.scan_streams_dev(rx, rx_off, r_len, MTU, 2 * WIN)
            wire.apply_acks_files_dev(rx, first=a_first, file_size=d_size, last_acked=d_la, next=d_nx, off=a_off,
                                      length=a_len, n=S * 2 * WIN)
            if rnd == WITHHELD[0]:  # the host's timeout: go back to the last acknowledged byte
                d_nx[WITHHELD[1]:WITHHELD[1] + 1].copy_(d_la[WITHHELD[1]:WITHHELD[1] + 1])
            states.append((d_la.clone(), d_nx.clone(), lay.written.clone()))
    side.synchronize()
    for rnd, (got, want) in enumerate(zip(states, rounds)):
        assert [_u64(t).tolist() for t in got] == [list(x) for x in want], rnd
    assert _u64(d_la).tolist() == _u64(d_nx).tolist() == list(LOOP_SIZES)
    canvas = lay.canvas.cpu().numpy()
    for s, size in enumerate(LOOP_SIZES):
        at = int(lay.pos[s])
        assert np.array_equal(canvas[at:at + size], src[int(fpos[s]):int(fpos[s]) + size]), s
