"""The VAL_RESUME_TAIL handshake of many GPU-resident files on the device:
val_resume_tail_files_dev, val_resume_request_files_dev and
val_resume_check_files_dev (include/val_crc32_gpu.h).

Expected values never come from the device path: the three resumed reference
sessions of tests/golden/session_vectors.json (what crossed the wire), and for
made-up states the rules in plain C (wire.resume_tail_window,
wire.resume_request_window, wire.resume_verdict) with the oracle's CRC-32 of
the host copy of each window. The chunk is forced to 4 KiB so that windows of a
few kilobytes have several chunks."""
import numpy as np
import pytest

from tests import _oracle, _prng, _sessions
from tests.test_gpu_unpack import DEV, Window, _d8, _d32, _d64, vc, wire  # noqa: F401 - vc and wire are fixtures
from tests.test_gpu_unpack_files import Files, _expect_files, _small_frames

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
START_ZERO, START_OFFSET, VERIFY_FIRST, SKIP_FILE, ABORT_FILE = 0, 1, 2, 3, 4
VAL_OK, VAL_SKIPPED, VAL_ERR_INVALID_ARG, VAL_ERR_RESUME_VERIFY = 0, 1, -1, -7
C64, C32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
RESUMED = ("resume_tail_cap8m", "resume_tail_cap1k", "resume_tail_mismatch")


@pytest.fixture(autouse=True)
def _small_chunks(vc):
    vc.set_file_window_chunk(12)
    yield
    vc.set_file_window_chunk(0)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _i32(t):
    return t.cpu().numpy()


def _di32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


class Disk:
    """Byte strings in one device buffer at odd addresses, guard bytes between them."""

    def __init__(self, datas, seed=4242):
        pos, at = 1, []
        for d in datas:
            pos |= 1
            at.append(pos)
            pos += d.size + 3
        host = _prng.prng_bytes(seed, pos + 8)
        for o, d in zip(at, datas):
            host[o:o + d.size] = d
        self.buf = torch.from_numpy(host).to(DEV)
        self.at = np.array(at, dtype=np.uint64)
        self.ptr = _d64(self.at + np.uint64(self.buf.data_ptr()))
        self.size = _d64(np.array([d.size for d in datas], dtype=np.uint64))


def _crc(data, off, length):
    return _oracle.crc32(data[off:off + length])


def _host_tail(wire, local, incoming, cap, min_verify, skip):
    action, roff, vlen = wire.resume_tail_window(local.size, incoming, cap, min_verify, skip)
    return action, roff, vlen, (_crc(local, roff - vlen, vlen) if action == VERIFY_FIRST else 0)


def _host_request(wire, file, action, roff, vlen, max_len):
    """-> (req_off, req_len, req_crc, status)"""
    send, start, v32 = wire.resume_request_window(roff, vlen)
    if action != VERIFY_FIRST or not send:
        return roff, 0, 0, VAL_OK
    if v32 > max_len or start > file.size or v32 > file.size - start:
        return start, v32, 0, VAL_ERR_INVALID_ARG
    return start, v32, _crc(file, start, v32), VAL_OK


def _host_check(wire, local, incoming, req_off, req_len, req_crc, rec_off, max_len, skip):
    """-> (local_crc, result, written)"""
    ok = req_len <= max_len and req_off <= local.size and req_len <= local.size - req_off
    crc = _crc(local, req_off, req_len) if ok else 0
    result, written = wire.resume_verdict(ok, crc, req_crc, skip, rec_off, incoming)
    return crc, result, written


# ---- 1. the reference's resumed sessions ----------------------------------------------------
@pytest.fixture(scope="module")
def golden_batch(vc):
    """The three sessions' files plus decoys, laid out once: index 0..2 the sessions, 3 an empty local
    file, 4 a local file larger than the incoming one, 5 a short local file."""
    sessions = _sessions.load()
    ss = [sessions[n] for n in RESUMED]
    ctl = [_sessions.control(s, vc.lib()) for s in ss]
    files = [_sessions.input_file(s) for s in ss]
    local = [_sessions.receiver_existing(s) for s in ss]
    d_in = [_prng.prng_bytes(71, 0), _prng.prng_bytes(72, 5000), _prng.prng_bytes(73, 9000)]
    d_local = [_prng.prng_bytes(71, 0), _prng.prng_bytes(74, 5001), d_in[2][:777].copy()]
    return dict(ss=ss, ctl=ctl, files=files + d_in, local=local + d_local, sender=Disk(files + d_in, 11),
                receiver=Disk(local + d_local, 12))


def test_golden_sessions_replayed_on_the_device(vc, wire, golden_batch):
    g = golden_batch
    ss, ctl, files, local, snd, rcv = g["ss"], g["ctl"], g["files"], g["local"], g["sender"], g["receiver"]
    n = len(files)
    incoming = _d64(np.array([f.size for f in files], dtype=np.uint64))
    # the receiver's proposal: the call takes one policy, so the batch runs once per session's
    # tail_cap_bytes; that session's entry must be what the reference sent, every entry the host rule's
    action = torch.zeros(n, dtype=torch.int32, device=DEV)
    resume_off = torch.zeros(n, dtype=torch.int64, device=DEV)
    verify_len = torch.zeros(n, dtype=torch.int64, device=DEV)
    for i, (s, c) in enumerate(zip(ss, ctl)):
        cap = s["tail_cap_bytes"]
        a, ro, vl, vcrc = wire.resume_tail_files_dev(rcv.ptr, rcv.size, incoming, tail_cap_bytes=cap)
        torch.cuda.synchronize()
        got = list(zip(_i32(a).tolist(), _u64(ro).tolist(), _u64(vl).tolist(), _u32(vcrc).tolist()))
        assert got[i] == (c["action"], c["resume_offset"], c["resp_verify_length"], c["resp_verify_crc"]), s["name"]
        assert got == [_host_tail(wire, local[k], files[k].size, cap, 0, False) for k in range(n)], s["name"]
        assert [x[0] for x in got[3:]] == [START_ZERO, START_ZERO, VERIFY_FIRST]
        action[i], resume_off[i], verify_len[i] = a[i], ro[i], vl[i]  # stays on the device
        if i == 0:
            action[3:], resume_off[3:], verify_len[3:] = a[3:], ro[3:], vl[3:]
    # the sender's answer, over its own files
    max_len = 8 << 20
    req_off, req_len, req_crc, status = wire.resume_request_files_dev(snd.ptr, snd.size, action, resume_off,
                                                                      verify_len, max_len)
    # the receiver's check, on the same stream with no read-back
    result = torch.full((n,), C32, dtype=torch.int32, device=DEV)
    written = _d64(np.full(n, C64, dtype=np.uint64))
    local_crc = torch.full((n,), C32, dtype=torch.int32, device=DEV)
    wire.resume_check_files_dev(rcv.ptr, rcv.size, incoming, req_off, req_len, req_crc, resume_off, max_len,
                                result=result, written=written, action=action, local_crc=local_crc)
    torch.cuda.synchronize()
    assert not _i32(status).any()
    for i, (s, c) in enumerate(zip(ss, ctl)):
        assert (int(_u64(req_off)[i]), int(_u32(req_len)[i]), int(_u32(req_crc)[i])) == \
            (c["req_offset"], c["req_length"], c["req_crc"]), s["name"]
        assert (int(_u32(local_crc)[i]), int(_i32(result)[i])) == (c["receiver_crc"], c["result"]), s["name"]
        assert int(_u64(written)[i]) == (0 if s["flip"] >= 0 else s["existing"]), s["name"]
    assert [c["result"] for c in ctl] == [VAL_OK, VAL_OK, VAL_ERR_RESUME_VERIFY]
    # decoys: 3 and 4 start at zero and are not checked (their sentinels survive); 5 verifies its 777 bytes
    assert _u64(req_off)[3:].tolist() == [0, 0, 0] and _u32(req_len)[3:].tolist() == [0, 0, 777]
    assert _u32(req_crc)[3:].tolist() == [0, 0, _crc(files[5], 0, 777)]
    assert _i32(result)[3:].tolist() == [C32, C32, VAL_OK] and _u64(written)[3:].tolist() == [C64, C64, 777]
    assert _u32(local_crc)[3:].tolist() == [C32, C32, _crc(local[5], 0, 777)]
    # the sender goes on from d_written: its first frame is the first DATA frame the reference sent
    for i, s in enumerate(ss):
        first = next(r for r in s["tx_frames"] if r[0] == _sessions.PKT_DATA)
        nxt = written[i:i + 1].clone()
        out = torch.zeros(s["mtu"] + 16, dtype=torch.uint8, device=DEV)
        zero = torch.zeros(1, dtype=torch.int64, device=DEV)
        frame_off, crc_len, crc, _, nframes, _ = wire.fill_files_dev(
            snd.buf, _d64(snd.at[i:i + 1]), snd.size[i:i + 1], nxt, written[i:i + 1], s["mtu"], 1, out=out,
            stream_off=zero, stream_cap=_d64(np.array([s["mtu"]], dtype=np.uint64)))
        torch.cuda.synchronize()
        assert int(nframes[0]) == 1 and int(frame_off[0]) == 0
        prefix = bytes.fromhex(first[4])
        got = out.cpu().numpy()
        assert bytes(got[:len(prefix)]) == prefix, s["name"]  # header, explicit flag and LE64 offset
        assert prefix[1] & 1 and int.from_bytes(prefix[8:16], "little") == first[3] == int(_u64(written)[i])
        assert int(_u32(crc)[0]) == first[2] and int(crc_len[0]) + 4 == first[1]  # the same trailer on the wire


# ---- 2. chained behind the unpack call ------------------------------------------------------
def test_tail_call_chained_behind_unpack(vc, wire):
    """Files delivered by val_frame_unpack_files_dev; its d_written is the tail call's d_existing on the
    same stream, with no read-back in between."""
    a, end_a = _small_frames(wire, 300, 0, seed=3, fixed=40)            # 12,000 bytes: three chunks
    b, end_b = _small_frames(wire, 5, 0, corrupt_at=[2], seed=9, fixed=40)
    d, end_d = _small_frames(wire, 2500, 2, gap_at=[1023, 1024], seed=5)
    win = Window(a + b + d)
    first = [0, 300, 305, 305, 2805]  # file 2 gets no frame and stays empty
    sizes = [end_a + 9, end_b + 50, 64, end_d + 40]
    lay = Files(sizes, written=[0, 0, 0, 2])
    incoming = np.array([end_a + 100, end_b, 64, 20], dtype=np.uint64)  # file 3: local larger than incoming
    lay.unpack(wire, _d8(win.stream), first, _d64(win.off), _d32(win.len))
    out = {}
    for skip in (False, True):
        out[skip] = wire.resume_tail_files_dev(lay.ptr, lay.written, _d64(incoming), tail_cap_bytes=8192,
                                               min_verify_bytes=100, mismatch_skip=skip)
    got = lay.result()  # synchronises
    want = _expect_files(vc, wire, win.stream, win.off, win.len, first, lay)
    assert np.array_equal(got["written"], want["written"]) and got["written"].tolist() == [end_a, end_b, 0, end_d]
    for skip in (False, True):
        action, roff, vlen, vcrc = out[skip]
        for s in range(4):
            at, w = int(lay.pos[s]), int(want["written"][s])
            local = want["canvas"][at:at + w]
            assert (int(action[s]), int(_u64(roff)[s]), int(_u64(vlen)[s]), int(_u32(vcrc)[s])) == \
                _host_tail(wire, local, int(incoming[s]), 8192, 100, skip), (skip, s)
        assert _i32(action).tolist() == [VERIFY_FIRST, VERIFY_FIRST, START_ZERO, SKIP_FILE if skip else START_ZERO]
        assert _u64(vlen).tolist() == [8192, end_b, 0, 0]


# ---- 3. every branch in one call ------------------------------------------------------------
def test_tail_mixture(vc, wire):
    cap, min_verify = 4096, 6000
    datas = [_prng.prng_bytes(300 + i, n) for i, n in enumerate((0, 5001, 3000, 20000, 5000, 1, 9000))]
    incoming = [100, 5000, 3000, 30000, 5000, 1, 8999]
    disk = Disk(datas)
    for skip in (False, True):
        a, ro, vl, vcrc = wire.resume_tail_files_dev(disk.ptr, disk.size, _d64(np.array(incoming, dtype=np.uint64)),
                                                     tail_cap_bytes=cap, min_verify_bytes=min_verify,
                                                     mismatch_skip=skip)
        torch.cuda.synchronize()
        got = list(zip(_i32(a).tolist(), _u64(ro).tolist(), _u64(vl).tolist(), _u32(vcrc).tolist()))
        assert got == [_host_tail(wire, d, inc, cap, min_verify, skip) for d, inc in zip(datas, incoming)]
        mism = SKIP_FILE if skip else START_ZERO
        assert [x[0] for x in got] == [START_ZERO, mism, VERIFY_FIRST, VERIFY_FIRST, VERIFY_FIRST, VERIFY_FIRST, mism]
        # a window shorter than the cap and than min_verify (the whole file), min_verify above the cap
        assert [x[2] for x in got] == [0, 0, 3000, 6000, 5000, 1, 0]
        assert all(x[1:] == (0, 0, 0) for x in got if x[0] != VERIFY_FIRST)
    # without min_verify the cap decides
    a, ro, vl, vcrc = wire.resume_tail_files_dev(disk.ptr, disk.size, _d64(np.array(incoming, dtype=np.uint64)),
                                                 tail_cap_bytes=cap)
    torch.cuda.synchronize()
    assert _u64(vl).tolist() == [0, 0, 3000, 4096, 4096, 1, 0]
    assert int(_u32(vcrc)[3]) == _crc(datas[3], 20000 - 4096, 4096)


def test_request_and_check_mixture(vc, wire):
    max_len = 10000
    file = _prng.prng_bytes(400, 30000)   # the sender's copy; the receivers hold prefixes of it
    actions = [VERIFY_FIRST, VERIFY_FIRST, START_ZERO, VERIFY_FIRST, VERIFY_FIRST, START_OFFSET, SKIP_FILE,
               VERIFY_FIRST, VERIFY_FIRST, ABORT_FILE]
    roffs = [20000, 500, 0, 0, 1 << 40, 7777, 0, 40000, 25000, 5]
    vlens = [8192, 4096, 0, 100, 1 << 32, 100, 0, 100, 10001, 5]
    n = len(actions)
    snd = Disk([file] * n, 21)
    req = wire.resume_request_files_dev(snd.ptr, snd.size, _di32(actions), _d64(np.array(roffs, dtype=np.uint64)),
                                        _d64(np.array(vlens, dtype=np.uint64)), max_len)
    torch.cuda.synchronize()
    got = list(zip(_u64(req[0]).tolist(), _u32(req[1]).tolist(), _u32(req[2]).tolist(), _i32(req[3]).tolist()))
    assert got == [_host_request(wire, file, a, r, v, max_len) for a, r, v in zip(actions, roffs, vlens)]
    # 1: resume_offset < verify_len; 3: resume_offset 0 and 4: a length of 2^32, both vlen32 == 0;
    # 7: a window behind the sender's file; 8: one above max_len
    assert got[1][:2] == (0, 500) and got[3] == (0, 0, 0, VAL_OK) and got[4] == (1 << 40, 0, 0, VAL_OK)
    assert got[7] == (39900, 100, 0, VAL_ERR_INVALID_ARG) and got[8] == (25000 - 10001, 10001, 0, VAL_ERR_INVALID_ARG)
    assert got[5] == (7777, 0, 0, VAL_OK) and got[0][3] == VAL_OK and got[0][2] == _crc(file, 20000 - 8192, 8192)
    # status is nullable
    req2 = wire.resume_request_files_dev(snd.ptr, snd.size, _di32(actions), _d64(np.array(roffs, dtype=np.uint64)),
                                         _d64(np.array(vlens, dtype=np.uint64)), max_len, want_status=False)
    torch.cuda.synchronize()
    assert req2[3] is None and all(np.array_equal(_u64(x) if x.dtype == torch.int64 else _u32(x),
                                                  _u64(y) if y.dtype == torch.int64 else _u32(y))
                                   for x, y in zip(req2[:3], req[:3]))

    # the receiver's side: local files and the VERIFY requests they answer
    local = [file[:20000].copy(), file[:20000].copy(), file[:3000].copy(), file[:5000].copy(), file[:20000].copy(),
             file[:100].copy(), file[:9000].copy(), file[:0].copy()]
    local[1][15000] ^= 0x5A  # a flipped byte inside the window
    c_act = [VERIFY_FIRST, VERIFY_FIRST, VERIFY_FIRST, START_ZERO, VERIFY_FIRST, VERIFY_FIRST, SKIP_FILE, VERIFY_FIRST]
    c_off = [20000 - 8192, 20000 - 8192, 2000, 0, 20000 - 8192, 90, U64 - 3, 0]
    c_len = [8192, 8192, 1001, 100, 8192, 10, 8, 0]
    c_crc = [_crc(file, o, l) if o < 30000 else 0 for o, l in zip(c_off, c_len)]
    c_crc[4] ^= 1  # the sender hashed other bytes
    c_rec = [20000, 20000, 3000, 0, 20000, 100, 9000, 0]
    incoming = [30000] * 8
    rcv = Disk(local, 22)
    m = len(local)
    for skip in (False, True):
        for with_action, with_crc in ((True, True), (False, True), (True, False)):
            result = torch.full((m,), C32, dtype=torch.int32, device=DEV)
            written = _d64(np.full(m, C64, dtype=np.uint64))
            local_crc = torch.full((m,), C32, dtype=torch.int32, device=DEV) if with_crc else None
            wire.resume_check_files_dev(rcv.ptr, rcv.size, _d64(np.array(incoming, dtype=np.uint64)),
                                        _d64(np.array(c_off, dtype=np.uint64)), _d32(np.array(c_len, dtype=np.uint32)),
                                        _d32(np.array(c_crc, dtype=np.uint32)),
                                        _d64(np.array(c_rec, dtype=np.uint64)), max_len, result=result, written=written,
                                        action=_di32(c_act) if with_action else None, local_crc=local_crc,
                                        mismatch_skip=skip)
            torch.cuda.synchronize()
            for s in range(m):
                if with_action and c_act[s] != VERIFY_FIRST:  # untouched: the sentinels survive
                    want = (C32, C32, C64)
                else:
                    want = _host_check(wire, local[s], incoming[s], c_off[s], c_len[s], c_crc[s], c_rec[s], max_len,
                                       skip)
                got_s = (int(_u32(local_crc)[s]) if with_crc else want[0], int(_i32(result)[s]), int(_u64(written)[s]))
                assert got_s == tuple(want), (skip, with_action, s)
            bad = VAL_SKIPPED if skip else VAL_ERR_RESUME_VERIFY
            back = 30000 if skip else 0
            res, wr = _i32(result).tolist(), _u64(written).tolist()
            # 0 matches; 1 a flipped byte; 2 a window one byte past the local file (local_crc 0);
            # 4 the sender's CRC differs; 5 matches at the file's end; 7 an empty window of an empty file
            assert (res[0], wr[0]) == (VAL_OK, 20000) and (res[1], wr[1]) == (bad, back)
            assert (res[2], wr[2]) == (bad, back) and (res[4], wr[4]) == (bad, back)
            assert (res[5], wr[5]) == (VAL_OK, 100) and (res[7], wr[7]) == (VAL_OK, 0)
            if with_crc:
                assert _u32(local_crc)[2] == 0 and _u32(local_crc)[1] != c_crc[1]
            if not with_action:  # every file is checked: 3 matches, 6's window wraps (a mismatch)
                assert (res[3], wr[3]) == (VAL_OK, 0) and (res[6], wr[6]) == (bad, back)


# ---- 4. fuzz ---------------------------------------------------------------------------------
def test_fuzz_against_the_rules(vc, wire):
    """200 rounds of random per-file states through all three calls. Files are at most 64 KiB."""
    rng = np.random.default_rng(2024)
    pool = _prng.prng_bytes(555, 1 << 16)
    S = 6
    for rnd in range(200):
        cap = int(rng.choice([0, 1, 100, 4096, 5000, 1 << 16]))
        min_verify = int(rng.choice([0, 0, 50, 4097, 30000]))
        skip = bool(rng.integers(0, 2))
        sizes = [int(rng.choice([0, 1, 3, int(rng.integers(1, 9000)), int(rng.integers(1, 1 << 16))])) for _ in range(S)]
        files = [pool[:max(sz, int(rng.integers(0, 1 << 16)))] if rng.integers(0, 4) else pool[:max(sz - 1, 0)]
                 for sz in sizes]  # the sender's file: longer than the local one, or (rarely) shorter
        local = [pool[:sz].copy() for sz in sizes]
        for d in local:
            if d.size and rng.integers(0, 3) == 0:
                d[int(rng.integers(0, d.size))] ^= 0x5A
        incoming = np.array([f.size for f in files], dtype=np.uint64)
        rcv, snd = Disk(local, 31), Disk(files, 32)
        max_len = max(min(cap if cap else 8 << 20, 256 << 20), min_verify)
        a, ro, vl, vcrc = wire.resume_tail_files_dev(rcv.ptr, rcv.size, _d64(incoming), tail_cap_bytes=cap,
                                                     min_verify_bytes=min_verify, mismatch_skip=skip)
        q_max = int(rng.choice([max_len, max_len, 64]))
        req_off, req_len, req_crc, status = wire.resume_request_files_dev(snd.ptr, snd.size, a, ro, vl, q_max)
        result = torch.full((S,), C32, dtype=torch.int32, device=DEV)
        written = _d64(np.full(S, C64, dtype=np.uint64))
        local_crc = torch.full((S,), C32, dtype=torch.int32, device=DEV)
        wire.resume_check_files_dev(rcv.ptr, rcv.size, _d64(incoming), req_off, req_len, req_crc, ro, max_len,
                                    result=result, written=written, action=a, local_crc=local_crc, mismatch_skip=skip)
        torch.cuda.synchronize()
        tail = list(zip(_i32(a).tolist(), _u64(ro).tolist(), _u64(vl).tolist(), _u32(vcrc).tolist()))
        request = list(zip(_u64(req_off).tolist(), _u32(req_len).tolist(), _u32(req_crc).tolist(),
                           _i32(status).tolist()))
        check = list(zip(_u32(local_crc).tolist(), _i32(result).tolist(), _u64(written).tolist()))
        for s in range(S):
            t = _host_tail(wire, local[s], int(incoming[s]), cap, min_verify, skip)
            assert tail[s] == t, (rnd, s)
            q = _host_request(wire, files[s], t[0], t[1], t[2], q_max)
            assert request[s] == q, (rnd, s)
            if t[0] == VERIFY_FIRST:
                c = _host_check(wire, local[s], int(incoming[s]), q[0], q[1], q[2], t[1], max_len, skip)
            else:
                c = (C32, C32, C64)  # untouched
            assert check[s] == c, (rnd, s)
