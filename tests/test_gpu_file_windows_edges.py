"""Directed tests for branches of k_win_count and k_win_hash
(csrc/windows_kernel.hpp) that only a shape beyond tests/test_gpu_file_windows.py
and tests/test_gpu_resume.py reaches: second and later trips of the persistent
hash grid over many files, the chunk sizes between 4 and 64 KiB, a batch with
max_len > 0 and no chunk at all, windows of up to 2^32 bytes (maps 28..31,
65,536 chunks of 64 KiB), the resume calls on long windows at every chunk size,
and the resume calls on 1,500 files.

Expected values never come from a device path: the oracle's CRC-32 of the host
copy of each window (for the long files, zeros with short runs of other bytes,
the oracle's update_state over the runs and its GF(2) shift over the zeros),
the header's validity rule in Python, and the three resume rules in plain C.
Every test that is there to reach a branch asserts that it reached it, from the
Python chunk counts and vc.plan_file_windows for the device it runs on."""
import numpy as np
import pytest

from tests import _oracle, _prng
from tests.test_gpu_file_windows import LENGTHS, STARTS, U64, VAL_ERR_INVALID_ARG, VAL_OK, Win, _place, _run, _u32, _want
from tests.test_gpu_resume import (C32, C64, START_ZERO, VAL_ERR_RESUME_VERIFY, VAL_SKIPPED, VERIFY_FIRST, Disk,
                                   _host_check, _host_request, _host_tail, _i32, _u64)
from tests.test_gpu_unpack import DEV, _d32, _d64, vc, wire  # noqa: F401 - vc and wire are fixtures

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MIB = 1 << 20
STEP = 16  # chunks a workgroup of k_win_hash takes per step, one per wave
TAIL_DEFAULT, TAIL_MAX = 8 * MIB, 256 * MIB


@pytest.fixture(autouse=True)
def _automatic_chunk(vc):
    yield
    vc.set_file_window_chunk(0)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(vc, k0, n_files, max_len, cus=None):
    """Sets the chunk knob (0: automatic) -> the call's three launches; both carry one k0."""
    vc.set_file_window_chunk(k0)
    plan = vc.plan_file_windows(_cus() if cus is None else cus, n_files, max_len)
    assert [p.kernel for p in plan] == [vc.KERNEL_WINDOWS_COUNT, vc.KERNEL_SCAN_FIRST, vc.KERNEL_WINDOWS_HASH]
    assert plan[0].k0 == plan[2].k0 and (k0 == 0 or plan[0].k0 >= k0)
    return plan


def _chunks(lens, k0):
    """Chunks of 2^k0 bytes per window length (0 for a window that is not hashed)."""
    return np.array([(int(n) + (1 << k0) - 1) >> k0 for n in lens], dtype=np.int64)


def _later_steps(cnt, grid):
    """What the steps of 16 chunks at or behind chunk grid * 16 hold, the steps a workgroup
    takes in its second and later trips -> counts of: whole steps (16 chunks of one file),
    whole steps whose first chunk is not a multiple of 16 inside its file, steps with chunks
    of three or more files, whole steps that end their file."""
    cnt = np.asarray(cnt, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)])
    total = int(first[-1])
    file_of = np.repeat(np.arange(cnt.size), cnt)
    inside = np.arange(total) - first[file_of]
    changes = np.concatenate([[0], np.cumsum(np.diff(file_of) != 0)])  # file changes in front of each chunk
    u0 = np.arange(grid * STEP, total, STEP)
    last = np.minimum(u0 + STEP, total) - 1
    whole = (u0 + STEP <= total) & (file_of[u0] == file_of[last])
    return dict(whole=int(whole.sum()),
                unaligned=int((whole & (inside[u0] % STEP != 0)).sum()),
                three_files=int((changes[last] - changes[u0] >= 2).sum()),
                ends_file=int((whole & (inside[last] + 1 == cnt[file_of[last]])).sum()))


def _windows_dev(vc, wire, ptr, size, off, length, max_len, crc, status):
    """val_crc32_file_windows_dev into outputs the test filled beforehand."""
    n = int(ptr.numel())
    work = torch.empty(max(wire.file_windows_work_bytes(n), 16), dtype=torch.uint8, device=DEV)
    st = vc.lib().val_crc32_file_windows_dev(vc._dptr(ptr), vc._dptr(size), vc._dptr(off), vc._dptr(length), n, max_len,
                                             vc._dptr(crc), vc._dptr(status), vc._dptr(work), int(work.numel()),
                                             vc._stream_ptr(None))
    assert st == VAL_OK, vc.last_error()
    torch.cuda.synchronize()


def _same(name, got, want, case):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (case, name, "first entries that differ", bad[:8].tolist(), got[bad[:8]].tolist(),
                           want[bad[:8]].tolist())


# ---- 1. later trips of the hash grid, many files --------------------------------------------------
def _views_batch(cus, seed, k0=12):
    """Files as views into one 1 MiB pool, lengths from the mix that gives every kind of step,
    until the batch has 3 * cus * 16 + 7 chunks; zero-chunk files in a row in front and behind.
    -> (pool, starts, wins, max_len)."""
    W = 1 << k0
    max_len = 50 * W
    rng = np.random.default_rng(seed)
    pool = _prng.prng_bytes(0x1A7E5, MIB)
    starts, wins = [], []

    def add(off, length, slack, refuse=None):
        size = off + length + slack
        if refuse == "past":  # off + len one past the file
            off += slack + 1
        elif refuse == "wraps":
            off = U64 - int(rng.integers(0, 7))
            length = max(length, 8)
        elif refuse == "long":  # inside the file, above max_len
            length = max_len + 1 + int(rng.integers(0, 3))
            size = off + length + slack
        start = int(rng.integers(0, pool.size - size + 1))
        starts.append(start)
        wins.append(Win(pool[start:start + size], off, length))

    def zero_chunk_run():
        for refuse in (None, "past", None, "wraps", "long", None):
            add(int(rng.integers(0, 200)), 0 if refuse is None else int(rng.integers(1, 3 * W)), 5, refuse)

    zero_chunk_run()
    chunks = 0
    while chunks < 3 * cus * STEP + 7:
        kind = int(rng.integers(0, 10))
        if kind == 0:
            length = 0
        elif kind == 1:
            length = int(rng.integers(1, 64))
        elif kind <= 4:
            length = int(rng.integers(64, 3 * W))
        elif kind <= 6:
            length = int(rng.integers(3 * W, 9 * W))
        elif kind == 7:
            length = W * int(rng.integers(15, 19)) + int(rng.integers(-1, 2))
        elif kind == 8:
            length = W * int(rng.integers(31, 50)) + int(rng.integers(0, W))
        else:
            length = W * int(rng.integers(1, 4))
        refuse = ("past", "wraps", "long")[int(rng.integers(0, 3))] if rng.integers(0, 30) == 0 else None
        add(int(rng.integers(0, 200)), length, int(rng.integers(0, 9)), refuse)
        if refuse is None:
            chunks += -(-length // W)
    zero_chunk_run()
    return pool, starts, wins, max_len


def test_later_passes_with_many_files(vc, wire):
    """k_win_hash: the second and later trips of `for (u0 ...; u0 += stride, slot ^= 1u)`, where u0 is
    no longer blockIdx.x * 16 and the LDS slots alternate, over some 1,500 files: steps that span files
    (a win_fold per chunk), whole steps that begin anywhere in their file, files finished by a 16-chunk
    arrival, and the search in first[] across runs of files without chunks."""
    cus = _cus()
    pool, starts, wins, max_len = _views_batch(cus, seed=2031)
    n = len(wins)
    plan = _plan(vc, 12, n, max_len)
    grid = plan[2].grid
    assert plan[2].k0 == 12
    want_crc, want_status = _want(wins, max_len)
    cnt = _chunks([w["len"] if st == VAL_OK else 0 for w, st in zip(wins, want_status)], 12)
    assert cnt.sum() >= 3 * grid * STEP + 7, (int(cnt.sum()), grid)  # every workgroup takes three trips or more
    assert not cnt[:6].any() and not cnt[-6:].any() and cnt[6:-6].any()
    assert (want_status[6:-6] != VAL_OK).sum() >= 20  # refused windows among the others
    reached = _later_steps(cnt, grid)
    assert reached["whole"] >= 20 and reached["unaligned"] >= 20 and reached["three_files"] >= 20, reached
    assert reached["ends_file"] >= 3, reached
    d_pool = torch.from_numpy(pool).to(DEV)
    ptr = _d64(np.array([d_pool.data_ptr() + s for s in starts], dtype=np.uint64))
    size = _d64(np.array([w["data"].size for w in wins], dtype=np.uint64))
    off = _d64(np.array([w["off"] for w in wins], dtype=np.uint64))
    length = _d64(np.array([w["len"] for w in wins], dtype=np.uint64))
    for k0 in (12, 0):
        vc.set_file_window_chunk(k0)
        crc, status = wire.file_windows_dev(ptr, size, off, length, max_len)
        torch.cuda.synchronize()
        _same("crc", _u32(crc), want_crc, (k0, n, grid))
        _same("status", status.cpu().numpy(), want_status, (k0, n, grid))


# ---- 2. every chunk size ----------------------------------------------------------------------------
def test_every_chunk_size(vc, wire):
    """lds_pow_issue(consts, k0) and C = ceil(len / 2^k0) at 8, 16 and 32 KiB: the lengths of
    test_length_and_start_sweep restated for W = 2^k0 at its starts; then one 40-file batch at every
    forced chunk and the automatic one."""
    pool = _prng.prng_bytes(1300, 2 * MIB)
    for k0 in (13, 14, 15):
        W = 1 << k0
        lengths = (0, 1, 3, 4, W - 1, W, W + 1, 2 * W + 5, 16 * W, 16 * W + 1, 17 * W + 3)
        assert len(lengths) == len(LENGTHS) and all(a == b for a, b in zip(lengths, LENGTHS) if b < 4095)
        wins = []
        for i, (length, start) in enumerate((n, s) for n in lengths for s in STARTS):
            at = 1009 * i % 4096
            wins.append(Win(pool[at:at + start + length + i % 5], start, length))
        assert _plan(vc, k0, len(wins), max(lengths))[2].k0 == k0
        _run(vc, wire, wins, max(lengths), k0s=(k0,))
    # 40 files of mixed lengths: one chunk, a few, a whole step of every chunk size and more
    rng = np.random.default_rng(40)
    mixed = []
    for i in range(40):
        kind = int(rng.integers(0, 8))
        w = 1 << int(rng.integers(12, 17))
        length = (0, int(rng.integers(1, 64)), int(rng.integers(64, 4096)), int(rng.integers(4096, 40000)),
                  int(rng.integers(40000, 300000)), w * int(rng.integers(1, 4)), 16 * w + int(rng.integers(-1, 2)),
                  17 * w + int(rng.integers(0, w)))[kind]
        start, at = int(rng.integers(0, 200)), int(rng.integers(0, 4096))
        mixed.append(Win(pool[at:at + start + length + int(rng.integers(0, 9))], start, length))
    max_len = max(w["len"] for w in mixed)
    want_crc, want_status = _want(mixed, max_len)
    assert not want_status.any()
    buf, ptr, size, off, length = _place(mixed)
    got = {}
    for forced in (12, 13, 14, 15, 16, 0):
        used = _plan(vc, forced, len(mixed), max_len)[2].k0
        assert forced == 0 or used == forced
        crc, status = wire.file_windows_dev(ptr, size, off, length, max_len)
        torch.cuda.synchronize()
        got[forced] = _u32(crc)
        _same("crc", got[forced], want_crc, (forced, used))
        assert not status.cpu().numpy().any()
    assert all(np.array_equal(g, got[0]) for g in got.values())


# ---- 3. max_len > 0 and no chunk in the batch ---------------------------------------------------------
def test_batch_with_no_chunks_at_all(vc, wire):
    """Every window is empty or refused: k_win_count finishes all 300 files, first[n] is 0 and no
    workgroup of k_win_hash enters its loop. The outputs hold a sentinel on entry, so a file that
    nobody finished shows."""
    n, max_len, fsize = 300, 4096, 5000
    data = _prng.prng_bytes(33, fsize)
    kinds = ((0, 0), (fsize, 0),        # empty at offset 0 and at the file's end
             (fsize - 99, 100),         # one past the file
             (U64 - 3, 8),              # off + len wraps
             (7, max_len + 1),          # inside the file, above max_len
             (fsize + 1, 0))            # an empty window behind the file
    wins = [Win(data, *kinds[(i * 7 + i // 11) % len(kinds)]) for i in range(n)]
    want_crc, want_status = _want(wins, max_len)
    assert not want_crc.any() and set(want_status.tolist()) == {VAL_OK, VAL_ERR_INVALID_ARG}
    assert [int(want_status[[i for i, w in enumerate(wins) if (w["off"], w["len"]) == k][0]]) for k in kinds] == \
        [VAL_OK, VAL_OK] + [VAL_ERR_INVALID_ARG] * 4
    assert (want_status[256:] == VAL_OK).any() and (want_status[256:] != VAL_OK).any()  # the second workgroup of k_win_count
    buf, ptr, size, off, length = _place(wins)
    for k0 in (12, 0, 16):
        assert len(_plan(vc, k0, n, max_len)) == 3 and len(vc.plan_file_windows(_cus(), n, 0)) == 1
        crc = torch.full((n,), C32, dtype=torch.int32, device=DEV)
        status = torch.full((n,), C32, dtype=torch.int32, device=DEV)
        _windows_dev(vc, wire, ptr, size, off, length, max_len, crc, status)
        _same("crc", _u32(crc), want_crc, k0)
        _same("status", status.cpu().numpy(), want_status, k0)


# ---- long files: zeros with short runs of other bytes ------------------------------------------------
class Sparse:
    """A file of `size` zero bytes with runs of other bytes, [(position, bytes)] in ascending order.
    The oracle's register walks a window of it run by run: update_state over the bytes of a run,
    the GF(2) shift over the zeros between two."""

    def __init__(self, size, runs):
        self.size, self.runs = size, [(int(p), np.asarray(b, dtype=np.uint8)) for p, b in runs]
        assert all(p + b.size <= q for (p, b), (q, _) in zip(self.runs[:-1], self.runs[1:]))
        assert self.runs[-1][0] + self.runs[-1][1].size <= size and all(b.size <= 100 for _, b in self.runs)

    def to_device(self):
        buf = torch.zeros(self.size, dtype=torch.uint8, device=DEV)
        for p, b in self.runs:
            buf[p:p + b.size] = torch.from_numpy(b).to(DEV)
        return buf

    def pieces(self, off, length):
        """[off, off + length) as (bytes or None for zeros, count) in order."""
        pos, end = off, off + length
        for p, b in self.runs:
            lo, hi = max(p, pos), min(p + b.size, end)
            if lo < hi:
                if lo > pos:
                    yield None, lo - pos
                yield b[lo - p:hi - p], hi - lo
                pos = hi
        if end > pos:
            yield None, end - pos

    def crc(self, off, length):
        assert off + length <= self.size
        state = 0xFFFFFFFF
        for b, k in self.pieces(off, length):
            state = _oracle.shift(state, k) if b is None else _oracle.update_state(state, b)
        return state ^ 0xFFFFFFFF

    def crc_by_combine(self, off, length):
        """The same from the CRCs of the pieces and the oracle's combine."""
        crc = 0
        for b, k in self.pieces(off, length):
            crc = _oracle.combine(crc, _oracle.shift(0xFFFFFFFF, k) ^ 0xFFFFFFFF if b is None else _oracle.crc32(b), k)
        return crc


# ---- 4. the call's largest window --------------------------------------------------------------------
def test_four_gib_window(vc, wire):
    """max_len = 2^32, where the plan raises any chunk to 64 KiB: a window of 2^32 bytes is 65,536
    chunks, and chunk 0 is advanced over 65,535 chunks by the maps "advance 2^16 .. 2^31 bytes", 28..31
    among them. 2^32 is also where a length kept in 32 bits would read 0. One buffer of zeros with short
    random runs serves the generic call and the three resume calls.

    On an MI355X the test takes 0.13 s, allocation and fill included."""
    G4, G2 = 1 << 32, 1 << 31
    ee, r = (lambda k: np.full(k, 0xEE, np.uint8)), _prng.prng_bytes
    sp = Sparse(3 + G4 + 8, [(0, ee(3)), (3, r(71, 100)), (G2 - 70, r(72, 68)), (G2 + 1, r(73, 89)),
                             (G4 - 65530 - 40, r(74, 50)), (G4 - 60, r(75, 63)), (G4 + 3, ee(8))])
    windows = [(3, G4),               # 65,536 chunks of 64 KiB: every map 16..31
               (5, G4 - 65535),       # still 65,536 chunks, the first one byte long
               (G2 - 10, G2 + 1),     # 32,769 chunks: chunk 0, one byte, is advanced by map 31 alone
               (3, G4 + 1),           # inside the file and above max_len: refused
               (0, 50), (G2 - 40, 100)]
    want = [sp.crc(o, n) if n <= G4 else 0 for o, n in windows]
    assert want[0] == sp.crc_by_combine(*windows[0]) and len(set(want)) == len(want)
    for k0 in (12, 0):
        assert _plan(vc, k0, len(windows), G4)[2].k0 == 16  # raised, so one run serves both
    assert _chunks([n if n <= G4 else 0 for _, n in windows], 16).tolist() == [65536, 65536, 32769, 0, 1, 1]
    try:
        buf = sp.to_device()
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no room for a buffer of 4 GiB")
    base = buf.data_ptr()
    m = len(windows)
    crc, status = wire.file_windows_dev(_d64(np.full(m, base, dtype=np.uint64)), _d64(np.full(m, sp.size, dtype=np.uint64)),
                                        _d64(np.array([o for o, _ in windows], dtype=np.uint64)),
                                        _d64(np.array([n for _, n in windows], dtype=np.uint64)), G4)
    torch.cuda.synchronize()
    assert _u32(crc).tolist() == want
    assert status.cpu().numpy().tolist() == [0, 0, 0, VAL_ERR_INVALID_ARG, 0, 0]

    # the receiver's proposal: a file of 2^32 + 8 bytes at buf + 3 whose policy asks for 2^32 bytes
    # (and a 50-byte file at buf)
    vc.set_file_window_chunk(0)
    ptr = _d64(np.array([base + 3, base], dtype=np.uint64))
    existing, incoming = [G4 + 8, 50], [G4 + 1000, 60]
    rule = [wire.resume_tail_window(e, i, 0, G4, False) for e, i in zip(existing, incoming)]
    assert rule == [(VERIFY_FIRST, G4 + 8, G4), (VERIFY_FIRST, 50, 50)]
    a, ro, vl, vcrc = wire.resume_tail_files_dev(ptr, _d64(np.array(existing, dtype=np.uint64)),
                                                 _d64(np.array(incoming, dtype=np.uint64)), min_verify_bytes=G4)
    # the sender's answer on the device: (uint32_t)2^32 is 0, an empty window, and no VERIFY goes out
    req = wire.resume_request_files_dev(ptr, _d64(np.array([sp.size - 3, sp.size], dtype=np.uint64)), a, ro, vl, G4)
    torch.cuda.synchronize()
    got = list(zip(_i32(a).tolist(), _u64(ro).tolist(), _u64(vl).tolist(), _u32(vcrc).tolist()))
    assert got == [rule[0] + (sp.crc(3 + 8, G4),), rule[1] + (sp.crc(0, 50),)]
    assert wire.resume_request_window(G4 + 8, G4) == (False, G4 + 8, 0)
    got = list(zip(_u64(req[0]).tolist(), _u32(req[1]).tolist(), _u32(req[2]).tolist(), _i32(req[3]).tolist()))
    assert got == [(G4 + 8, 0, 0, VAL_OK), (0, 50, sp.crc(0, 50), VAL_OK)]
    # the receiver's check of the longest request the wire can carry, matching and one bit off
    local = sp.crc(3 + 9, G4 - 1)
    req_crc = [local, local ^ (1 << 17)]
    ptr2 = _d64(np.array([base + 3, base + 3], dtype=np.uint64))
    for skip in (False, True):
        result = torch.full((2,), C32, dtype=torch.int32, device=DEV)
        written = _d64(np.full(2, C64, dtype=np.uint64))
        local_crc = torch.full((2,), C32, dtype=torch.int32, device=DEV)
        wire.resume_check_files_dev(ptr2, _d64(np.array([G4 + 8] * 2, dtype=np.uint64)),
                                    _d64(np.array([G4 + 1000] * 2, dtype=np.uint64)),
                                    _d64(np.array([9, 9], dtype=np.uint64)), _d32(np.array([G4 - 1] * 2, dtype=np.uint32)),
                                    _d32(np.array(req_crc, dtype=np.uint32)), _d64(np.array([G4 + 8] * 2, dtype=np.uint64)),
                                    G4, result=result, written=written, local_crc=local_crc, mismatch_skip=skip)
        torch.cuda.synchronize()
        verdict = [wire.resume_verdict(True, local, c, skip, G4 + 8, G4 + 1000) for c in req_crc]
        assert verdict == [(VAL_OK, G4 + 8), (VAL_SKIPPED, G4 + 1000) if skip else (VAL_ERR_RESUME_VERIFY, 0)]
        assert list(zip(_i32(result).tolist(), _u64(written).tolist())) == verdict, skip
        assert _u32(local_crc).tolist() == [local, local], skip


# ---- 5. the resume calls on long windows, at every chunk size ------------------------------------------
def _tail_max_len(cap, min_verify=0):
    return max(min(cap if cap else TAIL_DEFAULT, TAIL_MAX), min_verify)


def _rule_tail(wire, f, incoming, cap, skip=False):
    if not isinstance(f, Sparse):
        return _host_tail(wire, f, incoming, cap, 0, skip)
    action, roff, vlen = wire.resume_tail_window(f.size, incoming, cap, 0, skip)
    return action, roff, vlen, (f.crc(roff - vlen, vlen) if action == VERIFY_FIRST else 0)


def _rule_request(wire, f, t, max_len):
    if not isinstance(f, Sparse):
        return _host_request(wire, f, t[0], t[1], t[2], max_len)
    send, start, v32 = wire.resume_request_window(t[1], t[2])
    assert t[0] == VERIFY_FIRST and send and v32 <= max_len and start + v32 <= f.size
    return start, v32, f.crc(start, v32), VAL_OK


def _rule_check(wire, f, incoming, q, rec_off, max_len, skip):
    if not isinstance(f, Sparse):
        return _host_check(wire, f, incoming, q[0], q[1], q[2], rec_off, max_len, skip)
    assert q[1] <= max_len and q[0] + q[1] <= f.size
    crc = f.crc(q[0], q[1])
    return (crc,) + tuple(wire.resume_verdict(True, crc, q[2], skip, rec_off, incoming))


def test_resume_long_windows(vc, wire):
    """The three calls at 4 KiB, 64 KiB and the automatic chunk on: files of 16 W, 16 W + 1 and
    33 W + 5 bytes that lead the batch, so file 0's only step is a whole one and win_finish runs in
    tail, request and check mode from the 16-chunk arrival; a tail window of exactly the default 8 MiB;
    a file of 256 MiB + 5 B under tail_cap_bytes = 2^40, clamped to 256 MiB. The tail call's outputs
    feed the request call over the sender's copies, and that the check call, with nothing read back."""
    r = _prng.prng_bytes
    pool = r(91, 4 * MIB)
    big = r(92, TAIL_DEFAULT + 3)
    big_local = big.copy()
    big_local[2] ^= 0x5A  # the byte in front of the default window
    n_sp = TAIL_MAX + 5
    runs = [(5, r(94, 90)), (n_sp // 2 - 11, r(95, 77)), (n_sp - TAIL_DEFAULT - 30, r(96, 60)), (n_sp - 50, r(97, 50))]
    sp = Sparse(n_sp, [(0, r(93, 5))] + runs)
    sp_local = Sparse(n_sp, [(0, r(98, 5))] + runs)  # other bytes in front of the 256 MiB window
    assert sp.runs[0][1][4] != sp_local.runs[0][1][4]
    d_big, d_big_local, d_sp, d_sp_local = (torch.from_numpy(big).to(DEV), torch.from_numpy(big_local).to(DEV),
                                            sp.to_device(), sp_local.to_device())
    n = 6
    for forced in (0, 12, 16):
        for cap in (0, 1 << 40):
            max_len = _tail_max_len(cap)
            k0 = _plan(vc, forced, n, max_len)[2].k0
            assert forced == 0 or k0 == forced
            W = 1 << k0
            # the sender's files, and the receiver's shorter copies of them
            files = [pool[7:7 + 16 * W + 777], pool[100:100 + 16 * W + 1], pool[33:33 + 40 * W], big, sp, pool[:100]]
            local = [files[0][:16 * W].copy(), files[1].copy(), files[2][:33 * W + 5].copy(), big_local, sp_local,
                     pool[:0].copy()]
            local[2][20 * W + 1] ^= 0x5A  # inside the window
            snd, rcv = Disk([f for f in files if f is not big and f is not sp], 51), \
                Disk([f for f in local if f is not big_local and f is not sp_local], 52)

            def addresses(disk, d_long):
                at = (disk.at + np.uint64(disk.buf.data_ptr())).tolist()
                return _d64(np.array(at[:3] + [t.data_ptr() for t in d_long] + at[3:], dtype=np.uint64))

            snd_ptr, rcv_ptr = addresses(snd, (d_big, d_sp)), addresses(rcv, (d_big_local, d_sp_local))
            snd_size = _d64(np.array([f.size for f in files], dtype=np.uint64))
            existing = _d64(np.array([f.size for f in local], dtype=np.uint64))
            inc = [f.size for f in files]
            incoming = _d64(np.array(inc, dtype=np.uint64))
            case = f"chunk {forced} (2^{k0}) cap {cap}"
            # what the rules say, and that the batch is the one this test is for
            tail = [_rule_tail(wire, f, i, cap) for f, i in zip(local, inc)]
            assert [t[0] for t in tail] == [VERIFY_FIRST] * 5 + [START_ZERO]
            cnt = _chunks([t[2] for t in tail], k0)
            first = np.concatenate([[0], np.cumsum(cnt)])
            assert cnt[:3].tolist() == [16, 17, 34] and first[0] % STEP == 0 and first[1] % STEP == 0, case
            assert tail[3][2] == (TAIL_DEFAULT + 3 if cap else TAIL_DEFAULT) and tail[4][2] == (TAIL_MAX if cap else TAIL_DEFAULT)
            request = [_rule_request(wire, f, t, max_len) for f, t in zip(files, tail)]
            assert [q[3] for q in request] == [VAL_OK] * n and [q[1] for q in request] == [t[2] for t in tail]
            a, ro, vl, vcrc = wire.resume_tail_files_dev(rcv_ptr, existing, incoming, tail_cap_bytes=cap)
            q_off, q_len, q_crc, q_status = wire.resume_request_files_dev(snd_ptr, snd_size, a, ro, vl, max_len)
            out = {}
            for skip in (False, True):
                result = torch.full((n,), C32, dtype=torch.int32, device=DEV)
                written = _d64(np.full(n, C64, dtype=np.uint64))
                local_crc = torch.full((n,), C32, dtype=torch.int32, device=DEV)
                wire.resume_check_files_dev(rcv_ptr, existing, incoming, q_off, q_len, q_crc, ro, max_len, result=result,
                                            written=written, action=a, local_crc=local_crc, mismatch_skip=skip)
                out[skip] = local_crc, result, written
            torch.cuda.synchronize()
            got = list(zip(_i32(a).tolist(), _u64(ro).tolist(), _u64(vl).tolist(), _u32(vcrc).tolist()))
            assert got == tail, case
            got = list(zip(_u64(q_off).tolist(), _u32(q_len).tolist(), _u32(q_crc).tolist(), _i32(q_status).tolist()))
            assert got == request, case
            for skip in (False, True):
                check = [tuple(_rule_check(wire, f, i, q, t[1], max_len, skip)) if t[0] == VERIFY_FIRST else (C32, C32, C64)
                         for f, i, q, t in zip(local, inc, request, tail)]
                got = list(zip(_u32(out[skip][0]).tolist(), _i32(out[skip][1]).tolist(), _u64(out[skip][2]).tolist()))
                assert got == check, (case, skip)
                bad = (VAL_SKIPPED, None) if skip else (VAL_ERR_RESUME_VERIFY, 0)
                verdicts = [(c[1], c[2]) for c in check]
                # file 0: finished by its one whole step; 2: a flipped byte in the window; 3: one in front of the
                # default window, which is inside the whole file that the larger cap takes; 4: one in front of the
                # clamped window
                assert verdicts[0] == (VAL_OK, 16 * W) and verdicts[1] == (VAL_OK, 16 * W + 1), (case, skip)
                assert verdicts[2] == (bad[0], inc[2] if skip else 0), (case, skip)
                assert verdicts[3] == ((bad[0], inc[3] if skip else 0) if cap else (VAL_OK, big.size)), (case, skip)
                assert verdicts[4] == (VAL_OK, n_sp), (case, skip)


# ---- 6. the resume calls on many files ------------------------------------------------------------------
def test_resume_many_files(vc, wire):
    """k_win_count's three resume branches beyond its first workgroup of 256 threads, and k_win_hash's
    win_finish in every mode for files found deep in first[]: 1,500 files of at most 40 KiB in the
    states test_fuzz_against_the_rules draws, through tail, request and check with nothing read back."""
    S = 1500
    rng = np.random.default_rng(1500)
    pool = _prng.prng_bytes(556, 1 << 17)
    sizes = [int(rng.choice([0, 1, 3, int(rng.integers(1, 9000)), int(rng.integers(1, 40 << 10))])) for _ in range(S)]
    at = [int(rng.integers(0, 1 << 16)) for _ in range(S)]
    files = [pool[a:a + max(sz, int(rng.integers(0, 40 << 10)))] if rng.integers(0, 4) else pool[a:a + max(sz - 1, 0)]
             for a, sz in zip(at, sizes)]  # the sender's file: longer than the local one, or (rarely) shorter
    local = [pool[a:a + sz].copy() for a, sz in zip(at, sizes)]
    for d in local:
        if d.size and rng.integers(0, 3) == 0:
            d[int(rng.integers(0, d.size))] ^= 0x5A
    inc = [f.size for f in files]
    incoming = _d64(np.array(inc, dtype=np.uint64))
    rcv, snd = Disk(local, 61), Disk(files, 62)
    # three policies; the sender's max_len is below some of the windows asked of it, so it refuses those
    for cap, min_verify, skip, q_max in ((4096, 6000, False, 5000), (0, 0, True, 20000), (5000, 0, True, 64)):
        max_len = _tail_max_len(cap, min_verify)
        tail = [_host_tail(wire, d, i, cap, min_verify, skip) for d, i in zip(local, inc)]
        request = [_host_request(wire, f, t[0], t[1], t[2], q_max) for f, t in zip(files, tail)]
        check = [tuple(_host_check(wire, d, i, q[0], q[1], q[2], t[1], max_len, skip)) if t[0] == VERIFY_FIRST
                 else (C32, C32, C64) for d, i, q, t in zip(local, inc, request, tail)]
        verify = np.array([t[0] == VERIFY_FIRST for t in tail])
        refused = np.array([q[3] != VAL_OK for q in request])
        failed = np.array([c[1] not in (VAL_OK, C32) for c in check])
        passed = np.array([c[1] == VAL_OK for c in check])
        for what in (verify, ~verify, refused, failed, passed):  # in the second workgroup of k_win_count and the sixth
            assert what[256:1024].any() and what[1024:].any(), (cap, min_verify, skip)
        for k0 in (12, 0):
            case = f"cap {cap} min_verify {min_verify} skip {skip} q_max {q_max} chunk {k0}"
            for m in {max_len, q_max}:
                _plan(vc, k0, S, m)
            a, ro, vl, vcrc = wire.resume_tail_files_dev(rcv.ptr, rcv.size, incoming, tail_cap_bytes=cap,
                                                         min_verify_bytes=min_verify, mismatch_skip=skip)
            q_off, q_len, q_crc, q_status = wire.resume_request_files_dev(snd.ptr, snd.size, a, ro, vl, q_max)
            result = torch.full((S,), C32, dtype=torch.int32, device=DEV)
            written = _d64(np.full(S, C64, dtype=np.uint64))
            local_crc = torch.full((S,), C32, dtype=torch.int32, device=DEV)
            wire.resume_check_files_dev(rcv.ptr, rcv.size, incoming, q_off, q_len, q_crc, ro, max_len, result=result,
                                        written=written, action=a, local_crc=local_crc, mismatch_skip=skip)
            torch.cuda.synchronize()
            for name, got, col, rows in (("action", _i32(a), 0, tail), ("resume_off", _u64(ro), 1, tail),
                                         ("verify_len", _u64(vl), 2, tail), ("verify_crc", _u32(vcrc), 3, tail),
                                         ("req_off", _u64(q_off), 0, request), ("req_len", _u32(q_len), 1, request),
                                         ("req_crc", _u32(q_crc), 2, request), ("status", _i32(q_status), 3, request),
                                         ("local_crc", _u32(local_crc), 0, check), ("result", _i32(result), 1, check),
                                         ("written", _u64(written), 2, check)):
                _same(name, got, np.array([row[col] for row in rows], dtype=got.dtype), case)
