"""val_crc32_file_windows_dev: the CRC-32 of one byte window per GPU-resident
file, many files in one device call (include/val_crc32_gpu.h; DESIGN.md
section 4.12).

Expected values never come from the device path: the oracle's CRC-32 of the
host copy of the window, and the header's validity rule applied in Python.
Every batch goes through _run: the files lie in one device buffer at odd
addresses with guard bytes between them, and the batch is hashed with 4 KiB
chunks forced (so that the multi-chunk paths run on kilobytes), with the
automatic chunk and with 64 KiB chunks; the three results must be the oracle's."""
import numpy as np
import pytest

from tests import _oracle, _prng
from tests.test_gpu_unpack import DEV, _d64, vc, wire  # noqa: F401 - vc and wire are fixtures

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
W = 4096  # the forced chunk
K0S = (12, 0, 16)
VAL_OK, VAL_ERR_INVALID_ARG = 0, -1
LENGTHS = (0, 1, 3, 4, 4095, 4096, 4097, 2 * 4096 + 5, 16 * 4096, 16 * 4096 + 1, 17 * 4096 + 3)
STARTS = (0, 1, 2, 3, 127)


@pytest.fixture(autouse=True)
def _automatic_chunk(vc):
    yield
    vc.set_file_window_chunk(0)


def Win(data, off, length):
    """One file (its bytes) and the window asked of it."""
    return dict(data=np.asarray(data, dtype=np.uint8), off=off, len=length)


def _valid(w, max_len):
    return w["len"] <= max_len and w["off"] <= w["data"].size and w["len"] <= w["data"].size - w["off"]


def _want(wins, max_len):
    crc = np.zeros(len(wins), np.uint32)
    status = np.zeros(len(wins), np.int32)
    for i, w in enumerate(wins):
        if _valid(w, max_len):
            crc[i] = _oracle.crc32(w["data"][w["off"]:w["off"] + w["len"]])
        else:
            status[i] = VAL_ERR_INVALID_ARG
    return crc, status


def _place(wins):
    """The files in one device buffer, each at an odd address, 3 or 4 guard bytes apart
    -> (buffer, int64 tensors file_ptr, file_size, win_off, win_len)."""
    pos, at = 1, []
    for w in wins:
        pos |= 1
        at.append(pos)
        pos += w["data"].size + 3
    host = _prng.prng_bytes(977, pos + 8)
    for o, w in zip(at, wins):
        host[o:o + w["data"].size] = w["data"]
    buf = torch.from_numpy(host).to(DEV)
    base = buf.data_ptr()
    assert base % 2 == 0
    ptr = _d64(np.array([base + o for o in at], dtype=np.uint64))
    size = _d64(np.array([w["data"].size for w in wins], dtype=np.uint64))
    off = _d64(np.array([w["off"] for w in wins], dtype=np.uint64))
    length = _d64(np.array([w["len"] for w in wins], dtype=np.uint64))
    return buf, ptr, size, off, length


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _run(vc, wire, wins, max_len, *, k0s=K0S, want=None):
    want_crc, want_status = _want(wins, max_len) if want is None else want
    buf, ptr, size, off, length = _place(wins)
    for k0 in k0s:
        vc.set_file_window_chunk(k0)
        crc, status = wire.file_windows_dev(ptr, size, off, length, max_len)
        torch.cuda.synchronize()
        bad = np.nonzero(_u32(crc) != want_crc)[0]
        assert bad.size == 0, (k0, bad[:8], [(wins[i]["off"], wins[i]["len"]) for i in bad[:8]])
        assert np.array_equal(status.cpu().numpy(), want_status), k0
    return want_crc, want_status


def _bytes(seed, n):
    return _prng.prng_bytes(seed, n)


def test_length_and_start_sweep(vc, wire):
    """Every length at every start offset, in files at odd addresses: short first chunks of every
    alignment, whole chunks, a full workgroup of 16 chunks and one chunk past it."""
    wins = []
    for i, (length, start) in enumerate((l, s) for l in LENGTHS for s in STARTS):
        wins.append(Win(_bytes(100 + i, start + length + (i % 5)), start, length))
    crc, _ = _run(vc, wire, wins, max(LENGTHS))
    assert all(crc[i] == 0 for i, w in enumerate(wins) if w["len"] == 0)  # the empty window's CRC
    assert len(set(crc[[i for i, w in enumerate(wins) if w["len"]]])) > 40  # the oracle saw different bytes


@pytest.mark.parametrize("n_files", [1, 2, 17, 600])
def test_many_files_of_mixed_lengths(vc, wire, n_files):
    """600 files are more than the hash grid has workgroups; zeros, sub-chunk and multi-chunk windows mixed."""
    rng = np.random.default_rng(n_files)
    wins = []
    for i in range(n_files):
        kind = int(rng.integers(0, 6))
        length = (0, int(rng.integers(1, 64)), int(rng.integers(64, W)), int(rng.integers(W, 3 * W)),
                  int(rng.integers(3 * W, 9 * W)), W * int(rng.integers(1, 4)))[kind]
        start = int(rng.integers(0, 200))
        wins.append(Win(_bytes(7000 + i, start + length + int(rng.integers(0, 9))), start, length))
    _run(vc, wire, wins, 9 * W)


def test_refused_windows_leave_their_neighbours_exact(vc, wire):
    max_len = 5000
    data = _bytes(31, 8000)
    wins = [Win(data, 10, 5000),
            Win(data, 8000 - 99, 100),        # off + len one past the file
            Win(data, 17, 4099),
            Win(data, U64 - 3, 8),            # off + len wraps to 4
            Win(data, 3000, U64),             # len near 2^64
            Win(data, 1, max_len + 1),        # inside the file, above max_len
            Win(data, 8001, 0),               # an empty window behind the file
            Win(data, 8000, 0),               # an empty window at its end is valid
            Win(data, 8000 - 100, 100)]       # the file's last bytes
    crc, status = _run(vc, wire, wins, max_len)
    assert list(status) == [0, -1, 0, -1, -1, -1, -1, 0, 0]
    assert all(crc[i] == 0 for i in (1, 3, 4, 5, 6, 7)) and all(crc[i] != 0 for i in (0, 2, 8))


def test_max_len_zero_accepts_only_empty_windows(vc, wire):
    data = _bytes(32, 100)
    crc, status = _run(vc, wire, [Win(data, 0, 0), Win(data, 5, 1), Win(data, 100, 0), Win(data, 101, 0)], 0)
    assert list(status) == [0, -1, 0, -1] and not crc.any()


def test_one_long_window_among_short_ones(vc, wire):
    """16 MiB + 5 B is 4,097 chunks of 4 KiB: distances of 0 .. 4,096 chunks, 13 bits of the advance."""
    long_len = (16 << 20) + 5
    wins = [Win(_bytes(500 + i, 1024 + i % 3), i % 3, 1024) for i in range(63)]
    wins.insert(40, Win(_bytes(499, long_len + 9), 2, long_len))
    _run(vc, wire, wins, long_len)


def test_256_mib_window_uses_all_sixteen_maps(vc, wire):
    """2^28 bytes at 4 KiB chunks are 65,536 chunks: the first is advanced over 65,535 chunks, one map
    per bit. The file is zeros with 100 random bytes at the window's head and 7 at its tail; the oracle
    carries the head's register over the zeros with its GF(2) shift, so the host hashes nothing long."""
    n, start = 1 << 28, 3
    head, tail = _bytes(61, 100), _bytes(62, 7)
    buf = torch.zeros(start + n + 5, dtype=torch.uint8, device=DEV)
    buf[start:start + 100] = torch.from_numpy(head).to(DEV)
    buf[start + n - 7:start + n] = torch.from_numpy(tail).to(DEV)
    buf[:start] = 0xEE  # bytes around the window that must not count
    buf[start + n:] = 0xEE
    state = _oracle.update_state(0xFFFFFFFF, head)
    state = _oracle.shift(state, n - 107)
    want = _oracle.update_state(state, tail) ^ 0xFFFFFFFF
    # the same by the oracle's combine: crc(head | zeros) from crc(head) and the CRC of n - 107 zeros
    zeros_crc = _oracle.shift(0xFFFFFFFF, n - 107) ^ 0xFFFFFFFF
    assert want == _oracle.combine(_oracle.combine(_oracle.crc32(head), zeros_crc, n - 107), _oracle.crc32(tail), 7)
    small = _bytes(63, 2000)
    sbuf = torch.from_numpy(small).to(DEV)
    ptr = _d64(np.array([sbuf.data_ptr(), buf.data_ptr(), sbuf.data_ptr()], dtype=np.uint64))
    size = _d64(np.array([2000, start + n + 5, 2000], dtype=np.uint64))
    off = _d64(np.array([1, start, 1000], dtype=np.uint64))
    length = _d64(np.array([1999, n, 1000], dtype=np.uint64))
    want_all = [_oracle.crc32(small[1:]), want, _oracle.crc32(small[1000:])]
    for k0 in K0S:
        vc.set_file_window_chunk(k0)
        crc, status = wire.file_windows_dev(ptr, size, off, length, n)
        torch.cuda.synchronize()
        assert list(_u32(crc)) == want_all, k0
        assert not status.cpu().numpy().any()


def test_two_calls_share_one_workspace(vc, wire):
    """Back to back on one stream with one d_work whose contents are garbage on entry."""
    vc.set_file_window_chunk(12)
    a = [Win(_bytes(800 + i, 3 * W + i), i, 2 * W + 17 * i) for i in range(9)]
    b = [Win(_bytes(900 + i, 5 * W + i), 2 * i, W + 333 * i) for i in range(9)]
    pa, pb = _place(a), _place(b)
    work = torch.full((wire.file_windows_work_bytes(9) + 24,), 0xA5, dtype=torch.uint8, device=DEV)
    crc_a, st_a = wire.file_windows_dev(*pa[1:], 3 * W, work=work)
    crc_b, st_b = wire.file_windows_dev(*pb[1:], 5 * W, work=work)
    crc_c, _ = wire.file_windows_dev(*pa[1:], 3 * W, work=work)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(crc_a), _want(a, 3 * W)[0]) and np.array_equal(_u32(crc_b), _want(b, 5 * W)[0])
    assert np.array_equal(_u32(crc_c), _u32(crc_a))
    assert not st_a.cpu().numpy().any() and not st_b.cpu().numpy().any()


def test_on_a_side_stream(vc, wire):
    vc.set_file_window_chunk(12)
    wins = [Win(_bytes(1000 + i, 4 * W), i, 3 * W + i) for i in range(5)]
    placed = _place(wins)
    s = torch.cuda.Stream(device=DEV)
    crc, status = wire.file_windows_dev(*placed[1:], 4 * W, stream=s)
    s.synchronize()
    assert np.array_equal(_u32(crc), _want(wins, 4 * W)[0])


def test_status_is_nullable(vc, wire):
    vc.set_file_window_chunk(12)
    data = _bytes(33, 3 * W)
    wins = [Win(data, 1, 2 * W + 1), Win(data, 3 * W, 1), Win(data, 0, 0), Win(data, 5, W)]
    placed = _place(wins)
    crc, status = wire.file_windows_dev(*placed[1:], 3 * W, want_status=False)
    torch.cuda.synchronize()
    assert status is None
    want, st = _want(wins, 3 * W)
    assert np.array_equal(_u32(crc), want) and list(st) == [0, -1, 0, 0] and want[1] == 0
