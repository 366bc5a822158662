"""val_frame_unpack_files_dev: one window that holds frames of many files,
delivered in one device call (include/val_crc32_gpu.h; per file the ordering
decision of the reference's receive loop, src/val_receiver.c:871-895).

All files of a test live in ONE canvas filled with 0xA5, with guard bytes
between them, and the whole canvas is compared afterwards: a byte written into
a neighbouring file or a gap fails the test. Expected results never come from
the device path: the oracle's verdicts over all frames, then per file
val_frame_data_offsets / val_frame_payload_lens / val_frame_accept over that
file's frames and a numpy scatter; the state is
val_crc32_fold_payload_states_at over the oracle's payload states, and the
oracle's CRC of the delivered bytes is checked as well."""
import numpy as np
import pytest

from tests import _oracle, _prng
from tests.test_gpu_unpack import (CANARY, CTRL, DEV, File, Window, _built, _d8, _d32, _d64, _frame, _in_order,
                                   vc, wire)  # noqa: F401 - vc and wire are fixtures

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


class Files:
    """S device files in one 0xA5 canvas: file s at canvas[pos[s] : pos[s] + size[s]], `guard` or more
    bytes before, between and after them, pos[s] % 4 == phase[s] when given."""

    def __init__(self, sizes, written=None, state=None, caps=None, phase=None, guard=29):
        S = len(sizes)
        pos, p = [], guard
        for s, sz in enumerate(sizes):
            if phase is not None:
                p += (int(phase[s]) - p) % 4
            pos.append(p)
            p += int(sz) + guard
        self.S, self.total = S, p
        self.pos = np.array(pos, dtype=np.uint64)
        self.sizes = np.array(sizes, dtype=np.uint64)
        self.caps = self.sizes.copy() if caps is None else np.array(caps, dtype=np.uint64)
        assert (self.caps <= self.sizes).all()  # no capacity reaches into a guard
        self.w0 = np.zeros(S, np.uint64) if written is None else np.array(written, dtype=np.uint64)
        self.s0 = np.full(S, 0xFFFFFFFF, np.uint32) if state is None else np.array(state, dtype=np.uint32)
        self.canvas = torch.full((p,), CANARY, dtype=torch.uint8, device=DEV)
        assert self.canvas.data_ptr() % 4 == 0
        self.ptr = _d64(self.pos + np.uint64(self.canvas.data_ptr()))
        self.cap = _d64(self.caps)
        self.written = _d64(self.w0)
        self.state = _d32(self.s0)
        self.nacc, self.novf, self.fnbad = (torch.zeros(S, dtype=torch.int32, device=DEV) for _ in range(3))
        self.nbad = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ok, self.accept = [], []

    def unpack(self, wire, base, first, off, length, *, with_state=True, **kw):
        ok, acc, *_ = wire.unpack_data_files_dev(base, first=_d32(first), file_ptr=self.ptr, file_cap=self.cap,
                                                 written=self.written, off=off, length=length,
                                                 file_state=self.state if with_state else None, naccepted=self.nacc,
                                                 noverflow=self.novf, file_nbad=self.fnbad, nbad=self.nbad, **kw)
        self.ok.append(ok)
        self.accept.append(acc)

    def result(self):
        torch.cuda.synchronize()
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        return dict(canvas=self.canvas.cpu().numpy(), written=self.written.cpu().numpy().view(np.uint64),
                    state=u32(self.state), ok=np.concatenate([t.cpu().numpy() for t in self.ok]),
                    accept=np.concatenate([t.cpu().numpy() for t in self.accept]), nbad=int(self.nbad.item()),
                    nacc=u32(self.nacc), novf=u32(self.novf), fnbad=u32(self.fnbad))


def _segments(first, n):
    first = [int(x) for x in first]
    return [(min(a, n), min(max(a, b), n)) for a, b in zip(first[:-1], first[1:])]


def _expect_files(vc, wire, stream, off, length, first, lay, prev=None):
    """What S receivers' loops leave, each over its own frames: from `lay`'s starting values, or
    continuing the result `prev` of an earlier window."""
    off, length = np.asarray(off, dtype=np.uint64), np.asarray(length, dtype=np.uint32)
    n = off.size
    if n:
        ok, nbad = _oracle.verify_frames(stream, off, length, nthreads=8)
        fo = wire.data_offsets(stream, off, length)
        pl = wire.payload_lens(stream, off, length)
    else:
        ok, nbad, fo, pl = np.zeros(0, np.uint8), 0, np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    src = off + (length - pl)
    w = dict(canvas=np.full(lay.total, CANARY, np.uint8), written=lay.w0.copy(), state=lay.s0.copy(), nbad=0,
             nacc=np.zeros(lay.S, np.uint32), novf=np.zeros(lay.S, np.uint32), fnbad=np.zeros(lay.S, np.uint32),
             ok=np.zeros(0, np.uint8), accept=np.zeros(0, np.uint8))
    if prev is not None:
        w = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in prev.items()}
    accept = np.zeros(n, np.uint8)
    for s, (lo, hi) in enumerate(_segments(first, n)):
        if lo >= hi:
            continue
        W0, st0, cap, at = int(w["written"][s]), int(w["state"][s]), int(lay.caps[s]), int(lay.pos[s])
        assert cap <= int(lay.sizes[s])
        dst, W, nacc, novf = wire.frame_accept(fo[lo:hi], pl[lo:hi], W0, cap, ok[lo:hi])
        acc = dst != wire.NOT_ACCEPTED
        pay = np.zeros(hi - lo, np.uint32)
        for k in np.flatnonzero(acc):
            p = stream[int(src[lo + k]):int(src[lo + k]) + int(pl[lo + k])]
            w["canvas"][at + int(dst[k]):at + int(dst[k]) + p.size] = p
            pay[k] = _oracle.update_state(0, p)
        st, W2, nf = vc.fold_payload_states_at(st0, pay, pl[lo:hi], fo[lo:hi], W0, (ok[lo:hi] != 0) & acc)
        assert (W2, nf) == (W, nacc)
        if W0 <= W <= cap:  # the accepted payloads are the file bytes [W0, W), in order
            assert st == _oracle.update_state(st0, w["canvas"][at + W0:at + W])
        accept[lo:hi] = acc
        w["written"][s], w["state"][s] = W, st
        w["nacc"][s] += nacc
        w["novf"][s] += novf
        w["fnbad"][s] += int((ok[lo:hi] == 0).sum())
    w["nbad"] += int(nbad)
    w["ok"] = np.concatenate([w["ok"], ok.astype(np.uint8)])
    w["accept"] = np.concatenate([w["accept"], accept])
    return w


def _same_files(got, want, state=True):
    assert got["nbad"] == want["nbad"], (got["nbad"], want["nbad"])
    for k in ("written", "nacc", "novf", "fnbad", "ok", "accept") + (("state",) if state else ()):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
    bad = np.flatnonzero(got["canvas"] != want["canvas"])
    assert bad.size == 0, (bad.size, bad[:8])


def _run(vc, wire, win, first, lay, *, len_hint=0, with_state=True):
    lay.unpack(wire, _d8(win.stream), first, _d64(win.off), _d32(win.len), len_hint=len_hint, with_state=with_state)
    got = lay.result()
    want = _expect_files(vc, wire, win.stream, win.off, win.len, first, lay)
    _same_files(got, want, state=with_state)
    if not with_state:
        assert np.array_equal(got["state"], lay.s0)
    return got


def _small_frames(wire, n, start, gap_at=(), corrupt_at=(), seed=5, fixed=None):
    """n small frames in order from `start`; frames in gap_at announce an offset 1000 bytes ahead
    (and are skipped), frames in corrupt_at fail their CRC. -> frames, where `written` ends."""
    rng = np.random.default_rng(seed)
    pay_len = rng.integers(0, 24, n).astype(np.uint32) if fixed is None else np.full(n, fixed, np.uint32)
    inc = (rng.integers(0, 3, n) > 0).astype(np.uint8) if fixed is None else np.ones(n, np.uint8)
    skip = np.zeros(n, dtype=bool)
    skip[list(gap_at)] = True
    skip[list(corrupt_at)] = True
    inc[list(gap_at)] = 1
    eff = np.where(skip, 0, pay_len).astype(np.uint64)
    file_off = start + np.cumsum(eff) - eff
    file_off[list(gap_at)] += 1000
    frames, _ = _built(wire, pay_len, file_off, inc, seed)
    for i in corrupt_at:
        frames[i] = frames[i].copy()
        frames[i][9] ^= 0x01
    return frames, start + int(eff.sum())


# ---- 1. one file: the single-file call ----------------------------------------------------
def test_one_file_equals_the_single_file_call(vc, wire):
    """The go-back-N window of test_gpu_unpack.test_ordering_in_one_batch through both entry points."""
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
    lay = Files([size], written=[3], state=[0x1234ABCD])
    got = _run(vc, wire, win, [0, win.n], lay)
    one = File(size, 3, 0x1234ABCD)
    one.unpack(wire, _d8(win.stream), _d64(win.off), _d32(win.len))
    ref = one.result()
    at = int(lay.pos[0])
    assert np.array_equal(got["canvas"][at:at + size], ref["file"])  # (_run compared the bytes around the file)
    assert (int(got["written"][0]), int(got["state"][0])) == (ref["written"], ref["state"])
    assert np.array_equal(got["ok"], ref["ok"]) and np.array_equal(got["accept"], ref["accept"])
    assert (got["nbad"], int(got["nacc"][0]), int(got["novf"][0])) == (ref["nbad"], ref["nacc"], ref["novf"])
    assert int(got["fnbad"][0]) == ref["nbad"] == 1
    assert got["accept"].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1]


# ---- 2. three files, three histories --------------------------------------------------------
def test_three_files_with_different_histories(vc, wire):
    """One 40-frame window three times over: a receiver at 0, one a frame in, one past the window."""
    rng = np.random.default_rng(202)
    pay_len = rng.integers(1, 200, 40).astype(np.uint32)
    pay_len[16] = 120
    pos = _in_order(pay_len)
    inc = (np.arange(40) % 3 != 2).astype(np.uint8)  # frames 0 and 1 explicit
    frames, _ = _built(wire, pay_len, pos, inc, seed=202)
    frames[17] = frames[17].copy()
    frames[17][11] ^= 0x20
    total = int(pay_len.sum())
    past = total + 1000
    w0 = [0, int(pay_len[0]), past]
    sizes = [total + 40, total + 11, past + 150 + 64]
    caps = [total + 40, int(pos[17]) - 5, past + 150]  # file 1 ends inside frame 16, file 2 takes 150 bytes
    # where file 0 will stand after its segment: an explicit frame there would be in order for it
    ok = np.ones(40, np.uint8)
    ok[17] = 0
    fo = np.where(inc != 0, pos, wire.OFFSET_IMPLIED).astype(np.uint64)
    _, end0, _, _ = wire.frame_accept(fo, pay_len, 0, caps[0], ok)
    assert end0 not in (w0[1], w0[2]) and end0 + 9 <= caps[0]
    bait = _frame(wire, rng.integers(0, 256, 9, dtype=np.uint8), end0)
    win = Window(frames + frames + [bait] + frames)
    first = [0, 40, 81, 121]
    lay = Files(sizes, written=w0, state=[0xFFFFFFFF, 0x00C0FFEE, 0x5EED5EED], caps=caps)
    got = _run(vc, wire, win, first, lay)
    assert got["written"][0] == end0 and got["accept"][80] == 0  # the bait stayed out of file 0 (and of file 1)
    acc = [got["accept"][a:b] for a, b in zip(first[:-1], first[1:])]
    assert acc[0][:17].all() and not acc[0][17]
    assert not acc[1][0] and acc[1][1:16].all() and not acc[1][16]  # frame 0 is a duplicate one frame in; 16 does not fit
    assert got["written"][1] < end0  # so the bait is a gap for the file that owns it
    assert not acc[2][inc != 0].any() and acc[2][inc == 0].any()  # past the window only implied frames can land
    assert got["fnbad"].tolist() == [1, 1, 1] and got["nbad"] == 3
    assert got["nacc"].tolist() == [int(a.sum()) for a in acc] and len({a.tobytes() for a in (x[:40] for x in acc)}) == 3
    assert got["novf"][0] == 0 and got["novf"][1] > 0 and got["novf"][2] > 0


# ---- 3. segment edges -----------------------------------------------------------------------
def test_segment_edges(vc, wire):
    """Empty files first, in the middle and last, a one-frame file, a 2,500-frame file whose breaks
    sit on either side of the order pass's chunk boundary, a decreasing pair, frames that no file owns."""
    one, end_one = _small_frames(wire, 1, 7, seed=1, fixed=33)
    big, end_big = _small_frames(wire, 2500, 2, gap_at=[1023, 1024], seed=5)
    five, end_five = _small_frames(wire, 5, 0, corrupt_at=[2], seed=9, fixed=40)
    loose, _ = _small_frames(wire, 7, 0, corrupt_at=[3], seed=11, fixed=40)  # in order for a file at 0; nobody's
    win = Window(one + big + five + loose)
    n = win.n
    first = [0, 0, 1, 1, 2501, 2506, 2503, 2503]  # files 0, 2, 5 (decreasing) and 6 are empty
    assert first[-1] < n == 2513 and _segments(first, n) == [(0, 0), (0, 1), (1, 1), (1, 2501), (2501, 2506),
                                                            (2506, 2506), (2503, 2503)]
    w0 = [0, 7, 5, 2, 0, 0, 0]
    sizes = [64, end_one + 9, 64, end_big + 40, end_five + 13, 300, 300]
    state = [1, 2, 3, 0xFFFFFFFF, 5, 6, 7]
    lay = Files(sizes, written=w0, state=state)
    got = _run(vc, wire, win, first, lay, len_hint=24)
    assert got["written"].tolist() == [0, end_one, 5, end_big, end_five, 0, 0]
    assert got["state"][[0, 2, 5, 6]].tolist() == [1, 3, 6, 7]
    assert got["nacc"].tolist() == [0, 1, 0, 2498, 4, 0, 0] and got["fnbad"].tolist() == [0, 0, 0, 0, 1, 0, 0]
    assert got["ok"][2506:].tolist() == [1, 1, 1, 0, 1, 1, 1] and not got["accept"][2506:].any() and got["nbad"] == 2
    # bounds past n are clamped: the same window with the last file claiming frames up to 2^32 - 1
    lay2 = Files(sizes, written=w0, state=state)
    got2 = _run(vc, wire, win, [0, 0, 1, 1, 2501, 2506, 2506, 0xFFFFFFFF], lay2, len_hint=24)
    assert got2["nacc"].tolist() == [0, 1, 0, 2498, 4, 0, 6] and got2["fnbad"][6] == 1 and got2["written"][6] == 240


# ---- 4. more files than workgroups ----------------------------------------------------------
def test_more_files_than_workgroups(vc, wire):
    """3,000 files of 1..5 explicit 40-byte frames: every order workgroup takes several files, one
    after the other, and what it keeps for one file (written, state, counters, the chunk loaded
    ahead, the ballot slots) must not reach the next. Then the same call without states."""
    S = 3000
    grid = min(S, torch.cuda.get_device_properties(0).multi_processor_count)
    rng = np.random.default_rng(4)
    cnt = rng.integers(1, 6, S)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    n = int(first[-1])
    kind = rng.integers(0, 4, n)  # 0, 1: in order; 2: a gap; 3: corrupt
    w0 = rng.integers(0, 50, S).astype(np.uint64)
    file_off = np.zeros(n, np.uint64)
    for s in range(S):
        w = int(w0[s])
        for i in range(int(first[s]), int(first[s + 1])):
            file_off[i] = w + (1000 if kind[i] == 2 else 0)
            if kind[i] < 2:
                w += 40
    pattern = [(int(cnt[s]), tuple(np.maximum(kind[first[s]:first[s + 1]], 1))) for s in range(S)]
    differ = sum(pattern[s] != pattern[s + grid] for s in range(S - grid))
    assert S > 2 * grid and differ > (S - grid) // 2  # neighbours in one workgroup's stride mostly differ
    frames, _ = _built(wire, np.full(n, 40, np.uint32), file_off, np.ones(n, np.uint8), seed=4)
    for i in np.flatnonzero(kind == 3):
        frames[i] = frames[i].copy()
        frames[i][20] ^= 0x08
    win = Window(frames)
    state = rng.integers(0, 1 << 32, S, dtype=np.uint64).astype(np.uint32)
    sizes = w0 + 200 + 7
    caps = w0 + 40 * rng.integers(1, 6, S).astype(np.uint64)  # some files overflow
    lay = Files(sizes, written=w0, state=state, caps=caps, guard=5)
    got = _run(vc, wire, win, first, lay, len_hint=56)
    assert got["novf"].sum() > 100 and got["fnbad"].sum() == (kind == 3).sum() == got["nbad"]
    assert 0 < got["nacc"].sum() < n
    lay = Files(sizes, written=w0, state=state, caps=caps, guard=5)
    _run(vc, wire, win, first, lay, len_hint=56, with_state=False)


# ---- 5. alignment ---------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 8, 64])
def test_alignment(vc, wire, lanes):
    """File s begins at an address of phase s mod 4; every frame under test arrives when `written`
    is a multiple of 4 (a 1..3-byte frame in front of it sees to that), from every source phase."""
    lengths = (0, 1, 63, 64, 65, 140)
    frames, phase, first, sizes = [], [], [0], []
    for s in range(4):
        pay_len, ph, w = [], [], 0
        for L in lengths:
            for sp in range(4):
                if w % 4:
                    pay_len.append(4 - w % 4)
                    ph.append((sp + 2) % 4)
                    w += pay_len[-1]
                pay_len.append(L)
                ph.append(sp)
                w += L
        inc = (np.arange(len(pay_len)) % 3 == 0).astype(np.uint8)
        f, _ = _built(wire, pay_len, _in_order(pay_len), inc, seed=10 * lanes + s)
        frames += f
        phase += ph
        first.append(len(frames))
        sizes.append(w + 3)
    win = Window(frames, phase)
    lay = Files(sizes, phase=[0, 1, 2, 3], guard=13)
    assert ((lay.pos + np.uint64(lay.canvas.data_ptr())) % 4).tolist() == [0, 1, 2, 3]
    vc.set_lanes_per_frame(lanes)
    try:
        got = _run(vc, wire, win, first, lay)
    finally:
        vc.set_lanes_per_frame(0)
    assert got["accept"].all() and got["written"].tolist() == [sz - 3 for sz in sizes]


# ---- 6. capacity per file -------------------------------------------------------------------
def test_capacity_per_file(vc, wire):
    """A cap that ends inside, at the end of and one byte short of a frame, one file each."""
    pay_len = [100] * 6 + [100, 100, 10, 100]
    inc = [1, 0, 1, 0, 1, 0, 1, 0, 0, 1]
    frames, _ = _built(wire, pay_len, _in_order(pay_len, 1), inc)
    win = Window(frames * 3)
    lay = Files([1200, 1200, 1200], written=[1, 1, 1], caps=[1 + 650, 1 + 700, 1 + 699])
    got = _run(vc, wire, win, [0, 10, 20, 30], lay)
    assert got["accept"].tolist() == [1] * 6 + [0, 0, 1, 0] + [1] * 7 + [0, 0, 0] + [1] * 6 + [0, 0, 1, 0]
    assert got["novf"].tolist() == [2, 2, 2] and got["written"].tolist() == [611, 701, 611]


# ---- 7. strided mode and the ragged verify path ---------------------------------------------
def test_strided_mode_two_files(vc, wire):
    n, pl, stride, cut = 300, 1004, 1031, 130  # an odd stride: every source phase
    a, _ = _built(wire, [pl] * cut, _in_order([pl] * cut), np.ones(cut, np.uint8), seed=1)
    b, _ = _built(wire, [pl] * (n - cut), _in_order([pl] * (n - cut), 5), np.ones(n - cut, np.uint8), seed=2)
    frames = a + b
    frames[57] = frames[57].copy()
    frames[57][500] ^= 0x04
    flen = 16 + pl
    stream = _prng.prng_bytes(3, n * stride + 8)
    for i, f in enumerate(frames):
        stream[i * stride:i * stride + f.size] = f
    lay = Files([cut * pl + 19, 5 + (n - cut) * pl + 6], written=[0, 5])
    first = [0, cut, n]
    lay.unpack(wire, _d8(stream), first, None, None, stride=stride, flen=flen, n=n)
    got = lay.result()
    off = np.arange(n, dtype=np.uint64) * stride
    _same_files(got, _expect_files(vc, wire, stream, off, np.full(n, flen, np.uint32), first, lay))
    assert got["nacc"].tolist() == [57, n - cut] and got["fnbad"].tolist() == [1, 0]


def test_ragged_verify_path_two_files(vc, wire):
    """len_hint = 0 with the device-binned verify path pinned on."""
    n, cut = 700, 333
    rng = np.random.default_rng(12)
    pay_len = rng.choice([0, 1, 9, 64, 100, 700, 1012, 4000, 16376], n).astype(np.uint32)
    inc = rng.integers(0, 2, n).astype(np.uint8)
    inc[cut] = 1
    file_off = np.concatenate([_in_order(pay_len[:cut]), _in_order(pay_len[cut:], 9)])
    frames, _ = _built(wire, pay_len, file_off, inc)
    frames[400] = frames[400].copy()
    frames[400][3] ^= 0x40
    win = Window(frames)
    lay = Files([int(pay_len[:cut].sum()) + 40, 9 + int(pay_len[cut:].sum()) + 40], written=[0, 9])
    vc.set_ragged_min_frames(1)
    try:
        got = _run(vc, wire, win, [0, cut, n], lay, len_hint=0)
    finally:
        vc.set_ragged_min_frames(-1)
    assert got["accept"][:400].all() and not got["accept"][400] and got["fnbad"].tolist() == [0, 1]


# ---- 8. streams and chaining ----------------------------------------------------------------
def test_two_calls_on_a_side_stream_chain(vc, wire):
    """Two windows back to back on a side stream, nothing between them: the second continues every
    file's written and state; the counters accumulate."""
    parts, ends = [], []
    for s, (nf, gaps, bad) in enumerate([(300, [100], [250]), (1, [], []), (500, [20, 400], [450])]):
        f, end = _small_frames(wire, nf, 2 + s, gap_at=gaps, corrupt_at=bad, seed=21 + s)
        parts.append(f)
        ends.append(end)
    cuts = [140, 1, 260]  # file 1 has nothing in the second window
    w1 = Window(parts[0][:cuts[0]] + parts[1][:cuts[1]] + parts[2][:cuts[2]])
    w2 = Window(parts[0][cuts[0]:] + parts[1][cuts[1]:] + parts[2][cuts[2]:], front=3)
    f1 = [0, 140, 141, 401]
    f2 = [0, 160, 160, 400]
    lay = Files([e + 30 for e in ends], written=[2, 3, 4], state=[0xFFFFFFFF, 77, 0xDEADBEEF])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    b1, o1, l1 = _d8(w1.stream), _d64(w1.off), _d32(w1.len)
    b2, o2, l2 = _d8(w2.stream), _d64(w2.off), _d32(w2.len)
    torch.cuda.synchronize()
    lay.unpack(wire, b1, f1, o1, l1, len_hint=24, stream=side)
    lay.unpack(wire, b2, f2, o2, l2, len_hint=24, stream=side)
    side.synchronize()
    got = lay.result()
    want = _expect_files(vc, wire, w1.stream, w1.off, w1.len, f1, lay)
    want = _expect_files(vc, wire, w2.stream, w2.off, w2.len, f2, lay, prev=want)
    _same_files(got, want)
    assert got["written"].tolist() == ends and got["fnbad"].tolist() == [1, 0, 1] and got["nbad"] == 2
    assert got["nacc"].tolist() == [298, 1, 497]


# ---- 9. descriptor order --------------------------------------------------------------------
def test_descriptors_grouped_frames_interleaved(vc, wire):
    """Two files' frames alternate in memory (and file 1's lie there backwards); only the descriptors are grouped."""
    a, end_a = _small_frames(wire, 200, 0, gap_at=[50], seed=3)
    b, end_b = _small_frames(wire, 200, 6, corrupt_at=[120], seed=4)
    mixed = [f for pair in zip(a, reversed(b)) for f in pair]
    win = Window(mixed)
    order = np.concatenate([np.arange(0, 400, 2), np.arange(399, 0, -2)])
    win.off, win.len = win.off[order], win.len[order]
    lay = Files([end_a + 20, end_b + 20], written=[0, 6])
    got = _run(vc, wire, win, [0, 200, 400], lay, len_hint=24)
    assert got["written"].tolist() == [end_a, end_b] and got["nacc"].tolist() == [199, 199]
