"""The dynamic-tail queues of k_frames and the payload-state instantiations
beyond one pass of the grid (csrc/crc_kernels.hpp k_frames, k_frames_ragged;
csrc/launch_plan.hpp uniform_one; val_crc32_hip.hip slice_frames).

Every case takes its shape from the device's CU count, asks the planner for
the launches the call will get (vc.plan_frames) and asserts from that plan
that it reaches its branch: the 64-partition queue (qparts 64) with at least
one round of the machine behind the static rounds, the second launch of a
re-cut tail, a ragged launch with more items than waves. A threshold that
moves in launch_plan.hpp then fails the assertion instead of emptying the
test. The plan assertions are plain functions of the CU count (plan_case*),
which tests/test_launch_plan.py runs without a GPU for 64, 128, 256 and 304
CUs.

Expected values come only from tests/_oracle.py. Payload states (the raw
zero-init register of a frame's payload, reference src/val_receiver.c:794,
891) of a million frames are two oracle passes, by linearity:
  state = (crc32(payload) ^ 0xFFFFFFFF) ^ shift(0xFFFFFFFF, len(payload)),
and every test checks 1,000 random frames of that against
update_state(0, payload) directly."""
import numpy as np
import pytest

from tests import _oracle
from tests.test_gpu_unpack import _d8, _d32, _d64
from tests.test_gpu_unpack_files import Files, _expect_files, _same_files

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

KERNEL_RAGGED, KERNEL_FRAMES = 0, 2  # val_gpu_launch_t.kernel
RAGGED_LIMITS, RAGGED_LANES = (1024, 8192, 49152), (2, 4, 8, 16)  # crc_kernels.hpp length classes


# ---- shapes and plans: plain functions of the CU count, no GPU ------------------------------
def waves(cus):
    return cus * 16


def frames_for(cus, lanes, rounds, extra):
    return waves(cus) * (64 // lanes) * rounds + extra


def _queue_plan(vc, cus, n, hint, *, lanes, qparts, depth, launches, descriptors=True, flen=0, want_payload=False):
    """The plan of one call with what every queue case asserts of it."""
    plan = vc.plan_frames(cus, n, hint, descriptors=descriptors, flen=flen, want_payload=want_payload)
    per = 64 // lanes
    assert len(plan) == launches, [l.astuple() for l in plan]
    m = plan[0]
    assert m.kernel == KERNEL_FRAMES and m.lanes == lanes and m.depth == depth, m.astuple()
    assert m.qparts == qparts, m.astuple()
    assert m.grid == cus
    if qparts:
        assert m.static_rounds >= 1
        # at least one round of the whole machine is pulled from the queue
        assert m.count - m.static_rounds * waves(cus) * per >= waves(cus) * per, m.astuple()
    if launches == 2:  # the re-cut tail: the frames past the last full round
        assert plan[1].first == m.count == (n // (waves(cus) * per)) * waves(cus) * per
        assert plan[1].count == n - m.count and plan[1].kernel != KERNEL_RAGGED
    return plan


def plan_case1(vc, cus):
    """2 lanes, ring of three rounds, 64 partitions, a re-cut tail."""
    n = frames_for(cus, 2, 8, 1234)
    return n, _queue_plan(vc, cus, n, 600, lanes=2, qparts=64, depth=-3, launches=2)


def plan_case2(vc, cus):
    """The geometry of case 1 for verify (ring) and for payload states (depth 1: row pay-short)."""
    n = frames_for(cus, 2, 8, 1234)
    plain = _queue_plan(vc, cus, n, 600, lanes=2, qparts=64, depth=-3, launches=2)
    pay = _queue_plan(vc, cus, n, 600, lanes=2, qparts=64, depth=1, launches=2, want_payload=True)
    assert (plain[0].static_rounds, plain[0].count) == (pay[0].static_rounds, pay[0].count)
    return n, pay


def plan_case3(vc, cus):
    """4 lanes: the ring of two rounds, then depth 1 and depth 0 forced, then payload states."""
    n = frames_for(cus, 4, 8, 77)
    plans = {-1: _queue_plan(vc, cus, n, 1100, lanes=4, qparts=64, depth=-2, launches=2)}
    try:
        for depth in (1, 0):
            vc.set_geometry(0, depth)
            plans[depth] = _queue_plan(vc, cus, n, 1100, lanes=4, qparts=64, depth=depth, launches=2)
    finally:
        vc.set_geometry()
    plans["pay"] = _queue_plan(vc, cus, n, 1100, lanes=4, qparts=64, depth=1, launches=2, want_payload=True)
    return n, plans


CASE4_FLEN = 4096


def plan_case4(vc, cus):
    """8 lanes, strided: 47 rounds x 8 x 4,096 B = 1,540,096 B per wave, just over the rule's 1,520,000."""
    n = frames_for(cus, 8, 47, 333)
    return n, _queue_plan(vc, cus, n, CASE4_FLEN, lanes=8, qparts=64, depth=1, launches=2, descriptors=False,
                          flen=CASE4_FLEN)


def plan_case4_stream(vc, cus):
    """Case 4 with the stream loads forced on: the same launches, the first k_frames_stream out of the
    64 partitions behind 24 static rounds, the 333-frame tail at 64 lanes on ordinary loads."""
    n, plan = plan_case4(vc, cus)
    vc.set_stream_loads(1)
    try:
        forced = vc.plan_frames(cus, n, CASE4_FLEN, flen=CASE4_FLEN)
        loads = vc.plan_stream_loads(cus, n, CASE4_FLEN, flen=CASE4_FLEN)
    finally:
        vc.set_stream_loads(-1)
    assert [l.astuple() for l in forced] == [l.astuple() for l in plan]
    assert loads == [True, False], loads
    m = plan[0]
    assert (m.kernel, m.lanes, m.depth, m.qparts, m.static_rounds) == (KERNEL_FRAMES, 8, 1, 64, 24), m.astuple()
    assert (plan[1].lanes, plan[1].count) == (64, 333), plan[1].astuple()
    return n, plan


CASE5_HINT, CASE5_FLEN = 1000, 349


def plan_case5(vc, cus, G):
    """Payload states at G forced lanes: two static rounds and a second launch."""
    n = frames_for(cus, G, 2, 100)
    vc.set_geometry(G)
    try:
        plan = _queue_plan(vc, cus, n, CASE5_HINT, lanes=G, qparts=0, depth=1, launches=2, want_payload=True)
        assert plan[1].first == waves(cus) * (64 // G) * 2
        if G == 4:  # the strided batch
            _queue_plan(vc, cus, n, CASE5_FLEN, lanes=G, qparts=0, depth=1, launches=2, descriptors=False,
                        flen=CASE5_FLEN, want_payload=True)
    finally:
        vc.set_geometry()
    return n, plan


CASE6_N = 120000


def case6_lens():
    rng = np.random.default_rng(77)
    return np.exp(rng.uniform(np.log(40), np.log(20000), CASE6_N)).astype(np.uint32)


def plan_case6(vc, cus):
    """The ragged launch with payload states, more items than waves."""
    lens = case6_lens()
    vc.set_ragged_min_frames(1)
    try:
        plan = vc.plan_frames(cus, CASE6_N, 0, descriptors=True, want_payload=True)
    finally:
        vc.set_ragged_min_frames(-1)
    assert len(plan) == 1 and plan[0].kernel == KERNEL_RAGGED and plan[0].depth == 1, [l.astuple() for l in plan]
    assert plan[0].grid == cus  # the launch's waves are the machine's
    cls = np.searchsorted(np.array(RAGGED_LIMITS), lens, side="right")
    items = sum(-(-int((cls == c).sum()) // (64 // RAGGED_LANES[c])) for c in range(4))
    assert items > waves(cus), (items, waves(cus))
    return lens, plan


CASE7_HINT, CASE7_FILES = 2100, 300


def plan_case7(vc, cus):
    """The verify stage of the unpack call: payload states at 8 lanes, two rounds and a second launch."""
    n = frames_for(cus, 8, 2, 77)
    return n, _queue_plan(vc, cus, n, CASE7_HINT, lanes=8, qparts=0, depth=1, launches=2, want_payload=True)


# ---- the GPU side ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vc():
    import val_protocol_amd.crc as m

    m.init(0)
    m.set_geometry()
    yield m
    m.set_geometry()
    m.set_ragged_min_frames(-1)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _fresh(n, dtype=torch.int32):
    """An output no launch has written: 0xA5 in every byte, so an entry a launch skips cannot hold
    the value an earlier launch left in recycled memory."""
    return torch.full((n,), 0xA5 if dtype == torch.uint8 else -0x5A5A5A5B, dtype=dtype, device=DEV)


def _verify_ex(vc, count, base, **kw):
    ok, nbad, pay = vc.verify_frames_ex(base, out_ok=_fresh(count, torch.uint8), out_pay=_fresh(count), **kw)
    torch.cuda.synchronize()
    return ok.cpu().numpy(), int(nbad.item()), _u32(pay)


def _layout(seed, lens, permute=True):
    """Frames of lens[i] CRC bytes, each followed by room for its trailer and preceded by a gap of
    0..6 bytes (every start alignment), in random device bytes; the descriptors in a random order."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.uint32)
    gaps = rng.integers(0, 7, lens.size)
    wire = lens.astype(np.int64) + 4 + gaps
    offs = (np.cumsum(wire) - wire + gaps).astype(np.uint64)
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.randint(0, 256, (int(wire.sum()) + 16,), dtype=torch.uint8, device=DEV, generator=g)
    if permute:
        perm = rng.permutation(lens.size)
        offs, lens = offs[perm].copy(), lens[perm].copy()
    return buf, offs, lens


def _dev_desc(offs, lens):
    return torch.from_numpy(offs.view(np.int64)).to(DEV), torch.from_numpy(lens.view(np.int32)).to(DEV)


def _put_trailers(host, offs, lens, crc):
    tr = np.ascontiguousarray(crc.astype("<u4")).view(np.uint8).reshape(-1, 4)
    idx = (offs + lens.astype(np.uint64)).astype(np.int64)
    for k in range(4):
        host[idx + k] = tr[:, k]


def _corrupt(host, offs, lens, bad, seed):
    """One bit flipped per frame of `bad`: trailer bytes and frame bytes in turn (an empty frame's trailer)."""
    rng = np.random.default_rng(seed)
    for k, i in enumerate(bad):
        o, L = int(offs[i]), int(lens[i])
        pos = o + L + (k % 4) if (k % 2 == 0 or L == 0) else o + int(rng.integers(0, L))
        host[pos] ^= np.uint8(1 << (k % 8))


def _payload_parts(host, offs, lens):
    """(start, length) of every frame's payload; frames shorter than their prefix have none (-1)."""
    flags = host[(offs + np.uint64(1)).astype(np.int64)]
    pre = np.where((lens >= 8) & ((flags & 1) != 0), 16, 8).astype(np.uint32)
    has = lens >= pre
    plen = np.where(has, lens - pre, 0).astype(np.uint32)
    return offs + np.where(has, pre, 0).astype(np.uint64), plen, has


def _want_states(host, offs, lens, seed=1):
    """Payload states of every frame from two oracle passes, 1,000 of them checked directly."""
    start, plen, has = _payload_parts(host, offs, lens)
    crc = _oracle.frames(host, start, plen, nthreads=16)
    uniq, inv = np.unique(plen, return_inverse=True)
    tab = np.array([_oracle.shift(0xFFFFFFFF, int(u)) for u in uniq], np.uint32)  # once per distinct length
    want = (crc ^ np.uint32(0xFFFFFFFF)) ^ tab[inv.reshape(-1)]
    want[~has] = 0
    for i in np.random.default_rng(seed).integers(0, lens.size, 1000):
        direct = _oracle.update_state(0, host[int(start[i]):int(start[i]) + int(plen[i])]) if has[i] else 0
        assert want[i] == direct, (i, int(lens[i]))
    return want, plen


def _thirds(plan, n, count, seed):
    """`count` frame indices: a third in the static rounds, a third pulled from the queue (or, without
    one, anywhere in the main launch), a third in the second launch."""
    m = plan[0]
    dyn = m.static_rounds * m.grid * 16 * (64 // m.lanes) if m.qparts else m.count // 2
    rng = np.random.default_rng(seed)
    a = count // 3
    tail = n - m.count
    c = min(count - 2 * a, tail)
    lo = min(1000, dyn // 2)  # the first frames stay good: the fold of case 2 runs over them
    bad = np.concatenate([lo + rng.choice(dyn - lo, a, replace=False),
                          dyn + rng.choice(m.count - dyn, count - a - c, replace=False),
                          m.count + rng.choice(tail, c, replace=False)])
    assert np.unique(bad).size == count and (bad >= m.count).sum() == c > 0
    return bad


def test_partitions_two_lanes_ring(vc):
    """Case 1: 600-B frames through descriptors in shuffled order, 8 rounds and 1,234 frames: the last
    4 rounds come from the 64 partitions one group ahead (ring of three rounds), the rest from a second
    launch. CRC and header_crc of every frame, twice on one stream: the second call finds the 64 heads
    and the exit word as the first one's last workgroup left them."""
    n, plan = plan_case1(vc, _cus())
    buf, offs, lens = _layout(101, np.full(n, 600, np.uint32))
    host = buf.cpu().numpy()
    want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
    d_off, d_len = _dev_desc(offs, lens)
    for _ in range(2):
        crc, hdr = _fresh(n), _fresh(n)
        vc.frames(buf, off=d_off, length=d_len, len_hint=600, out_crc=crc, out_hdr=hdr)
        torch.cuda.synchronize()
        assert np.array_equal(_u32(crc), want)
        assert np.array_equal(_u32(hdr), want_h)


def test_partitions_mixed_lengths_verify_and_payload_states(vc):
    """Case 2: the same geometry with lengths 0..1,023 under the hint 600, flags & 1 random (the
    buffer's bytes): empty frames and frames shorter than their prefix in the queue's range and in the
    second launch. TX values; then verify with 97 corrupted frames spread over the static rounds, the
    queue's range and the second launch; then verify_frames_ex (k_frames<2, 1, true> out of the
    partitions): a payload state for every frame, corrupted ones included, and their fold."""
    n, plan = plan_case2(vc, _cus())
    buf, offs, lens = _layout(202, np.random.default_rng(202).integers(0, 1024, n).astype(np.uint32))
    host = buf.cpu().numpy()
    del buf
    want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
    d_off, d_len = _dev_desc(offs, lens)
    _put_trailers(host, offs, lens, want)
    bad = _thirds(plan, n, 97, 7)
    _corrupt(host, offs, lens, bad, 8)
    want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)
    assert want_bad == 97 and not want_ok[bad].any()
    want2, want2_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
    d = torch.from_numpy(host).to(DEV)
    tx, crc, hdr = _fresh(n), _fresh(n), _fresh(n)
    vc.frames(d, off=d_off, length=d_len, len_hint=600, out_crc=tx)
    ok, nbad = vc.verify_frames(d, off=d_off, length=d_len, len_hint=600, out_ok=_fresh(n, torch.uint8), out_crc=crc,
                                out_hdr=hdr)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(tx), want2)
    assert int(nbad.item()) == 97 and np.array_equal(ok.cpu().numpy(), want_ok)
    assert np.array_equal(_u32(crc), want2) and np.array_equal(_u32(hdr), want2_h)
    ok, nbad, got = _verify_ex(vc, n, d, off=d_off, length=d_len, len_hint=600)
    states, plen = _want_states(host, offs, lens)
    miss = np.flatnonzero(got != states)
    assert miss.size == 0, (miss.size, miss[:8], plan[0].astuple())
    assert nbad == 97 and np.array_equal(ok, want_ok)
    # the receiver's fold stops at the first bad frame
    first_bad = int(np.flatnonzero(want_ok == 0)[0])
    state, nf = vc.fold_payload_states(0xFFFFFFFF, got, plen, ok)
    start, _, _ = _payload_parts(host, offs, lens)
    file = np.concatenate([host[int(s):int(s) + int(l)] for s, l in zip(start[:first_bad], plen[:first_bad])])
    assert first_bad >= 1000 and nf == first_bad, (first_bad, nf)
    assert state == _oracle.update_state(0xFFFFFFFF, file)


def test_partitions_four_lanes_every_depth(vc):
    """Case 3: 1,100-B frames, 8 rounds and 77 frames at 4 lanes: the partitions behind the ring of
    two rounds, behind the copy-and-refill loop (depth 1) and without prefetch (depth 0), then payload
    states out of the same queue."""
    n, plans = plan_case3(vc, _cus())
    buf, offs, lens = _layout(303, np.full(n, 1100, np.uint32), permute=False)
    host = buf.cpu().numpy()
    want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
    d_off, d_len = _dev_desc(offs, lens)
    try:
        for depth in (-1, 1, 0):
            vc.set_geometry(0, depth)
            got = vc.plan_frames(_cus(), n, 1100, descriptors=True)
            assert [l.astuple() for l in got] == [l.astuple() for l in plans[depth]]
            crc, hdr = _fresh(n), _fresh(n)
            vc.frames(buf, off=d_off, length=d_len, len_hint=1100, out_crc=crc, out_hdr=hdr)
            torch.cuda.synchronize()
            assert np.array_equal(_u32(crc), want), depth
            assert np.array_equal(_u32(hdr), want_h), depth
    finally:
        vc.set_geometry()
    ok, nbad, pay = _verify_ex(vc, n, buf, off=d_off, length=d_len, len_hint=1100)
    states, _ = _want_states(host, offs, lens)
    want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)  # random trailers: nearly all bad
    assert np.array_equal(pay, states)
    assert nbad == want_bad and np.array_equal(ok, want_ok)


def test_partitions_eight_lanes_strided(vc):
    """Case 4: the smallest launch the bytes-per-wave rule gives the partitions at 8 lanes: 4,096-B
    frames, strided, 47 rounds and 333 frames (6.3 GB at 256 CUs). CRC and header_crc, twice. Then
    once more over the same buffer with the stream loads forced on: k_frames_stream out of the same 64
    partitions (by the rule the path starts at 8,192-B frames, and the shipped launches of that length
    with partitions are as large as this one)."""
    n, plan = plan_case4(vc, _cus())
    flen, stride = CASE4_FLEN, CASE4_FLEN + 4
    g = torch.Generator(device=DEV).manual_seed(404)
    buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=DEV, generator=g)
    host = buf.cpu().numpy()
    want, want_h = _oracle.frames_strided(host, stride, flen, n, header=True, nthreads=16)
    del host
    for _ in range(2):
        crc, hdr = _fresh(n), _fresh(n)
        vc.frames(buf, stride=stride, flen=flen, n=n, out_crc=crc, out_hdr=hdr)
        torch.cuda.synchronize()
        assert np.array_equal(_u32(crc), want)
        assert np.array_equal(_u32(hdr), want_h)
    plan_case4_stream(vc, _cus())
    crc, hdr = _fresh(n), _fresh(n)
    vc.set_stream_loads(1)
    try:
        before = vc.stream_load_launches()
        vc.frames(buf, stride=stride, flen=flen, n=n, out_crc=crc, out_hdr=hdr)
        torch.cuda.synchronize()
        assert vc.stream_load_launches() - before == 1
    finally:
        vc.set_stream_loads(-1)
    assert np.array_equal(_u32(crc), want)
    assert np.array_equal(_u32(hdr), want_h)
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("G", [2, 4, 8, 16, 32])
def test_payload_states_multi_pass_every_lane_count(vc, G):
    """Case 5: k_frames<G, 1, true> looping over two rounds and the second launch of the re-cut tail
    (slice_frames: out_pay + first): lengths 0..2,000, unaligned, trailers from the oracle, 31 frames
    corrupted, some of them in the second launch."""
    n, plan = plan_case5(vc, _cus(), G)
    buf, offs, lens = _layout(500 + G, np.random.default_rng(G).integers(0, 2001, n).astype(np.uint32))
    host = buf.cpu().numpy()
    del buf
    _put_trailers(host, offs, lens, _oracle.frames(host, offs, lens, nthreads=16))
    _corrupt(host, offs, lens, _thirds(plan, n, 31, G), G + 1)
    want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)
    assert want_bad == 31 and (want_ok[plan[1].first:] == 0).sum() >= 10
    states, _ = _want_states(host, offs, lens)
    d = torch.from_numpy(host).to(DEV)
    d_off, d_len = _dev_desc(offs, lens)
    vc.set_geometry(G)
    try:
        ok, nbad, pay = _verify_ex(vc, n, d, off=d_off, length=d_len, len_hint=CASE5_HINT)
    finally:
        vc.set_geometry()
    miss = np.flatnonzero(pay != states)
    assert miss.size == 0, (miss.size, miss[:8], plan[1].first)
    assert nbad == 31 and np.array_equal(ok, want_ok)


def test_payload_states_strided_second_launch(vc):
    """Case 5, strided: 349-B frames at a stride of 354, 4 lanes forced: the second launch starts at
    base + first * stride with the seed of every other frame; the states of all n frames."""
    G, flen, stride = 4, CASE5_FLEN, CASE5_FLEN + 5
    n, plan = plan_case5(vc, _cus(), G)
    g = torch.Generator(device=DEV).manual_seed(549)
    buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=DEV, generator=g)
    host = buf.cpu().numpy()
    rows = host.reshape(n, stride)
    crc = _oracle.frames_strided(host, stride, flen, n, nthreads=16)
    rows[:, flen:flen + 4] = np.ascontiguousarray(crc.astype("<u4")).view(np.uint8).reshape(n, 4)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    lens = np.full(n, flen, np.uint32)
    _corrupt(host, offs, lens, _thirds(plan, n, 31, 5), 6)
    want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)
    assert want_bad == 31
    states, _ = _want_states(host, offs, lens)
    d = torch.from_numpy(host).to(DEV)
    vc.set_geometry(G)
    try:
        ok, nbad, pay = _verify_ex(vc, n, d, stride=stride, flen=flen, n=n)
    finally:
        vc.set_geometry()
    miss = np.flatnonzero(pay != states)
    assert miss.size == 0, (miss.size, miss[:8], plan[1].first)
    assert nbad == 31 and np.array_equal(ok, want_ok)


def test_payload_states_ragged_more_items_than_waves(vc):
    """Case 6: k_frames_ragged<1, true> with more items than waves: every wave hashes its two static
    items and then pulls from its partition's head. 120,000 frames of 40..20,000 B, log-uniform,
    trailers from the oracle, 17 frames corrupted."""
    lens, plan = plan_case6(vc, _cus())
    n = lens.size
    buf, offs, lens = _layout(606, lens, permute=False)
    host = buf.cpu().numpy()
    del buf
    _put_trailers(host, offs, lens, _oracle.frames(host, offs, lens, nthreads=16))
    bad = np.random.default_rng(6).choice(n, 17, replace=False)
    _corrupt(host, offs, lens, bad, 66)
    want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)
    assert want_bad == 17
    states, _ = _want_states(host, offs, lens)
    d = torch.from_numpy(host).to(DEV)
    d_off, d_len = _dev_desc(offs, lens)
    vc.set_ragged_min_frames(1)
    ok, nbad, pay = _verify_ex(vc, n, d, off=d_off, length=d_len, len_hint=0)
    miss = np.flatnonzero(pay != states)
    assert miss.size == 0, (miss.size, miss[:8])
    assert nbad == 17 and np.array_equal(ok, want_ok)


def test_unpack_files_over_a_multi_pass_verify(vc):
    """Case 7: val_frame_unpack_files_dev over a verify stage of two rounds and a second launch at 8
    lanes: 300 files, DATA frames of 1,900..2,084 payload bytes from the host framer, per file in
    order except for about 1% corrupted frames, a few duplicates and a few gaps. The canvas, written,
    the states, the counters, ok and accept against the host rules."""
    import val_protocol_amd.wire as wire

    n, plan = plan_case7(vc, _cus())
    S = CASE7_FILES
    rng = np.random.default_rng(707)
    pay_len = rng.integers(1900, 2085, n).astype(np.uint32)
    inc = (rng.integers(0, 3, n) > 0).astype(np.uint8)
    first = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n), S - 1, replace=False)), [n]]).astype(np.uint32)
    kind = rng.choice(4, n, p=[0.97, 0.01, 0.01, 0.01])  # 0 in order, 1 corrupt, 2 duplicate, 3 gap
    kind[first[:-1]] = 0
    kind[1:][(kind[1:] == 2) & (kind[:-1] != 0)] = 0  # a duplicate repeats the in-order frame in front of it
    inc[kind >= 2] = 1
    file_off = np.zeros(n, np.uint64)
    sizes = []
    for s in range(S):
        lo, hi = int(first[s]), int(first[s + 1])
        k = kind[lo:hi]
        eff = np.where(k == 0, pay_len[lo:hi], 0).astype(np.uint64)  # the others leave `written` where it is
        fo = np.cumsum(eff) - eff
        fo[k == 3] += np.uint64(1000)
        dup = np.flatnonzero(k == 2)
        fo[dup] = fo[dup - 1]
        file_off[lo:hi] = fo
        sizes.append(int(eff.sum()) + 40)
    payload = rng.integers(0, 256, int(pay_len.sum()), dtype=np.uint8)
    pay_off = (np.cumsum(pay_len, dtype=np.uint64) - pay_len).astype(np.uint64)
    stream, off, cl = wire.build_data_batch(payload, pay_off, pay_len, file_off, inc)
    assert int(cl.max()) <= CASE7_HINT
    wire.put_trailers(stream, off, cl, _oracle.frames(stream, off, cl, nthreads=16))
    for i in np.flatnonzero(kind == 1):
        stream[int(off[i]) + int(rng.integers(0, int(cl[i]) + 4))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    assert min((kind == k).sum() for k in (1, 2, 3)) > n // 400
    lay = Files(sizes)
    lay.unpack(wire, _d8(stream), first, _d64(off), _d32(cl), len_hint=CASE7_HINT)
    got = lay.result()
    want = _expect_files(vc, wire, stream, off, cl, first, lay)
    _same_files(got, want)
    assert want["nbad"] == (kind == 1).sum() and 0.9 * n < got["nacc"].sum() < n
    assert got["accept"][plan[1].first:].sum() > 30  # frames of the second verify launch were delivered
