"""The ragged path where its other tests do not reach (DESIGN 4.3;
csrc/crc_kernels.hpp k_bin_count, k_bin_scatter, bin_starts_wave, bucket_slot,
the class table, ragged_item / item_frame and the partitioned one-ahead queue
of k_frames_ragged; val_crc32_hip.hip launch_ragged): later trips of the
binning loop, every bucket, every subset of the classes with partial items,
one-bucket batches at a small and at the full grid between mixed batches on
one stream, a queue several items deep across the class boundaries, both
reservation paths of bucket_slot into one bucket, and verify and payload
states through all of these.

Every shape is a function of the device's CU count (tests/_ragged_shapes.py),
and every case asserts from that restatement and from vc.plan_frames that it
reaches its branch: one ragged launch with the expected grid, and the trips,
items, partitions or waves the case is there for. tests/test_launch_plan.py
makes the same assertions without a GPU for 64, 128, 256 and 304 CUs. Expected
values come from tests/_oracle.py only, over the host copy of the same bytes.
Outputs are pre-filled with 0xA5 bytes and nbad with a sentinel, so a frame
that no item covers cannot show a value from recycled memory."""
import time

import numpy as np
import pytest
import torch

from tests import _oracle
from tests import _ragged_shapes as shapes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NBAD0 = 1000  # *d_nbad is incremented: the sentinel it starts from


@pytest.fixture(scope="module")
def vc():
    import val_protocol_amd.crc as vc

    vc.init(0)
    yield vc
    vc.set_geometry()
    vc.set_ragged_min_frames(-1)
    vc.set_host_chunk_bytes(0)


@pytest.fixture(autouse=True)
def _binned(vc):
    with shapes.binned(vc):
        yield


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _filled(n):
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV).repeat_interleave(4).view(torch.int32)


def _filled8(n):
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)


def _sentinel():
    return torch.full((1,), NBAD0, dtype=torch.int32, device=DEV)


def _random(total, seed):
    """total pseudo-random bytes on the device and their host copy."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    d = torch.randint(0, 256, (total,), dtype=torch.uint8, device=DEV, generator=g)
    return d, d.cpu().numpy()


def _d64(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).to(DEV)


def _d32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _patch(d, host, pos, val):
    """The same bytes into the device buffer and its host copy."""
    pos = np.asarray(pos, dtype=np.int64)
    val = np.asarray(val, dtype=np.uint8)
    assert np.unique(pos).size == pos.size and pos.min() >= 0 and pos.max() < host.size
    host[pos] = val
    d[torch.from_numpy(pos).to(DEV)] = torch.from_numpy(val).to(DEV)


def _store_trailers(d, host, offs, lens, crc):
    """Every frame's LE32 trailer, behind its last byte."""
    end = offs.astype(np.int64) + lens.astype(np.int64)
    pos = (end[:, None] + np.arange(4)).reshape(-1)
    _patch(d, host, pos, crc.astype("<u4").view(np.uint8))


def _flip(d, host, pos, bits):
    pos = np.asarray(pos, dtype=np.int64)
    _patch(d, host, pos, host[pos] ^ (np.uint8(1) << np.asarray(bits, dtype=np.uint8)))


def _flip_frames(d, host, offs, lens, bad):
    """One bit in each frame of `bad`: in its middle byte, in its last byte or in a trailer byte in
    turn (an empty frame: a trailer byte)."""
    pos = []
    for k, f in enumerate(bad):
        L = int(lens[f])
        pos.append(int(offs[f]) + ((L // 2, L - 1, L + k % 4)[k % 3] if L else k % 4))
    _flip(d, host, pos, [k % 8 for k in range(len(pos))])


def _want_states(host, offs, lens):
    """The payload state of every frame, update_state(0, payload): the payload starts behind the 8
    header bytes, or 16 where flags & 1 says the frame carries its offset; a frame shorter than
    that has none (0)."""
    out = np.zeros(lens.size, np.uint32)
    for i in range(lens.size):
        o, L = int(offs[i]), int(lens[i])
        pre = 16 if L >= 8 and host[o + 1] & 1 else 8
        if L >= pre:
            out[i] = _oracle.update_state(0, host[o + pre:o + L])
    return out


def _check_frames(vc, d, host, offs, lens, what="", stream=None):
    """CRC and header_crc of every frame into pre-filled outputs against the oracle; returns the CRCs."""
    n = lens.size
    want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
    d_off, d_len = _d64(offs), _d32(lens)
    crc, hdr = _filled(n), _filled(n)
    vc.frames(d, off=d_off, length=d_len, len_hint=0, out_crc=crc, out_hdr=hdr, stream=stream)
    got, got_h = _u32(crc), _u32(hdr)
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, (what, wrong.size, wrong[:8], lens[wrong[:8]])
    assert np.array_equal(got_h, want_h), what
    return want


def _check_verify(vc, d, host, offs, lens, bad, what="", ex=False):
    """verify (ex: with payload states) with every output given, against the oracle's verdicts over
    the same bytes; returns them."""
    n = lens.size
    want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)
    assert want_bad == len(set(bad)) and set(np.flatnonzero(want_ok == 0)) == set(bad), what
    ok, nbad = _filled8(n), _sentinel()
    if ex:
        pay = _filled(n)
        vc.verify_frames_ex(d, off=_d64(offs), length=_d32(lens), len_hint=0, out_ok=ok, nbad=nbad, out_pay=pay)
        wrong = np.flatnonzero(_u32(pay) != _want_states(host, offs, lens))
        assert wrong.size == 0, (what, wrong[:8], lens[wrong[:8]])
    else:
        vc.verify_frames(d, off=_d64(offs), length=_d32(lens), len_hint=0, out_ok=ok, nbad=nbad)
    assert int(nbad.item()) == NBAD0 + want_bad, what
    assert np.array_equal(ok.cpu().numpy(), want_ok), what
    return want_ok, want_bad


def _check_verify_nullable(vc, d, offs, lens, want_ok, want_bad):
    """verify with d_ok left out, then with d_nbad left out: the C ABI takes NULL for either."""
    lib, d_off, d_len, n = vc.lib(), _d64(offs), _d32(lens), lens.size
    s = torch.cuda.current_stream().cuda_stream
    nbad = _sentinel()
    st = lib.val_crc32_verify_frames_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), 0, 0, n, 0, None,
                                         nbad.data_ptr(), None, None, s)
    assert st == 0, vc.last_error()
    assert int(nbad.item()) == NBAD0 + want_bad
    ok = _filled8(n)
    st = lib.val_crc32_verify_frames_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), 0, 0, n, 0, ok.data_ptr(),
                                         None, None, None, s)
    assert st == 0, vc.last_error()
    assert np.array_equal(ok.cpu().numpy(), want_ok)


# ---- 1. later trips of the binning loop ---------------------------------------------------------
def test_binning_loop_three_trips(vc):
    """4,501,581 frames as views into a 4 MiB pool: 1,024 binning workgroups of 4,397 lengths, so
    for_each_bucket runs three trips in k_bin_count and in k_bin_scatter with a scatter behind
    them; the third is one full row, a row of 45 and the workgroup-uniform break. 99.5% of the
    frames are 0..96 B; frames of classes 1, 2 and 3 are planted in the third trip of workgroup 0
    and of workgroup 1,022 and in the last trip (five rows and one of 122) of the last workgroup,
    which has 3,450 lengths. CRC and header_crc of every frame."""
    lens, plants = shapes.trips_batch()
    n = lens.size
    assert shapes.ragged_plan(vc, _cus(), n) == _cus()
    nbin, chunk, trips = shapes.bin_grid(n)
    assert (nbin, chunk, trips) == (1024, 4397, 3)
    for i in plants:  # every planted frame is past its workgroup's first trip, the first six in a third trip
        lo, hi = shapes.bin_slice(n, i // chunk)
        assert lo <= i < hi and (i - lo) // shapes.BIN_TRIP == (2 if i // chunk < nbin - 1 else 1)
    offs = shapes.views(lens, np.random.default_rng(0x7219), shapes.TRIPS_POOL)
    d, host = _random(shapes.TRIPS_POOL, 0x7219)
    t0 = time.perf_counter()
    _check_frames(vc, d, host, offs, lens)
    print(f"binning trips: {n} frames, {int(lens.astype(np.int64).sum()) >> 20} MiB hashed, call + oracle "
          f"{time.perf_counter() - t0:.2f} s", flush=True)


# ---- 2. every bucket ----------------------------------------------------------------------------
def test_every_bucket(vc):
    """Two frames in each of the 136 buckets at its lowest and highest length (bucket 0: 0 and 128;
    bucket 135: 65,537 and 2^20 + 3) and one of 2^24 + 5, in a seeded permutation at gaps of 0..7
    bytes: every rank of bin_starts_wave's three-ranks-per-lane scan holds two frames, so a rank
    that is off shows as a hole or an overlap in order[]. CRC and header_crc; verify with a bit
    flipped in a frame of every eighth bucket and in the longest; the same through
    verify_frames_ex with payload states."""
    lens, offs, total, bad = shapes.every_bucket_batch()
    assert shapes.ragged_plan(vc, _cus(), lens.size) == 5 == shapes.ragged_plan(vc, _cus(), lens.size, want_payload=True)
    d, host = _random(total, 0xB0C)
    want = _check_frames(vc, d, host, offs, lens)
    _store_trailers(d, host, offs, lens, want)
    _check_verify(vc, d, host, offs, lens, [], "good")
    _flip_frames(d, host, offs, lens, bad)
    _check_verify(vc, d, host, offs, lens, bad, "corrupted")
    _check_verify(vc, d, host, offs, lens, bad, "payload states", ex=True)


# ---- 3. class subsets and partial items ---------------------------------------------------------
@pytest.mark.parametrize("si", range(len(shapes.SUBSETS)), ids=["c" + "".join(map(str, s)) for s in shapes.SUBSETS])
def test_class_subsets_and_partial_items(vc, si):
    """Each non-empty subset of the four classes, every class with 1, per - 1, per, per + 1 or
    3 per + 1 frames (per = 32, 16, 8, 4) at its edge lengths 0, 1, 1,023 | 1,024, 1,025, 8,191 |
    8,192, 8,193, 49,151 | 49,152, 65,536, 65,537, on a grid of at most four workgroups (P < 64).
    CRC and header_crc; verify with a corrupted frame in every class's first item and in its
    partial last item, with d_ok and d_nbad, then with each left out; one subset of each size
    also with payload states."""
    lens, offs, total, tab, bad = shapes.subset_batch(si)
    grid = shapes.ragged_plan(vc, _cus(), lens.size)
    assert shapes.parts(grid) == grid < shapes.QUEUE_PARTS
    d, host = _random(total, 0x5B5 + si)
    want = _check_frames(vc, d, host, offs, lens)
    _store_trailers(d, host, offs, lens, want)
    _flip_frames(d, host, offs, lens, bad)
    want_ok, want_bad = _check_verify(vc, d, host, offs, lens, bad)
    _check_verify_nullable(vc, d, offs, lens, want_ok, want_bad)
    if si in (3, 4, 10, 14):  # {3}, {0, 1}, {0, 1, 2}, all four
        assert [len(shapes.SUBSETS[k]) for k in (3, 4, 10, 14)] == [1, 2, 3, 4]
        shapes.ragged_plan(vc, _cus(), lens.size, want_payload=True)
        _check_verify(vc, d, host, offs, lens, bad, "payload states", ex=True)


# ---- 4. one bucket at a small grid and at the full grid -----------------------------------------
@pytest.mark.parametrize("n,L", shapes.IDENTITY_SMALL)
def test_one_bucket_small_grid(vc, n, L):
    """One-bucket batches (identity order, items dealt to the partitions in runs of four) on grids
    of 1 to 18 workgroups, P = the grid: 1, 1, 2, 4, 32, 35 and 7 items, so the last run of four
    is partial or (4 and 32 items) exactly full."""
    grid, items = shapes.identity_small_facts(_cus(), n, L)
    assert shapes.ragged_plan(vc, _cus(), n) == grid
    lens, offs, total = shapes.identity_batch(n, L, 0x1D + n)
    d, host = _random(total, 0x1D + n)
    _check_frames(vc, d, host, offs, lens)


def test_one_bucket_full_grid_three_items_per_wave(vc):
    """Frames of 100 B in identity order at P = 64 on the full grid: at least three items per wave,
    so every wave's items past its second come from its partition's head in runs of four, and the
    last item is partial."""
    cus = _cus()
    n = shapes.identity_full_n(cus)
    assert shapes.ragged_plan(vc, cus, n) == cus
    lens, offs, total = shapes.identity_batch(n, shapes.IDENTITY_FULL_LEN, 0xF011)
    d, host = _random(total, 0xF011)
    _check_frames(vc, d, host, offs, lens)


def test_one_bucket_between_mixed_batches_on_one_stream(vc):
    """On one side stream, through one scratch: a mixed batch of 4,000 frames, a mixed batch of 900,
    an identity batch of 1,000 and the first batch again. Batches 2 and 3 run while order[] still
    holds batch 1's indices beyond their own n, and the identity batch while order[] holds a
    mixed batch's permutation."""
    cus = _cus()
    n1, n2, n3 = shapes.CHAIN_N
    batches = []
    for k, n in enumerate((n1, n2)):
        lens = shapes.mixed_lens(n, k)
        offs, total = shapes.packed(lens, np.random.default_rng(k))
        batches.append((lens, offs, total))
    batches.append(shapes.identity_batch(n3, 600, 3))
    assert shapes.class_table(batches[2][0])["one_bucket"] and n2 * 4 < n1
    data = [_random(b[2], 0xC4A + k) for k, b in enumerate(batches)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for k in (0, 1, 2, 0):
            lens, offs, _ = batches[k]
            shapes.ragged_plan(vc, cus, lens.size)
            _check_frames(vc, data[k][0], data[k][1], offs, lens, what=f"batch {k}", stream=side)
    side.synchronize()


# ---- 5. a deep queue across class boundaries ----------------------------------------------------
@pytest.fixture(scope="module")
def deep():
    lens, offs, total, tab, bad, chunks = shapes.deep_batch(_cus())
    d, host = _random(total, 0xDEE9)
    want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
    want.setflags(write=False)
    want_h.setflags(write=False)
    return lens, offs, tab, bad, chunks, d, host, want, want_h


def test_deep_queue_across_class_boundaries(vc, deep):
    """Items >= 4 x waves on the full grid (P = 64), every class non-empty, no class's item count a
    multiple of 64: every wave dequeues three times or more, and partitions 0..19 take an item
    of class 3, 2, 1 and 0 in turn. CRC and header_crc, then verify with 1% of the frames
    corrupted, among them frames of every class's first item and of its partial last item."""
    lens, offs, tab, bad, _, d0, host0, want, want_h = deep
    cus, n = _cus(), lens.size
    assert shapes.ragged_plan(vc, cus, n) == cus and tab["total"] >= 4 * shapes.waves(cus)
    d_desc = (_d64(offs), _d32(lens))
    crc, hdr = _filled(n), _filled(n)
    vc.frames(d0, off=d_desc[0], length=d_desc[1], len_hint=0, out_crc=crc, out_hdr=hdr)
    assert np.array_equal(_u32(crc), want)
    assert np.array_equal(_u32(hdr), want_h)
    d, host = d0.clone(), host0.copy()
    _store_trailers(d, host, offs, lens, want)
    _flip_frames(d, host, offs, lens, bad)
    _check_verify(vc, d, host, offs, lens, bad.tolist())


def test_deep_queue_batch_through_host_chunks(vc, deep):
    """The same batch from pageable host memory in chunks of 1 MiB at the default ragged minimum:
    every chunk holds 4,096 frames or more (asserted from the offsets), so the call is one ragged
    launch per chunk, each on d_off + i0 through the same scratch."""
    lens, offs, _, _, chunks, _, host, want, want_h = deep
    cus = _cus()
    vc.set_ragged_min_frames(-1)
    assert vc.ragged_min_frames() == shapes.RAGGED_MIN_DEFAULT
    assert chunks == shapes.host_chunks(offs, lens, shapes.HOST_CHUNK) and len(chunks) >= 8
    for i, j in chunks:
        assert j - i >= shapes.RAGGED_MIN_DEFAULT
        shapes.ragged_plan(vc, cus, j - i)
    vc.set_host_chunk_bytes(shapes.HOST_CHUNK)
    try:
        got, got_h = vc.frames_host(host, offs, lens, header=True)
    finally:
        vc.set_host_chunk_bytes(0)
    assert np.array_equal(got, want)
    assert np.array_equal(got_h, want_h)


# ---- 6. both reservation paths into one bucket --------------------------------------------------
@pytest.mark.parametrize("n", [8192, 8192 - 37])
def test_both_reservation_paths_into_one_bucket(vc, n):
    """Four binning workgroups; in each, bucket 10 gets slots from waves wholly in it (one LDS atomic
    and a popcount rank), from waves with one or two lanes elsewhere and from fully mixed waves
    (one atomic per lane). n = 8,192: slices of 2,048, waves at multiples of 64. n = 8,155:
    slices of 2,039, every workgroup's last wave partial, the last one (54 lanes) wholly in
    bucket 10. Which waves are uniform is asserted from the restatement."""
    lens, uniform = shapes.slot_batch(n)
    nbin, chunk, trips, last = shapes.slot_facts(n)
    assert (nbin, trips) == (4, 1) and (chunk, last) == ((2048, 64) if n == 8192 else (2039, 54))
    assert uniform[-1] and 0 < sum(uniform) < len(uniform)
    shapes.ragged_plan(vc, _cus(), n)
    offs, total = shapes.packed(lens, np.random.default_rng(n))
    d, host = _random(total, 0x5107 + n)
    _check_frames(vc, d, host, offs, lens)
