"""k_frames_split where tests/test_gpu_split.py does not reach (DESIGN 4.4,
csrc/crc_kernels.hpp k_frames_split, csrc/launch_plan.hpp use_split / split,
val_crc32_hip.hip slice_frames): later trips of the grid-stride loop (what a
workgroup carries from one frame into its next), chunks of 8 KiB to 16 MiB,
the deterministic chunk and group edges, split as the second launch of a
uniform batch, verify through all of these, and a seeded fuzz.

Every shape is a function of the device's CU count (tests/_split_shapes.py),
and every case asserts from vc.plan_frames for that count that its call is a
k_frames_split launch with the expected chunk size, grid and first frame;
tests/test_launch_plan.py makes the same assertions without a GPU for 64,
128, 256 and 304 CUs. Expected values come from tests/_oracle.py only:
stored trailers are the oracle's, and the verdicts of a corrupted batch are
the oracle's over the same bytes. Outputs are pre-filled with 0xA5 bytes, so
a frame that a launch skips cannot show a value from recycled memory."""
import time

import numpy as np
import pytest
import torch

from tests import _oracle
from tests import _split_shapes as shapes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def vc():
    import val_protocol_amd.crc as vc

    vc.init(0)
    yield vc
    vc.lib().val_gpu_set_tail_pieces(-1)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _filled(n):
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV).repeat_interleave(4).view(torch.int32)


def _filled8(n):
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)


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


def _check_verify(vc, d, host, offs, lens, bad_frames, *, hint=0, stride=0, flen=0, what=""):
    """verify with both outputs against the oracle's verdicts over the same bytes; returns them."""
    n = lens.size
    want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)
    assert want_bad == len(set(bad_frames)) and set(np.nonzero(want_ok == 0)[0]) == set(bad_frames), what
    ok = _filled8(n)
    if stride:
        _, nbad = vc.verify_frames(d, stride=stride, flen=flen, n=n, out_ok=ok)
    else:
        _, nbad = vc.verify_frames(d, off=_d64(offs), length=_d32(lens), len_hint=hint, out_ok=ok)
    assert int(nbad.item()) == want_bad, what
    assert np.array_equal(ok.cpu().numpy(), want_ok), what
    return want_ok, want_bad


# ---- 1. later trips of the grid loop --------------------------------------------------------
def test_three_trips_strided(vc):
    """2 CUs + 3 frames of 32,784 B on a grid of one workgroup per CU: every workgroup hashes three
    frames (the last three workgroups' third), CRC and header_crc."""
    n, _ = shapes.trips_plan(vc, _cus(), descriptors=False)
    flen, stride = shapes.TRIPS_FLEN, shapes.TRIPS_FLEN + 4
    d, host = _random(n * stride + 8, 0x7B1)
    crc, hdr = _filled(n), _filled(n)
    vc.frames(d, stride=stride, flen=flen, n=n, out_crc=crc, out_hdr=hdr)
    want, want_h = _oracle.frames_strided(host, stride, flen, n, header=True, nthreads=16)
    assert np.array_equal(_u32(crc), want)
    assert np.array_equal(_u32(hdr), want_h)


@pytest.fixture(scope="module")
def trips_batch():
    """The descriptor batch of the three-trip cases, its bytes and the oracle's CRCs, computed once."""
    lens, offs, total = shapes.trips_descriptors(_cus())
    d, host = _random(total, 0x7B2)
    want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
    want.setflags(write=False)
    want_h.setflags(write=False)
    return lens, offs, d, host, want, want_h


def test_three_trips_descriptors(vc, trips_batch):
    """Frames of 0, 1 and 7 bytes, of exactly one group, one group and a byte, four groups and random
    lengths up to five hints, in a permuted order: a workgroup's second and third frame follow
    frames of every other kind (workgroup 0: four groups, one byte, four groups)."""
    lens, offs, d, _, want, want_h = trips_batch
    n, _ = shapes.trips_plan(vc, _cus(), descriptors=True)
    assert n == lens.size
    crc, hdr = _filled(n), _filled(n)
    vc.frames(d, off=_d64(offs), length=_d32(lens), len_hint=shapes.TRIPS_FLEN, out_crc=crc, out_hdr=hdr)
    assert np.array_equal(_u32(crc), want)
    assert np.array_equal(_u32(hdr), want_h)


def test_three_trips_verify(vc, trips_batch):
    """The same batch with the oracle's trailers and about 5% of the frames corrupted, in every trip:
    a flipped bit in the first byte, in the last chunk, in each trailer byte and in the first group
    of a frame of several groups (that bit reaches the result through the group fold). With d_ok and
    d_nbad, then with each left out: the C ABI takes NULL for either (frames_dev checks neither;
    the kernel tests both pointers)."""
    lens, offs, d0, host0, want, _ = trips_batch
    cus, n, hint = _cus(), lens.size, shapes.TRIPS_FLEN
    shapes.trips_plan(vc, cus, descriptors=True)
    d, host = d0.clone(), host0.copy()
    _store_trailers(d, host, offs, lens, want)
    _check_verify(vc, d, host, offs, lens, [], hint=hint, what="no corruption")
    bad = shapes.trips_bad(cus, lens)
    pos = [int(offs[f]) + shapes.bad_position(kind, int(lens[f]), shapes.TRIPS_K0) for f, kind in bad]
    _flip(d, host, pos, [i % 8 for i in range(len(bad))])
    want_ok, want_bad = _check_verify(vc, d, host, offs, lens, [f for f, _ in bad], hint=hint, what="corrupted")
    # each nullable output left out
    lib, d_off, d_len = vc.lib(), _d64(offs), _d32(lens)
    nbad = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = lib.val_crc32_verify_frames_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), 0, 0, n, hint, None,
                                         nbad.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream)
    assert st == 0, vc.last_error()
    assert int(nbad.item()) == want_bad
    ok = _filled8(n)
    st = lib.val_crc32_verify_frames_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), 0, 0, n, hint,
                                         ok.data_ptr(), None, None, None, torch.cuda.current_stream().cuda_stream)
    assert st == 0, vc.last_error()
    assert np.array_equal(ok.cpu().numpy(), want_ok)


# ---- 2. the k0 ladder and the chunk edges ---------------------------------------------------
@pytest.mark.parametrize("i", range(len(shapes.LADDER)), ids=[f"{f}-k{k}" for f, k in shapes.LADDER])
def test_k0_ladder_strided(vc, i):
    """Three strided frames at each side of 16 << k0 < flen, chunks of 1 KiB to 2 MiB (k0 10..21);
    the strides put the frame ends at every address mod 4. The last frame is verified too, good and
    with a bit flipped in its first byte."""
    flen, stride = shapes.ladder_plan(vc, _cus(), i)
    n = shapes.LADDER_N
    d, host = _random(n * stride + 8, 0x1ADD + i)
    crc, hdr = _filled(n), _filled(n)
    vc.frames(d, stride=stride, flen=flen, n=n, out_crc=crc, out_hdr=hdr)
    want, want_h = _oracle.frames_strided(host, stride, flen, n, header=True, nthreads=16)
    assert np.array_equal(_u32(crc), want)
    assert np.array_equal(_u32(hdr), want_h)
    offs, lens = np.arange(n, dtype=np.uint64) * np.uint64(stride), np.full(n, flen, np.uint32)
    _store_trailers(d, host, offs, lens, want)
    _check_verify(vc, d, host, offs, lens, [], stride=stride, flen=flen)
    _flip(d, host, [int(offs[n - 1])], [3])
    _check_verify(vc, d, host, offs, lens, [n - 1], stride=stride, flen=flen)


@pytest.mark.parametrize("hint,k0", shapes.EDGE_HINTS)
def test_chunk_and_group_edges(vc, hint, k0):
    """L = m W + r for m in 0, 1, 15, 16, 17, 31, 32, 33, 48 and r in 0, 1, 3, 4, 63, 64, 65, W - 1,
    each at start addresses 0..3 mod 4: C = 16, 17, 32, 33 chunks, front chunks of 1, 3, 4, W - 1
    and W bytes, and (m = 16, r = 1) a first group of one one-byte chunk and 15 padded waves. Hint
    8,192 (W = 1 KiB) admits one trip of the grid, so the 288 frames go in slices of at most a
    grid, each asserted to plan as split; hint 100,000 (W = 8 KiB) takes them in one call."""
    lens, offs, total = shapes.edge_descriptors(k0)
    calls = shapes.edge_calls(vc, _cus(), hint, k0)
    assert sum(b - a for a, b in calls) == lens.size == 288
    d, host = _random(total, 0xED6E + k0)
    want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
    n = lens.size
    crc, hdr = _filled(n), _filled(n)
    d_off, d_len = _d64(offs), _d32(lens)
    for a, b in calls:
        vc.frames(d, off=d_off[a:b], length=d_len[a:b], len_hint=hint, out_crc=crc[a:b], out_hdr=hdr[a:b])
    got, got_h = _u32(crc), _u32(hdr)
    wrong = np.nonzero(got != want)[0]
    assert wrong.size == 0, [(int(lens[f]) >> k0, int(lens[f]) & ((1 << k0) - 1), int(offs[f]) % 4) for f in wrong[:8]]
    assert np.array_equal(got_h, want_h)
    # verify: good, then a bit flipped in the front chunk of every frame of more than 16 chunks that has one
    _store_trailers(d, host, offs, lens, want)
    bad = [f for f in range(0, n, 3) if shapes.groups(int(lens[f]), k0) > 1][:40]
    _flip(d, host, [int(offs[f]) for f in bad], [f % 8 for f in bad])
    want_ok, _ = _oracle.verify_frames(host, offs, lens, nthreads=16)
    assert set(np.nonzero(want_ok == 0)[0]) == set(bad)
    ok = _filled8(n)
    nbad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for a, b in calls:
        vc.verify_frames(d, off=d_off[a:b], length=d_len[a:b], len_hint=hint, out_ok=ok[a:b], nbad=nbad)
    assert int(nbad.item()) == len(bad)
    assert np.array_equal(ok.cpu().numpy(), want_ok)


def test_one_frame_of_256_mib(vc):
    """One frame of 2^28 + 5 bytes at offset 3 under the hint 2^28: chunks of 16 MiB, two groups (the
    first one 5-byte chunk and 15 padded waves), the group fold advances 2^28 bytes. CRC,
    header_crc and verify, good and with a bit flipped in the 5-byte front chunk. One workgroup
    reads the whole frame: the call's time is printed."""
    shapes.big_plan(vc, _cus())
    L, off, hint = shapes.BIG_LEN, shapes.BIG_OFF, 1 << 28
    d, host = _random(off + L + 12, 0xB16)
    offs, lens = np.array([off], np.uint64), np.array([L], np.uint32)
    d_off, d_len = _d64(offs), _d32(lens)
    crc, hdr = _filled(1), _filled(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vc.frames(d, off=d_off, length=d_len, len_hint=hint, out_crc=crc, out_hdr=hdr)
    torch.cuda.synchronize()
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    want, want_h = _oracle.frames(host, offs, lens, header=True)
    print(f"2^28 + 5 bytes in one workgroup: {t_gpu * 1e3:.1f} ms; oracle {time.perf_counter() - t0:.2f} s", flush=True)
    assert np.array_equal(_u32(crc), want)
    assert np.array_equal(_u32(hdr), want_h)
    _store_trailers(d, host, offs, lens, want)
    ok, nbad = vc.verify_frames(d, off=d_off, length=d_len, len_hint=hint, out_ok=_filled8(1))
    assert (int(ok.item()), int(nbad.item())) == (1, 0)
    d[off + 2] ^= 0x40  # CRC-32 detects every single-bit error
    ok, nbad = vc.verify_frames(d, off=d_off, length=d_len, len_hint=hint, out_ok=_filled8(1))
    assert (int(ok.item()), int(nbad.item())) == (0, 1)


# ---- 3. split as the second launch ----------------------------------------------------------
@pytest.mark.parametrize("descriptors", [False, True], ids=["strided", "descriptors"])
@pytest.mark.parametrize("two_trips", [False, True], ids=["tail6", "tail-cus+5"])
def test_split_is_the_second_launch(vc, two_trips, descriptors):
    """One full wave-round of 65,532-B frames and a tail of 6, or of CUs + 5 (two trips of the split
    grid), with the in-launch tail pieces off: launch 2 is k_frames_split over slice_frames' part of
    the batch (descriptors, base and every output pointer shifted, the seed of a later frame). CRC
    and header_crc of every frame, then verify with two corrupted frames in the main part and
    three in the tail."""
    cus = _cus()
    tail = shapes.tail_counts(cus)[two_trips]
    flen, stride, hint = shapes.TAIL_FLEN, 0, 0
    with shapes.tail_pieces_off(vc):
        n, _ = shapes.tail_plan(vc, cus, tail, descriptors)
        if descriptors:
            lens, offs, total = shapes.tail_descriptors(cus, tail)
            hint = flen
        else:
            stride = flen + 4
            lens, offs, total = np.full(n, flen, np.uint32), np.arange(n, dtype=np.uint64) * np.uint64(stride), n * stride + 8
        d, host = _random(total, 0x7A11 + tail)
        crc, hdr = _filled(n), _filled(n)
        if descriptors:
            d_off, d_len = _d64(offs), _d32(lens)
            vc.frames(d, off=d_off, length=d_len, len_hint=hint, out_crc=crc, out_hdr=hdr)
        else:
            vc.frames(d, stride=stride, flen=flen, n=n, out_crc=crc, out_hdr=hdr)
        want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
        assert np.array_equal(_u32(crc), want)
        assert np.array_equal(_u32(hdr), want_h)
        _store_trailers(d, host, offs, lens, want)
        bad = shapes.tail_bad(cus, tail)
        assert sum(f >= shapes.tail_main(cus) for f in bad) == 3 and len(set(bad)) == 5
        # a payload byte, the last byte, a trailer byte: whatever the frame's length allows
        pos = [int(offs[f]) + (0, int(lens[f]) - 1, int(lens[f]) + 2)[i % 3 if lens[f] else 2] for i, f in enumerate(bad)]
        _flip(d, host, pos, [i % 8 for i in range(len(bad))])
        _check_verify(vc, d, host, offs, lens, bad, hint=hint, stride=stride, flen=flen)


# ---- 4. the seeded fuzz ---------------------------------------------------------------------
def test_split_fuzz(vc):
    """FUZZ_SPLIT_ROUNDS (60) small batches of long frames, every one on k_frames_split by the plan
    (tests/_split_shapes.py fuzz_rounds): strided or descriptors, 1 .. 3 CUs frames, a hint or flen
    of 8 KiB .. 2 MiB weighted towards powers of two +- 1, descriptor lengths of 0 .. 4 hints at
    gaps of 4-7 bytes, at most 64 MiB per round; CRC and header_crc, or verify with none to four
    flipped bits. FUZZ_SEED reseeds it. At the default rounds it asserts what the rounds reached."""
    cus, seed = _cus(), shapes.fuzz_seed()
    rounds = shapes.fuzz_rounds(vc, cus)
    on_split = 0
    for r, c in enumerate(rounds):
        n, typical, lens, offs = c["n"], c["typical"], c["lens"], c["offs"]
        case = (f"seed {seed} round {r}: {'descriptors' if c['descriptors'] else 'strided'} n={n} len={typical} "
                f"k0={c['k0']} trips={c['trips']} verify={c['verify']} bad={c['bad']}")
        plan = shapes.split_plan(vc, cus, n, typical, descriptors=c["descriptors"], k0=c["k0"])
        on_split += plan[0].kernel == vc.KERNEL_SPLIT
        d, host = _random(c["total"], seed + r)
        want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
        kw = dict(off=_d64(offs), length=_d32(lens), len_hint=typical) if c["descriptors"] else \
            dict(stride=c["stride"], flen=typical, n=n)
        if not c["verify"]:
            crc, hdr = _filled(n), _filled(n)
            vc.frames(d, out_crc=crc, out_hdr=hdr, **kw)
            assert np.array_equal(_u32(crc), want), case
            assert np.array_equal(_u32(hdr), want_h), case
            continue
        _store_trailers(d, host, offs, lens, want)
        if c["bad"]:
            _flip(d, host, [int(offs[f]) + p for f, p, _ in c["bad"]], [b for _, _, b in c["bad"]])
        want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)
        assert set(np.nonzero(want_ok == 0)[0]) == set(f for f, _, _ in c["bad"]), case
        ok, nbad = vc.verify_frames(d, out_ok=_filled8(n), **kw)
        assert int(nbad.item()) == want_bad, case
        assert np.array_equal(ok.cpu().numpy(), want_ok), case
    assert on_split == len(rounds)  # a round is never skipped, and every round ran on split
    print(f"split fuzz: {len(rounds)} rounds, k0 {sorted(set(c['k0'] for c in rounds))}, trips "
          f"{sorted(set(c['trips'] for c in rounds))}, {sum(c['total'] for c in rounds) >> 20} MiB", flush=True)
    if len(rounds) >= shapes.FUZZ_DEFAULT_ROUNDS:
        shapes.fuzz_coverage(rounds)
