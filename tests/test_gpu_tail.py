"""In-launch tail pieces of the uniform frames kernel (crc_kernels.hpp
tail_pieces, launch_plan.hpp tail_piece_k0): a uniform batch whose frame
groups do not fill the last round of the persistent grid hashes the frames
past the last full round in 1-4 KiB pieces inside the same launch, each
piece's register advanced over the bytes after it and folded into its frame
by device atomics. Bit-exact against the oracle (reference src/val_core.c:
150-160, framing :718-834, RX compare :963-974) with the path on and off,
for strided and descriptor batches, one or several full rounds (with the
dynamic tail), frames of 8-64 KiB at 8 and 16 lanes, a short and an empty
frame among the tail frames, unaligned offsets, header_crc, verify with
corrupted tail frames, and the same batch twice (the accumulators must be
re-zeroed by the launch that used them)."""
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
    vc.set_geometry()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _waves():
    return torch.cuda.get_device_properties(0).multi_processor_count * 16


def _planned_tail(vc, n, typical_len, descriptors=False):
    """Tail frames the planner hashes inside the launch, at this device's CU count."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = vc.plan_frames(cus, n, typical_len, descriptors=descriptors, flen=0 if descriptors else typical_len)
    return [l.tail_n for l in plan]


def _off_run_is_split(vc, n, typical_len, tail, descriptors=False):
    """With the path off the tail frames are a second launch. Whether the planner gives that launch to
    k_frames_split at this device's CU count: asserted equal to the rule restated in
    tests/_split_shapes.py, with the launch's first frame, count, chunk size and grid."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    with shapes.tail_pieces_off(vc):
        plan = vc.plan_frames(cus, n, typical_len, descriptors=descriptors, flen=0 if descriptors else typical_len)
    rows = [l.astuple() for l in plan]
    if len(plan) == 1:  # a tail that would not fit one round at twice the lanes stays in the one launch
        assert plan[0].count == n and plan[0].tail_n == 0 and -(-tail // (32 // plan[0].lanes)) > _waves(), rows
        return False, cus
    assert len(plan) == 2 and plan[1].first == plan[0].count == n - tail and plan[1].count == tail, rows
    split = plan[1].kernel == vc.KERNEL_SPLIT
    assert split == shapes.rule_says_split(cus, tail, typical_len), rows
    if split:
        assert plan[1].k0 == shapes.k0_for(typical_len) and plan[1].grid == min(tail, cus), rows
    return split, cus


def _run_both(vc, fn):
    """fn() with the in-launch tail on, then off; returns both results and
    whether the on-run used the path."""
    lib = vc.lib()
    lib.val_gpu_set_tail_pieces(1)
    before = lib.val_gpu_tail_piece_launches()
    on = fn()
    torch.cuda.synchronize()
    used = lib.val_gpu_tail_piece_launches() - before
    lib.val_gpu_set_tail_pieces(0)
    off = fn()
    torch.cuda.synchronize()
    lib.val_gpu_set_tail_pieces(-1)
    return on, off, used


@pytest.mark.parametrize("flen,rounds,tail", [
    (65532, 1, 6),      # a 1 GiB eighth of the cfg4 file: one round and 6 frames
    (65532, 1, 1024),   # the most tail frames at 16 lanes: 4 KiB pieces (1-2 KiB ones need more groups than waves)
    (65532, 2, 41),
    (16400, 1, 100),    # 8 lanes, 17 pieces of 1 KiB per frame (the front one 16 B)
    (8192, 1, 3),       # the shortest frames that take the path: 8 pieces
    (24580, 4, 777),    # four static rounds in front of the pieces (8 lanes take the dynamic tail from 1.45 MiB per wave)
])
def test_strided_tail_every_frame(vc, flen, rounds, tail):
    G = vc.lanes_per_frame(flen)
    assert G in (8, 16)
    n = _waves() * (64 // G) * rounds + tail
    stride = flen + 4
    g = torch.Generator(device=DEV).manual_seed(flen + tail)
    buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=DEV, generator=g)
    hdr_on = torch.empty(n, dtype=torch.int32, device=DEV)
    hdr_off = torch.empty(n, dtype=torch.int32, device=DEV)
    outs = []

    def fn():
        h = hdr_on if not outs else hdr_off
        outs.append(0)
        return vc.frames(buf, stride=stride, flen=flen, n=n, out_hdr=h).clone()

    on, off, used = _run_both(vc, fn)
    assert used == 1
    assert _planned_tail(vc, n, flen) == [tail]
    # the off-run's second launch: k_frames_split on 256 CUs for every case but the 777 frames of 24,580 B
    # (4 trips x 3 round-times against 7 rounds), which k_frames hashes at 64 lanes
    split, cus = _off_run_is_split(vc, n, flen, tail)
    assert cus != 256 or split == (flen != 24580)
    host = buf.cpu().numpy()
    want, want_h = _oracle.frames_strided(host, stride, flen, n, header=True, nthreads=16)
    assert np.array_equal(_u32(on), want)
    assert np.array_equal(_u32(off), want)
    assert np.array_equal(_u32(hdr_on), want_h) and np.array_equal(_u32(hdr_off), want_h)
    # again, path on: the accumulators were re-zeroed by the first launch
    vc.lib().val_gpu_set_tail_pieces(1)
    again = vc.frames(buf, stride=stride, flen=flen, n=n)
    torch.cuda.synchronize()
    vc.lib().val_gpu_set_tail_pieces(-1)
    assert np.array_equal(_u32(again), want)


@pytest.mark.parametrize("hint,rounds,tail", [(65532, 1, 6), (65532, 8, 41), (16400, 1, 33)])
def test_descriptor_tail_short_and_empty_frames(vc, hint, rounds, tail):
    """Descriptor batches with the uniform length hint, as bench.py's cfg4
    slices: the file's last frame (816 B) and an empty frame among the tail
    frames, frame starts unaligned (odd gaps), one frame longer than the hint
    (its front piece absorbs the excess). The 8-round batch (8 GiB) is the
    suite's case of the one-word dynamic-tail queue, asserted from the plan;
    it also sends payload states through that queue (verify_frames_ex on the
    same buffer, whose trailers are random bytes: nearly every frame is bad,
    and every frame gets its state)."""
    G = vc.lanes_per_frame(hint)
    n = _waves() * (64 // G) * rounds + tail
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = vc.plan_frames(cus, n, hint, descriptors=True)
    assert plan[0].qparts == (1 if rounds == 8 else 0), plan[0].astuple()
    if rounds == 8:
        assert plan[0].static_rounds >= 1 and plan[0].static_rounds < rounds
    rng = np.random.default_rng(hint + tail)
    lens = np.full(n, hint, np.uint32)
    lens[-1] = 816
    lens[-3] = 0
    lens[-2] = hint + 5000
    lens[n - tail] = 7
    gaps = rng.integers(4, 7, n)
    wire = lens.astype(np.int64) + gaps
    offs = np.concatenate([[3], 3 + np.cumsum(wire)[:-1]]).astype(np.uint64)
    total = int(offs[-1]) + int(wire[-1]) + 8
    g = torch.Generator(device=DEV).manual_seed(hint ^ tail)
    buf = torch.randint(0, 256, (total,), dtype=torch.uint8, device=DEV, generator=g)
    d_off = torch.from_numpy(offs.view(np.int64)).to(DEV)
    d_len = torch.from_numpy(lens.view(np.int32)).to(DEV)
    hdr = torch.empty(n, dtype=torch.int32, device=DEV)

    def fn():
        return vc.frames(buf, off=d_off, length=d_len, len_hint=hint, out_hdr=hdr).clone(), hdr.clone()

    (on, hon), (off, hoff), used = _run_both(vc, fn)
    assert used == 1
    assert _planned_tail(vc, n, hint, descriptors=True) == [tail]
    split, _ = _off_run_is_split(vc, n, hint, tail, descriptors=True)  # the off-run's second launch
    assert split or cus != 256
    host = buf.cpu().numpy()
    want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
    assert np.array_equal(_u32(on), want) and np.array_equal(_u32(off), want)
    assert np.array_equal(_u32(hon), want_h) and np.array_equal(_u32(hoff), want_h)
    if rounds != 8:
        return
    # payload states out of the one-word queue (k_frames<16, 1, true>; its last 41 frames from a second launch)
    from tests.test_gpu_dyn_queue import _want_states

    plan = vc.plan_frames(cus, n, hint, descriptors=True, want_payload=True)
    assert len(plan) == 2 and plan[0].qparts == 1 and plan[0].static_rounds >= 1, [l.astuple() for l in plan]
    del on, off, hon, hoff
    pay = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ok, nbad, _ = vc.verify_frames_ex(buf, off=d_off, length=d_len, len_hint=hint, out_pay=pay)
    torch.cuda.synchronize()
    states, _ = _want_states(host, offs, lens)
    want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)
    assert np.array_equal(_u32(pay), states)
    assert int(nbad.item()) == want_bad and np.array_equal(ok.cpu().numpy(), want_ok)


def test_verify_tail_with_corruption(vc):
    """RX verify through the in-launch tail: trailers written from the oracle,
    frames corrupted in the main rounds and among the tail frames (payload
    bytes and trailer bytes): verdicts and the mismatch count."""
    flen, tail = 32784, 57
    G = vc.lanes_per_frame(flen)
    n = _waves() * (64 // G) + tail
    stride = flen + 4
    g = torch.Generator(device=DEV).manual_seed(5)
    buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=DEV, generator=g)
    host = buf.cpu().numpy()
    want = _oracle.frames_strided(host, stride, flen, n, nthreads=16)
    rows = host.reshape(n, stride)
    rows[:, flen:] = want.astype("<u4").view(np.uint8).reshape(n, 4)
    rng = np.random.default_rng(9)
    bad = np.concatenate([rng.choice(n - tail, 20, replace=False), n - tail + rng.choice(tail, 11, replace=False)])
    for k, i in enumerate(bad):
        rows[i, flen + (k % 4) if k % 2 else int(rng.integers(0, flen))] ^= np.uint8(1 << (k % 8))
    d = torch.from_numpy(rows.reshape(-1).copy()).to(DEV)

    def fn():
        ok, nbad = vc.verify_frames(d, stride=stride, flen=flen, n=n)
        return ok.cpu().numpy(), int(nbad.item())

    (ok_on, nb_on), (ok_off, nb_off), used = _run_both(vc, fn)
    assert used == 1
    split, cus = _off_run_is_split(vc, n, flen, tail)  # the off-run verifies the 57 tail frames in k_frames_split
    assert split or cus != 256
    want_ok = np.ones(n, np.uint8)
    want_ok[bad] = 0
    assert nb_on == nb_off == bad.size
    assert np.array_equal(ok_on, want_ok) and np.array_equal(ok_off, want_ok)


def test_forced_lanes_and_the_path_off_for_others(vc):
    """Forced 8 or 16 lanes take the path; 32 lanes and payload states do
    not (their kernels do not carry it) and still hash every frame right."""
    flen, tail = 65532, 9
    stride = flen + 4
    for G, expect in ((8, 1), (16, 1), (32, 0)):
        n = _waves() * (64 // G) + tail
        g = torch.Generator(device=DEV).manual_seed(G)
        buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=DEV, generator=g)
        vc.set_geometry(G)
        try:
            on, off, used = _run_both(vc, lambda: vc.frames(buf, stride=stride, flen=flen, n=n).clone())
        finally:
            vc.set_geometry()
        assert used == expect, G
        want = _oracle.frames_strided(buf.cpu().numpy(), stride, flen, n, nthreads=16)
        assert np.array_equal(_u32(on), want) and np.array_equal(_u32(off), want), G


def test_tail_fuzz(vc):
    """Random uniform batches around the path's edges, each bit-exact against
    the oracle with the path on and off: frame length 8-64 KiB, 1-3 full
    rounds, 1 .. one round minus one tail frames, strided or descriptor
    (unaligned start, one short and one empty frame among the tail frames),
    header_crc, then verify with one corrupted tail frame. TAIL_FUZZ_CASES and
    TAIL_FUZZ_SEED scale and reseed it."""
    import os

    cases = int(os.environ.get("TAIL_FUZZ_CASES", "4"))
    rng = np.random.default_rng(int(os.environ.get("TAIL_FUZZ_SEED", "20261018")))
    used_total = 0
    for c in range(cases):
        flen = int(rng.integers(8192, 65537))
        G = vc.lanes_per_frame(flen)
        assert G in (8, 16), flen
        per_round = _waves() * (64 // G)
        rounds = int(rng.integers(1, 4)) if flen <= 32768 else int(rng.integers(1, 3))
        tail = int(rng.integers(1, per_round))
        n = per_round * rounds + tail
        case = f"case {c}: flen {flen} G {G} rounds {rounds} tail {tail}"
        stride = flen + 4
        g = torch.Generator(device=DEV).manual_seed(int(rng.integers(1 << 62)))
        strided = bool(rng.random() < 0.5)
        case += " strided" if strided else " descriptor"
        if strided:
            buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=DEV, generator=g)
            hdr = torch.empty(n, dtype=torch.int32, device=DEV)

            def fn():
                return vc.frames(buf, stride=stride, flen=flen, n=n, out_hdr=hdr).clone(), hdr.clone()

            host = buf.cpu().numpy()
            want, want_h = _oracle.frames_strided(host, stride, flen, n, header=True, nthreads=16)
            offs = np.arange(n, dtype=np.uint64) * stride
            lens = np.full(n, flen, np.uint32)
        else:
            lens = np.full(n, flen, np.uint32)
            lens[n - 1 - int(rng.integers(0, tail))] = int(rng.integers(1, flen))
            lens[n - 1 - int(rng.integers(0, tail))] = 0
            wire = lens.astype(np.int64) + 4 + rng.integers(0, 3, n)
            first = int(rng.integers(0, 16))
            offs = np.concatenate([[first], first + np.cumsum(wire)[:-1]]).astype(np.uint64)
            buf = torch.randint(0, 256, (int(offs[-1]) + int(wire[-1]) + 8,), dtype=torch.uint8, device=DEV,
                                generator=g)
            d_off = torch.from_numpy(offs.view(np.int64)).to(DEV)
            d_len = torch.from_numpy(lens.view(np.int32)).to(DEV)
            hdr = torch.empty(n, dtype=torch.int32, device=DEV)

            def fn():
                return vc.frames(buf, off=d_off, length=d_len, len_hint=flen, out_hdr=hdr).clone(), hdr.clone()

            host = buf.cpu().numpy()
            want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
        (on, hon), (off_, hoff), used = _run_both(vc, fn)
        used_total += used
        split, _ = _off_run_is_split(vc, n, flen, tail, descriptors=not strided)
        case += " off-run tail on split" if split else " off-run tail on k_frames"
        assert np.array_equal(_u32(on), want) and np.array_equal(_u32(off_), want), case
        assert np.array_equal(_u32(hon), want_h) and np.array_equal(_u32(hoff), want_h), case
        # verify: trailers from the oracle, one tail frame with a flipped bit
        for o, L, w in zip(offs[n - tail:], lens[n - tail:], want[n - tail:]):
            host[int(o) + int(L):int(o) + int(L) + 4] = np.frombuffer(int(w).to_bytes(4, "little"), np.uint8)
        # the main rounds' trailers too, vectorised for the strided layout
        if strided:
            rows = host[:(n - tail) * stride].reshape(n - tail, stride)
            rows[:, flen:] = want[:n - tail].astype("<u4").view(np.uint8).reshape(n - tail, 4)
        else:
            for o, L, w in zip(offs[:n - tail], lens[:n - tail], want[:n - tail]):
                host[int(o) + int(L):int(o) + int(L) + 4] = np.frombuffer(int(w).to_bytes(4, "little"), np.uint8)
        bad = n - tail + int(rng.integers(0, tail))
        host[int(offs[bad]) + int(rng.integers(0, int(lens[bad]) + 4))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        d = torch.from_numpy(host).to(DEV)
        d_off = torch.from_numpy(offs.view(np.int64)).to(DEV)
        d_len = torch.from_numpy(lens.view(np.int32)).to(DEV)

        def vfn():
            ok, nbad = vc.verify_frames(d, off=d_off, length=d_len, len_hint=flen)
            return ok.cpu().numpy(), int(nbad.item())

        (ok_on, nb_on), (ok_off, nb_off), vused = _run_both(vc, vfn)
        used_total += vused
        want_ok = np.ones(n, np.uint8)
        want_ok[bad] = 0
        assert nb_on == nb_off == 1, case + " verify"
        assert np.array_equal(ok_on, want_ok) and np.array_equal(ok_off, want_ok), case + " verify"
        print(f"{case}: tail-piece launches {used}+{vused}", flush=True)
        del buf, d, host
        torch.cuda.empty_cache()
    assert used_total >= 1 or cases < 3  # about half the cases take the path (tails under ~half a round)
