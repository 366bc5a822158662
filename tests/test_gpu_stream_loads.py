"""Stream loads of the uniform frames kernel (crc_kernels.hpp hash_frame_stream,
launch_plan.hpp Planner::stream_loads): rounds >= 1 of long frames read through
non-temporal LDS-DMA beside the compact rotated tables. Bit-exact against the
oracle with the path forced on and forced off; the launch counter must move
exactly when the path is on. The kernels that carry the path hash 8 lanes per
frame, so the small batches here force 8 lanes (a small batch would otherwise
get more lanes per frame and leave the path); 16-lane batches must come out
right with the path forced on and not take it.

Every start and end alignment of a frame occurs: the unit grid of this path is
anchored at floor128(frame end), the bytes before the first whole line and the
up to 127 bytes after the last are read by ordinary loads
(tests/test_stream_grid_model.py proves the geometry on the CPU)."""
import numpy as np
import pytest
import torch

from tests import _oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def vc():
    import val_protocol_amd.crc as vc

    vc.init(0)
    yield vc
    vc.set_stream_loads(-1)
    vc.lib().val_gpu_set_tail_pieces(-1)
    vc.set_geometry()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _round8():
    """Frames in one group round of the device's grid at 8 lanes per frame."""
    return _cus() * 16 * 8


def _on_off(vc, fn, lanes=8, expect=1):
    """fn() with the path forced on, then off, at `lanes` lanes per frame (0: the planner's)."""
    vc.set_geometry(lanes)
    try:
        vc.set_stream_loads(1)
        before = vc.stream_load_launches()
        on = fn()
        torch.cuda.synchronize()
        used = vc.stream_load_launches() - before
        vc.set_stream_loads(0)
        before = vc.stream_load_launches()
        off = fn()
        torch.cuda.synchronize()
        assert vc.stream_load_launches() == before
    finally:
        vc.set_stream_loads(-1)
        vc.set_geometry()
    assert used == expect, used
    return on, off


def _rand(nbytes, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=DEV, generator=g)


@pytest.mark.parametrize("flen", [8192, 8193, 8319, 16400])
@pytest.mark.parametrize("n_of", ["67", "2 rounds + 13"])
def test_strided_every_alignment(vc, flen, n_of):
    n = 67 if n_of == "67" else 2 * _round8() + 13
    stride = flen + 4
    buf = _rand(n * stride, flen + n)
    hdr = torch.empty(n, dtype=torch.int32, device=DEV)
    plan = vc.plan_frames(_cus(), n, flen, flen=flen)
    assert all(l.qparts == 0 for l in plan)  # the dynamic tail is off at these sizes
    on, off = _on_off(vc, lambda: (vc.frames(buf, stride=stride, flen=flen, n=n, out_hdr=hdr).clone(), hdr.clone()))
    want, want_h = _oracle.frames_strided(buf.cpu().numpy(), stride, flen, n, header=True, nthreads=16)
    for crc, h in (on, off):
        assert np.array_equal(_u32(crc), want)
        assert np.array_equal(_u32(h), want_h)


@pytest.mark.parametrize("shift", [1, 4, 64, 127])
def test_base_pointer_offsets_and_short_last_frames(vc, shift):
    flen, n = 16400, 67
    stride = flen + 4
    whole = _rand(n * stride + 128, shift)
    buf = whole[shift:shift + n * stride]
    host = buf.cpu().numpy()
    for last in (flen, 816, 0):
        if last == flen:
            on, off = _on_off(vc, lambda: vc.frames(buf, stride=stride, flen=flen, n=n).clone())
            want = _oracle.frames_strided(host, stride, flen, n, nthreads=16)
            assert np.array_equal(_u32(on), want) and np.array_equal(_u32(off), want)
            continue
        # a short (or empty) last frame: the same batch through descriptors, whose last length differs
        offs = (np.arange(n, dtype=np.uint64) * np.uint64(stride))
        lens = np.full(n, flen, np.uint32)
        lens[-1] = last
        d_off = torch.from_numpy(offs.view(np.int64)).to(DEV)
        d_len = torch.from_numpy(lens.view(np.int32)).to(DEV)
        on, off = _on_off(vc, lambda: vc.frames(buf, off=d_off, length=d_len, len_hint=flen).clone())
        want = _oracle.frames(host, offs, lens, nthreads=16)
        assert np.array_equal(_u32(on), want) and np.array_equal(_u32(off), want)


@pytest.mark.parametrize("flen", [49152, 65532])
def test_sixteen_lane_batches_stay_on_ordinary_loads(vc, flen):
    n, stride = 37, flen + 4
    buf = _rand(n * stride, flen)
    vc.set_stream_loads(1)
    try:
        assert not any(vc.plan_stream_loads(_cus(), n, flen, flen=flen))
        assert not any(vc.plan_stream_loads(_cus(), 4 * _round8(), flen, flen=flen))
    finally:
        vc.set_stream_loads(-1)
    on, off = _on_off(vc, lambda: vc.frames(buf, stride=stride, flen=flen, n=n).clone(), lanes=0, expect=0)
    want = _oracle.frames_strided(buf.cpu().numpy(), stride, flen, n, nthreads=16)
    assert np.array_equal(_u32(on), want) and np.array_equal(_u32(off), want)


def _packed(n, hint, seed):
    """Byte-unaligned packed descriptors with odd frames among them; the first
    frame at offset 0 of the allocation, the last ending at its last byte."""
    rng = np.random.default_rng(seed)
    lens = np.full(n, hint, np.uint32)
    for i, v in zip(rng.choice(np.arange(1, n - 1), 8, replace=False), (0, 3, 130, 2 * hint, hint - 1, hint + 1, 127, 129)):
        lens[i] = v
    gaps = rng.integers(4, 8, n)
    gaps[-1] = 0
    wire = lens.astype(np.int64) + gaps
    offs = np.concatenate([[0], np.cumsum(wire)[:-1]]).astype(np.uint64)
    return offs, lens, int(offs[-1]) + int(lens[-1])


@pytest.mark.parametrize("n_of", ["67", "2 rounds + 13"])
def test_descriptor_batches_with_a_hint(vc, n_of):
    hint = 8319
    n = 67 if n_of == "67" else 2 * _round8() + 13
    offs, lens, total = _packed(n, hint, n)
    buf = _rand(total, n)
    assert buf.numel() == total and int(offs[0]) == 0 and int(offs[-1]) + int(lens[-1]) == total
    d_off = torch.from_numpy(offs.view(np.int64)).to(DEV)
    d_len = torch.from_numpy(lens.view(np.int32)).to(DEV)
    hdr = torch.empty(n, dtype=torch.int32, device=DEV)
    on, off = _on_off(vc, lambda: (vc.frames(buf, off=d_off, length=d_len, len_hint=hint, out_hdr=hdr).clone(), hdr.clone()))
    want, want_h = _oracle.frames(buf.cpu().numpy(), offs, lens, header=True, nthreads=16)
    for crc, h in (on, off):
        assert np.array_equal(_u32(crc), want)
        assert np.array_equal(_u32(h), want_h)


def test_verify_with_corruption_in_every_part_of_a_frame(vc):
    flen, n = 16400, 2 * _round8() + 13
    stride = flen + 4
    host = _rand(n * stride, 11).cpu().numpy()
    rows = host.reshape(n, stride)
    rows[:, flen:] = _oracle.frames_strided(host, stride, flen, n, nthreads=16).astype("<u4").view(np.uint8).reshape(n, 4)
    # frame f starts at 16404 f: first line, a body line, the bytes past the last whole line, the trailer
    bad = {5: 3, n // 2: 8000, n - 2: flen - 1, 33: flen + 2, n - 1: 0}
    for f, at in bad.items():
        rows[f, at] ^= np.uint8(0x40)
    assert (((n - 2) * stride + flen) % 128) > 1  # frame n - 2's last byte lies past its last whole line
    d = torch.from_numpy(host).to(DEV)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    want_ok, want_bad = _oracle.verify_frames(host, offs, np.full(n, flen, np.uint32), nthreads=16)
    assert want_bad == len(bad)

    def fn():
        ok, nbad = vc.verify_frames(d, stride=stride, flen=flen, n=n)
        return ok.cpu().numpy(), int(nbad.item())

    on, off = _on_off(vc, fn)
    for ok, nb in (on, off):
        assert nb == want_bad and np.array_equal(ok, want_ok)


def test_reuse_and_two_streams(vc):
    flen, stride = 8193, 8197
    n1, n2 = 2 * _round8() + 13, _round8() + 5
    buf = _rand(n1 * stride, 21)
    host = buf.cpu().numpy()
    want = _oracle.frames_strided(host, stride, flen, n1, nthreads=16)

    def back_to_back():
        a = vc.frames(buf, stride=stride, flen=flen, n=n1)
        b = vc.frames(buf, stride=stride, flen=flen, n=n2)
        return a.clone(), b.clone()

    vc.set_geometry(8)
    try:
        vc.set_stream_loads(1)
        before = vc.stream_load_launches()
        a, b = back_to_back()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            c = vc.frames(buf, stride=stride, flen=flen, n=n1, stream=s1)
        with torch.cuda.stream(s2):
            d = vc.frames(buf, stride=stride, flen=flen, n=n2, stream=s2)
        torch.cuda.synchronize()
        assert vc.stream_load_launches() - before == 4
    finally:
        vc.set_stream_loads(-1)
        vc.set_geometry()
    assert np.array_equal(_u32(a), want) and np.array_equal(_u32(c), want)
    assert np.array_equal(_u32(b), want[:n2]) and np.array_equal(_u32(d), want[:n2])


@pytest.mark.parametrize("pieces", [1, 0])
def test_tail_pieces_on_and_off_with_the_path_on(vc, pieces):
    flen, stride = 16400, 16404
    n = 2 * _round8() + 13
    buf = _rand(n * stride, 31)
    vc.lib().val_gpu_set_tail_pieces(pieces)
    try:
        before = vc.lib().val_gpu_tail_piece_launches()
        on, off = _on_off(vc, lambda: vc.frames(buf, stride=stride, flen=flen, n=n).clone(), expect=1)  # without pieces the 13 tail frames are a launch at more lanes
        assert vc.lib().val_gpu_tail_piece_launches() - before == 2 * pieces
    finally:
        vc.lib().val_gpu_set_tail_pieces(-1)
    want = _oracle.frames_strided(buf.cpu().numpy(), stride, flen, n, nthreads=16)
    assert np.array_equal(_u32(on), want) and np.array_equal(_u32(off), want)


def test_dynamic_tail_with_the_path_on_by_the_rule(vc):
    """A launch long enough for the one-word dynamic-tail queue (the smaller
    cases above are statically dealt, asserted from their plans): 12 group
    rounds and 13 frames of cfg3's frames, the path by the rule, not forced."""
    flen, stride = 16400, 16404
    n = 12 * _round8() + 13
    plan = vc.plan_frames(_cus(), n, flen, flen=flen)
    assert plan[0].lanes == 8 and plan[0].qparts == 1 and plan[0].tail_n == 13, [l.astuple() for l in plan]
    assert vc.plan_stream_loads(_cus(), n, flen, flen=flen) == [True]
    buf = _rand(n * stride, 41)
    before = vc.stream_load_launches()
    on = vc.frames(buf, stride=stride, flen=flen, n=n).clone()
    torch.cuda.synchronize()
    assert vc.stream_load_launches() - before == 1
    vc.set_stream_loads(0)
    try:
        off = vc.frames(buf, stride=stride, flen=flen, n=n).clone()
        torch.cuda.synchronize()
    finally:
        vc.set_stream_loads(-1)
    want = _oracle.frames_strided(buf.cpu().numpy(), stride, flen, n, nthreads=16)
    assert np.array_equal(_u32(on), want) and np.array_equal(_u32(off), want)
