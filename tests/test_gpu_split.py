"""k_frames_split (small batches of long frames, one workgroup per frame):
bit-exact against the oracle (reference src/val_core.c:150-160, framing
:718-834, RX compare :963-974) for strided and descriptor batches, frames of
one chunk group and of many (the front-to-back group fold), short and empty
frames inside a split batch, unaligned offsets, header_crc, verify with
corruption, and region windows that take the split path (the seed).

Every case asks the planner (vc.plan_frames, for this device's CU count)
which launch its call gets and asserts that it is one k_frames_split launch
with the expected chunk size and grid (tests/_split_shapes.py split_plan);
outputs are pre-filled with 0xA5 bytes. Later trips of the grid loop, the
k0 ladder, the chunk edges, split as a second launch and the fuzz are in
tests/test_gpu_split_edges.py."""
import numpy as np
import pytest
import torch

from tests import _oracle, _prng
from tests import _split_shapes as shapes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def vc():
    import val_protocol_amd.crc as vc

    vc.init(0)
    return vc


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _filled(n):
    """An int32 output of 0xA5 bytes: a frame that a launch skips cannot show an old value."""
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV).repeat_interleave(4).view(torch.int32)


@pytest.mark.parametrize("n,payload", [(1, 8192), (3, 16384), (17, 16384), (256, 65516), (300, 8176), (64, 65520)])
def test_strided_long_frames(vc, n, payload):
    k0 = shapes.STRIDED_K0[payload]
    stream = _prng.frames_stream(n, payload, seed=0x5B + n + payload)
    flen = 16 + payload
    stride = flen + 4
    if (n, payload) == (300, 8176):
        # 8,192-B frames are 3 rounds at one wave per frame, so split takes one trip of the grid only: on 256
        # CUs these 300 frames are a k_frames case (the multi-trip split cases are in test_gpu_split_edges.py)
        assert shapes.rule_says_split(_cus(), n, flen) == (n <= _cus())
        if n <= _cus():
            shapes.split_plan(vc, _cus(), n, flen, k0=k0)
        else:
            shapes.not_split_plan(vc, _cus(), n, flen)
    else:
        shapes.split_plan(vc, _cus(), n, flen, k0=k0)
    d = torch.from_numpy(stream).to(DEV)
    crc, hdr = _filled(n), _filled(n)
    vc.frames(d, stride=stride, flen=flen, n=n, out_crc=crc, out_hdr=hdr)
    want, want_h = _oracle.frames_strided(stream, stride, flen, n, header=True)
    assert np.array_equal(_u32(crc), want)
    assert np.array_equal(_u32(hdr), want_h)


@pytest.mark.parametrize("hint,lo,hi", [(8192, 0, 110_000), (16400, 16000, 16800), (65532, 60000, 65540)])
def test_descriptor_long_frames(vc, hint, lo, hi):
    """Frames longer than 16 chunks of the hint's W fold several groups; short
    and empty frames ride in the same batch. 200 frames, or a grid of a
    smaller device (hint 8,192 admits one trip)."""
    rng = np.random.default_rng(hint)
    n = min(200, _cus())
    k0 = {8192: 10, 16400: 11, 65532: 12}[hint]
    shapes.split_plan(vc, _cus(), n, hint, descriptors=True, k0=k0)
    lens = rng.integers(lo, hi, n).astype(np.uint32)
    lens[:4] = [0, 1, 3, 7]
    wire = lens.astype(np.int64) + 4 + rng.integers(0, 3, n)
    off = np.concatenate([[1], 1 + np.cumsum(wire)[:-1]]).astype(np.uint64)
    buf = _prng.prng_bytes(hint ^ 0x51, int(off[-1]) + int(wire[-1]) + 4)
    d = torch.from_numpy(buf).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_len = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    crc, hdr = _filled(n), _filled(n)
    vc.frames(d, off=d_off, length=d_len, out_crc=crc, out_hdr=hdr, len_hint=hint)
    want, want_h = _oracle.frames(buf, off, lens, header=True)
    assert np.array_equal(_u32(crc), want)
    assert np.array_equal(_u32(hdr), want_h)


def test_verify_long_frames_with_corruption(vc):
    n, payload = 120, 32768
    stream = _prng.frames_stream(n, payload, seed=0x7E)
    flen = 16 + payload
    stride = flen + 4
    shapes.split_plan(vc, _cus(), n, flen, k0=12)
    want = _oracle.frames_strided(stream, stride, flen, n)
    rows = stream.reshape(n, stride)
    rows[:, flen:] = want.astype("<u4").view(np.uint8).reshape(n, 4)
    rng = np.random.default_rng(5)
    bad = rng.choice(n, 9, replace=False)
    for i in bad:
        rows[i, int(rng.integers(0, flen + 4))] ^= 0x10
    d = torch.from_numpy(rows.reshape(-1).copy()).to(DEV)
    ok = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
    ok, nbad = vc.verify_frames(d, stride=stride, flen=flen, n=n, out_ok=ok)
    got = ok.cpu().numpy()
    assert int(nbad.item()) == 9
    assert set(np.nonzero(got == 0)[0]) == set(bad)
    assert set(np.unique(got)) == {0, 1}


@pytest.mark.parametrize("L", [8192, 8191])
def test_region_windows_through_split(vc, L):
    """Windows up to 8 KiB are one frame of the frames path; at 8 KiB that
    frame takes the split kernel, with the caller's state as its seed. One
    byte less is under the rule's 8 KiB floor and takes k_frames."""
    if L == 8192:
        shapes.split_plan(vc, _cus(), 1, L, k0=10)
    else:
        plan = shapes.not_split_plan(vc, _cus(), 1, L)
        assert len(plan) == 1 and plan[0].kernel == vc.KERNEL_FRAMES_C0
    data = _prng.prng_bytes(0xE9 + L, L)
    d = torch.from_numpy(data).to(DEV)
    for st in (0xFFFFFFFF, 0x12345678, 0):
        out = vc.region(d, state_in=st, out=_filled(1))
        assert int(out.item()) & 0xFFFFFFFF == _oracle.update_state(st, data)
