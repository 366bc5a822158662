"""val_frame_scan_streams_dev (include/val_crc32_gpu.h): the argument checks
answer before any device is touched, so they run without a GPU. The pointers
handed in are made-up addresses that a call which got past its checks would
have to give to the HIP runtime; a refused call never reads them."""
import ctypes
import os
import re

import pytest

import val_protocol_amd.crc as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, MAXF = 3, 10
FAKE = 0x7000_0000_1000  # 8-byte aligned, never dereferenced
NAMES = ["d_base", "d_stream_off", "d_stream_len", "n_streams", "mtu", "max_frames", "d_frame_off", "d_crc_len",
         "d_first", "d_nframes", "d_consumed", "d_status", "d_work", "work_bytes", "stream"]


def _work_bytes(n_streams, max_frames):
    return int(vc.lib().val_frame_scan_work_bytes(n_streams, max_frames))


def _call(**kw):
    a = dict(base=FAKE, stream_off=FAKE + 0x100, stream_len=FAKE + 0x200, n_streams=S, mtu=1024, max_frames=MAXF,
             frame_off=FAKE + 0x300, crc_len=FAKE + 0x400, first=FAKE + 0x500, nframes=None, consumed=None,
             status=None, work=FAKE + 0x800, work_bytes=None, stream=None)
    a.update(kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = _work_bytes(a["n_streams"], a["max_frames"])
    return vc.lib().val_frame_scan_streams_dev(a["base"], a["stream_off"], a["stream_len"], a["n_streams"], a["mtu"],
                                               a["max_frames"], a["frame_off"], a["crc_len"], a["first"], a["nframes"],
                                               a["consumed"], a["status"], a["work"], a["work_bytes"], a["stream"])


def test_symbols_are_exported_and_declared():
    lib = vc.lib()
    for name in ("val_frame_scan_streams_dev", "val_frame_scan_work_bytes"):
        assert hasattr(lib, name) and name in vc.EXPORTS
    f = lib.val_frame_scan_streams_dev
    assert f.restype is ctypes.c_int32 and len(f.argtypes) == 15
    hdr = open(os.path.join(ROOT, "include", "val_crc32_gpu.h")).read()
    m = re.search(r"^val_status_t val_frame_scan_streams_dev\(([^;]*)\);", hdr, re.M)
    assert m, "not declared in include/val_crc32_gpu.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == NAMES
    assert re.search(r"^uint64_t val_frame_scan_work_bytes\(uint32_t n_streams, uint32_t max_frames\);", hdr, re.M)
    assert lib.val_gpu_abi_version() == 1  # adding symbols is compatible
    assert vc.VAL_ERR_PROTOCOL == -5
    import val_protocol_amd.wire as wire

    assert callable(wire.scan_streams_dev) and "scan_streams_dev" in wire.__all__
    assert vc.lib().val_gpu_build_flags() == b""


def test_work_bytes_is_monotone_and_aligned():
    sizes = (0, 1, 2, 3, 7, 64, 65, 300, 65535)
    for s in sizes:
        row = [_work_bytes(s, f) for f in sizes]
        col = [_work_bytes(f, s) for f in sizes]
        assert row == sorted(row) and col == sorted(col), (s, row, col)
        assert all(v % 8 == 0 for v in row + col)
        # room for 12 bytes per descriptor and a count per stream
        assert all(v >= s * f * 12 + 4 * s for v, f in zip(row, sizes))
    assert _work_bytes(0, 0) == 0 and _work_bytes(0, 1000) == 0
    assert _work_bytes(1, 1) == 16 and _work_bytes(3, 10) == 376
    # the largest product the call takes, and one that it refuses: no buffer is that large
    top = _work_bytes(1, 0xFFFFFFFF)
    assert top % 8 == 0 and top >= 0xFFFFFFFF * 12
    over = _work_bytes(0x10000, 0x10000)
    assert over % 8 == 0 and over > top


# what fails -> a word val_gpu_last_error must hold
ANY_N = [("mtu 11", dict(mtu=11), "mtu"),
         ("mtu 0", dict(mtu=0), "mtu"),
         ("work NULL", dict(work=None), "work is NULL"),
         ("work misaligned", dict(work=FAKE + 0x804), "aligned"),
         ("work_bytes one short", dict(work_bytes=S * MAXF * 12 + S * 4 - 1), "work_bytes")]
WITH_FRAMES = [("stream_off", dict(stream_off=None), "stream_off"),
               ("stream_len", dict(stream_len=None), "stream_len"),
               ("frame_off", dict(frame_off=None), "frame_off"),
               ("crc_len", dict(crc_len=None), "crc_len"),
               ("first", dict(first=None), "first"),
               ("base", dict(base=None), "base")]

# no workspace is too small for no streams, so that one case exists at n_streams > 0 only
ANY_N_CASES = [(n, *c) for n in (S, 0) for c in ANY_N if n or "work_bytes" not in c[1]]


@pytest.mark.parametrize("n,what,kw,word", ANY_N_CASES, ids=[f"{c[1]}, n_streams={c[0]}" for c in ANY_N_CASES])
def test_checks_that_hold_at_any_stream_count(n, what, kw, word):
    assert _call(n_streams=n, **kw) == vc.VAL_ERR_INVALID_ARG, what
    assert word in vc.last_error(), (what, vc.last_error())


@pytest.mark.parametrize("what,kw,word", WITH_FRAMES, ids=[c[0] for c in WITH_FRAMES])
def test_null_pointers_with_streams_and_frames(what, kw, word):
    assert _call(**kw) == vc.VAL_ERR_INVALID_ARG, what
    err = vc.last_error()
    assert re.search(rf"\b{word}\b", err) and "NULL" in err, (what, err)
    # exactly this argument is named
    others = {c[0] for c in WITH_FRAMES} - {what}
    assert not any(re.search(rf"\b{o}\b", err) for o in others), err
    # without streams there is nothing to refuse
    assert _call(n_streams=0, **kw) == vc.VAL_OK


def test_product_beyond_32_bits_is_refused():
    for s, f in ((0x10000, 0x10000), (2, 0x80000000), (0xFFFFFFFF, 0xFFFFFFFF)):
        assert _call(n_streams=s, max_frames=f, work_bytes=(1 << 64) - 1) == vc.VAL_ERR_INVALID_ARG
        assert "32 bits" in vc.last_error(), vc.last_error()


def test_no_streams_is_a_no_op_that_clears_the_error():
    assert _call(work=None) == vc.VAL_ERR_INVALID_ARG and vc.last_error()
    assert _call(n_streams=0) == vc.VAL_OK and vc.last_error() == ""
    assert _call(n_streams=0, max_frames=0, work_bytes=0) == vc.VAL_OK
    assert _call(n_streams=0, base=None, stream_off=None, stream_len=None, frame_off=None, crc_len=None,
                 first=None) == vc.VAL_OK
    assert _call(n_streams=0, mtu=12) == vc.VAL_OK


def test_scan_front_setter_takes_its_three_values_only():
    lib = vc.lib()
    for lanes in (64, 1024, 0):
        assert lib.val_gpu_set_scan_front(lanes) == vc.VAL_OK
    for lanes in (1, 63, 128, 256, 2048, 0xFFFFFFFF):
        assert lib.val_gpu_set_scan_front(lanes) == vc.VAL_ERR_INVALID_ARG
        assert "scan front" in vc.last_error()
    vc.set_scan_front(0)
