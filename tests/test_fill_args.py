"""val_frame_fill_files_dev (include/val_crc32_gpu.h): the argument checks
answer before any device is touched, so they run without a GPU. The pointers
handed in are made-up addresses that a call which got past its checks would
have to give to the HIP runtime; a refused call never reads them."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import val_protocol_amd.crc as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, MAXF = 3, 10
FAKE = 0x7000_0000_1000  # 8-byte aligned, never dereferenced
NAMES = ["d_payload", "d_file_pos", "d_file_size", "d_next", "d_last_acked", "d_budget", "n_files", "mtu",
         "max_frames", "d_out", "d_stream_off", "d_stream_cap", "d_stream_len", "d_nframes", "d_first", "d_frame_off",
         "d_crc_len", "d_crc", "d_hdr", "d_work", "work_bytes", "stream"]
REQUIRED = ["payload", "file_pos", "file_size", "next", "last_acked", "out", "stream_off", "stream_cap", "first",
            "frame_off"]


def _work_bytes(n_files, max_frames):
    return int(vc.lib().val_frame_fill_work_bytes(n_files, max_frames))


def _call(**kw):
    a = dict(payload=FAKE, file_pos=FAKE + 0x100, file_size=FAKE + 0x200, next=FAKE + 0x300, last_acked=FAKE + 0x400,
             budget=None, n_files=S, mtu=1024, max_frames=MAXF, out=FAKE + 0x10000, stream_off=FAKE + 0x500,
             stream_cap=FAKE + 0x600, stream_len=None, nframes=None, first=FAKE + 0x700, frame_off=FAKE + 0x800,
             crc_len=None, crc=None, hdr=None, work=FAKE + 0x1000, work_bytes=None, stream=None)
    a.update(kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = _work_bytes(a["n_files"], a["max_frames"])
    return vc.lib().val_frame_fill_files_dev(a["payload"], a["file_pos"], a["file_size"], a["next"], a["last_acked"],
                                             a["budget"], a["n_files"], a["mtu"], a["max_frames"], a["out"],
                                             a["stream_off"], a["stream_cap"], a["stream_len"], a["nframes"],
                                             a["first"], a["frame_off"], a["crc_len"], a["crc"], a["hdr"], a["work"],
                                             a["work_bytes"], a["stream"])


def test_symbols_are_exported_and_declared():
    lib = vc.lib()
    for name in ("val_frame_fill_files_dev", "val_frame_fill_work_bytes", "val_frame_fill_window"):
        assert hasattr(lib, name) and name in vc.EXPORTS
    f = lib.val_frame_fill_files_dev
    assert f.restype is ctypes.c_int32 and len(f.argtypes) == 22
    hdr = open(os.path.join(ROOT, "include", "val_crc32_gpu.h")).read()
    m = re.search(r"^val_status_t val_frame_fill_files_dev\(([^;]*)\);", hdr, re.M)
    assert m, "not declared in include/val_crc32_gpu.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == NAMES
    assert re.search(r"^uint64_t val_frame_fill_work_bytes\(uint32_t n_files, uint32_t max_frames\);", hdr, re.M)
    assert lib.val_gpu_abi_version() == 1  # adding symbols is compatible
    import val_protocol_amd.wire as wire

    assert callable(wire.fill_files_dev) and "fill_files_dev" in wire.__all__
    assert wire.fill_work_bytes(S, MAXF) == _work_bytes(S, MAXF)
    assert vc.lib().val_gpu_build_flags() == b""


def test_work_bytes_is_monotone_and_aligned():
    sizes = (0, 1, 2, 3, 7, 64, 65, 300, 65535)
    for s in sizes:
        row = [_work_bytes(s, f) for f in sizes]
        col = [_work_bytes(f, s) for f in sizes]
        assert row == sorted(row) and col == sorted(col), (s, row, col)
        assert all(v % 8 == 0 for v in row + col)
        # room for the framer's inputs of every slot (u64, u64, u32, u8), a position and a count per transfer
        assert all(v >= s * f * 21 + 12 * s for v, f in zip(row, sizes))
    assert _work_bytes(0, 0) == 0 and _work_bytes(0, 1000) == 0
    assert _work_bytes(1, 1) == 40 and _work_bytes(3, 10) == 672
    # the largest product the call takes, and one that it refuses: no buffer is that large
    top = _work_bytes(1, 0xFFFFFFFF)
    assert top % 8 == 0 and top >= 0xFFFFFFFF * 21
    over = _work_bytes(0x10000, 0x10000)
    assert over % 8 == 0 and over > top


# what fails -> a word val_gpu_last_error must hold
ANY_N = [("mtu 20", dict(mtu=20), "mtu below 21"),
         ("mtu 0", dict(mtu=0), "mtu below 21"),
         ("mtu 65548", dict(mtu=65548), "mtu above 65547"),
         ("mtu 2^32 + 1024", dict(mtu=(1 << 32) + 1024), "mtu above 65547"),
         ("work NULL", dict(work=None), "work is NULL"),
         ("work misaligned", dict(work=FAKE + 0x1004), "aligned"),
         ("work_bytes one short", dict(work_bytes=S * MAXF * 21 + S * 12 - 1), "work_bytes")]
# no workspace is too small for no transfers, so that one case exists at n_files > 0 only
ANY_N_CASES = [(n, *c) for n in (S, 0) for c in ANY_N if n or "work_bytes" not in c[1]]


@pytest.mark.parametrize("n,what,kw,word", ANY_N_CASES, ids=[f"{c[1]}, n_files={c[0]}" for c in ANY_N_CASES])
def test_checks_that_hold_at_any_transfer_count(n, what, kw, word):
    assert _call(n_files=n, **kw) == vc.VAL_ERR_INVALID_ARG, what
    assert word in vc.last_error(), (what, vc.last_error())


@pytest.mark.parametrize("what", REQUIRED)
def test_null_pointers_with_transfers_and_frames(what):
    assert _call(**{what: None}) == vc.VAL_ERR_INVALID_ARG, what
    err = vc.last_error()
    assert re.search(rf"\b{what}\b", err) and "NULL" in err, (what, err)
    # exactly this argument is named
    assert not any(re.search(rf"\b{o}\b", err) for o in set(REQUIRED) - {what}), err
    # without transfers there is nothing to refuse
    assert _call(n_files=0, **{what: None}) == vc.VAL_OK


def test_mtu_bounds_are_the_rules():
    """21 and 65547 pass the mtu check (the next check, a NULL workspace, answers instead)."""
    for mtu in (21, 65547):
        assert _call(mtu=mtu, work=None) == vc.VAL_ERR_INVALID_ARG and "work is NULL" in vc.last_error()
        assert _call(mtu=mtu, n_files=0) == vc.VAL_OK


def test_product_beyond_32_bits_is_refused():
    for s, f in ((0x10000, 0x10000), (2, 0x80000000), (0xFFFFFFFF, 0xFFFFFFFF)):
        assert _call(n_files=s, max_frames=f, work_bytes=(1 << 64) - 1) == vc.VAL_ERR_INVALID_ARG
        assert "32 bits" in vc.last_error(), vc.last_error()


def test_no_transfers_is_a_no_op_that_clears_the_error():
    assert _call(work=None) == vc.VAL_ERR_INVALID_ARG and vc.last_error()
    assert _call(n_files=0) == vc.VAL_OK and vc.last_error() == ""
    assert _call(n_files=0, max_frames=0, work_bytes=0) == vc.VAL_OK
    assert _call(n_files=0, **{k: None for k in REQUIRED}) == vc.VAL_OK


_NO_DEVICE = r"""
import sys
import val_protocol_amd.crc as vc
FAKE = 0x7000_0000_1000
lib = vc.lib()
wb = int(lib.val_frame_fill_work_bytes(3, 10))
def call(n_files, work):
    return lib.val_frame_fill_files_dev(FAKE, FAKE + 0x100, FAKE + 0x200, FAKE + 0x300, FAKE + 0x400, None, n_files,
                                        1024, 10, FAKE + 0x10000, FAKE + 0x500, FAKE + 0x600, None, None, FAKE + 0x700,
                                        FAKE + 0x800, None, None, None, work, wb, None)
assert call(3, None) == vc.VAL_ERR_INVALID_ARG
assert call(0, FAKE + 0x1000) == vc.VAL_OK
assert lib.val_gpu_current_device() == -1, "a refused call or a no-op initialised a device"
print("untouched")
"""


def test_refusals_and_no_ops_initialise_no_device():
    """In a fresh process: the checks and the n_files == 0 answer come before the library looks for a
    device (val_gpu_current_device stays -1), with or without a GPU in the machine."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE], capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "untouched", r.stderr[-2000:]


def test_without_a_device_a_valid_call_fails_loudly():
    if vc.device_count() > 0:
        pytest.skip("GPU present")
    assert _call() == vc.VAL_ERR_IO and vc.last_error()
