"""val_frame_unpack_files_dev (include/val_crc32_gpu.h): the argument checks
answer before any device is touched, so they run without a GPU. The pointers
handed in are made-up addresses that a call which got past its checks would
have to give to the HIP runtime; a refused call never reads them."""
import ctypes
import os
import re

import pytest

import val_protocol_amd.crc as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S = 10, 3
FAKE = 0x7000_0000_1000  # 8-byte aligned, never dereferenced


def _call(**kw):
    a = dict(base=FAKE, off=FAKE + 0x100, length=FAKE + 0x200, stride=0, flen=0, n=N, len_hint=0, n_files=S,
             first=FAKE + 0x300, file_ptr=FAKE + 0x400, file_cap=FAKE + 0x500, written=FAKE + 0x600,
             file_state=FAKE + 0x700, naccepted=None, noverflow=None, file_nbad=None, ok=None, nbad=None, accept=None,
             work=FAKE + 0x800, work_bytes=None, stream=None)
    a.update(kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = int(vc.lib().val_frame_unpack_work_bytes(a["n"]))
    return vc.lib().val_frame_unpack_files_dev(a["base"], a["off"], a["length"], a["stride"], a["flen"], a["n"],
                                               a["len_hint"], a["n_files"], a["first"], a["file_ptr"], a["file_cap"],
                                               a["written"], a["file_state"], a["naccepted"], a["noverflow"],
                                               a["file_nbad"], a["ok"], a["nbad"], a["accept"], a["work"],
                                               a["work_bytes"], a["stream"])


def test_symbol_is_exported_and_declared():
    lib = vc.lib()
    assert hasattr(lib, "val_frame_unpack_files_dev")
    assert "val_frame_unpack_files_dev" in vc.EXPORTS
    f = lib.val_frame_unpack_files_dev
    assert f.restype is ctypes.c_int32 and len(f.argtypes) == 22
    hdr = open(os.path.join(ROOT, "include", "val_crc32_gpu.h")).read()
    m = re.search(r"^val_status_t val_frame_unpack_files_dev\(([^;]*)\);", hdr, re.M)
    assert m, "not declared in include/val_crc32_gpu.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 22
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "d_base", "d_off", "d_len", "stride", "flen", "n", "len_hint", "n_files", "d_first", "d_file_ptr", "d_file_cap",
        "d_written", "d_file_state", "d_naccepted", "d_noverflow", "d_file_nbad", "d_ok", "d_nbad", "d_accept",
        "d_work", "work_bytes", "stream"]
    assert lib.val_gpu_abi_version() == 1  # adding a symbol is compatible
    import val_protocol_amd.wire as wire

    assert callable(wire.unpack_data_files_dev) and "unpack_data_files_dev" in wire.__all__


# what fails -> a word val_gpu_last_error must hold
ANY_N = [("off without len", dict(length=None), "off/len"),
         ("len without off", dict(off=None), "off/len"),
         ("work NULL", dict(work=None), "work is NULL"),
         ("work misaligned", dict(work=FAKE + 0x804), "aligned"),
         ("work_bytes one short", dict(work_bytes=N * 25 - 1), "work_bytes")]
WITH_FRAMES = [("first", dict(first=None), "first"),
               ("file_ptr", dict(file_ptr=None), "file_ptr"),
               ("file_cap", dict(file_cap=None), "file_cap"),
               ("written", dict(written=None), "written"),
               ("base", dict(base=None), "base")]


# no workspace is too small for no frames, so that one case exists at n > 0 only
ANY_N_CASES = [(n, *c) for n in (N, 0) for c in ANY_N if n or "work_bytes" not in c[1]]


@pytest.mark.parametrize("n,what,kw,word", ANY_N_CASES, ids=[f"{c[1]}, n={c[0]}" for c in ANY_N_CASES])
def test_checks_that_hold_at_any_n(n, what, kw, word):
    assert _call(n=n, **kw) == vc.VAL_ERR_INVALID_ARG, what
    assert word in vc.last_error(), (what, vc.last_error())


@pytest.mark.parametrize("what,kw,word", WITH_FRAMES, ids=[c[0] for c in WITH_FRAMES])
def test_null_pointers_with_frames_and_files(what, kw, word):
    assert _call(**kw) == vc.VAL_ERR_INVALID_ARG, what
    err = vc.last_error()
    assert word in err and "NULL" in err, (what, err)
    # exactly this argument is named
    others = {"first", "file_ptr", "file_cap", "written", "base"} - {what}
    assert not any(re.search(rf"\b{o}\b", err) for o in others), err
    # without frames, or without files, there is nothing to refuse
    assert _call(n=0, **kw) == vc.VAL_OK
    assert _call(n_files=0, **kw) == vc.VAL_OK


def test_empty_calls_return_ok_and_clear_the_error():
    assert _call(work=None) == vc.VAL_ERR_INVALID_ARG and vc.last_error()
    assert _call(n=0) == vc.VAL_OK and vc.last_error() == ""
    assert _call(n_files=0) == vc.VAL_OK and vc.last_error() == ""
    assert _call(n=0, n_files=0, base=None, first=None, file_ptr=None, file_cap=None, written=None,
                 file_state=None) == vc.VAL_OK
    # strided mode with nothing in it
    assert _call(n=0, off=None, length=None, stride=64, flen=52) == vc.VAL_OK
