"""val_frame_respond_files_dev and val_frame_apply_acks_files_dev
(include/val_crc32_gpu.h): the argument checks answer before any device is
touched, so they run without a GPU, on made-up addresses that a refused call
never reads. Also the work-byte helpers and the launches
val_gpu_plan_ack_calls reports."""
import ctypes
import os
import re

import pytest

import val_protocol_amd.crc as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S = 10, 3
FAKE = 0x7000_0000_1000  # 8-byte aligned, never dereferenced
CUS = 256


def _p(k):
    return FAKE + 0x100 * k


RESPOND = dict(base=_p(0), off=_p(1), length=_p(2), stride=0, flen=0, n=N, n_files=S, first=_p(3), ok=_p(4),
               accept=_p(5), written=_p(6), total=_p(7), ack_stride=1, since=_p(8), out=_p(9), resp_off=_p(10),
               resp_cap=_p(11), resp_len=_p(12), nresp=_p(13), ndropped=None, work=_p(14), work_bytes=None, stream=None)
APPLY = dict(base=_p(0), off=_p(1), length=_p(2), stride=0, flen=0, n=N, len_hint=0, n_files=S, first=_p(3),
             file_size=_p(4), last_acked=_p(5), next=_p(6), nretrans=None, file_nbad=None, ok=None, nbad=None,
             work=_p(7), work_bytes=None, stream=None)


def _respond(**kw):
    a = dict(RESPOND, **kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = int(vc.lib().val_frame_respond_work_bytes(a["n"]))
    return vc.lib().val_frame_respond_files_dev(*a.values())


def _apply(**kw):
    a = dict(APPLY, **kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = int(vc.lib().val_frame_apply_acks_work_bytes(a["n"]))
    return vc.lib().val_frame_apply_acks_files_dev(*a.values())


CALLS = {"respond": (_respond, "val_frame_respond_files_dev", 23,
                     ["d_base", "d_off", "d_len", "stride", "flen", "n", "n_files", "d_first", "d_ok", "d_accept",
                      "d_written", "d_total", "ack_stride", "d_since", "d_out", "d_resp_off", "d_resp_cap",
                      "d_resp_len", "d_nresp", "d_ndropped", "d_work", "work_bytes", "stream"]),
         "apply": (_apply, "val_frame_apply_acks_files_dev", 19,
                   ["d_base", "d_off", "d_len", "stride", "flen", "n", "len_hint", "n_files", "d_first", "d_file_size",
                    "d_last_acked", "d_next", "d_nretrans", "d_file_nbad", "d_ok", "d_nbad", "d_work", "work_bytes",
                    "stream"])}


@pytest.mark.parametrize("which", sorted(CALLS))
def test_symbols_are_exported_and_declared(which):
    _, name, nargs, names = CALLS[which]
    lib = vc.lib()
    assert hasattr(lib, name) and name in vc.EXPORTS
    f = getattr(lib, name)
    assert f.restype is ctypes.c_int32 and len(f.argtypes) == nargs
    hdr = open(os.path.join(ROOT, "include", "val_crc32_gpu.h")).read()
    m = re.search(rf"^val_status_t {name}\(([^;]*)\);", hdr, re.M)
    assert m, "not declared in include/val_crc32_gpu.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == names
    assert lib.val_gpu_abi_version() == 1  # adding a symbol is compatible
    import val_protocol_amd.wire as wire

    for w in ("respond_files_dev", "apply_acks_files_dev", "respond_window", "apply_acks", "put_response",
              "ack_offsets"):
        assert callable(getattr(wire, w)) and w in wire.__all__


ANY_N = [("off without len", dict(length=None), "off/len"),
         ("len without off", dict(off=None), "off/len"),
         ("work NULL", dict(work=None), "work is NULL"),
         ("work misaligned", dict(work=_p(14) + 4), "aligned"),
         ("work_bytes one short", dict(work_bytes=-1), "work_bytes")]
ANY_N_CASES = [(w, n, *c) for w in sorted(CALLS) for n in (N, 0) for c in ANY_N if n or "work_bytes" not in c[1]]


@pytest.mark.parametrize("which,n,what,kw,word", ANY_N_CASES, ids=[f"{c[0]}: {c[2]}, n={c[1]}" for c in ANY_N_CASES])
def test_checks_that_hold_at_any_n(which, n, what, kw, word):
    call, name = CALLS[which][:2]
    if kw.get("work_bytes") == -1:
        helper = name.replace("_files_dev", "_work_bytes")
        kw = dict(work_bytes=int(getattr(vc.lib(), helper)(n)) - 1)
    assert call(n=n, **kw) == vc.VAL_ERR_INVALID_ARG, what
    assert word in vc.last_error(), (what, vc.last_error())


NULLS = [("respond", k, dict({k: None}), k) for k in
         ("first", "ok", "accept", "written", "total", "since", "out", "resp_off", "resp_cap", "resp_len", "nresp",
          "base")]
NULLS += [("apply", k, dict({k: None}), k) for k in ("first", "file_size", "last_acked", "next", "base")]


@pytest.mark.parametrize("which,what,kw,word", NULLS, ids=[f"{c[0]}: {c[1]}" for c in NULLS])
def test_null_pointers_with_frames_and_files(which, what, kw, word):
    call = CALLS[which][0]
    assert call(**kw) == vc.VAL_ERR_INVALID_ARG, what
    err = vc.last_error()
    assert re.search(rf"\b{word}\b", err) and "NULL" in err, (what, err)
    # without frames, or without files, there is nothing to refuse
    assert call(n=0, **kw) == vc.VAL_OK and vc.last_error() == ""
    assert call(n_files=0, **kw) == vc.VAL_OK and vc.last_error() == ""


def test_since_is_optional_at_stride_zero_only():
    assert _respond(since=None, ack_stride=3) == vc.VAL_ERR_INVALID_ARG and "since" in vc.last_error()
    # ack_stride == 0 passes the check on since and is refused for the next NULL in line
    assert _respond(since=None, ack_stride=0, out=None) == vc.VAL_ERR_INVALID_ARG
    assert "since" not in vc.last_error() and "out" in vc.last_error()


def test_work_bytes_and_bound():
    lib = vc.lib()
    assert lib.val_frame_respond_bytes_max(0) == 0 and lib.val_frame_respond_bytes_max(7) == 280
    assert lib.val_frame_respond_bytes_max(1 << 32) == 40 << 32
    assert lib.val_frame_respond_bytes_max((1 << 64) - 1) == (1 << 64) - 1  # saturates, never wraps
    prev_r = prev_a = 0
    for n in (0, 1, 2, 1023, 1024, 1025, 100000, (1 << 32) - 1):
        r, a = lib.val_frame_respond_work_bytes(n), lib.val_frame_apply_acks_work_bytes(n)
        assert r % 8 == 0 and a % 8 == 0
        assert r >= 28 * n and a >= n  # three u64 and a u32 per frame; a verdict per frame
        assert r >= prev_r and a >= prev_a
        prev_r, prev_a = r, a


SIZES = (0, 1, 1024, 1025, 100000)


def test_the_workgroup_size_turns_at_256_frames_per_file():
    lanes = lambda n, f: vc.plan_ack_calls(vc.ACK_RESPOND, CUS, n, f)[1].lanes  # noqa: E731
    assert (lanes(256 * 7, 7), lanes(257 * 7 - 1, 7), lanes(257 * 7, 7)) == (256, 256, 1024)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_files", SIZES)
def test_planned_launches(n, n_files):
    resp = vc.plan_ack_calls(vc.ACK_RESPOND, CUS, n, n_files)
    appl = vc.plan_ack_calls(vc.ACK_APPLY, CUS, n, n_files)
    if n == 0 or n_files == 0:
        assert resp == [] and appl == []
        return
    files_grid = min(n_files, CUS)
    per_frame = (n + 255) // 256
    # files of 256 frames or fewer on average: workgroups of 256 threads, up to eight per CU
    small = n // n_files <= 256
    assert [(l.kernel, l.grid, l.count, l.lanes) for l in resp] == [
        (vc.KERNEL_UNPACK_PARSE, per_frame, n, 0),
        (vc.KERNEL_ACK_RESPOND_FILES, min(n_files, 8 * CUS) if small else files_grid, n_files, 256 if small else 1024),
        (vc.KERNEL_ACK_EMIT, per_frame, n, 0)]
    assert [(l.kernel, l.grid, l.count) for l in appl] == [(vc.KERNEL_ACK_APPLY_FILES, files_grid, n_files)]
    assert (vc.KERNEL_ACK_RESPOND_FILES, vc.KERNEL_ACK_EMIT, vc.KERNEL_ACK_APPLY_FILES) == (16, 17, 18)


def test_plan_of_an_unknown_call_and_of_no_cus():
    assert vc.plan_ack_calls(2, CUS, 10, 10) == []
    assert [l.grid for l in vc.plan_ack_calls(vc.ACK_APPLY, 0, 10, 10)] == [1]
    # the window planner does not know these calls
    assert vc.plan_window(5, CUS, 10, groups=10) == []
