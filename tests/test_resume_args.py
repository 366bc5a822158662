"""val_crc32_file_windows_dev and the three resume calls
(include/val_crc32_gpu.h): the argument checks answer before any device is
touched, so they run without a GPU. The pointers handed in are made-up
addresses that a call which got past its checks would have to give to the HIP
runtime; a refused call never reads them."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import val_protocol_amd.crc as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 3
FAKE = 0x7000_0000_1000  # 8-byte aligned, never dereferenced
MAX_LEN = 8 << 20

# call -> (parameter names of the header in order, the pointers that must not be NULL, the nullable ones)
CALLS = {
    "val_crc32_file_windows_dev": (
        ["d_file_ptr", "d_file_size", "d_win_off", "d_win_len", "n_files", "max_len", "d_crc", "d_status", "d_work",
         "work_bytes", "stream"],
        ["file_ptr", "file_size", "win_off", "win_len", "crc"], ["status"]),
    "val_resume_tail_files_dev": (
        ["d_file_ptr", "d_existing", "d_incoming", "n_files", "tail_cap_bytes", "min_verify_bytes", "mismatch_skip",
         "d_action", "d_resume_off", "d_verify_len", "d_verify_crc", "d_work", "work_bytes", "stream"],
        ["file_ptr", "existing", "incoming", "action", "resume_off", "verify_len", "verify_crc"], []),
    "val_resume_request_files_dev": (
        ["d_file_ptr", "d_file_size", "d_action", "d_resume_off", "d_verify_len", "n_files", "max_len", "d_req_off",
         "d_req_len", "d_req_crc", "d_status", "d_work", "work_bytes", "stream"],
        ["file_ptr", "file_size", "action", "resume_off", "verify_len", "req_off", "req_len", "req_crc"], ["status"]),
    "val_resume_check_files_dev": (
        ["d_file_ptr", "d_existing", "d_incoming", "d_action", "d_req_off", "d_req_len", "d_req_crc",
         "d_rec_resume_off", "n_files", "max_len", "mismatch_skip", "d_local_crc", "d_result", "d_written", "d_work",
         "work_bytes", "stream"],
        ["file_ptr", "existing", "incoming", "req_off", "req_len", "req_crc", "rec_resume_off", "result", "written"],
        ["action", "local_crc"]),
}
NAMES = sorted(CALLS)


def _work_bytes(n_files):
    return int(vc.lib().val_file_windows_work_bytes(n_files))


def _call(name, **kw):
    """The call with a made-up address for every pointer (nullable ones NULL), overridden by kw."""
    params, required, _ = CALLS[name]
    a = dict(n_files=S, max_len=MAX_LEN, tail_cap_bytes=0, min_verify_bytes=0, mismatch_skip=0, work=FAKE + 0x10000,
             work_bytes=None, stream=None)
    for i, r in enumerate(required):
        a[r] = FAKE + 0x100 * (i + 1)
    a.update(kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = _work_bytes(a["n_files"])
    args = [a.get(p[2:] if p.startswith("d_") else p) for p in params]
    return getattr(vc.lib(), name)(*args)


def test_symbols_are_exported_and_declared():
    lib = vc.lib()
    hdr = open(os.path.join(ROOT, "include", "val_crc32_gpu.h")).read()
    for name, (params, _, _) in CALLS.items():
        assert hasattr(lib, name) and name in vc.EXPORTS
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int32 and len(f.argtypes) == len(params)
        m = re.search(rf"^val_status_t {name}\(([^;]*)\);", hdr, re.M)
        assert m, f"{name} is not declared in include/val_crc32_gpu.h"
        got = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
        assert got == params
    for name in ("val_file_windows_work_bytes", "val_gpu_plan_file_windows", "val_gpu_set_file_window_chunk"):
        assert hasattr(lib, name) and name in vc.EXPORTS
    assert re.search(r"^uint64_t val_file_windows_work_bytes\(uint32_t n_files\);", hdr, re.M)
    assert re.search(r"^val_status_t val_gpu_set_file_window_chunk\(uint32_t k0\);", hdr, re.M)
    assert re.search(r"^uint32_t val_gpu_plan_file_windows\(uint32_t cus, uint32_t n_files, uint64_t max_len, "
                     r"val_gpu_launch_t out\[3\]\);", hdr, re.M)
    assert lib.val_gpu_abi_version() == 1  # adding symbols is compatible
    import val_protocol_amd.wire as wire

    for w in ("file_windows_dev", "resume_tail_files_dev", "resume_request_files_dev", "resume_check_files_dev",
              "file_windows_work_bytes"):
        assert callable(getattr(wire, w)) and w in wire.__all__
    assert wire.file_windows_work_bytes(S) == _work_bytes(S)
    assert lib.val_gpu_build_flags() == b""


def test_work_bytes_is_monotone_and_aligned():
    sizes = (0, 1, 2, 3, 7, 64, 65, 300, 65535, 1 << 20, 0xFFFFFFFF)
    got = [_work_bytes(n) for n in sizes]
    assert got == sorted(got) and all(v % 8 == 0 for v in got)
    # per file: the window's address and length (u64), its count, accumulator and arrivals (u32), and
    # n + 1 prefix entries (u32)
    assert all(v >= 32 * n + 4 for v, n in zip(got, sizes))
    assert _work_bytes(0) == 8 and _work_bytes(1) == 40 and _work_bytes(3) == 104


# what fails -> a word val_gpu_last_error must hold
ANY_N = [("work NULL", dict(work=None), "work is NULL"),
         ("work misaligned", dict(work=FAKE + 0x10004), "aligned"),
         ("work_bytes one short", dict(work_bytes="short"), "work_bytes"),
         ("work_bytes zero", dict(work_bytes=0), "work_bytes")]
WITH_MAX_LEN = [("max_len above 2^32", dict(max_len=(1 << 32) + 1), "max_len"),
                ("max_len 2^64 - 1", dict(max_len=(1 << 64) - 1), "max_len"),
                ("chunk product", dict(n_files=0x20000, max_len=1 << 32, work_bytes=(1 << 64) - 1), "32 bits"),
                ("chunk product, most files", dict(n_files=0xFFFFFFFF, max_len=(1 << 32) - 1,
                                                   work_bytes=(1 << 64) - 1), "32 bits")]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("what,kw,word", ANY_N, ids=[c[0] for c in ANY_N])
def test_workspace_checks(name, what, kw, word):
    for n in (S, 0):  # the prefix sum's one entry makes even no files need 8 bytes
        k = dict(work_bytes=_work_bytes(n) - 1) if kw.get("work_bytes") == "short" else kw
        assert _call(name, **dict(dict(n_files=n), **k)) == vc.VAL_ERR_INVALID_ARG, (what, n)
        assert word in vc.last_error(), (what, vc.last_error())


@pytest.mark.parametrize("name", [n for n in NAMES if "max_len" in CALLS[n][0]])
@pytest.mark.parametrize("what,kw,word", WITH_MAX_LEN, ids=[c[0] for c in WITH_MAX_LEN])
def test_max_len_and_chunk_product(name, what, kw, word):
    assert _call(name, **kw) == vc.VAL_ERR_INVALID_ARG, what
    assert word in vc.last_error(), (what, vc.last_error())


def test_max_len_bounds():
    """0, 2^32 - 1 and 2^32 pass the max_len check (the next check that fails, a NULL pointer, answers)."""
    for name in (n for n in NAMES if "max_len" in CALLS[n][0]):
        for max_len in (0, 1, (1 << 32) - 1, 1 << 32):
            assert _call(name, max_len=max_len, file_ptr=None) == vc.VAL_ERR_INVALID_ARG
            assert "file_ptr is NULL" in vc.last_error(), (name, max_len, vc.last_error())
            assert _call(name, max_len=max_len, n_files=0) == vc.VAL_OK
    # the largest product: 65,535 files of 2^32 bytes are 2^32 - 65,536 chunks of 64 KiB
    assert _call("val_crc32_file_windows_dev", n_files=0xFFFF, max_len=1 << 32, file_ptr=None) == vc.VAL_ERR_INVALID_ARG
    assert "file_ptr is NULL" in vc.last_error()


def test_tail_policy_bounds():
    """The tail call derives max_len from its policy: any cap is clamped, a min_verify_bytes above 2^32 is refused."""
    name = "val_resume_tail_files_dev"
    for cap in (0, 1, (1 << 32) - 1, (1 << 64) - 1):
        assert _call(name, tail_cap_bytes=cap, n_files=0) == vc.VAL_OK
    assert _call(name, min_verify_bytes=1 << 32, n_files=0) == vc.VAL_OK
    for n in (S, 0):
        assert _call(name, min_verify_bytes=(1 << 32) + 1, n_files=n) == vc.VAL_ERR_INVALID_ARG
        assert "min_verify_bytes" in vc.last_error()
    # 65,536 files whose windows may reach 2^32 bytes: the chunk product
    assert _call(name, min_verify_bytes=1 << 32, n_files=0x10000, work_bytes=(1 << 64) - 1) == vc.VAL_ERR_INVALID_ARG
    assert "32 bits" in vc.last_error()


REQUIRED_CASES = [(n, r) for n in NAMES for r in CALLS[n][1]]


@pytest.mark.parametrize("name,what", REQUIRED_CASES, ids=[f"{n}-{r}" for n, r in REQUIRED_CASES])
def test_null_pointers_with_files(name, what):
    required = CALLS[name][1]
    assert _call(name, **{what: None}) == vc.VAL_ERR_INVALID_ARG, what
    err = vc.last_error()
    assert re.search(rf"\b{what}\b", err) and "NULL" in err, (what, err)
    # exactly this argument is named
    assert not any(re.search(rf"\b{o}\b", err) for o in set(required) - {what}), err
    # without files there is nothing to refuse
    assert _call(name, n_files=0, **{what: None}) == vc.VAL_OK


@pytest.mark.parametrize("name", NAMES)
def test_no_files_is_a_no_op_that_clears_the_error(name):
    assert _call(name, work=None) == vc.VAL_ERR_INVALID_ARG and vc.last_error()
    assert _call(name, n_files=0) == vc.VAL_OK and vc.last_error() == ""
    assert _call(name, n_files=0, work_bytes=8) == vc.VAL_OK
    assert _call(name, n_files=0, **{k: None for k in CALLS[name][1]}) == vc.VAL_OK


def test_chunk_knob_values():
    lib = vc.lib()
    try:
        for k0 in (12, 13, 14, 15, 16, 0):
            assert lib.val_gpu_set_file_window_chunk(k0) == vc.VAL_OK
        for k0 in (1, 11, 17, 64, 4096, 0xFFFFFFFF):
            assert lib.val_gpu_set_file_window_chunk(k0) == vc.VAL_ERR_INVALID_ARG
            assert "12..16" in vc.last_error()
        with pytest.raises(vc.ValError):
            vc.set_file_window_chunk(11)
    finally:
        vc.set_file_window_chunk(0)


_NO_DEVICE = r"""
import val_protocol_amd.crc as vc
FAKE = 0x7000_0000_1000
lib = vc.lib()
wb = int(lib.val_file_windows_work_bytes(3))
def call(n_files, work):
    return lib.val_crc32_file_windows_dev(FAKE, FAKE + 0x100, FAKE + 0x200, FAKE + 0x300, n_files, 1 << 20,
                                          FAKE + 0x400, None, work, wb, None)
def tail(n_files, work):
    return lib.val_resume_tail_files_dev(FAKE, FAKE + 0x100, FAKE + 0x200, n_files, 0, 0, 0, FAKE + 0x300,
                                         FAKE + 0x400, FAKE + 0x500, FAKE + 0x600, work, wb, None)
for f in (call, tail):
    assert f(3, None) == vc.VAL_ERR_INVALID_ARG
    assert f(0, FAKE + 0x1000) == vc.VAL_OK
assert lib.val_gpu_set_file_window_chunk(12) == vc.VAL_OK
assert lib.val_gpu_plan_file_windows(256, 64, 8 << 20, None) == 3
assert lib.val_gpu_current_device() == -1, "a refused call, a no-op or the planner initialised a device"
print("untouched")
"""


def test_refusals_and_no_ops_initialise_no_device():
    """In a fresh process: the checks, the n_files == 0 answer, the knob and the planner come before the
    library looks for a device (val_gpu_current_device stays -1), with or without a GPU in the machine."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE], capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "untouched", r.stderr[-2000:]


@pytest.mark.parametrize("name", NAMES)
def test_without_a_device_a_valid_call_fails_loudly(name):
    if vc.device_count() > 0:
        pytest.skip("GPU present")
    assert _call(name) == vc.VAL_ERR_IO and vc.last_error()
