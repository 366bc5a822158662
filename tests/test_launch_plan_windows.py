"""val_gpu_plan_file_windows (include/val_crc32_gpu.h; launch_plan.hpp
plan_file_windows): the launches of val_crc32_file_windows_dev and the resume
calls for a table of shapes. What the kernels rely on is asserted as
properties: the order of the launches, a persistent hash grid of at most one
workgroup per CU, one chunk size 2^k0 with k0 in 12..16, at most 2^16 chunks
per window (the fold has 16 maps) and fewer than 2^32 chunks in all. Needs no
GPU."""
import itertools

import pytest

import val_protocol_amd.crc as vc

CUS = (1, 8, 256, 304)
N_FILES = (0, 1, 64, 5000)
MAX_LEN = (0, 1, 4 << 10, (4 << 10) + 1, 8 << 20, 256 << 20, (256 << 20) + 1, (1 << 32) - 1, 1 << 32)
KNOBS = (0, 12, 13, 16)
WAVES_PER_BLOCK = 16


@pytest.fixture(autouse=True)
def _automatic_chunk():
    vc.set_file_window_chunk(0)
    yield
    vc.set_file_window_chunk(0)


def _chunks(n_files, max_len, k0):
    return n_files * -(-max_len // (1 << k0))


@pytest.mark.parametrize("knob", KNOBS)
def test_plan_properties(knob):
    vc.set_file_window_chunk(knob)
    for cus, n, max_len in itertools.product(CUS, N_FILES, MAX_LEN):
        plan = vc.plan_file_windows(cus, n, max_len)
        what = (knob, cus, n, max_len, [p.astuple() for p in plan])
        if n == 0:
            assert plan == [], what
            continue
        kernels = [p.kernel for p in plan]
        if max_len == 0:  # only empty windows are valid: the count launch finishes every file
            assert kernels == [vc.KERNEL_WINDOWS_COUNT], what
        else:
            assert kernels == [vc.KERNEL_WINDOWS_COUNT, vc.KERNEL_SCAN_FIRST, vc.KERNEL_WINDOWS_HASH], what
        count = plan[0]
        assert count.count == n and count.grid == -(-n // 256), what
        k0 = count.k0
        assert 12 <= k0 <= 16, what
        assert max_len <= 1 << (k0 + 16), what  # one map per bit of a chunk's distance to its window's end
        assert _chunks(n, max_len, k0) < 1 << 32, what
        if knob:  # honoured, and raised only as far as the call needs
            need = next(k for k in range(knob, 17) if max_len <= 1 << (k + 16) and _chunks(n, max_len, k) < 1 << 32)
            assert k0 == need, what
        else:  # the smallest chunk at which the call's bound is one chunk per wave, else 64 KiB
            fits = [k for k in range(12, 17) if _chunks(n, max_len, k) <= cus * WAVES_PER_BLOCK]
            assert k0 == (fits[0] if fits else 16), what
        if max_len == 0:
            continue
        first, hash_ = plan[1], plan[2]
        assert (first.grid, first.count) == (1, n), what
        assert hash_.k0 == k0 and hash_.count == _chunks(n, max_len, k0), what
        assert 1 <= hash_.grid <= cus, what
        assert hash_.grid == min(cus, -(-hash_.count // WAVES_PER_BLOCK)), what


def test_named_shapes_at_256_cus():
    """The automatic chunk of the shapes tools/timing_resume.py times."""
    def k0(n, max_len):
        return vc.plan_file_windows(256, n, max_len)[0].k0

    assert k0(1, 8 << 20) == 12  # one 8 MiB window: 2,048 chunks of 4 KiB, as the region call cuts it
    assert k0(1, 256 << 20) == 16  # 4,096 chunks of 64 KiB
    assert k0(64, 8 << 20) == 16
    assert k0(8, 256 << 20) == 16
    assert k0(1024, 64 << 10) == 14  # 4,096 chunks of 16 KiB
    assert k0(64, 1 << 10) == 12
    plan = vc.plan_file_windows(256, 64, 8 << 20)
    assert (plan[2].grid, plan[2].count) == (256, 64 * 128)
    plan = vc.plan_file_windows(256, 3, 5000)
    assert (plan[2].grid, plan[2].count, plan[2].k0) == (1, 6, 12)


def test_refused_calls_have_no_plan():
    for knob in KNOBS:
        vc.set_file_window_chunk(knob)
        for cus in CUS:
            assert vc.plan_file_windows(cus, 1, (1 << 32) + 1) == []  # more than 2^16 chunks of 64 KiB
            assert vc.plan_file_windows(cus, 1, (1 << 64) - 1) == []
            assert vc.plan_file_windows(cus, 0x10000, 1 << 32) == []  # 2^32 chunks of 64 KiB
            assert vc.plan_file_windows(cus, 0xFFFFFFFF, (1 << 32) - 1) == []
            assert len(vc.plan_file_windows(cus, 0xFFFF, 1 << 32)) == 3  # the largest product
            assert len(vc.plan_file_windows(cus, 0xFFFFFFFF, 1)) == 3
    assert vc.lib().val_gpu_plan_file_windows(256, 64, 8 << 20, None) == 3  # the count alone, without an array


def test_the_window_calls_plans_are_untouched():
    """The five window calls keep their planner entry; the file windows have their own."""
    assert vc.plan_window(5, 256, 64) == []
    assert vc.KERNEL_WINDOWS_COUNT == 14 and vc.KERNEL_WINDOWS_HASH == 15
