"""val_frame_fill_window (include/val_wire.h): the sender's window-fill rule in
plain C, host only. It is pinned twice: against the reference's own sender, as
recorded in tests/golden/session_vectors.json (every DATA frame the reference
sent, split at its explicit-offset frames), and against a restatement of the
rule in Python kept here, over the edges of every input."""
import numpy as np
import pytest

import val_protocol_amd.crc as vc
import val_protocol_amd.wire as wire
from tests import _sessions

U64 = (1 << 64) - 1
SESSIONS = ("window64_mtu1024", "window64_mtu16404", "resume_tail_cap8m", "resume_tail_cap1k", "resume_tail_mismatch")


def restated(next, last_acked, size, mtu, budget, cap):
    """The rule as include/val_wire.h states it -> [(file_off, pay, explicit, frame_off, crc_len)], used, next."""
    M, out, used = mtu - 12, [], 0
    while len(out) < budget and next < size:
        explicit = next == last_acked
        pay = min(size - next, M - 8 if explicit else M)
        content = pay + (8 if explicit else 0)
        if 12 + content > cap - used:
            break
        out.append((next, pay, int(explicit), used, 8 + content))
        used += 12 + content
        next += pay
    return out, used, next


def _rule(next, last_acked, size, mtu, budget, cap=U64):
    fo, pl, inc, off, cl, used, nxt = wire.fill_window(next, last_acked, size, mtu, budget, cap)
    assert fo.size == pl.size == inc.size == off.size == cl.size
    return list(zip(fo.tolist(), pl.tolist(), inc.tolist(), off.tolist(), cl.tolist())), used, nxt


def _same(*args):
    got, want = _rule(*args), restated(*args)
    assert got == want, (args, got[0][:3], want[0][:3], got[1:], want[1:])
    return got


def segments(s):
    """The session's DATA frames as (file_off, wire_len, explicit), split in front of every explicit one."""
    segs = []
    for rec in s["tx_frames"]:
        if rec[0] != _sessions.PKT_DATA:
            continue
        explicit = bytes.fromhex(rec[4])[1] & 1
        if explicit or not segs:
            segs.append([])
        segs[-1].append((rec[3], rec[1], explicit))
    return segs


def test_binding_is_exported():
    assert "val_frame_fill_window" in vc.EXPORTS and hasattr(vc.lib(), "val_frame_fill_window")
    assert {"fill_window", "fill_files_dev", "fill_work_bytes"} <= set(wire.__all__)


@pytest.mark.parametrize("name", SESSIONS)
def test_rule_reproduces_the_reference_sender(name):
    s = _sessions.load()[name]
    segs = segments(s)
    assert segs and all(seg[0][2] == 1 for seg in segs)
    for seg in segs:
        start = seg[0][0]
        frames, used, nxt = _rule(start, start, s["bytes"], s["mtu"], len(seg))
        assert [(f[0], f[4] + 4, f[2]) for f in frames] == seg
        assert used == sum(w for _, w, _ in seg) and nxt == seg[-1][0] + seg[-1][1] - 12 - (8 if len(seg) == 1 else 0)
    # the five sessions are all the fixture holds: 108 window fills, 1,791 DATA frames
    every = _sessions.load()
    assert sorted(every) == sorted(SESSIONS)
    assert sum(len(segments(x)) for x in every.values()) == 108
    assert sum(len(g) for x in every.values() for g in segments(x)) == 1791


@pytest.mark.parametrize("mtu", [21, 40, 1024, 65547])
def test_remainders_around_a_frame(mtu):
    M = mtu - 12
    for explicit in (True, False):
        for rem in sorted({M - 8, M - 7, M, M + 1, 1, 0, 2 * M - 8, 2 * M - 7, 3 * M}):
            if rem < 0:
                continue
            for nxt in (0, 5, 1 << 33):
                la = nxt if explicit else nxt + 1
                frames, used, end = _same(nxt, la, nxt + rem, mtu, 10, U64)
                assert end == nxt + rem and sum(f[1] for f in frames) == rem
                assert [f[2] for f in frames] == ([int(explicit)] + [0] * (len(frames) - 1))[:len(frames)]
    # the explicit frame of a remainder of M - 8 is full and alone; M - 7 spills one byte into a second frame
    assert [f[1] for f in _same(0, 0, M - 8, mtu, 10, U64)[0]] == [M - 8]
    assert [f[1] for f in _same(0, 0, M - 7, mtu, 10, U64)[0]] == [M - 8, 1]
    assert [f[1] for f in _same(0, 9, M, mtu, 10, U64)[0]] == [M]
    assert [f[1] for f in _same(0, 9, M + 1, mtu, 10, U64)[0]] == [M, 1]


def test_finished_and_overrun_files_make_no_frame():
    for nxt, size in ((100, 100), (101, 100), (U64, 0), (U64, U64), (0, 0)):
        for la in (nxt, 0):
            assert _same(nxt, la, size, 1024, 8, U64) == ([], 0, nxt)


def test_only_the_first_frame_can_be_explicit():
    frames, used, end = _same(1000, 1000, 10_000, 112, 50, U64)
    assert [f[2] for f in frames] == [1] + [0] * 49 and frames[1][0] == 1092 and end == 1092 + 49 * 100
    frames, used, end = _same(1000, 0, 10_000, 112, 50, U64)
    assert not any(f[2] for f in frames) and end == 6000 and used == 50 * 112
    # A sender never has last_acked ahead of next. The rule is the reference's loop all the same: a
    # frame that starts exactly there is explicit, one that merely covers it is not.
    frames, _, end = _same(1000, 1100, 10_000, 112, 5, U64)
    assert [f[:3] for f in frames[:3]] == [(1000, 100, 0), (1100, 92, 1), (1192, 100, 0)] and end == 1492
    frames, _, _ = _same(1000, 1101, 10_000, 112, 5, U64)
    assert not any(f[2] for f in frames)


def test_budget():
    assert _same(0, 0, 5000, 112, 0, U64) == ([], 0, 0)
    frames, used, end = _same(0, 0, 5000, 112, 1, U64)
    assert frames == [(0, 92, 1, 0, 108)] and (used, end) == (112, 92)
    frames, used, end = _same(7, 0, 5000, 112, 1, U64)
    assert frames == [(7, 100, 0, 0, 108)] and (used, end) == (112, 107)


@pytest.mark.parametrize("explicit", [True, False])
def test_capacity(explicit):
    mtu, size = 112, 350  # frames of 112, 112, 112 and a short last one
    la = 0 if explicit else 1
    full, used_full, _ = _same(0, la, size, mtu, 10, U64)
    ends = [f[3] + f[4] + 4 for f in full]
    assert len(full) == 4 and ends[-1] == used_full and ends[:3] == [112, 224, 336] and ends[3] < 448
    for k, end in enumerate(ends):
        frames, used, nxt = _same(0, la, size, mtu, 10, end)  # exactly at a frame end
        assert len(frames) == k + 1 and used == end
        frames, used, nxt = _same(0, la, size, mtu, 10, end - 1)  # one byte less
        assert len(frames) == k and used == (ends[k - 1] if k else 0)
    for cap in (0, 1, 11, 12, 20, 111):
        assert _same(0, la, size, mtu, 10, cap) == ([], 0, 0)
    # a short only frame fits a capacity below the mtu
    assert len(_same(0, la, 3, mtu, 10, 12 + 3 + (8 if explicit else 0))[0]) == 1
    assert len(_same(0, la, 3, mtu, 10, 11 + 3 + (8 if explicit else 0))[0]) == 0


def test_mtu_bounds():
    for mtu in (0, 11, 12, 20, 65548, 1 << 32, U64):
        with pytest.raises(wire.ValError) as e:
            wire.fill_window(0, 0, 1000, mtu, 4)
        assert e.value.status == vc.VAL_ERR_INVALID_ARG
    # mtu 21: an explicit frame carries one byte, an implied one nine
    assert [f[1] for f in _same(0, 0, 20, 21, 3, U64)[0]] == [1, 9, 9]
    assert [f[4] for f in _same(0, 0, 20, 21, 3, U64)[0]] == [17, 17, 17]
    # mtu 65547: content 65,535, the most a header can say
    frames, used, end = _same(0, 0, 200_000, 65547, 3, U64)
    assert [f[4] for f in frames] == [65543] * 3 and [f[1] for f in frames] == [65527, 65535, 65535]
    assert used == 3 * 65547


def test_refused_mtu_sets_the_results():
    import ctypes

    nf, used, nxt = ctypes.c_uint32(9), ctypes.c_uint64(9), ctypes.c_uint64(9)
    st = vc.lib().val_frame_fill_window(77, 77, 1000, 20, 4, U64, None, None, None, None, None, ctypes.byref(nf),
                                        ctypes.byref(used), ctypes.byref(nxt))
    assert st == vc.VAL_ERR_INVALID_ARG and (nf.value, used.value, nxt.value) == (0, 0, 77)
    # every output is nullable
    assert vc.lib().val_frame_fill_window(0, 0, 1000, 1024, 4, U64, None, None, None, None, None, None, None,
                                          None) == vc.VAL_OK


def test_positions_beyond_32_bits_and_at_the_top():
    for base in ((1 << 32) + 5, (1 << 33), (1 << 63) + 1):
        frames, used, end = _same(base, base, base + 3000, 1024, 8, U64)
        assert frames[0][0] == base and end == base + 3000 and len(frames) == 3
    # a file that ends at 2^64 - 1: no sum wraps
    top = U64
    frames, used, end = _same(top - 2500, top - 2500, top, 1024, 8, U64)
    assert end == top and [f[1] for f in frames] == [1004, 1012, 484]
    frames, used, end = _same(top - 2500, 0, top, 1024, 2, U64)
    assert end == top - 2500 + 2024
    frames, used, end = _same(top - 1, top - 1, top, 1024, 8, U64)
    assert frames == [(top - 1, 1, 1, 0, 17)] and end == top
    # a huge file from 0: the budget ends the call long before the file does
    frames, used, end = _same(0, 1, top, 65547, 64, U64)
    assert len(frames) == 64 and end == 64 * 65535
    # a capacity near the top does not wrap either
    assert len(_same(0, 0, 10_000, 1024, 5, U64 - 1)[0]) == 5


def test_randomised_against_the_restatement():
    rng = np.random.default_rng(2024)
    for _ in range(3000):
        mtu = int(rng.choice([21, 22, 29, 30, 64, 1024, 4096, 65547]))
        M = mtu - 12
        nxt = int(rng.integers(0, 5000))
        size = nxt + int(rng.integers(-3, 12 * M))
        la = [nxt, int(rng.integers(0, 5000)), nxt + M * int(rng.integers(0, 6))][int(rng.integers(0, 3))]
        budget = int(rng.integers(0, 14))
        cap = U64 if rng.integers(0, 2) else int(rng.integers(0, 14 * mtu))
        _same(nxt, la, max(size, 0), mtu, budget, cap)
