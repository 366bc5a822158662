"""val_frame_accept (include/val_wire.h): the receiver's ordering rule
(reference src/val_receiver.c:871-895) in plain C, the oracle of the device
unpacker (val_frame_unpack_batch_dev). Checked against a Python restatement of
the rule and against val_crc32_fold_payload_states_at. No GPU."""
import numpy as np
import pytest

import val_protocol_amd.crc as vc
import val_protocol_amd.wire as wire

U64 = (1 << 64) - 1
IMPLIED, NOT_DATA, NOT_ACCEPTED = wire.OFFSET_IMPLIED, wire.OFFSET_NOT_DATA, wire.NOT_ACCEPTED


def _rule(file_off, pay_len, ok, cap, written):
    """The rule, restated with Python integers (no wrap-around anywhere)."""
    w, dst, nacc, novf = written, [], 0, 0
    for fo, pl, k in zip(file_off, pay_len, ok):
        fo, pl = int(fo), int(pl)
        dst.append(NOT_ACCEPTED)
        if not k or fo == NOT_DATA:
            continue
        eff = w if fo == IMPLIED else fo
        if eff != w:
            continue
        if eff + pl > cap:
            novf += 1
            continue
        dst[-1] = w
        w += pl
        nacc += 1
    return np.array(dst, dtype=np.uint64), w, nacc, novf


def _sequence(rng, n, start):
    """A window as a receiver may see it: mostly in-order frames, with
    duplicates, gaps, control frames, corrupt frames and empty payloads mixed in."""
    file_off, pay_len, ok = [], [], []
    w = start
    for _ in range(n):
        pl = int(rng.choice([0, 1, 3, 7, 100, 1012, 65527]))
        kind = rng.integers(0, 10)
        good = 1
        if kind <= 2:
            fo = IMPLIED
        elif kind <= 5:
            fo = w
        elif kind == 6:
            fo = NOT_DATA
        elif kind == 7:  # duplicate of something earlier (or the same place when w == 0)
            fo = int(rng.integers(0, w + 1))
        elif kind == 8:  # gap
            fo = w + int(rng.integers(1, 5000))
        else:  # right place, broken trailer
            fo, good = w, 0
        file_off.append(fo)
        pay_len.append(pl)
        ok.append(good)
        if good and fo in (IMPLIED, w):
            w += pl
    return (np.array(file_off, dtype=np.uint64), np.array(pay_len, dtype=np.uint32), np.array(ok, dtype=np.uint8), w)


@pytest.mark.parametrize("seed", range(8))
def test_accept_equals_the_rule(seed):
    rng = np.random.default_rng(4000 + seed)
    seen = set()
    for _ in range(400):
        n = int(rng.integers(0, 41))
        start = int(rng.choice([0, 5, 1 << 33]))
        fo, pl, ok, end = _sequence(rng, n, start)
        # no cap, a cap past the end, and caps that cut the sequence
        caps = [U64, end + 10, end, max(end - 1, 0), int(rng.integers(start, end + 1)), int(rng.integers(0, start + 1))]
        for cap in caps:
            want = _rule(fo, pl, ok, cap, start)
            dst, w, nacc, novf = wire.frame_accept(fo, pl, start, cap, ok)
            assert np.array_equal(dst, want[0]) and (w, nacc, novf) == want[1:], (seed, n, start, cap)
            seen.add((nacc > 0, novf > 0))
        # ok = NULL: every trailer good
        want = _rule(fo, pl, np.ones(n), U64, start)
        dst, w, nacc, novf = wire.frame_accept(fo, pl, start)
        assert np.array_equal(dst, want[0]) and (w, nacc, novf) == want[1:]
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("seed", range(4))
def test_accept_without_cap_equals_fold_at(seed):
    """file_cap = UINT64_MAX: exactly the frames val_crc32_fold_payload_states_at folds."""
    rng = np.random.default_rng(5000 + seed)
    for _ in range(300):
        n = int(rng.integers(0, 41))
        start = int(rng.choice([0, 77]))
        fo, pl, ok, _ = _sequence(rng, n, start)
        pay = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        _, w_fold, n_fold = vc.fold_payload_states_at(0xFFFFFFFF, pay, pl, fo, start, ok)
        dst, w, nacc, novf = wire.frame_accept(fo, pl, start, U64, ok)
        assert (w, nacc, novf) == (w_fold, n_fold, 0)
        # and the fold over the accepted frames alone, all in order, is the same state
        a = dst != NOT_ACCEPTED
        s_at, _, _ = vc.fold_payload_states_at(0xFFFFFFFF, pay, pl, fo, start, ok)
        s_in, _ = vc.fold_payload_states(0xFFFFFFFF, pay[a], pl[a])
        assert s_at == s_in


def test_no_wrap_around_near_2_64():
    """eff + pay_len past 2^64 is an overflow, never a small number."""
    w0 = U64 - 19
    NA = NOT_ACCEPTED
    fo = np.array([w0, IMPLIED, IMPLIED, w0 + 9], dtype=np.uint64)
    pl = np.array([30, 20, 9, 11], dtype=np.uint32)
    for cap, want in ((U64, ([NA, NA, w0, NA], w0 + 9, 1, 3)),  # the last one: 10 bytes left, 11 wanted
                      (w0 + 8, ([NA] * 4, w0, 0, 3)),            # the last one is a gap here, not an overflow
                      (5, ([NA] * 4, w0, 0, 3))):                # written already past the capacity
        dst, w, nacc, novf = wire.frame_accept(fo, pl, w0, cap)
        assert (list(map(int, dst)), w, nacc, novf) == want, cap
    # exactly up to 2^64 - 1 fits
    dst, w, nacc, novf = wire.frame_accept(fo[2:], np.array([9, 10], np.uint32), w0, U64)
    assert (list(map(int, dst)), w, nacc, novf) == ([w0, w0 + 9], U64, 2, 0)


def test_nothing_and_nulls():
    dst, w, nacc, novf = wire.frame_accept(np.zeros(0, np.uint64), np.zeros(0, np.uint32), 123, 50)
    assert dst.size == 0 and (w, nacc, novf) == (123, 0, 0)
