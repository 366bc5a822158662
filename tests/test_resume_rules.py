"""The three rules of a VAL_RESUME_TAIL handshake in plain C
(include/val_wire.h: val_resume_tail_window, val_resume_request_window,
val_resume_verdict), pinned against a Python restatement kept here over the
edges of every input, and against the three resumed reference sessions of
tests/golden/session_vectors.json: every action, offset, length and verdict
that crossed the wire there follows from the rules. No GPU."""
import itertools

import pytest

import val_protocol_amd.crc as vc
import val_protocol_amd.wire as wire
from tests import _oracle, _sessions

U64 = (1 << 64) - 1
MIB = 1 << 20
START_ZERO, VERIFY_FIRST, SKIP_FILE = 0, 2, 3
VAL_OK, VAL_SKIPPED, VAL_ERR_RESUME_VERIFY = 0, 1, -7


def py_tail(existing, incoming, tail_cap, min_verify, skip):
    """src/val_receiver.c:119-181, TAIL mode -> (action, resume_offset, verify_len)."""
    if existing == 0:
        return START_ZERO, 0, 0
    if existing > incoming:
        return (SKIP_FILE if skip else START_ZERO), 0, 0
    cap = min(max(tail_cap if tail_cap else 8 * MIB, 1), 256 * MIB)
    vlen = min(existing, cap)
    if min_verify > 0 and vlen < min_verify:
        vlen = min(existing, min_verify)
    return VERIFY_FIRST, existing, vlen


def py_request(resume_off, verify_len):
    """src/val_sender.c:208-215 -> (send, start, vlen32)."""
    v32 = min(verify_len, resume_off) & 0xFFFFFFFF
    return v32 != 0, resume_off - v32, v32


def py_verdict(window_ok, local, sender, skip, rec_off, file_size):
    """src/val_receiver.c:689-721 -> (result, resume_off)."""
    if window_ok and local == sender:
        return VAL_OK, rec_off
    return (VAL_SKIPPED, file_size) if skip else (VAL_ERR_RESUME_VERIFY, 0)


CAPS = (0, 1, 1024, 8 * MIB, 256 * MIB, 256 * MIB + 1, (1 << 32) - 1, U64)


def _existing_edges(cap_arg):
    cap = min(max(cap_arg if cap_arg else 8 * MIB, 1), 256 * MIB)
    return sorted({0, 1, 2, max(cap - 1, 0), cap, cap + 1, 1 << 32, (1 << 32) + 5, U64 - 1, U64})


def test_symbols_and_constants():
    for name in ("val_resume_tail_window", "val_resume_request_window", "val_resume_verdict"):
        assert hasattr(vc.lib(), name) and name in vc.EXPORTS
    for name in ("resume_tail_window", "resume_request_window", "resume_verdict"):
        assert name in wire.__all__ and callable(getattr(wire, name))


@pytest.mark.parametrize("cap_arg", CAPS)
def test_tail_window_edges(cap_arg):
    cap = min(max(cap_arg if cap_arg else 8 * MIB, 1), 256 * MIB)
    min_verifies = (0, 1, max(cap - 1, 0), cap, cap + 1, 4 * cap + 3, 1 << 33, U64)
    n = 0
    for existing in _existing_edges(cap_arg):
        incomings = sorted({0, max(existing - 1, 0), existing, min(existing + 1, U64), U64})
        for incoming, mv, skip in itertools.product(incomings, min_verifies, (False, True)):
            got = wire.resume_tail_window(existing, incoming, cap_arg, mv, skip)
            assert got == py_tail(existing, incoming, cap_arg, mv, skip), (existing, incoming, cap_arg, mv, skip)
            action, off, vlen = got
            if action == VERIFY_FIRST:
                assert off == existing and 1 <= vlen <= existing <= incoming
            else:
                assert (off, vlen) == (0, 0)
            n += 1
    assert n > 300


def test_tail_window_named_cases():
    t = wire.resume_tail_window
    assert t(0, 100) == (START_ZERO, 0, 0)
    assert t(101, 100) == (START_ZERO, 0, 0) and t(101, 100, mismatch_skip=True) == (SKIP_FILE, 0, 0)
    assert t(100, 100) == (VERIFY_FIRST, 100, 100)  # equal sizes still verify
    assert t(9 * MIB, 10 * MIB) == (VERIFY_FIRST, 9 * MIB, 8 * MIB)  # tail_cap_bytes 0 -> 8 MiB
    assert t(5, 10, tail_cap_bytes=1) == (VERIFY_FIRST, 5, 1)
    assert t(1 << 30, 1 << 31, tail_cap_bytes=(1 << 32) - 1) == (VERIFY_FIRST, 1 << 30, 256 * MIB)  # clamp
    assert t(5000, 9000, tail_cap_bytes=1024, min_verify_bytes=512) == (VERIFY_FIRST, 5000, 1024)  # below the cap
    assert t(5000, 9000, tail_cap_bytes=1024, min_verify_bytes=4096) == (VERIFY_FIRST, 5000, 4096)  # above the cap
    assert t(5000, 9000, tail_cap_bytes=1024, min_verify_bytes=8192) == (VERIFY_FIRST, 5000, 5000)  # above existing
    assert t(U64, U64, tail_cap_bytes=U64, min_verify_bytes=U64) == (VERIFY_FIRST, U64, U64)
    # nullable outputs
    assert vc.lib().val_resume_tail_window(100, 100, 0, 0, 0, None, None) == VERIFY_FIRST


def test_request_window_edges():
    values = (0, 1, 2, 1023, 1024, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 33) + 7, U64 - 1, U64)
    for roff, vlen in itertools.product(values, values):
        assert wire.resume_request_window(roff, vlen) == py_request(roff, vlen), (roff, vlen)
    r = wire.resume_request_window
    assert r(300005, 1024) == (True, 298981, 1024)
    assert r(100, 1024) == (True, 0, 100)  # resume_offset < verify_len
    assert r(0, 1024) == (False, 0, 0) and r(77, 0) == (False, 77, 0)
    assert r(1 << 40, 1 << 32) == (False, 1 << 40, 0)  # the reference's truncation: 2^32 asks for nothing
    assert r(1 << 40, (1 << 32) + 5) == (True, (1 << 40) - 5, 5)
    assert r(U64, U64) == (True, U64 - 0xFFFFFFFF, 0xFFFFFFFF)
    assert vc.lib().val_resume_request_window(300005, 1024, None, None) == 1


def test_verdict_edges():
    crcs = (0, 1, 0xDEADBEEF, 0xFFFFFFFF)
    offs = (0, 1, 300005, 1 << 40, U64)
    for ok, a, b, skip, roff, size in itertools.product((0, 1), crcs, crcs, (False, True), offs, offs):
        assert wire.resume_verdict(ok, a, b, skip, roff, size) == py_verdict(ok, a, b, skip, roff, size)
    v = wire.resume_verdict
    assert v(True, 5, 5, False, 300005, 400000) == (VAL_OK, 300005)
    assert v(True, 5, 5, True, 300005, 400000) == (VAL_OK, 300005)
    assert v(True, 5, 6, False, 300005, 400000) == (VAL_ERR_RESUME_VERIFY, 0)
    assert v(True, 5, 6, True, 300005, 400000) == (VAL_SKIPPED, 400000)
    assert v(False, 0, 0, False, 300005, 400000) == (VAL_ERR_RESUME_VERIFY, 0)  # a short read never matches
    assert v(False, 0, 0, True, 300005, 400000) == (VAL_SKIPPED, 400000)
    assert vc.lib().val_resume_verdict(1, 5, 5, 0, 300005, 400000, None) == VAL_OK


@pytest.fixture(scope="module")
def sessions():
    return _sessions.load()


@pytest.mark.parametrize("name", ["resume_tail_cap8m", "resume_tail_cap1k", "resume_tail_mismatch"])
def test_rules_reproduce_the_reference_sessions(sessions, name):
    s = sessions[name]
    c = _sessions.control(s, vc.lib())
    part, file = _sessions.receiver_existing(s), _sessions.input_file(s)
    # the receiver's proposal (the sessions ran with min_verify_bytes 0 and mismatch_skip 0)
    action, roff, vlen = wire.resume_tail_window(part.size, file.size, s["tail_cap_bytes"], 0, False)
    assert (action, roff, vlen) == (c["action"], c["resume_offset"], c["resp_verify_length"])
    assert action == VERIFY_FIRST and roff == s["existing"]
    assert _oracle.crc32(part[roff - vlen:roff]) == c["resp_verify_crc"]
    # the sender's request
    send, start, v32 = wire.resume_request_window(c["resume_offset"], c["resp_verify_length"])
    assert send and (start, v32) == (c["req_offset"], c["req_length"])
    assert _oracle.crc32(file[start:start + v32]) == c["req_crc"]
    # the receiver's verdict
    ok = c["req_offset"] + c["req_length"] <= part.size
    local = _oracle.crc32(part[c["req_offset"]:c["req_offset"] + c["req_length"]])
    assert ok and local == c["receiver_crc"]
    result, written = wire.resume_verdict(ok, local, c["req_crc"], False, c["resume_offset"], file.size)
    assert result == c["result"]
    assert result == (VAL_ERR_RESUME_VERIFY if s["flip"] >= 0 else VAL_OK)
    # the first DATA frame the sender put on the wire afterwards starts where the verdict says
    first = next(r for r in s["tx_frames"] if r[0] == _sessions.PKT_DATA)
    assert first[3] == written == (0 if s["flip"] >= 0 else s["existing"])
