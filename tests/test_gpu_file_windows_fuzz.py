"""Seeded differential test of val_crc32_file_windows_dev against the oracle's
CRC-32 of the host copy of every window and the header's validity rule in
Python (tests/test_gpu_file_windows.py: _want). The resume calls have their own
fuzz in tests/test_gpu_resume.py; its windows are tails of short files, here they
lie anywhere in files that are views into one pool and share bytes.

Expected values never come from a device path. The function asserts, from the
reference side alone (the Python chunk counts and vc.plan_file_windows), that
its rounds reached the cases it is there for.

Seeded: every assertion message names the seed, the round and its shape.
FUZZ_SEED and FUZZ_WINDOW_ROUNDS mean what they mean in
tests/test_gpu_window_fuzz.py. At the default the function runs FILE_SHARE
rounds, which take 1.3 s on an MI355X (most of it the oracle's)."""
import numpy as np
import pytest

from tests import _prng
from tests.test_gpu_file_windows import U64, VAL_OK, Win, _u32, _valid, _want
from tests.test_gpu_unpack import DEV, _d64, vc, wire  # noqa: F401 - vc and wire are fixtures
from tests.test_gpu_window_fuzz import SEED, _case, _covered, _rounds

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILE_SHARE = 1000
K0S = (0, 12, 13, 14, 15, 16)
REFUSALS = ("past", "wraps", "long", "behind")
BUDGET = 3 << 19  # window bytes of a round: the oracle hashes them on one core
POOL = 3 << 20


@pytest.fixture(autouse=True)
def _automatic_chunk(vc):
    yield
    vc.set_file_window_chunk(0)


def _refusal(w, max_len):
    """Why the header's rule refuses a window (None: it does not)."""
    if _valid(w, max_len):
        return None
    if w["len"] > max_len:
        return "long"
    if w["off"] + w["len"] > U64:
        return "wraps"
    return "behind" if w["off"] > w["data"].size else "past"


def _round(rng, vc, cus, pool):
    """1 to 80 files as views into the pool -> (k0 forced, k0 used, max_len, starts, wins)."""
    S = int(rng.integers(1, 81))
    forced = int(rng.choice(K0S))
    Wg = 1 << (forced or 13)
    max_len = int(rng.choice([40 * Wg, 18 * Wg + 5, 3 * Wg, 100]))
    vc.set_file_window_chunk(forced)
    plan = vc.plan_file_windows(cus, S, max_len)
    k0 = plan[2].k0
    assert len(plan) == 3 and plan[0].k0 == k0 and (forced == 0 or k0 == forced)
    W = 1 << k0
    left = BUDGET
    starts, wins = [], []
    for _ in range(S):
        r = rng.random()
        if r < 0.10:
            length = 0
        elif r < 0.18:
            length = int(rng.integers(1, 4))
        elif r < 0.40 or left <= 0:
            length = int(rng.integers(4, 64))
        elif r < 0.60:
            length = int(rng.integers(64, W))
        elif r < 0.85:
            length = int(rng.integers(W, 4 * W))
        elif r < 0.95:
            length = W * int(rng.choice([1, 2, 16, 17])) + int(rng.integers(-1, 2))
        else:
            length = int(rng.integers(17 * W, 40 * W))
        if length > max(left, 64):
            length = int(rng.integers(4, 64))
        off, slack = int(rng.integers(0, 300)), int(rng.integers(0, 70))
        size = off + length + slack
        r = rng.random()
        if r < 0.03:  # off + len one past the file
            off += slack + 1
        elif r < 0.06:  # off + len wraps
            off, length = U64 - int(rng.integers(0, 7)), max(length, 8)
        elif r < 0.09:  # inside the file, above max_len
            length = max_len + 1 + int(rng.integers(0, 3))
            size = off + length + slack
        elif r < 0.12:  # an empty window behind the file, or one at its end
            off, length = size + int(rng.integers(0, 2)), 0
        elif r < 0.15:  # a window that ends with the file
            size = off + length
        start = int(rng.integers(0, pool.size - size + 1))
        starts.append(start)
        wins.append(Win(pool[start:start + size], off, length))
        if _valid(wins[-1], max_len):
            left -= length
    return forced, k0, max_len, starts, wins


def test_fuzz_file_windows(vc, wire):
    """file_windows_dev against _want: every forced chunk and the automatic one, max_len at and below
    the windows, starts and ends of every alignment mod 64, files that overlap in memory, each kind of
    refused window, d_status given and left out, a garbage-filled workspace that two rounds share."""
    rng = np.random.default_rng(SEED + 6)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pool = _prng.prng_bytes(0xF11E, POOL)
    d_pool = torch.from_numpy(pool).to(DEV)
    base = d_pool.data_ptr()
    shared = torch.empty(wire.file_windows_work_bytes(80) + 24, dtype=torch.uint8, device=DEV)
    share = 0
    seen = dict(k0=set(), refused=set(), head=set(), tail=set(), end_empty=0, tiny=0, long_file=0, ragged=0, shared=0)
    for r in range(_rounds(FILE_SHARE)):
        forced, k0, max_len, starts, wins = _round(rng, vc, cus, pool)
        want_status = bool(rng.integers(0, 4))
        if share == 0 and rng.random() < 0.2:
            shared.fill_(0xA5)
            share = 2  # this round and the next: the second finds what the first left
        work = shared if share else None
        share = max(share - 1, 0)
        case = (f"seed {SEED + 6} round {r} files={len(wins)} chunk={forced} (2^{k0}) max_len={max_len} "
                f"status={want_status} shared_work={work is not None}")
        want_crc, status = _want(wins, max_len)
        # what this round reaches, from the reference side alone
        ok = status == VAL_OK
        cnt = np.array([-(-w["len"] // (1 << k0)) if v else 0 for w, v in zip(wins, ok)])
        seen["k0"].add(forced)
        seen["refused"] |= {_refusal(w, max_len) for w in wins} - {None}
        seen["head"] |= {(s + w["off"]) % 64 for s, w, v in zip(starts, wins, ok) if v and w["len"]}
        seen["tail"] |= {(s + w["off"] + w["len"]) % 64 for s, w, v in zip(starts, wins, ok) if v and w["len"]}
        seen["end_empty"] += sum(v and w["len"] == 0 and w["off"] == w["data"].size for w, v in zip(wins, ok))
        seen["tiny"] += sum(v and 0 < w["len"] < 4 for w, v in zip(wins, ok))
        seen["long_file"] += int((cnt > 16).sum())
        seen["ragged"] += int(cnt.sum() % 16 != 0)
        seen["shared"] += work is not None
        crc, st = wire.file_windows_dev(_d64(np.array([base + s for s in starts], dtype=np.uint64)),
                                        _d64(np.array([w["data"].size for w in wins], dtype=np.uint64)),
                                        _d64(np.array([w["off"] for w in wins], dtype=np.uint64)),
                                        _d64(np.array([w["len"] for w in wins], dtype=np.uint64)), max_len,
                                        want_status=want_status, work=work)
        torch.cuda.synchronize()
        with _case(case):
            bad = np.flatnonzero(_u32(crc) != want_crc)
            assert bad.size == 0, ("files", bad[:8].tolist(), [(wins[i]["off"], wins[i]["len"]) for i in bad[:8]])
            assert (st is None) == (not want_status)
            assert st is None or np.array_equal(st.cpu().numpy(), status)
    print(f"file windows: {_rounds(FILE_SHARE)} rounds, files of more than 16 chunks {seen['long_file']}, windows "
          f"under 4 bytes {seen['tiny']}, empty at the file's end {seen['end_empty']}, rounds with a partial last "
          f"step {seen['ragged']}, on the shared workspace {seen['shared']}", flush=True)
    if _covered(FILE_SHARE):
        what = f"seed {SEED + 6}"
        assert seen["k0"] == set(K0S) and seen["refused"] == set(REFUSALS), (what, seen["k0"], seen["refused"])
        assert seen["head"] == set(range(64)) and seen["tail"] == set(range(64)), (what, "alignments mod 64")
        for k in ("end_empty", "tiny", "long_file", "ragged", "shared"):
            assert seen[k] >= 1, (what, k)
