"""val_frame_data_layout (include/val_wire.h): where val_frame_data_batch puts
each frame, computed without writing one. The device framer
(val_frame_data_batch_dev) places its frames by it, so the two must agree
with the host framer on every length, and refuse what it refuses. No GPU."""
import numpy as np
import pytest

import val_protocol_amd.crc as vc
import val_protocol_amd.wire as wire


def _lengths(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    pools = [np.arange(0, 71), np.arange(1003, 1014), np.arange(65519, 65536)]
    pick = rng.integers(0, 3, n)
    return np.array([rng.choice(pools[k]) for k in pick], dtype=np.uint32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_layout_equals_host_framer(seed):
    rng = np.random.default_rng(100 + seed)
    pay_len = _lengths(seed, 200)
    inc = rng.integers(0, 2, pay_len.size).astype(np.uint8)
    inc[pay_len > 65527] = 0  # an explicit frame holds at most 65527 payload bytes
    assert inc.any() and not inc.all() and (pay_len > 65527).any() and (pay_len < 4).any()
    pay_off = np.concatenate([[0], np.cumsum(pay_len)[:-1]]).astype(np.uint64)
    payload = rng.integers(0, 256, int(pay_len.sum()), dtype=np.uint8)
    stream, fo, cl = wire.build_data_batch(payload, pay_off, pay_len, pay_off, inc)
    fo2, cl2, total = wire.data_layout(pay_len, inc)
    assert np.array_equal(fo, fo2) and np.array_equal(cl, cl2) and total == stream.size
    assert fo2.dtype == np.uint64 and cl2.dtype == np.uint32
    # include_offset = None: every frame explicit
    small = pay_len[pay_len <= 65527]
    off_s = np.concatenate([[0], np.cumsum(small)[:-1]]).astype(np.uint64)
    stream, fo, cl = wire.build_data_batch(payload, off_s, small, off_s)
    fo2, cl2, total = wire.data_layout(small)
    assert np.array_equal(fo, fo2) and np.array_equal(cl, cl2) and total == stream.size


def test_layout_of_nothing():
    fo, cl, total = wire.data_layout(np.zeros(0, dtype=np.uint32))
    assert fo.size == 0 and cl.size == 0 and total == 0


@pytest.mark.parametrize("plen,explicit", [(65528, 1), (65536, 0)])
def test_layout_and_framer_refuse_the_same(plen, explicit):
    pay_len = np.array([10, plen, 10], dtype=np.uint32)
    inc = np.array([1, explicit, 0], dtype=np.uint8)
    pay_off = np.zeros(3, dtype=np.uint64)
    payload = np.zeros(plen, dtype=np.uint8)
    with pytest.raises(vc.ValError) as e:
        wire.data_layout(pay_len, inc)
    assert e.value.status == vc.VAL_ERR_INVALID_ARG
    with pytest.raises(vc.ValError) as e:
        wire.build_data_batch(payload, pay_off, pay_len, pay_off, inc)
    assert e.value.status == vc.VAL_ERR_INVALID_ARG
    # one byte less is the largest frame both accept
    pay_len[1] -= 1
    stream, fo, cl = wire.build_data_batch(payload, pay_off, pay_len, pay_off, inc)
    fo2, cl2, total = wire.data_layout(pay_len, inc)
    assert np.array_equal(fo, fo2) and np.array_equal(cl, cl2) and total == stream.size and cl[1] == 8 + 65535
