"""Seeded fuzz of the ragged path against the oracle. The rounds
are drawn by tests/_ragged_shapes.py fuzz_rounds without a device, so
tests/test_launch_plan.py can check what the default seed reaches for 64, 128,
256 and 304 CUs; here every round is asserted to plan as one ragged launch
with the restated grid, runs into pre-filled outputs, and is compared with
tests/_oracle.py over the host copy of the same bytes."""
import numpy as np
import pytest
import torch

from tests import _oracle
from tests import _ragged_shapes as shapes
from tests.test_gpu_ragged_edges import (NBAD0, _d32, _d64, _filled, _filled8, _flip, _random, _sentinel,
                                         _store_trailers, _u32, _want_states)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    import val_protocol_amd.crc as vc

    vc.init(0)
    yield vc
    vc.set_geometry()
    vc.set_ragged_min_frames(-1)


def test_ragged_fuzz(vc):
    """FUZZ_RAGGED_ROUNDS (60) batches through the binned path, each of at most 32 MiB: n log-uniform
    in 1..40,000, class weights with zeros, runs of 1..300 equal lengths weighted to the bucket and
    class edges +- 1, now and then one length only, many short class-1 frames, or a few frames of up
    to 2 MiB; packed with gaps of 0..7 bytes, listed in a permutation, or as views into a pool; CRC
    and header_crc, verify with none to four flipped bits, or verify_frames_ex with payload states.
    FUZZ_SEED reseeds it. At the default rounds it asserts what the rounds reached."""
    cus, seed = torch.cuda.get_device_properties(0).multi_processor_count, shapes.fuzz_seed()
    rounds = shapes.fuzz_rounds(cus)
    ran = 0
    with shapes.binned(vc):
        for r, c in enumerate(rounds):
            n, lens, offs = c["n"], c["lens"], c["offs"]
            case = (f"seed {seed} round {r}: n={n} {c['layout']} {c['mode']} classes={c['classes']} grid={c['grid']} "
                    f"items={c['items']} one_bucket={c['one_bucket']} bad={c['bad']}")
            assert shapes.ragged_plan(vc, cus, n, want_payload=c["mode"] == "ex") == c["grid"], case
            d, host = _random(c["total"], seed + r)
            want, want_h = _oracle.frames(host, offs, lens, header=True, nthreads=16)
            d_off, d_len = _d64(offs), _d32(lens)
            ran += 1
            if c["mode"] == "crc":
                crc, hdr = _filled(n), _filled(n)
                vc.frames(d, off=d_off, length=d_len, len_hint=0, out_crc=crc, out_hdr=hdr)
                assert np.array_equal(_u32(crc), want), case
                assert np.array_equal(_u32(hdr), want_h), case
                continue
            _store_trailers(d, host, offs, lens, want)
            if c["bad"]:
                _flip(d, host, [int(offs[f]) + p for f, p, _ in c["bad"]], [b for _, _, b in c["bad"]])
            want_ok, want_bad = _oracle.verify_frames(host, offs, lens, nthreads=16)
            assert set(np.flatnonzero(want_ok == 0)) == set(f for f, _, _ in c["bad"]), case
            ok, nbad = _filled8(n), _sentinel()
            if c["mode"] == "ex":
                pay = _filled(n)
                vc.verify_frames_ex(d, off=d_off, length=d_len, len_hint=0, out_ok=ok, nbad=nbad, out_pay=pay)
                assert np.array_equal(_u32(pay), _want_states(host, offs, lens)), case
            else:
                vc.verify_frames(d, off=d_off, length=d_len, len_hint=0, out_ok=ok, nbad=nbad)
            assert int(nbad.item()) == NBAD0 + want_bad, case
            assert np.array_equal(ok.cpu().numpy(), want_ok), case
    assert ran == len(rounds)  # a round is never skipped
    print(f"ragged fuzz: {len(rounds)} rounds, {sum(c['n'] for c in rounds)} frames, "
          f"{sum(int(c['lens'].astype(np.int64).sum()) for c in rounds) >> 20} MiB, P "
          f"{sorted(set(c['P'] for c in rounds))}, most items {max(c['items'] for c in rounds)}", flush=True)
    if len(rounds) >= shapes.FUZZ_DEFAULT_ROUNDS and seed == shapes.FUZZ_DEFAULT_SEED:
        shapes.fuzz_coverage(rounds, cus)
