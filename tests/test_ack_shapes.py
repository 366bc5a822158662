"""The shapes of tests/test_gpu_acks_edges.py (tests/_ack_shapes.py) on 64, 128,
256 and 304 CUs, without a GPU: each must get the plan its GPU test asserts,
more files than twice the grid with the long files in the workgroups the test
means, and long files whose frames reach every slot and the second step of
k_ack_respond_files' first pass. A threshold that moves in launch_plan.hpp
fails here."""
import pytest

import val_protocol_amd.crc as vc
from tests import _ack_shapes as shp

CUS = (64, 128, 256, 304)


@pytest.mark.parametrize("lanes", (1024, 256))
@pytest.mark.parametrize("cus", CUS)
def test_shared_respond_shapes(cus, lanes):
    counts, n_pad, grid, longs = shp.shared_respond(vc, cus, lanes)
    S, n = len(counts), int(counts.sum())
    assert grid == (cus if lanes == 1024 else 8 * cus) and S == 2 * grid + 3 > 2 * grid
    shp.check_shared(counts, grid, longs, shp.CHUNK[lanes], shp.SHARED_LONG[lanes])
    plan = vc.plan_ack_calls(vc.ACK_RESPOND, cus, n + n_pad, S)
    assert (plan[1].lanes, plan[1].grid) == (lanes, grid)
    if lanes == 1024:  # padding alone decides the workgroup size: the frames are few
        assert n_pad > 0 and (n + n_pad) // S > 256 >= n // S
    else:
        assert n_pad == 0 and n // S <= 256
    # k_unpack_order_files runs the same window in one workgroup per CU: there too a workgroup takes a
    # long file and further files behind and in front of it
    og = shp.order_grid(vc, cus, n + n_pad, S)
    assert og == cus and S > 2 * og
    assert any(s - og >= 0 and s + og < S for s in longs) and any(s < og for s in longs)


@pytest.mark.parametrize("cus", CUS)
def test_shared_apply_shape(cus):
    counts, grid, longs = shp.shared_apply(vc, cus)
    assert grid == cus and len(counts) == 2 * grid + 3
    shp.check_shared(counts, grid, longs, 1024, (2049, 1025, 4097, 1024))
    assert set(shp.SHARED_APPLY_LONG) <= set(longs.values())


@pytest.mark.parametrize("lanes", (1024, 256))
@pytest.mark.parametrize("cus", CUS)
def test_pass1_shapes(cus, lanes):
    files, fill = shp.pass1_shape(vc, cus, lanes)
    S = len(files) + fill
    n = sum(f[0] for f in files) + fill
    plan = vc.plan_ack_calls(vc.ACK_RESPOND, cus, n, S)
    assert plan[1].lanes == lanes
    assert (fill == 0) == (lanes == 1024)
    shp.check_pass1(lanes)
    block = shp.CHUNK[lanes]
    for count, what, i in files:
        if what.startswith("u"):
            assert shp.pass1_slot(i, block) == (0, int(what[1])), (count, what, i)


def test_pass1_slots():
    assert shp.pass1_slot(1023, 1024) is None and shp.pass1_slot(1024, 1024) == (0, 0)
    assert shp.pass1_slot(2048, 1024) == (0, 1)  # the one frame a file of 2,049 puts into slot 1
    assert shp.pass1_slot(5119, 1024) == (0, 3) and shp.pass1_slot(5120, 1024) == (1, 0)
    assert shp.pass1_slot(1280, 256) == (1, 0) and shp.pass1_slot(2304, 256) == (2, 0)
