#!/usr/bin/env python3
"""Send windows of transfers whose files lie in HBM: the device window fill
against the route there was before it and against the framer alone, same box,
same process, same bytes.

Side A: one val_frame_fill_files_dev call (outputs and workspace allocated
before the clock starts; d_next is put back by a device copy in front of the
clock).
Side B: the route before it: the host's val_frame_fill_window per transfer into
pinned arrays, the five descriptor arrays uploaded (H2D), then
val_frame_data_batch_dev.
Side C: val_frame_data_batch_dev alone with B's descriptors already resident:
the floor, and the figure tools/timing_pack.py reports for its shapes. It is
timed into B's output buffer and again into A's: the same launch runs at
slightly different speeds into different allocations, and A minus C into A's
own buffer is the cost of the planning launches.
Every side is timed by device events around its calls and by the host clock
from the first call to the end of a synchronise; B's host work lies between
its two events, so both clocks count it.

Shapes (every frame full, the first of each transfer explicit): 1 transfer of
65,535 frames of 16 KiB; 256 transfers of 64 frames of 1,024 B; 16 transfers of
4,096 frames of 16 KiB. At least 100 ms of warm-up, then the sides alternate;
medians, with the minimum and maximum of each. After the warm-up A's wire bytes
and trailers are checked against B's. A's kernels are reported from a separate
profiled pass of calls back to back (null when the profiler is not available).
Prints one JSON object; --out also writes it. Needs a GPU.

usage: timing_fill.py [--iters 24] [--out profiles/fill_timing.json]"""
import argparse
import ctypes
import json
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import val_protocol_amd.crc as vc  # noqa: E402
import val_protocol_amd.wire as wire  # noqa: E402
from timing_unpack import random_bytes  # noqa: E402
from val_protocol_amd import _build  # noqa: E402

KERNELS = (("count_ms", "k_fill_count"), ("first_ms", "k_scan_first"), ("desc_ms", "k_fill_desc"),
           ("pack_ms", "k_pack"))


def kernel_times(fn, reps=5):
    """Mean device time per call of A's kernels, in ms."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {k: 0.0 for k, _ in KERNELS}
        for e in prof.events():
            t = getattr(e, "device_time", None)
            if t is None:
                t = getattr(e, "cuda_time", 0.0)
            for key, name in KERNELS:
                if name in e.name:
                    out[key] += t
        if not any(out.values()):
            return None
        return {k: round(v / reps / 1000.0, 4) for k, v in out.items()}
    except Exception:  # noqa: BLE001 - the figures are optional
        return None


def med(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def shape(name, S, per, mtu, iters, dev):
    M = mtu - 12
    size = per * M - 8  # `per` full frames, the first explicit
    n = S * per
    room = per * mtu
    files = random_bytes(S * size, dev)
    fpos = torch.arange(S, dtype=torch.int64, device=dev) * size
    fsize = torch.full((S,), size, dtype=torch.int64, device=dev)
    zero = torch.zeros(S, dtype=torch.int64, device=dev)
    nxt = torch.zeros(S, dtype=torch.int64, device=dev)
    soff = torch.arange(S, dtype=torch.int64, device=dev) * room
    cap = torch.full((S,), room, dtype=torch.int64, device=dev)
    out_a = torch.zeros(S * room + 8, dtype=torch.uint8, device=dev)
    out_b = torch.zeros(S * room + 8, dtype=torch.uint8, device=dev)
    slen = torch.empty(S, dtype=torch.int64, device=dev)
    nfr = torch.empty(S, dtype=torch.int32, device=dev)
    first = torch.empty(S + 1, dtype=torch.int32, device=dev)
    foff = torch.empty(n, dtype=torch.int64, device=dev)
    clen_a, crc_a = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    clen_b, crc_b = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    work = torch.empty(wire.fill_work_bytes(S, per), dtype=torch.uint8, device=dev)
    lib = vc.lib()
    cur = torch.cuda.current_stream().cuda_stream

    def side_a():
        st = lib.val_frame_fill_files_dev(files.data_ptr(), fpos.data_ptr(), fsize.data_ptr(), nxt.data_ptr(),
                                          zero.data_ptr(), None, S, mtu, per, out_a.data_ptr(), soff.data_ptr(),
                                          cap.data_ptr(), slen.data_ptr(), nfr.data_ptr(), first.data_ptr(),
                                          foff.data_ptr(), clen_a.data_ptr(), crc_a.data_ptr(), None, work.data_ptr(),
                                          work.numel(), cur)
        assert st == vc.VAL_OK, vc.last_error()

    # side B: pinned descriptor arrays, the host's rule per transfer, the uploads, the framer
    h = dict(pay_off=torch.empty(n, dtype=torch.int64, pin_memory=True),
             file_off=torch.empty(n, dtype=torch.int64, pin_memory=True),
             frame_off=torch.empty(n, dtype=torch.int64, pin_memory=True),
             pay_len=torch.empty(n, dtype=torch.int32, pin_memory=True),
             inc=torch.empty(n, dtype=torch.uint8, pin_memory=True))
    d = {k: torch.empty(n, dtype=v.dtype, device=dev) for k, v in h.items()}
    hv = {k: v.numpy() for k, v in h.items()}
    nf, used, new = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def pack(out=out_b):
        st = lib.val_frame_data_batch_dev(files.data_ptr(), d["pay_off"].data_ptr(), d["pay_len"].data_ptr(),
                                          d["file_off"].data_ptr(), d["inc"].data_ptr(), n, out.data_ptr(),
                                          d["frame_off"].data_ptr(), 0, mtu - 4, clen_b.data_ptr(), crc_b.data_ptr(),
                                          None, None, cur)
        assert st == vc.VAL_OK, vc.last_error()

    def side_b():
        k = 0
        for s in range(S):
            lib.val_frame_fill_window(0, 0, size, mtu, per, room, h["file_off"].data_ptr() + 8 * k,
                                      h["pay_len"].data_ptr() + 4 * k, h["inc"].data_ptr() + k,
                                      h["frame_off"].data_ptr() + 8 * k, None, ctypes.byref(nf), ctypes.byref(used),
                                      ctypes.byref(new))
            hv["pay_off"][k:k + nf.value] = hv["file_off"][k:k + nf.value] + s * size
            hv["frame_off"][k:k + nf.value] += s * room
            k += nf.value
        assert k == n
        for key in d:
            d[key].copy_(h[key], non_blocking=True)
        pack()

    def timed(fn, before=None):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, e0.elapsed_time(e1)

    reset = lambda: nxt.zero_()  # noqa: E731
    turn = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1 or turn < 2:
        reset()
        side_a()
        side_b()
        pack()
        torch.cuda.synchronize()
        turn += 1
    assert torch.equal(out_a, out_b) and torch.equal(crc_a, crc_b) and torch.equal(clen_a, clen_b)
    assert torch.equal(foff, d["frame_off"]) and int(first[-1].item()) == n and bool((nxt == size).all())
    assert bool((slen == room).all()) and bool((nfr == per).all())
    a, b, c, ca = [], [], [], []
    for _ in range(iters):
        a.append(timed(side_a, reset))
        b.append(timed(side_b))
        c.append(timed(pack))
        ca.append(timed(lambda: pack(out_a)))
    reset()
    kern = kernel_times(lambda: (reset(), side_a()))
    wall = lambda xs: med([x[0] for x in xs])  # noqa: E731
    event = lambda xs: med([x[1] for x in xs])  # noqa: E731
    res = {"shape": name, "transfers": S, "frames_per_transfer": per, "frames": n, "mtu": mtu, "wire_bytes": S * room,
           "calls_per_side": iters, "lanes_for_len_hint": int(lib.val_gpu_lanes_per_frame(mtu - 4)),
           "a_fill_dev_event": event(a), "a_fill_dev_wall": wall(a),
           "b_host_rule_upload_pack_event": event(b), "b_host_rule_upload_pack_wall": wall(b),
           "c_pack_resident_event": event(c), "c_pack_resident_wall": wall(c),
           "c_into_a_buffer_event": event(ca), "c_into_a_buffer_wall": wall(ca),
           "a_minus_c_event_ms": round(event(a)["median_ms"] - event(c)["median_ms"], 4),
           "a_minus_c_wall_ms": round(wall(a)["median_ms"] - wall(c)["median_ms"], 4),
           "a_minus_c_into_a_buffer_event_ms": round(event(a)["median_ms"] - event(ca)["median_ms"], 4),
           "b_over_a_wall": round(wall(b)["median_ms"] / wall(a)["median_ms"], 2),
           "c_bytes_per_s": int(S * room * 2 / (event(c)["median_ms"] * 1e-3)),
           "a_kernels_back_to_back": kern}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.iters < 8:
        ap.error("--iters must be at least 8")
    if not torch.cuda.is_available():
        sys.exit("timing_fill.py: no GPU (there is no CPU side)")
    vc.init(0)
    dev = torch.device("cuda:0")
    shapes = [shape("1x65535_16KiB", 1, 65535, 16388, args.iters, dev),
              shape("256x64_1024B", 256, 64, 1024, args.iters, dev),
              shape("16x4096_16KiB", 16, 4096, 16388, args.iters, dev)]
    res = {"tool": "tools/timing_fill.py", "device": torch.cuda.get_device_name(0),
           "tree": os.environ.get("VAL_TREE") or "sources " + _build.source_hash()[:12], "box": socket.gethostname(),
           "times": "medians with minimum and maximum; *_event: device events around the side's calls; *_wall: host "
                    "clock from the first call to the end of a synchronise; c_bytes_per_s: payload read plus wire "
                    "written over c's event time; a_kernels_back_to_back: mean kernel durations of a profiled pass "
                    "of consecutive calls",
           "shapes": shapes}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
