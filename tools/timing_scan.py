#!/usr/bin/env python3
"""Frame boundaries of received streams that lie in HBM: the device scan
against the only route there was before it, same box, same process, same bytes.

Side A: one val_frame_scan_streams_dev call (outputs and workspace allocated
before the clock starts), with the width of the walk left to the library and
forced to 64 and to 1,024 lanes per stream. Timed twice: by device events
around the call, and by the host clock from the call to the end of a
synchronise.
Side B: the streams copied to pinned host memory (one D2H), the host's
val_frame_scan per stream, the descriptors and `first` copied back (H2D).
Host clock, from the start of the D2H to the end of the last H2D.

Shapes: one stream of 65,535 frames of 16 KiB (16,376 payload bytes); 256
streams of 512 frames of 1,100 wire bytes plus a short last frame; one stream
of 4,096 frames that alternate between 1,100 and 612 wire bytes (the bad case:
one frame per memory round trip). The frames are made on the device by
val_frame_data_batch_dev. At least 100 ms of warm-up, then the sides
alternate; medians. After the warm-up A's outputs are checked against B's.
Every timed A follows a B, whose copy leaves little of the streams in the
caches. The kernels of A are reported from a separate profiled pass of calls
back to back, which find the headers in the caches (null when the profiler is
not available), and for one-stream shapes the walk's time per round there, a
round being one dependent memory round trip of the front.
Prints one JSON object; --out also writes it. Needs a GPU.

usage: timing_scan.py [--iters 24] [--out profiles/scan_timing.json]"""
import argparse
import ctypes
import json
import os
import socket
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import val_protocol_amd.crc as vc  # noqa: E402
import val_protocol_amd.wire as wire  # noqa: E402
from timing_unpack import random_bytes  # noqa: E402
from val_protocol_amd import _build  # noqa: E402

MTU = 16388
FRONTS = (0, 64, 1024)  # val_gpu_set_scan_front: automatic, a wave per stream, a workgroup per stream


def kernel_times(fn, reps=5):
    """Mean device time per call of the scan kernels, in ms."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {"walk_ms": 0.0, "first_ms": 0.0, "compact_ms": 0.0}
        for e in prof.events():
            t = getattr(e, "device_time", None)
            if t is None:
                t = getattr(e, "cuda_time", 0.0)
            for key, name in (("walk_ms", "k_scan_streams"), ("first_ms", "k_scan_first"),
                              ("compact_ms", "k_scan_compact")):
                if name in e.name:
                    out[key] += t
        if not any(out.values()):
            return None
        return {k: round(v / reps / 1000.0, 4) for k, v in out.items()}
    except Exception:  # noqa: BLE001 - the figures are optional
        return None


def run_rounds(frames, front):
    """Rounds the walk takes through a run of equal frames: one for the first frame, then 64 lanes
    look, and every round in which all of them matched widens the next fourfold up to the front
    (the frame that ends the run is judged in the run's last round)."""
    rounds, left, act = 1, frames - 1, 64
    while left > 0:
        rounds += 1
        left -= min(act, left)
        act = min(act * 4, front)
    return rounds


def shape(name, S, wires, rounds, iters, dev):
    """S equal streams; `wires` the wire sizes of one stream's frames; `rounds` the walk's memory
    round trips per stream (None: not reported)."""
    wires = np.asarray(wires, dtype=np.int64)
    per = wires.size
    n = S * per
    stream_bytes = int(wires.sum())
    total = S * stream_bytes
    w = torch.from_numpy(np.tile(wires, S)).to(dev)
    pay_len = (w - 12).to(torch.int32)
    frame_off = torch.cumsum(w, 0) - w
    pay_off = torch.cumsum(w - 12, 0) - (w - 12)
    src = random_bytes(int((w - 12).sum().item()), dev)
    base = torch.zeros(total + 8, dtype=torch.uint8, device=dev)
    inc = torch.zeros(n, dtype=torch.uint8, device=dev)
    wire.build_data_batch_dev(src, pay_off, pay_len, torch.zeros(n, dtype=torch.int64, device=dev), inc, out=base,
                              frame_off=frame_off, len_hint=int(wires.max()) - 4)
    del src, pay_off, pay_len, inc, w
    max_frames = per
    soff = torch.arange(S, dtype=torch.int64, device=dev) * stream_bytes
    slen = torch.full((S,), stream_bytes, dtype=torch.int64, device=dev)
    foff = torch.empty(n, dtype=torch.int64, device=dev)
    clen = torch.empty(n, dtype=torch.int32, device=dev)
    first = torch.empty(S + 1, dtype=torch.int32, device=dev)
    nfr = torch.empty(S, dtype=torch.int32, device=dev)
    cons = torch.empty(S, dtype=torch.int64, device=dev)
    stat = torch.empty(S, dtype=torch.int32, device=dev)
    work = torch.empty(wire.scan_work_bytes(S, max_frames), dtype=torch.uint8, device=dev)
    lib = vc.lib()
    cur = torch.cuda.current_stream().cuda_stream

    def side_a():
        st = lib.val_frame_scan_streams_dev(base.data_ptr(), soff.data_ptr(), slen.data_ptr(), S, MTU, max_frames,
                                            foff.data_ptr(), clen.data_ptr(), first.data_ptr(), nfr.data_ptr(),
                                            cons.data_ptr(), stat.data_ptr(), work.data_ptr(), work.numel(), cur)
        assert st == vc.VAL_OK, vc.last_error()

    # side B: pinned landing buffers, the host's scan, the uploads
    h_base = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    h_off = torch.empty(n, dtype=torch.int64, pin_memory=True)
    h_len = torch.empty(n, dtype=torch.int32, pin_memory=True)
    h_first = torch.empty(S + 1, dtype=torch.int32, pin_memory=True)
    b_off = torch.empty(n, dtype=torch.int64, device=dev)
    b_len = torch.empty(n, dtype=torch.int32, device=dev)
    b_first = torch.empty(S + 1, dtype=torch.int32, device=dev)
    nf, used = ctypes.c_uint32(0), ctypes.c_size_t(0)

    def side_b():
        h_base.copy_(base[:total], non_blocking=True)
        torch.cuda.synchronize()
        k = 0
        h_first[0] = 0
        for s in range(S):
            at = s * stream_bytes
            lib.val_frame_scan(h_base.data_ptr() + at, stream_bytes, MTU, max_frames, h_off.data_ptr() + 8 * k,
                               h_len.data_ptr() + 4 * k, ctypes.byref(nf), ctypes.byref(used))
            h_off[k:k + nf.value] += at
            k += nf.value
            h_first[s + 1] = k
        b_off.copy_(h_off, non_blocking=True)
        b_len.copy_(h_len, non_blocking=True)
        b_first.copy_(h_first, non_blocking=True)
        torch.cuda.synchronize()

    turn = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1 or turn < 2:
        side_a()
        side_b()
        turn += 1
    assert torch.equal(foff, b_off) and torch.equal(clen, b_len) and torch.equal(first, b_first)
    assert int(first[-1].item()) == n and bool((cons == stream_bytes).all()) and not bool(stat.any())
    assert bool((nfr == per).all())
    ev, a_wall, b_wall = {f: [] for f in FRONTS}, {f: [] for f in FRONTS}, []
    for _ in range(iters):
        for f in FRONTS:  # every A directly behind a B, which leaves the streams' headers out of the caches
            vc.set_scan_front(f)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record()
            side_a()
            e1.record()
            torch.cuda.synchronize()
            a_wall[f].append((time.perf_counter() - t) * 1e3)
            ev[f].append((e0, e1))
            t = time.perf_counter()
            side_b()
            b_wall.append((time.perf_counter() - t) * 1e3)
    res = {"shape": name, "streams": S, "frames_per_stream": per, "frames": n, "stream_bytes": stream_bytes,
           "calls_per_side": iters, "b_d2h_host_scan_h2d_wall_ms": round(statistics.median(b_wall), 4),
           "b_min_ms": round(min(b_wall), 4), "b_max_ms": round(max(b_wall), 4), "a_by_front": {}}
    for f in FRONTS:
        vc.set_scan_front(f)
        a_dev = [x.elapsed_time(y) for x, y in ev[f]]
        kern = kernel_times(side_a)
        r = {"scan_dev_event_ms": round(statistics.median(a_dev), 4), "scan_dev_wall_ms": round(statistics.median(a_wall[f]), 4),
             "min_ms": round(min(a_dev), 4), "max_ms": round(max(a_dev), 4),
             "b_over_a_wall": round(statistics.median(b_wall) / statistics.median(a_wall[f]), 2),
             "kernels_back_to_back": kern, "walk_rounds_per_stream": None, "walk_us_per_round_back_to_back": None}
        lanes = f or (1024 if S <= torch.cuda.get_device_properties(0).multi_processor_count else 64)
        if rounds:
            r["walk_rounds_per_stream"] = rounds(lanes)
            if kern and S == 1:
                r["walk_us_per_round_back_to_back"] = round(kern["walk_ms"] * 1000.0 / rounds(lanes), 4)
        res["a_by_front"]["auto" if f == 0 else str(f)] = r
    vc.set_scan_front(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.iters < 8:
        ap.error("--iters must be at least 8")
    if not torch.cuda.is_available():
        sys.exit("timing_scan.py: no GPU (there is no CPU side)")
    vc.init(0)
    dev = torch.device("cuda:0")
    shapes = [shape("1x65535_16KiB", 1, [16388] * 65535, lambda w: run_rounds(65535, w), args.iters, dev),
              shape("256x512_1100B_plus_short", 256, [1100] * 512 + [300], lambda w: run_rounds(512, w), args.iters, dev),
              shape("1x4096_alternating_1100_612", 1, [1100, 612] * 2048, lambda w: 4096, args.iters, dev)]
    res = {"tool": "tools/timing_scan.py", "device": torch.cuda.get_device_name(0),
           "tree": os.environ.get("VAL_TREE") or "sources " + _build.source_hash()[:12], "box": socket.gethostname(),
           "times": "medians; scan_dev_event_ms: device events around the call; *_wall_ms: host clock to the end "
                    "of a synchronise; kernels_back_to_back: mean kernel durations of a profiled pass of "
                    "consecutive calls",
           "shapes": shapes}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
