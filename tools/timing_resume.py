#!/usr/bin/env python3
"""Resume tail windows of many GPU-resident files: the batched device call
against what a caller did before it, same box, same process, same bytes.

Side A: one val_resume_tail_files_dev call over n files whose sizes lie in HBM
(outputs and workspace allocated before the clock starts), at the automatic
chunk size and again with every chunk size forced (k0 = 12..16), so that the
automatic rule can be read against the alternatives.
Side B: the route before it: the sizes copied to the host (D2H, synchronised),
val_resume_tail_window per file on the host, n val_crc32_region_dev calls on
one stream, one state each, then the n states copied back (D2H, synchronised).
Every side is timed by the host clock from the first call to the end of the
last synchronise, which is what a caller waits for, and by device events
around its calls (B's host work and its first copy lie between the events).

Shapes (every window is the whole local file, any alignment): 64 x 8 MiB,
8 x 256 MiB, 1,024 x 64 KiB, and 63 x 1 KiB plus 1 x 256 MiB. At least 100 ms
of warm-up, then the sides alternate; medians, with the minimum and maximum of
each. After the warm-up A's CRCs are checked against B's. bytes_per_s is the
window bytes over A's event time.
Prints one JSON object; --out also writes it. Needs a GPU.

usage: timing_resume.py [--iters 24] [--out profiles/resume_timing.json]"""
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

VERIFY_FIRST = 2
K0S = (12, 13, 14, 15, 16)


def med(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def shape(name, sizes, cap, iters, dev):
    n = len(sizes)
    pos, at = 1, []
    for sz in sizes:  # odd addresses, as files in a pool lie
        pos |= 1
        at.append(pos)
        pos += sz + 3
    pool = random_bytes(pos + 8, dev)
    ptr = torch.tensor([pool.data_ptr() + o for o in at], dtype=torch.int64, device=dev)
    existing = torch.tensor(sizes, dtype=torch.int64, device=dev)
    incoming = existing + 1
    action = torch.empty(n, dtype=torch.int32, device=dev)
    roff, vlen = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    vcrc = torch.empty(n, dtype=torch.int32, device=dev)
    work = torch.empty(wire.file_windows_work_bytes(n), dtype=torch.uint8, device=dev)
    states = torch.empty(n, dtype=torch.int32, device=dev)
    h_sizes = torch.empty(n, dtype=torch.int64, pin_memory=True)
    h_states = torch.empty(n, dtype=torch.int32, pin_memory=True)
    lib = vc.lib()
    cur = torch.cuda.current_stream().cuda_stream
    base = pool.data_ptr()
    off, ln = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def side_a():
        st = lib.val_resume_tail_files_dev(ptr.data_ptr(), existing.data_ptr(), incoming.data_ptr(), n, cap, 0, 0,
                                           action.data_ptr(), roff.data_ptr(), vlen.data_ptr(), vcrc.data_ptr(),
                                           work.data_ptr(), work.numel(), cur)
        assert st == vc.VAL_OK, vc.last_error()

    def side_b():
        h_sizes.copy_(existing, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        hs = h_sizes.tolist()
        for s in range(n):
            act = lib.val_resume_tail_window(hs[s], hs[s] + 1, cap, 0, 0, ctypes.byref(off), ctypes.byref(ln))
            assert act == VERIFY_FIRST
            st = lib.val_crc32_region_dev(base + at[s] + off.value - ln.value, ln.value, 0xFFFFFFFF,
                                          states.data_ptr() + 4 * s, cur)
            assert st == vc.VAL_OK, vc.last_error()
        h_states.copy_(states, non_blocking=True)
        torch.cuda.current_stream().synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, e0.elapsed_time(e1)

    vc.set_file_window_chunk(0)
    turn = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1 or turn < 2:
        side_a()
        side_b()
        torch.cuda.synchronize()
        turn += 1
    assert torch.equal(vcrc, states ^ -1), "the batched call and the region loop disagree"
    assert bool((action == VERIFY_FIRST).all()) and torch.equal(roff, existing) and torch.equal(vlen, existing)
    for k0 in K0S:  # warm every forced geometry, and check it
        vc.set_file_window_chunk(k0)
        vcrc.zero_()
        side_a()
        torch.cuda.synchronize()
        assert torch.equal(vcrc, states ^ -1), k0
    a, b = [], []
    forced = {k0: [] for k0 in K0S}
    for _ in range(iters):
        vc.set_file_window_chunk(0)
        a.append(timed(side_a))
        b.append(timed(side_b))
        for k0 in K0S:
            vc.set_file_window_chunk(k0)
            forced[k0].append(timed(side_a))
    vc.set_file_window_chunk(0)
    wall = lambda xs: med([x[0] for x in xs])  # noqa: E731
    event = lambda xs: med([x[1] for x in xs])  # noqa: E731
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = vc.plan_file_windows(cus, n, max(sizes) if cap == 0 else min(max(cap, 1), 256 << 20))
    total = sum(sizes)
    res = {"shape": name, "files": n, "window_bytes": total, "tail_cap_bytes": cap, "calls_per_side": iters,
           "cus": cus, "automatic_k0": plan[0].k0, "hash_grid": plan[2].grid,
           "a_tail_files_dev_event": event(a), "a_tail_files_dev_wall": wall(a),
           "b_readback_region_loop_event": event(b), "b_readback_region_loop_wall": wall(b),
           "b_over_a_wall": round(wall(b)["median_ms"] / wall(a)["median_ms"], 2),
           "a_bytes_per_s": int(total / (event(a)["median_ms"] * 1e-3)),
           "b_us_per_file_wall": round(wall(b)["median_ms"] * 1e3 / n, 2),
           "a_forced_k0_event": {str(k0): event(v) for k0, v in forced.items()},
           "a_forced_k0_wall": {str(k0): wall(v) for k0, v in forced.items()}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.iters < 8:
        ap.error("--iters must be at least 8")
    if not torch.cuda.is_available():
        sys.exit("timing_resume.py: no GPU (there is no CPU side)")
    vc.init(0)
    dev = torch.device("cuda:0")
    MIB = 1 << 20
    shapes = [shape("64x8MiB", [8 * MIB] * 64, 0, args.iters, dev),
              shape("8x256MiB", [256 * MIB] * 8, 256 * MIB, args.iters, dev),
              shape("1024x64KiB", [64 << 10] * 1024, 64 << 10, args.iters, dev),
              shape("63x1KiB+1x256MiB", [1 << 10] * 40 + [256 * MIB] + [1 << 10] * 23, 256 * MIB, args.iters, dev)]
    res = {"tool": "tools/timing_resume.py", "device": torch.cuda.get_device_name(0),
           "tree": os.environ.get("VAL_TREE") or "sources " + _build.source_hash()[:12], "box": socket.gethostname(),
           "times": "medians with minimum and maximum; *_wall: host clock from the first call to the end of the last "
                    "synchronise; *_event: device events around the side's calls; a_bytes_per_s: window bytes over "
                    "a's event time; a_forced_k0_*: side a with val_gpu_set_file_window_chunk(k0)",
           "shapes": shapes}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
