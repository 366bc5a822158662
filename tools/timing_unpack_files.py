#!/usr/bin/env python3
"""One window for many receivers: val_frame_unpack_files_dev against S calls of
the single-file entry point, same box, same process, same frames.

Side A: one val_frame_unpack_files_dev call over all n frames and S files.
Side B: S consecutive val_frame_unpack_batch_dev calls on one stream, call s
over file s's frames (the same bytes, the same slots). Their arguments are
made before the clock starts; what is timed is the calls themselves.

Shapes: 262,144 frames of 16,376 implied payload bytes back to back, all
accepted, split evenly over S = 1, 4, 16, 64 files; 65,536 frames of 1,012
bytes in slots of 1,024 over S = 16 files, rotated over 16 copies so no launch
finds its bytes in the caches. The frames are made on the device by
val_frame_data_batch_dev. The method is tools/timing_unpack.py's: device events
around every call (side B: around its S calls), at least 100 ms of warm-up,
then the sides alternate; medians. `written` and the CRC states are reset
before each side, outside its events. After the warm-up both sides' files,
`written`, states and counters are checked against each other and the source.
The stages of A are reported from a separate profiled pass (null when the
profiler is not available).
Prints one JSON object; --out also writes it. Needs a GPU.

usage: timing_unpack_files.py [--iters 24] [--out profiles/unpack_files_timing.json]"""
import argparse
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
from timing_unpack import random_bytes, stage_times  # noqa: E402
from val_protocol_amd import _build  # noqa: E402


def shape(name, n, plen, slot, S, iters, dev):
    assert n % S == 0
    per = n // S
    wire_len = 8 + plen + 4
    stride = slot or wire_len
    flen = 8 + plen
    nbytes = n * plen
    pay_len = torch.full((n,), plen, dtype=torch.int32, device=dev)
    inc = torch.zeros(n, dtype=torch.uint8, device=dev)
    pay_off = torch.arange(n, dtype=torch.int64, device=dev) * plen
    file_off = pay_off % (per * plen)  # every file starts at 0 (implied frames do not carry it)
    rot = min(16, max(1, -(-(1 << 30) // (n * stride))))
    src = random_bytes(nbytes, dev)
    bases = []
    for _ in range(rot):
        b = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        wire.build_data_batch_dev(src, pay_off, pay_len, file_off, inc, out=b, out_stride=stride, len_hint=flen)
        bases.append(b)
    del pay_off, file_off, pay_len, inc
    # file s is bytes [s * per * plen, (s + 1) * per * plen) of one buffer per copy and side: delivered, it equals src
    files = [[torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(rot)] for _ in range(2)]
    fbytes = per * plen
    first = torch.arange(S + 1, dtype=torch.int32, device=dev) * per
    cap = torch.full((S,), fbytes, dtype=torch.int64, device=dev)
    ptrs = [torch.tensor([f.data_ptr() + s * fbytes for s in range(S)], dtype=torch.int64, device=dev) for f in files[0]]
    written = [torch.zeros(S, dtype=torch.int64, device=dev) for _ in range(2)]
    state = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2)]
    nacc = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2)]
    novf = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2)]
    nbad = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2)]
    fnbad = torch.zeros(S, dtype=torch.int32, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    acc = torch.empty(n, dtype=torch.uint8, device=dev)
    work = torch.empty(wire.unpack_work_bytes(n), dtype=torch.uint8, device=dev)
    # side B's arguments, one set per copy and file
    b_args = [[dict(base=bases[k][s * per * stride:], file=files[1][k][s * fbytes:(s + 1) * fbytes],
                    written=written[1][s:s + 1], file_state=state[1][s:s + 1], out_ok=ok[s * per:(s + 1) * per],
                    accept=acc[s * per:(s + 1) * per], nbad=nbad[1], naccepted=nacc[1][s:s + 1],
                    noverflow=novf[1][s:s + 1]) for s in range(S)] for k in range(rot)]
    turn = [0]

    def reset(side):
        written[side].zero_()
        state[side].fill_(-1)

    def side_a():
        k = turn[0] % rot
        wire.unpack_data_files_dev(bases[k], first=first, file_ptr=ptrs[k], file_cap=cap, written=written[0],
                                   stride=stride, flen=flen, n=n, file_state=state[0], naccepted=nacc[0],
                                   noverflow=novf[0], file_nbad=fnbad, out_ok=ok, nbad=nbad[0], accept=acc, work=work)

    def side_b():
        for a in b_args[turn[0] % rot]:
            wire.unpack_data_batch_dev(a["base"], file=a["file"], written=a["written"], stride=stride, flen=flen, n=per,
                                       file_state=a["file_state"], out_ok=a["out_ok"], nbad=a["nbad"],
                                       accept=a["accept"], naccepted=a["naccepted"], noverflow=a["noverflow"],
                                       work=work)

    def timed(fn, side):
        reset(side)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1 or turn[0] < 2:
        reset(0)
        side_a()
        reset(1)
        side_b()
        turn[0] += 1
        torch.cuda.synchronize()
    calls = turn[0]
    k = (turn[0] - 1) % rot
    for side in range(2):
        assert int(nbad[side].item()) == 0 and int(novf[side].sum().item()) == 0
        assert bool((nacc[side] == calls * per).all()) and bool((written[side] == fbytes).all())
        assert torch.equal(files[side][k], src)
    assert torch.equal(state[0], state[1]) and int(fnbad.sum().item()) == 0
    ev = []
    for _ in range(iters):
        ev.append((timed(side_a, 0), timed(side_b, 1)))
        turn[0] += 1
    torch.cuda.synchronize()
    ms = [[x[s][0].elapsed_time(x[s][1]) for x in ev] for s in range(2)]
    a_ms, b_ms = (statistics.median(m) for m in ms)

    def profiled():
        reset(0)
        side_a()

    return {"shape": name, "frames": n, "payload_bytes": plen, "stride": stride, "files": S, "frames_per_file": per,
            "buffer_copies": rot, "calls_per_side": iters, "a_files_call_ms": round(a_ms, 4),
            "b_single_file_calls_ms": round(b_ms, 4), "a_over_b": round(a_ms / b_ms, 4),
            "a_min_ms": round(min(ms[0]), 4), "a_max_ms": round(max(ms[0]), 4), "b_min_ms": round(min(ms[1]), 4),
            "b_max_ms": round(max(ms[1]), 4), "stages_of_a": stage_times(profiled),
            "order_workgroups": min(S, torch.cuda.get_device_properties(0).multi_processor_count)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.iters < 24:
        ap.error("--iters must be at least 24")
    if not torch.cuda.is_available():
        sys.exit("timing_unpack_files.py: no GPU (there is no CPU side)")
    vc.init(0)
    dev = torch.device("cuda:0")
    shapes = [shape(f"16KiB_back_to_back_S{S}", 262144, 16376, 0, S, args.iters, dev) for S in (1, 4, 16, 64)]
    shapes.append(shape("1KiB_slots_1024_S16", 65536, 1012, 1024, 16, args.iters, dev))
    res = {"tool": "tools/timing_unpack_files.py", "device": torch.cuda.get_device_name(0),
           "tree": os.environ.get("VAL_TREE") or "sources " + _build.source_hash()[:12], "box": socket.gethostname(),
           "times": "median of device-event intervals around one call (A) or around the S calls (B); "
                    "stages_of_a: mean kernel durations of a profiled pass",
           "shapes": shapes}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
