#!/usr/bin/env python3
"""Device unpacker against what it is made of, same box, same process.

Side A: val_frame_unpack_batch_dev (verify, order, scatter on one stream).
Side B: val_crc32_verify_frames_ex_dev alone: A - B is what the added stages cost.
Side C: B, then one torch device-to-device copy of as many bytes as the batch's
payloads. C is a flattering floor for any scatter: one contiguous copy, no
per-frame work.

Shapes: k_pack's two (262,144 frames of 16,376 implied payload bytes back to
back; 65,536 frames of 1,012 bytes in slots of 1,024, rotated over 16 copies so
no launch finds its bytes in the caches), and 262,144 small explicit frames of
which every one after the first is a gap, for the order pass. The frames are
made on the device by val_frame_data_batch_dev. Device events around every
call; at least 100 ms of warm-up, then the sides alternate. `written` and the
CRC state are reset before each call of A, outside its events. The stages of A
(parse, order, scatter) are reported from a separate profiled pass
(torch.profiler kernel durations; null when the profiler is not available).
Prints one JSON object; --out also writes it. Needs a GPU.

usage: timing_unpack.py [--iters 24] [--out profiles/unpack_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import val_protocol_amd.crc as vc  # noqa: E402
import val_protocol_amd.wire as wire  # noqa: E402

PEAK = 8e12  # MI355X HBM3E, bytes/s


def random_bytes(n, dev):
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    step = 1 << 28
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        out[lo:hi] = torch.randint(0, 256, (hi - lo,), dtype=torch.uint8, device=dev)
    return out


def stage_times(fn, reps=5):
    """Mean device time per call of the unpack kernels, by stage, in ms."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {"parse_ms": 0.0, "order_ms": 0.0, "scatter_ms": 0.0, "verify_ms": 0.0}
        for e in prof.events():
            t = getattr(e, "device_time", None)
            if t is None:
                t = getattr(e, "cuda_time", 0.0)
            name = e.name
            if "k_unpack_parse" in name:
                out["parse_ms"] += t
            elif "k_unpack_order" in name:
                out["order_ms"] += t
            elif "k_unpack" in name:
                out["scatter_ms"] += t
            elif "vcrc" in name:
                out["verify_ms"] += t
        if out["order_ms"] == 0.0:
            return None
        return {k: round(v / reps / 1e3, 4) for k, v in out.items()}
    except Exception as exc:  # the profiler is optional equipment
        return {"error": repr(exc)[:200]}


def shape(name, n, plen, slot, explicit, all_gaps, iters, dev):
    prefix = 16 if explicit else 8
    wire_len = prefix + plen + 4
    stride = slot or wire_len
    flen = prefix + plen
    pay_len = torch.full((n,), plen, dtype=torch.int32, device=dev)
    inc = torch.full((n,), 1 if explicit else 0, dtype=torch.uint8, device=dev)
    pay_off = torch.arange(n, dtype=torch.int64, device=dev) * plen
    file_off = pay_off.clone()
    if all_gaps:  # frame 1 was lost: every later frame announces an offset ahead of `written`
        file_off[1:] += plen
    nbytes = n * plen
    rot = min(16, max(1, -(-(1 << 30) // (n * stride))))
    src = random_bytes(nbytes, dev)
    bases = []
    for _ in range(rot):
        b = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        wire.build_data_batch_dev(src, pay_off, pay_len, file_off, inc, out=b, out_stride=stride, len_hint=flen)
        bases.append(b)
    files = [torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(rot)]
    del pay_off, file_off, pay_len, inc
    written = torch.zeros(1, dtype=torch.int64, device=dev)
    state = torch.zeros(1, dtype=torch.int32, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    acc = torch.empty(n, dtype=torch.uint8, device=dev)
    pay = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3)]
    work = torch.empty(wire.unpack_work_bytes(n), dtype=torch.uint8, device=dev)
    turn = [0]

    def reset():
        written.zero_()
        state.fill_(-1)

    def side_a():
        k = turn[0] % rot
        wire.unpack_data_batch_dev(bases[k], file=files[k], written=written, stride=stride, flen=flen, n=n,
                                   file_state=state, out_ok=ok, nbad=cnt[0], accept=acc, naccepted=cnt[1],
                                   noverflow=cnt[2], work=work)

    def side_b():
        k = turn[0] % rot
        vc.verify_frames_ex(bases[k], stride=stride, flen=flen, n=n, out_ok=ok, nbad=cnt[0], out_pay=pay)

    def side_c():
        k = turn[0] % rot
        side_b()
        files[k].copy_(src)

    def timed(fn, before=None):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1 or turn[0] < 2:
        reset()
        side_a()
        side_b()
        side_c()
        turn[0] += 1
        torch.cuda.synchronize()
    calls = turn[0]
    want_acc = 1 if all_gaps else n
    assert int(cnt[0].item()) == 0 and int(cnt[2].item()) == 0 and int(cnt[1].item()) == calls * want_acc
    assert int(written.item()) == want_acc * plen
    if not all_gaps:
        assert torch.equal(files[(turn[0] - 1) % rot], src)
    ev = []
    for _ in range(iters):
        ev.append((timed(side_a, reset), timed(side_b), timed(side_c)))
        turn[0] += 1
    torch.cuda.synchronize()
    ms = [[x[s][0].elapsed_time(x[s][1]) for x in ev] for s in range(3)]
    a_ms, b_ms, c_ms = (statistics.median(m) for m in ms)

    def profiled():
        reset()
        side_a()

    stages = stage_times(profiled)
    moved = 3 * nbytes if not all_gaps else n * flen  # read to hash, read to copy, write
    return {"shape": name, "frames": n, "payload_bytes": plen, "stride": stride, "explicit_offsets": bool(explicit),
            "accepted_per_call": want_acc, "buffer_copies": rot, "launches_per_side": iters,
            "a_unpack_ms": round(a_ms, 4), "b_verify_ms": round(b_ms, 4), "c_verify_then_copy_ms": round(c_ms, 4),
            "a_min_ms": round(min(ms[0]), 4), "b_min_ms": round(min(ms[1]), 4), "c_min_ms": round(min(ms[2]), 4),
            "a_minus_b_ms": round(a_ms - b_ms, 4), "c_minus_b_ms": round(c_ms - b_ms, 4),
            "a_bytes_per_s": round(moved / (a_ms * 1e-3)), "a_fraction_of_8TBs": round(moved / (a_ms * 1e-3) / PEAK, 4),
            "stages_of_a": stages, "lanes_for_len_hint": vc.lanes_per_frame(flen)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.iters < 24:
        ap.error("--iters must be at least 24")
    if not torch.cuda.is_available():
        sys.exit("timing_unpack.py: no GPU (there is no CPU side)")
    vc.init(0)
    dev = torch.device("cuda:0")
    res = {"tool": "tools/timing_unpack.py", "device": torch.cuda.get_device_name(0),
           "times": "median of device-event intervals; stages_of_a: mean kernel durations of a profiled pass",
           "shapes": [shape("16KiB_back_to_back", 262144, 16376, 0, 0, False, args.iters, dev),
                      shape("1KiB_slots_1024", 65536, 1012, 1024, 0, False, args.iters, dev),
                      shape("all_gaps_262144", 262144, 40, 64, 1, True, args.iters, dev)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
