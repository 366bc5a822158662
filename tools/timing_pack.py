#!/usr/bin/env python3
"""Device framer against the cheapest unfused pipeline, same box, same process.

Side A: val_frame_data_batch_dev (one fused copy-and-hash launch).
Side B: a torch device-to-device copy of the payload bytes into the frame
slots, then val_crc32_frames_dev (strided) over the frames. B is flattered: it
writes neither headers nor trailers.

Shapes: 262,144 frames of 16,376 implied payload bytes, back to back (cfg3's
frame size); 65,536 frames of 1,012 bytes in slots of 1,024, rotated over
copies spanning 1 GiB so no launch finds its bytes in the caches (as bench.py
does for cfg2). Device events around every launch; at least 100 ms of warm-up,
then the two sides alternate. Prints one JSON object; --out also writes it.
Needs a GPU: there is no CPU side.

usage: timing_pack.py [--iters 20] [--out profiles/pack_timing.json]"""
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


def shape(name, n, plen, slot, iters, dev):
    wire_len = 12 + plen  # implied frames: 8-byte header, payload, trailer
    stride = slot or wire_len
    pay_len = np.full(n, plen, dtype=np.uint32)
    inc = np.zeros(n, dtype=np.uint8)
    pay_off = np.arange(n, dtype=np.uint64) * np.uint64(plen)
    frame_off, _, total = wire.data_layout(pay_len, inc)
    d_len = torch.from_numpy(pay_len.view(np.int32)).to(dev)
    d_inc = torch.from_numpy(inc).to(dev)
    d_off = torch.from_numpy(pay_off.view(np.int64)).to(dev)
    d_fo = None if slot else torch.from_numpy(frame_off.view(np.int64)).to(dev)
    nbytes = n * plen
    rot = min(16, max(1, -(-(1 << 30) // nbytes)))
    pays = [random_bytes(nbytes, dev) for _ in range(rot)]
    outs = [torch.zeros(n * stride, dtype=torch.uint8, device=dev) for _ in range(rot)]
    crc = torch.empty(n, dtype=torch.int32, device=dev)
    nrej = torch.zeros(1, dtype=torch.int32, device=dev)
    turn = [0]

    def side_a():
        k = turn[0] % rot
        wire.build_data_batch_dev(pays[k], d_off, d_len, d_off, d_inc, out=outs[k], frame_off=d_fo,
                                  out_stride=slot, len_hint=8 + plen, out_crc=crc, nrejected=nrej)

    def side_b():
        k = turn[0] % rot
        outs[k].view(n, stride)[:, 8:8 + plen].copy_(pays[k].view(n, plen))
        vc.frames(outs[k], stride=stride, flen=8 + plen, n=n, out_crc=crc)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1 or turn[0] < 2:
        side_a()
        side_b()
        turn[0] += 1
        torch.cuda.synchronize()
    ev = []
    for _ in range(iters):
        ev.append((timed(side_a), timed(side_b)))
        turn[0] += 1
    torch.cuda.synchronize()
    a = [x[0].elapsed_time(x[1]) for x, _ in ev]
    b = [y[0].elapsed_time(y[1]) for _, y in ev]
    assert int(nrej.item()) == 0
    a_ms, b_ms = statistics.median(a), statistics.median(b)
    moved = 2 * nbytes + 12 * n
    return {"shape": name, "frames": n, "payload_bytes": plen, "out_stride": stride, "buffer_copies": rot,
            "launches_per_side": iters, "a_fused_ms": round(a_ms, 4), "b_copy_then_hash_ms": round(b_ms, 4),
            "a_min_ms": round(min(a), 4), "b_min_ms": round(min(b), 4), "ratio_a_over_b": round(a_ms / b_ms, 4),
            "a_bytes_per_s": round(moved / (a_ms * 1e-3)), "a_fraction_of_8TBs": round(moved / (a_ms * 1e-3) / PEAK, 4),
            "lanes_for_len_hint": vc.lanes_per_frame(8 + plen)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("timing_pack.py: no GPU (there is no CPU side)")
    vc.init(0)
    dev = torch.device("cuda:0")
    res = {"tool": "tools/timing_pack.py", "device": torch.cuda.get_device_name(0), "times": "median of device-event intervals",
           "shapes": [shape("16KiB_back_to_back", 262144, 16376, 0, args.iters, dev),
                      shape("1KiB_slots_1024", 65536, 1012, 1024, args.iters, dev)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
