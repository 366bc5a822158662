"""Time val_frame_respond_files_dev beside val_frame_unpack_files_dev, the call it follows, over the
same window: 65,536 files x 16 frames of 16 KiB, and one file of 1,048,576 frames.
Device events around every call, two warm-up calls per side, then 5 timed calls; all times are kept,
sorted. Needs an MI355X and about 35 GB of HBM.

    python tools/timing_acks.py --out profiles/acks_timing.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import val_protocol_amd.crc as vc  # noqa: E402
import val_protocol_amd.wire as wire  # noqa: E402

DEV = "cuda:0"
PAY, N = 16384, 1 << 20
FLEN, SLOT = 8 + 8 + PAY, 8 + 8 + PAY + 4
REPS = 5


def d64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def d32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def timed(fn, before=None):
    for _ in range(2):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "acks_timing.json"))
    args = ap.parse_args()
    vc.init(0)
    records = []
    payload = torch.randint(0, 256, (PAY,), dtype=torch.uint8, device=DEV)
    stream = torch.empty(N * SLOT + 8, dtype=torch.uint8, device=DEV)
    canvas = torch.empty(N * PAY, dtype=torch.uint8, device=DEV)
    pay_off = torch.zeros(N, dtype=torch.int64, device=DEV)
    pay_len = torch.full((N,), PAY, dtype=torch.int32, device=DEV)
    work = torch.empty(wire.unpack_work_bytes(N), dtype=torch.uint8, device=DEV)
    rwork = torch.empty(wire.respond_work_bytes(N), dtype=torch.uint8, device=DEV)
    ok = torch.empty(N, dtype=torch.uint8, device=DEV)
    acc = torch.empty(N, dtype=torch.uint8, device=DEV)
    rx = torch.empty(N * 16 + 64, dtype=torch.uint8, device=DEV)
    for name, S in (("65536 files x 16 frames", 65536), ("1 file x 1048576 frames", 1)):
        per = N // S
        file_off = (np.arange(N, dtype=np.uint64) % np.uint64(per)) * np.uint64(PAY)
        wire.build_data_batch_dev(payload, pay_off, pay_len, d64(file_off), None, out=stream, out_stride=SLOT,
                                  len_hint=FLEN)
        first = d32(np.arange(S + 1, dtype=np.uint64) * np.uint64(per))
        fsize = np.full(S, per * PAY, np.uint64)
        ptr = d64(np.arange(S, dtype=np.uint64) * np.uint64(per * PAY) + np.uint64(canvas.data_ptr()))
        cap, total = d64(fsize), d64(fsize)
        written = torch.zeros(S, dtype=torch.int64, device=DEV)
        counters = [torch.zeros(S, dtype=torch.int32, device=DEV) for _ in range(3)]
        nbad = torch.zeros(1, dtype=torch.int32, device=DEV)
        since = torch.zeros(S, dtype=torch.int32, device=DEV)
        r_off = d64(np.arange(S, dtype=np.uint64) * np.uint64(per * 16))
        r_cap = d64(np.full(S, per * 16, np.uint64))
        ndrop = torch.zeros(S, dtype=torch.int32, device=DEV)

        def unpack():
            wire.unpack_data_files_dev(stream, first=first, file_ptr=ptr, file_cap=cap, written=written, stride=SLOT,
                                       flen=FLEN, n=N, naccepted=counters[0], noverflow=counters[1],
                                       file_nbad=counters[2], out_ok=ok, nbad=nbad, accept=acc, work=work)

        def respond():
            return wire.respond_files_dev(stream, first=first, ok=ok, accept=acc, written=written, total=total, out=rx,
                                          resp_off=r_off, resp_cap=r_cap, ack_stride=1, since=since, stride=SLOT,
                                          flen=FLEN, n=N, ndropped=ndrop, work=rwork)

        t_unpack = timed(unpack, before=written.zero_)
        t_respond = timed(respond)
        rlen, nresp, _ = respond()
        torch.cuda.synchronize()
        rec = dict(shape=name, frames=N, frame_bytes=SLOT, unpack_ms=t_unpack, respond_ms=t_respond,
                   accepted=int(acc.sum().item()), responses=int(nresp.sum().item()),
                   response_bytes=int(rlen.sum().item()), dropped=int(ndrop.sum().item()),
                   written_ok=bool((written.cpu().numpy().view(np.uint64) == fsize).all()))
        print(json.dumps(rec), flush=True)
        records.append(rec)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_properties(0).name, shapes=records), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
