#!/usr/bin/env python3
"""Per-kernel traffic of a micro-benchmark from rocprofv3 counter CSVs: the
mean FETCH_SIZE / WRITE_SIZE per launch of every kernel whose name contains
one of the given substrings, as one JSON line per kernel and counter. The
directories are searched for *counter_collection.csv. FETCH_SIZE is in KiB and
counts half the bytes of a wide coalesced stream on gfx950 (tools/pmc_traffic.py);
the raw counter is printed, the arms of one micro are compared like for like.
Usage: pmc_micro.py <dir> [<dir> ...] -- <name substring> [...]"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def main():
    cut = sys.argv.index("--")
    dirs, names = sys.argv[1:cut], sys.argv[cut + 1:]
    for d in dirs:
        for path in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
            vals = defaultdict(lambda: defaultdict(float))
            for r in csv.DictReader(open(path)):
                for n in names:
                    if n in r["Kernel_Name"]:
                        vals[(n, r["Counter_Name"])][r["Dispatch_Id"]] += float(r["Counter_Value"])
            for (n, c), per in sorted(vals.items()):
                print(json.dumps({"kernel": n, "counter": c, "dispatches": len(per),
                                  "KiB_per_launch": sum(per.values()) / len(per)}))


if __name__ == "__main__":
    main()
