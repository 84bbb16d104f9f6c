#!/usr/bin/env python3
"""Last N launches of the row-gather SpMV kernel in a rocprofv3 CSV: duration statistics and achieved bandwidth on a given
byte count (a --kernel-trace file), or the mean of every counter per launch (a --pmc counter_collection file).

usage: python benchmarks/last_launches.py KERNEL_TRACE.csv BYTES [N]
       python benchmarks/last_launches.py --pmc COUNTER_COLLECTION.csv [N]
The protocol of profiles/MEASUREMENTS_narrow_cols.md section 4 / MEASUREMENTS_block_patterns.md: both legs under one forced
block order, so that every launch of the kernel after the plan build is a launch of the step."""
import collections
import csv
import sys

KERNEL = "spmv_rowgather_kernel"


def trace(path, nbytes, last):
    rows = [r for r in csv.DictReader(open(path, newline="")) if KERNEL in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    tail = rows[-last:]
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in tail]
    names = sorted({r["Kernel_Name"].split("(")[0] for r in tail})
    mean = sum(us) / len(us)
    print(f"launches_total={len(rows)} last{len(tail)}: kernel={names} mean_us={mean:.2f} min_us={min(us):.2f} max_us={max(us):.2f} "
          f"bytes={nbytes} GB/s={nbytes / mean / 1e3:.1f}")
    # launches of one matrix alternate their sweep direction (HPCLA_SPMV_SWEEP): the two parities of the launch index apart
    for parity in (0, 1):
        sel = [u for i, u in enumerate(us, len(rows) - len(tail)) if i % 2 == parity]
        if sel:
            print(f"  launch index {'even' if parity == 0 else 'odd'}: n={len(sel)} mean_us={sum(sel) / len(sel):.2f} "
                  f"min_us={min(sel):.2f} max_us={max(sel):.2f}")


def pmc(path, last):
    per = collections.defaultdict(dict)                    # dispatch -> {counter: value summed over instances}
    for r in csv.DictReader(open(path, newline="")):
        if KERNEL in r["Kernel_Name"]:
            d = per[int(r["Dispatch_Id"])]
            d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    ids = sorted(per)[-last:]
    for c in sorted({c for i in ids for c in per[i]}):
        v = [per[i][c] for i in ids if c in per[i]]
        print(f"last{len(ids)} launches: {c} mean={sum(v) / len(v):.1f} min={min(v):.1f} max={max(v):.1f}")


if __name__ == "__main__":
    if sys.argv[1] == "--pmc":
        pmc(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 50)
    else:
        trace(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 50)
