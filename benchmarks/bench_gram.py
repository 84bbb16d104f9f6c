#!/usr/bin/env python3
"""transpose(X) * Y of two tall blocks (csrc/gram.hip) on one GPU at nrows = 2^24: one JSON line.

Cases: m = k = 16 with X != Y (8 n (m + k) = 4 294 967 296 algorithmic bytes), m = k = 16 with X == Y (the block read once:
2 147 483 648 B), m = k = 64 and m = k = 4.  Each case: `hpcla_gram_f64` through the C ABI on preallocated C and scratch,
>= 5 warm-ups, then every call timed on its own between HIP events; median and min, fraction of 8.0 TB/s, FP64 TFLOP/s
(2 n m k; the symmetric case counts the same useful FLOPs).  Also the public operator `transpose(X) @ Y` at m = k = 16
(allocations and the result slice included) and the reference's column loop -- k x (`Y[:, j]` copy + `dense_matvec_t`),
src/dense.jl:1286-1310 -- for the speed-up.
usage: python benchmarks/bench_gram.py [--rows N] [--calls C] [--warmup W]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, e in ev:
        a.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(e) for a, e in ev])        # ms
    return float(np.median(t)), float(t.min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from hpcla_amd.vectors import current_stream_ptr, dptr

    n = args.rows
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    lib = hp._capi.load()
    gen = torch.Generator(device="cuda").manual_seed(5)
    out = {"bench": "gram", "nrows": n, "calls": args.calls, "warmup": args.warmup, "peak_bytes_per_s": PEAK, "cases": {}}

    def block(w):
        return torch.rand((n, w), dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0

    for name, m, k, same in [("16x16", 16, 16, False), ("16x16_sym", 16, 16, True), ("64x64", 64, 64, False),
                             ("4x4", 4, 4, False)]:
        X = block(m)
        Y = X if same else block(k)
        C = torch.empty((m, k), dtype=torch.float64, device="cuda")
        work = torch.empty(max(1, lib.hpcla_gram_work_bytes(n, m, k) // 8), dtype=torch.float64, device="cuda")
        s = current_stream_ptr()

        def call():
            hp._capi.call("hpcla_gram_f64", backend.rccl, dptr(X), m, hp._capi.LAYOUT_ROW, dptr(Y), k, hp._capi.LAYOUT_ROW,
                          n, m, k, dptr(C), dptr(work), s)
        med, mn = timed(call, args.calls, args.warmup)
        nbytes = 8 * n * (m if same else m + k)
        flops = 2 * n * m * k
        # check against torch's product once (tolerance: different summation order)
        ref = (X.T @ Y)
        err = float(((C - ref).abs() / (X.abs().T @ Y.abs())).max())
        rec = {"m": m, "k": k, "x_is_y": same, "bytes": nbytes, "median_ms": round(med, 4), "min_ms": round(mn, 4),
               "frac_of_8TBps": round(nbytes / (med * 1e-3) / PEAK, 3), "tflops_fp64": round(flops / (med * 1e-3) / 1e12, 2),
               "max_rel_err": err}
        if same:
            rec["exactly_symmetric"] = bool(torch.equal(C, C.T))
        if name == "16x16":
            Xm = hp.HPCMatrix(np.array([0, n]), np.array([0, m]), X, backend)
            Ym = hp.HPCMatrix(np.array([0, n]), np.array([0, k]), Y, backend)
            med_op, min_op = timed(lambda: hp.transpose(Xm) @ Ym, args.calls, args.warmup)
            rec["operator_median_ms"], rec["operator_min_ms"] = round(med_op, 4), round(min_op, 4)

            def loop():                                   # the reference's form: k columns, X read k times
                return [hp.dense_matvec_t(Xm, Ym[:, j]) for j in range(k)]
            med_l, min_l = timed(loop, args.calls, args.warmup)
            rec["column_loop_median_ms"], rec["column_loop_min_ms"] = round(med_l, 4), round(min_l, 4)
            rec["column_loop_bytes"] = 8 * n * (m + 1) * k + 16 * n * k      # X k times, each column copied and read
            rec["speedup_vs_column_loop"] = round(med_l / med, 2)
            del Xm, Ym
        out["cases"][name] = rec
        del X, Y, C, work
        torch.cuda.empty_cache()
    out["target_16x16_frac"] = 0.60
    out["meets_target_16x16"] = out["cases"]["16x16"]["frac_of_8TBps"] >= 0.60
    print(json.dumps(out))


if __name__ == "__main__":
    main()
