#!/usr/bin/env python3
"""Sweep direction of repeated SpMV launches in real use: x changes from product to product.

Times a power-iteration loop ``y = A*x; x, y = y, x`` on the 2-D 5-point matrix (default 4096^2) through hp.mul_, in ONE
process, with every launch forwards (hpcla_set_spmv_sweep(0)) and with the alternating sweep (1), the two legs alternating
over a few rounds.  No norm is taken and the values run off: only time is measured.  ``--plan-build`` instead times
hp.get_vector_plan with the block order forced to natural (no tuner launches) and measured (HPCLA_BLOCK_ORDER unset),
plan cache cleared in between.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--plan-build", action="store_true")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from benchmarks.extra_workloads import device_stencil
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    n = args.n * args.n
    A = device_stencil(hp, torch, backend, (args.n, args.n), 0, n)
    x = hp.HPCVector.zeros(A.row_partition, backend)
    s = torch.cuda.current_stream().cuda_stream
    hp._capi.call("hpcla_fill_uniform_f64", x.v.data_ptr(), 0, n, 12345, s)

    if args.plan_build:
        out = {"natural_ms": [], "measured_ms": [], "chosen": []}
        for _ in range(args.rounds):
            for key, env in (("natural_ms", "natural"), ("measured_ms", None)):
                if env is None:
                    os.environ.pop("HPCLA_BLOCK_ORDER", None)
                else:
                    os.environ["HPCLA_BLOCK_ORDER"] = env
                hp.clear_plan_cache()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                plan = hp.get_vector_plan(A, x)
                torch.cuda.synchronize()
                out[key].append(round((time.perf_counter() - t0) * 1e3, 2))
                if env is None:
                    out["chosen"].append(plan.block_group)
        print(json.dumps({"bench": "plan_build", "n": args.n, **out}))
        return

    plan = hp.get_vector_plan(A, x)
    y = x.similar()

    def loop(steps):
        nonlocal x, y
        for _ in range(steps):
            hp.mul_(y, A, x)
            x, y = y, x

    def timed(mode):
        hp._capi.call("hpcla_set_spmv_sweep", mode)
        loop(args.warmup)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loop(args.steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    fwd, alt = [], []
    for _ in range(args.rounds):
        fwd.append(timed(0))
        alt.append(timed(1))
    hp._capi.call("hpcla_set_spmv_sweep", -1)
    print(json.dumps({"bench": "power_loop", "n": args.n, "steps": args.steps, "block_group": plan.block_group,
                      "patterns": plan.patterns is not None,
                      "forward_ms": [round(t, 5) for t in fwd], "alternate_ms": [round(t, 5) for t in alt],
                      "ratio_of_medians": round(float(np.median(fwd) / np.median(alt)), 4)}))


if __name__ == "__main__":
    main()
