#!/usr/bin/env python3
"""The converging CG solver (``hp.cg``) on config 4's per-GPU share -- the 7-point Laplacian of a 512 x 512 x 64 slab
(16 777 216 rows; the matrix of ``bench.py --workload poisson3d_cg``) -- and on 64^3, one GPU, Float64, Int32 indices.

Every figure is ms per iteration of a WHOLE public call of 100 iterations (``rtol=0``: the stop rule never fires, the work
is fixed): HIP events on the stream around the call, which therefore contain the set-up (r0, p0, the norms and their one
read-back), the iterations, the chunk read-backs and the history read-back.  ``--runs`` timed calls (default 21) after
``--warmup`` untimed ones, the variants of one table ALTERNATING call by call so that a drift of the card hits all of them
alike; median, with the minimum and maximum next to it.

  (i)   gating overhead    hp.cg(M=None, check_every=8)  against  hp.cg_fixed_iterations: the same SpMV + p.Ap launch, the
                           gated update kernels against the plain ones, one 16-byte read-back per 8 iterations against
                           none.  cg_fixed_iterations and the kernels under it are the parent commit's, unchanged.
                           Allowed: 1.05 (up to two single-workgroup launches and one read-back per chunk against 488.8 us of
                           kernels and 4.1 us of gaps per iteration).  Its native loop runs on Int32 columns; hp.cg hands the
                           plan's 16-bit columns and pattern table to its loop, so a ratio below 1 is that, not the gating:
                           the third row (hp.cg with the plan's narrow forms withheld from its loop) separates the two.
  (ii)  Jacobi             hp.cg(M="jacobi") against hp.cg(M=None): byte model SpMV + 80 against SpMV + 64 per row.
  (iii) check_every        {1, 4, 8, 16, 32} on both matrices.

Prints one JSON line and writes <out>/bench_pcg.json and <out>/bench_pcg_tables.md (default out: profiles/).
usage: python benchmarks/bench_pcg.py [--runs R] [--warmup W] [--iters K] [--out DIR] [--small-only]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_table(torch, variants, runs, warmup, iters):
    """variants: {name: callable}.  Returns {name: (median, min, max)} in ms per iteration, calls alternating."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(runs):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            samples[name].append(e0.elapsed_time(e1) / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small-only", action="store_true", help="64^3 only (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from hpcla_amd import workloads as wl
    from benchmarks.extra_workloads import device_stencil
    if not torch.cuda.is_available():
        raise SystemExit("bench_pcg.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    K = args.iters
    record = {"iters_per_call": K, "runs": args.runs, "warmup": args.warmup, "unit": "ms per iteration, median (min, max)"}
    lines = []
    for label, dims in ([] if args.small_only else [("512x512x64", (512, 512, 64))]) + [("64x64x64", (64, 64, 64))]:
        n = int(np.prod(dims))
        A = device_stencil(hp, torch, backend, dims, 0, n)
        b = hp.HPCVector.zeros(A.row_partition, backend)
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, n, wl.SEED_RHS, torch.cuda.current_stream().cuda_stream)
        ws_fixed = hp.CGWorkspace(b, K + 2)
        ws = hp.PCGWorkspace(b, K + 2)
        plan = hp.get_vector_plan(A, ws.p)
        narrow = (plan.cols16, plan.patterns)

        def solve(M=None, chunk=8, with_narrow=True):
            if not with_narrow:
                plan.cols16, plan.patterns = None, None
            try:
                _, info = hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=K, M=M, check_every=chunk, workspace=ws)
            finally:
                plan.cols16, plan.patterns = narrow
            assert info.iterations == K and info.status == "maxiter", info.status

        # same bits before anything is timed: the gated loop without a preconditioner is the harness's iteration
        x_ref, h_ref = hp.cg_fixed_iterations(A, b, K, workspace=ws_fixed)
        _, info = hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=K, workspace=ws)
        assert info.residual_norms == h_ref and torch.equal(ws.x.v.view(torch.int64), x_ref.v.view(torch.int64)), "bits differ"

        gate = timed_table(torch, {"cg_fixed_iterations": lambda: hp.cg_fixed_iterations(A, b, K, workspace=ws_fixed),
                                   "hp.cg M=None": lambda: solve(),
                                   "hp.cg M=None, Int32 columns": lambda: solve(with_narrow=False),
                                   "hp.cg M=jacobi": lambda: solve(M="jacobi")}, args.runs, args.warmup, K)
        chunks = timed_table(torch, {str(c): (lambda c=c: solve(chunk=c)) for c in (1, 4, 8, 16, 32)}, args.runs, args.warmup, K)
        base = gate["cg_fixed_iterations"][0]
        rec = {"rows": n, "nnz": int(A.nnz), "narrow_columns_in_plan": narrow[0] is not None,
               "pattern_table_in_plan": narrow[1] is not None,
               "gating": {k: [round(x, 5) for x in v] for k, v in gate.items()},
               "gating_ratio": round(gate["hp.cg M=None"][0] / base, 4),
               "gating_ratio_int32_columns": round(gate["hp.cg M=None, Int32 columns"][0] / base, 4),
               "jacobi_ratio": round(gate["hp.cg M=jacobi"][0] / gate["hp.cg M=None"][0], 4),
               "check_every": {k: [round(x, 5) for x in v] for k, v in chunks.items()}}
        record[label] = rec
        lines += [f"### {label} ({n} rows, {int(A.nnz)} stored entries; 16-bit columns in the plan: {rec['narrow_columns_in_plan']}, "
                  f"pattern table: {rec['pattern_table_in_plan']})", "",
                  "| call (100 iterations) | ms / iteration, median | min | max | ratio to cg_fixed_iterations |", "|---|---|---|---|---|"]
        lines += [f"| {k} | {v[0]:.4f} | {v[1]:.4f} | {v[2]:.4f} | {v[0] / base:.4f} |" for k, v in gate.items()]
        lines += ["", f"Jacobi against unpreconditioned: {rec['jacobi_ratio']:.4f}", "",
                  "| check_every | ms / iteration, median | min | max | ratio to 8 |", "|---|---|---|---|---|"]
        lines += [f"| {k} | {v[0]:.4f} | {v[1]:.4f} | {v[2]:.4f} | {v[0] / chunks['8'][0]:.4f} |" for k, v in chunks.items()]
        lines.append("")
        del A, b, ws, ws_fixed
        hp.clear_plan_cache()
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_pcg.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out, "bench_pcg_tables.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
