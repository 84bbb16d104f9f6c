#!/usr/bin/env python3
"""``hp.cg`` with the smoothed-aggregation multigrid preconditioner (``hp.amg``) against ``"jacobi"`` and ``hp.fsai(A)``, one GPU,
Float64, Int32 indices: the 5-point Laplacian at 2048 x 2048 and 4096 x 4096, and config 4's per-GPU share, the 7-point Laplacian
of a 512 x 512 x 64 slab (the matrix of ``bench.py --workload poisson3d_cg``).  b = fill_uniform.  All in one run, on one tree.

Per matrix:
  to 1e-8      per preconditioner, iterations and milliseconds of ``hp.cg(rtol=1e-8, check_every=32)``, HIP events around the
               call, median (min, max) of ``--solves`` calls.
  setup        ``hp.amg(A)`` whole, events around the public call: the FIRST call (which builds every plan of the hierarchy: the
               products', the transposes', the SpMVs') and each of ``--setups`` later calls on the same structure; levels,
               operator complexity, the rounds of the independent set and the runs the Galerkin product was split into per
               level.  A hierarchy that cannot be built (a product over ``hp.spgemm``'s bound) is recorded as that, and the run
               goes on.
  ms / iter    a whole public call of ``--iters`` iterations (``rtol=0``): events around the call, and next to it the HOST's time
               in the same call's enqueueing (``PCGWorkspace.enqueue_ms``; the chunk's 16-byte read-back lies outside).  Where
               the two agree the iteration is bound by the host's enqueueing and a cycle below the C ABI would pay; where the event time is the larger the device is the limit.
  coarse_size  128 (the default) against 512: levels, iterations and time to 1e-8.

Prints one JSON line and writes <out>/bench_amg.json and <out>/bench_amg_tables.md after every matrix (default out: profiles/).
usage: python benchmarks/bench_amg.py [--cases 2048,3d,4096] [--runs R] [--iters K] [--solves S] [--out DIR] [--small]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"2048": ("2048x2048", (2048, 2048)), "4096": ("4096x4096", (4096, 4096)), "3d": ("512x512x64", (512, 512, 64))}
SMALL = {"2048": ("256x256", (256, 256)), "4096": ("384x384", (384, 384)), "3d": ("32x32x32", (32, 32, 32))}


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def spread(values, digits=3):
    return [round(statistics.median(values), digits), round(min(values), digits), round(max(values), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048,3d,4096")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--setups", type=int, default=6, help="later hp.amg calls on the same structure")
    ap.add_argument("--maxiter", type=int, default=60000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small", action="store_true", help="small grids (a rehearsal of the script)")
    ap.add_argument("--trace-iters", type=int, default=0, help="setup and one call of this many iterations only (for a kernel trace)")
    ap.add_argument("--trace-diff", nargs=4, metavar=("STATS_A", "ITERS_A", "STATS_B", "ITERS_B"),
                    help="device ms per iteration from two kernel_stats.csv files of --trace-iters runs; needs no GPU")
    args = ap.parse_args()
    if args.trace_diff:
        import csv

        def busy_ms(path):
            with open(path, newline="") as f:
                return sum(float(row["TotalDurationNs"]) for row in csv.DictReader(f)) * 1e-6

        (pa, ka, pb, kb) = args.trace_diff
        ta, tb = busy_ms(pa), busy_ms(pb)
        print(json.dumps({"kernel_ms": [round(ta, 3), round(tb, 3)], "iterations": [int(ka), int(kb)],
                          "device_ms_per_iteration": round((tb - ta) / (int(kb) - int(ka)), 4)}))
        return
    import torch
    import hpcla_amd as hp
    from hpcla_amd import workloads as wl
    from benchmarks.extra_workloads import device_stencil
    if not torch.cuda.is_available():
        raise SystemExit("bench_amg.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    if args.trace_iters:
        # under `rocprofv3 --kernel-trace --stats`: the setup and ONE call of that many iterations, nothing else.  Two such runs
        # with different counts differ by the iterations alone; --trace-diff turns their kernel_stats.csv into device ms / iteration
        label, dims = (SMALL if args.small else CASES)[args.cases.split(",")[0].strip()]
        n = int(np.prod(dims))
        A = device_stencil(hp, torch, backend, dims, 0, n)
        b = hp.HPCVector.zeros(A.row_partition, backend)
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, n, wl.SEED_RHS, torch.cuda.current_stream().cuda_stream)
        _, info = hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=args.trace_iters, M=hp.amg(A), check_every=args.trace_iters)
        torch.cuda.synchronize()
        print(json.dumps({"case": label, "iterations": info.iterations, "status": info.status}))
        return
    K = args.iters
    record = {"device": torch.cuda.get_device_name(0), "iters_per_call": K, "runs": args.runs, "solves": args.solves, "rtol": 1e-8}
    lines = []

    def write():
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_amg.json"), "w") as f:
            json.dump(record, f, indent=1)
        with open(os.path.join(args.out, "bench_amg_tables.md"), "w") as f:
            f.write("\n".join(lines) + "\n")

    for key in args.cases.split(","):
        label, dims = (SMALL if args.small else CASES)[key.strip()]
        n = int(np.prod(dims))
        A = device_stencil(hp, torch, backend, dims, 0, n)
        b = hp.HPCVector.zeros(A.row_partition, backend)
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, n, wl.SEED_RHS, torch.cuda.current_stream().cuda_stream)
        y = b.similar()
        hp.mul_(y, A, b)
        spmv = statistics.median(event_ms(torch, lambda: hp.mul_(y, A, b))[0] for _ in range(50))
        rec = {"rows": n, "nnz": int(A.nnz), "spmv_ms": round(spmv, 4), "setup": {}, "per_iteration": {}, "solve": {}}

        def describe(M):
            return {"levels": [l.n for l in M.levels], "rounds": [l.rounds for l in M.levels],
                    "operator_complexity": round(M.operator_complexity, 4),
                    "last_level": "dense" if M.levels[-1].inverse is not None else f"{M.levels[-1].sweeps} sweeps"}

        M, failed = {"jacobi": "jacobi"}, []
        t, M["fsai(A)"] = event_ms(torch, lambda: hp.fsai(A))
        rec["setup"]["fsai(A)"] = {"first_call_ms": round(t, 2)}
        for name, cs in (("amg(A)", 128), ("amg(A, coarse_size=512)", 512)):
            try:
                first, M[name] = event_ms(torch, lambda: hp.amg(A, coarse_size=cs))
            except NotImplementedError as exc:                   # a product over hp.spgemm's bound: the outcome, recorded
                rec["setup"][name] = {"failed": str(exc)}
                failed.append(f"{name} could not be built: {exc}")
                continue
            # later calls on the same structure, each one listed: hp.spgemm builds its product lists on the third product of
            # a structure (one slower call), after which the numeric products are single streaming passes
            later = [round(event_ms(torch, lambda: hp.amg(A, coarse_size=cs))[0], 2) for _ in range(args.setups)] if cs == 128 else []
            rec["setup"][name] = {"first_call_ms": round(first, 2), "later_calls_each_ms": later,
                                  "later_calls_ms": spread(later, 2) if later else None,
                                  "galerkin": [l.galerkin for l in M[name].levels[:-1]], **describe(M[name])}
        ws = hp.PCGWorkspace(b, K + 2)

        for name, m in M.items():
            ev, host = [], []
            for run in range(args.runs + 1):                     # the first call is the warm-up
                torch.cuda.synchronize()
                t, (_, info) = event_ms(torch, lambda: hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=K, M=m, check_every=K, workspace=ws))
                if info.iterations != K:                         # a breakdown on rounding noise far below 1e-8: the figure is void
                    raise SystemExit(f"{label} {name}: {info.status} after {info.iterations} of {K} iterations; lower --iters")
                if run:
                    ev.append(t / K)
            # the host alone: the same K iterations, one chunk, timed from the first library call of the chunk to the return of
            # the last (the chunk's read-back, which waits for the device, lies outside)
            ws.enqueue_ms = host                                 # PCGWorkspace's clock around each chunk's enqueueing
            for run in range(args.runs):
                torch.cuda.synchronize()
                hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=K, M=m, check_every=K, workspace=ws)
            ws.enqueue_ms = None
            rec["per_iteration"][name] = {"event_ms": spread(ev, 4), "host_enqueue_ms": spread([h / K for h in host], 4)}
        for name, m in M.items():
            times, its = [], None
            for _ in range(args.solves):
                t, (x, info) = event_ms(torch, lambda: hp.cg(A, b, rtol=1e-8, maxiter=args.maxiter, M=m, check_every=32, workspace=ws))
                times.append(t)
                its = info.iterations
            true = hp.norm(b - A @ x) / hp.norm(b)
            rec["solve"][name] = {"iterations": its, "status": info.status, "ms": spread(times, 2), "true_residual": float(f"{true:.3e}")}
        record[label] = rec
        jac = rec["solve"]["jacobi"]
        lines += [f"### {label} ({n} rows, {int(A.nnz)} stored entries; one SpMV of A: {spmv:.3f} ms)", "",
                  "| M | setup, first call (ms) | setup, later calls (ms) | levels | operator complexity | ms / iteration by events, "
                  "median (min, max) | host enqueue ms / iteration | iterations to 1e-8 | ms to 1e-8, median (min, max) | time against "
                  "Jacobi | true residual |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        for name in M:
            st, it, so = rec["setup"].get(name) or {}, rec["per_iteration"][name], rec["solve"][name]
            later = st.get("later_calls_ms")
            lines.append(f"| {name} | {st.get('first_call_ms', '-')} | {later[0] if later else '-'} | {st.get('levels', '-')} | "
                         f"{st.get('operator_complexity', '-')} | {it['event_ms'][0]:.4f} ({it['event_ms'][1]:.4f}, "
                         f"{it['event_ms'][2]:.4f}) | {it['host_enqueue_ms'][0]:.4f} | {so['iterations']} ({so['status']}) | "
                         f"{so['ms'][0]:.1f} ({so['ms'][1]:.1f}, {so['ms'][2]:.1f}) | {so['ms'][0] / jac['ms'][0]:.3f} | "
                         f"{so['true_residual']:.2e} |")
        lines += [""] + failed + ([""] if failed else [])
        write()
        del A, b, y, ws, M
        hp.clear_plan_cache()
        hp.clear_matrix_plan_cache()
        hp.clear_transpose_plan_cache()
        torch.cuda.empty_cache()
    print(json.dumps(record))


if __name__ == "__main__":
    main()
