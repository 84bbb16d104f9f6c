#!/usr/bin/env python3
"""``hp.cg`` with the factorised sparse approximate inverse preconditioner (``hp.fsai``) against Jacobi, one GPU, Float64, Int32
indices: the 5-point Laplacian at 2048 x 2048 and 4096 x 4096, and config 4's per-GPU share, the 7-point Laplacian of a
512 x 512 x 64 slab (the matrix of ``bench.py --workload poisson3d_cg``).  b = fill_uniform.

Per matrix and per preconditioner -- ``"jacobi"``, ``hp.fsai(A)``, ``hp.fsai(A, pattern=hp.spgemm(A, A))``:

  setup        HIP events around the whole public call ``hp.fsai(...)`` (the count, its read-back, the factor kernel, the error
               word's read-back, the assembly of G and the transpose): the FIRST call, which also builds the transpose plan and
               is followed by the first products' plan construction, and the median of ``--runs`` later calls on the same
               structure; next to one SpMV of A (median of 50) for scale.  The A^2 pattern's ``hp.spgemm`` is timed on its own.
  ms / iter    a whole public call of ``--iters`` iterations (``rtol=0``: the stop rule never fires), the three variants
               ALTERNATING call by call, ``--runs`` timed calls after ``--warmup`` untimed ones; median (min, max).
  to 1e-8      iterations and milliseconds of ``hp.cg(rtol=1e-8, check_every=32)``, events around the call, median of
               ``--solves`` calls (the count is the same in each).

Prints one JSON line and writes <out>/bench_fsai.json and <out>/bench_fsai_tables.md (default out: profiles/).
usage: python benchmarks/bench_fsai.py [--cases 2048,4096,3d] [--runs R] [--warmup W] [--iters K] [--solves S] [--out DIR] [--small]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048,4096,3d")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=60000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small", action="store_true", help="small grids (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from hpcla_amd import workloads as wl
    from benchmarks.bench_pcg import timed_table
    from benchmarks.extra_workloads import device_stencil
    if not torch.cuda.is_available():
        raise SystemExit("bench_fsai.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    K = args.iters
    record = {"device": torch.cuda.get_device_name(0), "iters_per_call": K, "runs": args.runs, "warmup": args.warmup,
              "solves": args.solves, "rtol": 1e-8}
    lines = []
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

        M = {"jacobi": "jacobi"}
        t_sq, P = event_ms(torch, lambda: hp.spgemm(A, A))
        rec["spgemm_pattern_ms"] = round(t_sq, 3)
        for name, pattern in (("fsai(A)", None), ("fsai(A, A^2)", P)):
            first, F = event_ms(torch, lambda: hp.fsai(A, pattern=pattern))
            later = [event_ms(torch, lambda: hp.fsai(A, pattern=pattern))[0] for _ in range(args.runs)]
            M[name] = F
            rec["setup"][name] = {"first_call_ms": round(first, 3), "later_calls_ms": [round(statistics.median(later), 3),
                                  round(min(later), 3), round(max(later), 3)], "nnz_G": int(F.G.nnz), "max_row": F.max_row}
        del P
        ws = hp.PCGWorkspace(b, K + 2)

        def fixed(m):
            _, info = hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=K, M=m, workspace=ws)
            assert info.iterations == K and info.status == "maxiter", info.status

        table = timed_table(torch, {k: (lambda m=m: fixed(m)) for k, m in M.items()}, args.runs, args.warmup, K)
        rec["per_iteration"] = {k: [round(x, 5) for x in v] for k, v in table.items()}
        for name, m in M.items():
            times, its = [], None
            for _ in range(args.solves):
                t, (x, info) = event_ms(torch, lambda: hp.cg(A, b, rtol=1e-8, maxiter=args.maxiter, M=m, check_every=32, workspace=ws))
                times.append(t)
                its = info.iterations
            true = hp.norm(b - A @ x) / hp.norm(b)
            rec["solve"][name] = {"iterations": its, "status": info.status, "ms": [round(statistics.median(times), 2),
                                  round(min(times), 2), round(max(times), 2)], "true_residual": float(f"{true:.3e}")}
        record[label] = rec
        jac = rec["solve"]["jacobi"]
        lines += [f"### {label} ({n} rows, {int(A.nnz)} stored entries; one SpMV of A: {spmv:.3f} ms; hp.spgemm(A, A): {t_sq:.1f} ms)", "",
                  "| M | setup, first call (ms) | setup, later calls (ms) | entries of G | ms / iteration, median (min, max) | "
                  "iterations to 1e-8 | ms to 1e-8, median (min, max) | time against Jacobi | true residual |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for name in M:
            st, it, so = rec["setup"].get(name), rec["per_iteration"][name], rec["solve"][name]
            lines.append(f"| {name} | {st['first_call_ms'] if st else '-'} | {st['later_calls_ms'][0] if st else '-'} | "
                         f"{st['nnz_G'] if st else '-'} | {it[0]:.4f} ({it[1]:.4f}, {it[2]:.4f}) | {so['iterations']} ({so['status']}) | "
                         f"{so['ms'][0]:.1f} ({so['ms'][1]:.1f}, {so['ms'][2]:.1f}) | {so['ms'][0] / jac['ms'][0]:.3f} | "
                         f"{so['true_residual']:.2e} |")
        lines.append("")
        del A, b, y, ws, M
        hp.clear_plan_cache()
        hp.clear_matrix_plan_cache()
        hp.clear_transpose_plan_cache()
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_fsai.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out, "bench_fsai_tables.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
