#!/usr/bin/env python3
"""``hp.gmres`` and ``hp.bicgstab`` with the nonsymmetric multigrid preconditioner (``hp.amg(A, symmetric=False)``) against Jacobi
and ``hp.ilu0(A)`` measured in the same run, one GPU, Float64, Int32 indices: the matrices of benchmarks/bench_ilu0.py -- the
unscaled 5-point convection-diffusion stencil (4, -1.5, -0.5, -1.3, -0.7) at 2048 x 2048 and 4096 x 4096 and the 7-point one
on the 512 x 512 x 64 slab.  b = fill_uniform.

Per matrix:

  kernels      one SpMV of A (median of 50); one ``apply`` of the cycle and one of ILU(0) (median of ``--runs`` after a warm-up).
  setup        HIP events around ``hp.amg(A, symmetric=False)``: the first call and the median of ``--setups`` later calls; the
               levels, the rounds of the independent set, the splits of the two products and the operator complexity; the
               same for ``hp.ilu0(A)``.
  to 1e-8      iterations and milliseconds of ``hp.gmres(restart=30)`` and ``hp.bicgstab`` with ``"jacobi"``, ``hp.ilu0(A)`` and
               the hierarchy, ``check_every=32``, events around the call, median (min, max) of ``--solves`` calls, capped at
               ``--maxiter`` steps; the true residual of the last call.

Prints one JSON line and writes <out>/bench_amg_nonsym.json and <out>/bench_amg_nonsym_tables.md (default out: profiles/).
usage: python benchmarks/bench_amg_nonsym.py [--cases 2048,4096,3d] [--runs R] [--setups T] [--solves S] [--maxiter K] [--out DIR]
                                             [--small]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048,4096,3d")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--setups", type=int, default=3)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small", action="store_true", help="small grids (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from benchmarks.bench_ilu0 import CASES, SMALL, event_ms, median_ms, stencil
    from hpcla_amd import workloads as wl
    if not torch.cuda.is_available():
        raise SystemExit("bench_amg_nonsym.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    record = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "setups": args.setups, "solves": args.solves, "rtol": 1e-8,
              "maxiter": args.maxiter}
    lines = []
    for key in args.cases.split(","):
        label, dims = (SMALL if args.small else CASES)[key.strip()]
        n = int(np.prod(dims))
        A = stencil(hp, torch, backend, dims)
        b = hp.HPCVector.zeros(A.row_partition, backend)
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, n, wl.SEED_RHS, torch.cuda.current_stream().cuda_stream)
        y, z = b.similar(), b.similar()
        hp.mul_(y, A, b)
        spmv = median_ms(torch, lambda: hp.mul_(y, A, b), 50)
        rec = {"rows": n, "nnz": int(A.nnz), "spmv_ms": round(spmv, 4), "setup": {}, "apply_ms": {}, "solve": {}}

        # -- setup
        try:
            first, M = event_ms(torch, lambda: hp.amg(A, symmetric=False))
        except (ValueError, NotImplementedError) as exc:         # a coarse diagonal that is not positive, a product over the bound
            M, first = None, None
            rec["setup"]["amg"] = {"error": str(exc)}
        if M is not None:
            later = [event_ms(torch, lambda: hp.amg(A, symmetric=False))[0] for _ in range(args.setups)]
            rec["setup"]["amg"] = {"first_call_ms": round(first, 2), "later_calls_ms": round(statistics.median(later), 2),
                                   "levels": [l.n for l in M.levels], "rounds": [l.rounds for l in M.levels[:-1]],
                                   "galerkin_split": [l.galerkin for l in M.levels[:-1]],
                                   "restriction_split": [l.restriction_split for l in M.levels[:-1]],
                                   "last_level": "dense inverse" if M.levels[-1].inverse is not None else f"{M.levels[-1].sweeps} sweeps",
                                   "operator_complexity": round(M.operator_complexity, 4)}
        first_ilu, ilu = event_ms(torch, lambda: hp.ilu0(A))
        later = [event_ms(torch, lambda: hp.ilu0(A))[0] for _ in range(args.setups)]
        rec["setup"]["ilu0"] = {"first_call_ms": round(first_ilu, 2), "later_calls_ms": round(statistics.median(later), 2)}

        # -- one application
        rec["apply_ms"]["ilu0"] = round(median_ms(torch, lambda: ilu.apply(b, out=z), args.runs), 4)
        if M is not None:
            rec["apply_ms"]["amg"] = round(median_ms(torch, lambda: M.apply(b, out=z), args.runs), 4)

        # -- the solves
        pre = {"jacobi": "jacobi", "ilu0": ilu}
        if M is not None:
            pre["amg"] = M
        for sname, solver in (("gmres(30)", hp.gmres), ("bicgstab", hp.bicgstab)):
            for pname, m in pre.items():
                times = []
                for _ in range(args.solves):
                    t, (x, info) = event_ms(torch, lambda: solver(A, b, rtol=1e-8, maxiter=args.maxiter, M=m, check_every=32))
                    times.append(t)
                true = hp.norm(b - A @ x) / hp.norm(b)
                rec["solve"][f"{sname}, {pname}"] = {"iterations": info.iterations, "status": info.status,
                                                     "ms": [round(statistics.median(times), 2), round(min(times), 2), round(max(times), 2)],
                                                     "true_residual": float(f"{true:.3e}")}
        record[label] = rec
        lines += [f"### {label} ({n} rows, {int(A.nnz)} stored entries; one SpMV of A: {spmv:.3f} ms)", ""]
        s = rec["setup"]
        if M is not None:
            a = s["amg"]
            lines += [f"amg setup: first call {a['first_call_ms']:.1f} ms, later calls {a['later_calls_ms']:.1f} ms; levels {a['levels']}, "
                      f"rounds {a['rounds']}, splits of Tt A {a['restriction_split']} and of R (A P) {a['galerkin_split']}, last level: "
                      f"{a['last_level']}, operator complexity {a['operator_complexity']:.3f}", ""]
        else:
            lines += [f"amg setup: {s['amg']['error']}", ""]
        lines += [f"ilu0 setup: first call {s['ilu0']['first_call_ms']:.1f} ms, later calls {s['ilu0']['later_calls_ms']:.1f} ms", "",
                  "| apply | ms | SpMVs of A |", "|---|---|---|"]
        lines += [f"| {k} | {v:.4f} | {v / spmv:.2f} |" for k, v in rec["apply_ms"].items()]
        lines += ["", "| solve | iterations | status | ms to 1e-8, median (min, max) | time against Jacobi | time against ILU(0) | true residual |",
                  "|---|---|---|---|---|---|---|"]
        for k, v in rec["solve"].items():
            jac = rec["solve"][k.split(",")[0] + ", jacobi"]["ms"][0]
            il = rec["solve"][k.split(",")[0] + ", ilu0"]["ms"][0]
            lines.append(f"| {k} | {v['iterations']} | {v['status']} | {v['ms'][0]:.1f} ({v['ms'][1]:.1f}, {v['ms'][2]:.1f}) | "
                         f"{v['ms'][0] / jac:.3f} | {v['ms'][0] / il:.3f} | {v['true_residual']:.2e} |")
        lines.append("")
        del A, b, y, z, M, ilu, pre
        hp.clear_plan_cache()
        torch.cuda.empty_cache()
        os.makedirs(args.out, exist_ok=True)                     # after every case: a cut-off run keeps what it measured
        with open(os.path.join(args.out, "bench_amg_nonsym.json"), "w") as f:
            json.dump(record, f, indent=1)
        with open(os.path.join(args.out, "bench_amg_nonsym_tables.md"), "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
