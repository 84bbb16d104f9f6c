#!/usr/bin/env python3
"""``hp.gmres`` and ``hp.bicgstab`` with the fine-grained ILU(0) preconditioner (``hp.ilu0``) against Jacobi, one GPU, Float64,
Int32 indices: the 5-point convection-diffusion stencil of the test case (4, -1.5, -0.5, -1.3, -0.7, unscaled) at 2048 x 2048
and 4096 x 4096, and the 7-point one of benchmarks/bench_bicgstab.py on the 512 x 512 x 64 slab.  b = fill_uniform.

Per matrix:

  kernels      one SpMV of A (median of 50); one ``apply`` at solve_sweeps = 3 and 2 with 1, 2, 4 and 8 lanes per row (median of
               ``--runs`` after a warm-up); one lower and one upper triangular sweep alone with 1 and 4 lanes, next to the bytes
               the sweep has to move when every value is moved once (per row: rhs, out, in, the row pointer and the diagonal
               position, dinv for the upper sweep; per stored entry of the triangle: 4 + 8) and the rate that makes.
  setup        HIP events around ``hp.ilu0(A)``: the first call and the median of later calls, split into the structure (count,
               fill, the stable sort that builds the column view) and the factorisation (gather, init, sweeps, pivots, the
               read-back); ``ILU0.update(A)``: the repeated structure.
  to 1e-8      iterations and milliseconds of ``hp.gmres(restart=30)`` and ``hp.bicgstab`` with ``"jacobi"``, ``hp.ilu0(A)`` and
               ``hp.ilu0(A, solve_sweeps=2)``, ``check_every=32``, events around the call, median of ``--solves`` calls, capped at
               ``--maxiter`` steps.

Prints one JSON line and writes <out>/bench_ilu0.json and <out>/bench_ilu0_tables.md (default out: profiles/).
usage: python benchmarks/bench_ilu0.py [--cases 2048,4096,3d] [--runs R] [--solves S] [--maxiter K] [--out DIR] [--small]"""
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
OFFDIAG_2D = (-1.5, -0.5, -1.3, -0.7)            # column offsets -1, +1, -nx, +nx: tests/_bicgstab_cases.py


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def median_ms(torch, fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    return statistics.median(event_ms(torch, fn)[0] for _ in range(runs))


def stencil(hp, torch, backend, dims):
    if len(dims) == 3:
        from benchmarks.bench_bicgstab import convection_diffusion
        return convection_diffusion(hp, torch, backend, dims)
    n = int(np.prod(dims))
    nnz = hp._capi.load().hpcla_poisson2d_nnz(dims[0], dims[1], 0, n)
    rp = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ci = torch.empty(nnz, dtype=torch.int64, device="cuda")
    va = torch.empty(nnz, dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_gen_poisson2d", dims[0], dims[1], 0, n, rp.data_ptr(), ci.data_ptr(), va.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    off = ci - torch.repeat_interleave(torch.arange(n, device="cuda"), rp[1:] - rp[:-1])
    for o, val in zip((-1, 1, -dims[0], dims[0]), OFFDIAG_2D):
        va[off == o] = val
    del off
    return hp.HPCSparseMatrix_local_device(rp, ci, va, n, backend, col_window=(0, n - 1))


def triangle_bytes(M, upper):
    """Bytes one triangular sweep moves when every value is moved once."""
    import torch
    rows = torch.repeat_interleave(torch.arange(M.n, device=M._cols.device, dtype=torch.int32), (M._rowptr[1:] - M._rowptr[:-1]).long())
    entries = int(((M._cols > rows) if upper else (M._cols < rows)).sum().item())
    return M.n * (8 + 8 + 8 + 4 + 4 + (8 if upper else 0)) + entries * 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048,4096,3d")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small", action="store_true", help="small grids (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from hpcla_amd import workloads as wl
    from hpcla_amd.vectors import current_stream_ptr, dptr
    if not torch.cuda.is_available():
        raise SystemExit("bench_ilu0.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    record = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "solves": args.solves, "rtol": 1e-8, "maxiter": args.maxiter}
    lines = []
    for key in args.cases.split(","):
        label, dims = (SMALL if args.small else CASES)[key.strip()]
        n = int(np.prod(dims))
        A = stencil(hp, torch, backend, dims)
        b = hp.HPCVector.zeros(A.row_partition, backend)
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, n, wl.SEED_RHS, torch.cuda.current_stream().cuda_stream)
        y = b.similar()
        hp.mul_(y, A, b)
        spmv = median_ms(torch, lambda: hp.mul_(y, A, b), 50)
        rec = {"rows": n, "nnz": int(A.nnz), "spmv_ms": round(spmv, 4), "setup": {}, "apply_ms": {}, "trisweep": {}, "solve": {}}

        # -- setup
        first, M = event_ms(torch, lambda: hp.ilu0(A))
        later = [event_ms(torch, lambda: hp.ilu0(A))[0] for _ in range(args.runs)]
        structure = [event_ms(torch, lambda: M._structure(A))[0] for _ in range(args.runs)]
        update = [event_ms(torch, lambda: M.update(A))[0] for _ in range(args.runs)]
        rec["setup"] = {"first_call_ms": round(first, 3), "later_calls_ms": round(statistics.median(later), 3),
                        "structure_ms": round(statistics.median(structure), 3), "update_ms": round(statistics.median(update), 3)}

        # -- one application, one sweep
        z = b.similar()
        for s in (3, 2):
            M.solve_sweeps = s
            for lanes in (1, 2, 4, 8):
                M.lanes = lanes
                rec["apply_ms"][f"solve_sweeps={s},lanes={lanes}"] = round(median_ms(torch, lambda: M.apply(b, out=z), args.runs), 4)
        M.solve_sweeps, M.lanes = 3, 1
        for upper in (0, 1):
            nbytes = triangle_bytes(M, upper)
            for lanes in (1, 4):
                fn = lambda: hp._capi.call("hpcla_ilu_trisweep_f64", dptr(M._rowptr), dptr(M._cols), dptr(M._diag), dptr(M._f), dptr(b.v),
                                           dptr(y.v), dptr(M._dinv) if upper else None, dptr(z.v), n, upper, lanes, current_stream_ptr())
                t = median_ms(torch, fn, args.runs)
                rec["trisweep"][f"{'upper' if upper else 'lower'},lanes={lanes}"] = {
                    "ms": round(t, 4), "algorithmic_bytes": nbytes, "GBps_of_algorithmic_bytes": round(nbytes / t / 1e6, 1)}

        # -- the solves
        pre = {"jacobi": "jacobi", "ilu0": hp.ilu0(A), "ilu0, solve_sweeps=2": hp.ilu0(A, solve_sweeps=2)}
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
        lines += [f"### {label} ({n} rows, {int(A.nnz)} stored entries; one SpMV of A: {spmv:.3f} ms)", "",
                  f"setup: first call {first:.1f} ms, later calls {rec['setup']['later_calls_ms']:.1f} ms (of which the structure "
                  f"{rec['setup']['structure_ms']:.1f} ms), update on the same structure {rec['setup']['update_ms']:.2f} ms", "",
                  "| apply | ms | SpMVs of A |", "|---|---|---|"]
        lines += [f"| {k} | {v:.4f} | {v / spmv:.2f} |" for k, v in rec["apply_ms"].items()]
        lines += ["", "| triangular sweep | ms | algorithmic bytes | GB/s of them |", "|---|---|---|---|"]
        lines += [f"| {k} | {v['ms']:.4f} | {v['algorithmic_bytes']} | {v['GBps_of_algorithmic_bytes']} |" for k, v in rec["trisweep"].items()]
        lines += ["", "| solve | iterations | status | ms to 1e-8, median (min, max) | time against Jacobi | true residual |", "|---|---|---|---|---|---|"]
        for k, v in rec["solve"].items():
            jac = rec["solve"][k.split(",")[0] + ", jacobi"]["ms"][0]
            lines.append(f"| {k} | {v['iterations']} | {v['status']} | {v['ms'][0]:.1f} ({v['ms'][1]:.1f}, {v['ms'][2]:.1f}) | "
                         f"{v['ms'][0] / jac:.3f} | {v['true_residual']:.2e} |")
        lines.append("")
        del A, b, y, z, M, pre
        hp.clear_plan_cache()
        torch.cuda.empty_cache()
        os.makedirs(args.out, exist_ok=True)                     # after every case: a cut-off run keeps what it measured
        with open(os.path.join(args.out, "bench_ilu0.json"), "w") as f:
            json.dump(record, f, indent=1)
        with open(os.path.join(args.out, "bench_ilu0_tables.md"), "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
