#!/usr/bin/env python3
"""Range indexing of a sparse matrix (csrc/submatrix.hip) on the config-2 matrix: the 5-point Laplacian of a 4096 x 4096 grid
(n = 16 777 216 rows, 83 869 696 stored entries), Int32 indices, Float64 values, one GPU.  Four cuts:

  interior   A[n/4:3n/4, n/4:3n/4]
  slab       A[n/4:3n/4, :]
  extract    plan.extract(A) of the first (the values pass alone)
  column     A[:, n/2]

For each, measured in ONE process:
  (a) the time of the public call (HIP events on the stream around the whole call: kernels, the one stream synchronisation
      that returns the sizes, the allocations of the FRESH output arrays every call makes, the read-back of col_indices), the
      host wall time of the same call ending in a device synchronise, and the bytes by the model below;
  (b) a plain device-to-device copy moving the same number of bytes (a copy of B / 2 bytes reads B / 2 and writes B / 2), and
      the ratio of (a) to it: the floor;
  (c) the route a user has without the feature: scipy's slice of the host CSR plus HPCSparseMatrix_local (the upload and the
      host-side column compression) -- host wall time ending in a device synchronise.

Byte model (I = 4 index bytes, E = 8 value bytes; nsel selected rows, nnz' kept entries, span = stored entries of the
selected rows, width = compressed columns in the window, ncomp = columns that occur):
  locate   reads 2 row bounds per row (I (nsel + 1)), writes start and count (16 nsel)            [binary-search probes not counted]
  mark     reads the span's columns (I span), clears and sets the bitmap (2 width)
  scans    counts read twice (16 nsel), rowptr' written (I (nsel + 1)); bitmap read twice (2 width), look-up table written
           (8 width), col_indices written (8 ncomp)
  fill     reads rowptr' and the starts (I nsel + 8 nsel), reads the kept runs ((I + E) nnz'), writes colval' and nzval'
           ((I + E) nnz')                                                                        [look-up table reads: L2, not counted]
  extract  reads rowptr' and the starts, reads and writes E nnz'
  column   reads 2 row bounds per row, writes E per row                                           [binary-search probes not counted]

Writes one JSON record to <out>/bench_submatrix.json and a table to <out>/MEASUREMENTS_submatrix.md (default out: profiles/),
and prints the JSON line.
usage: python benchmarks/bench_submatrix.py [--grid N] [--calls C] [--warmup W] [--host-calls H] [--out DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
I_B, E_B = 4, 8


def timed_events(fn, calls, warmup):
    """median / min of the device time of fn (HIP events around every call) and of its host wall time (device drained)"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(calls):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(e))
        del out
    return float(np.median(dev)), float(np.min(dev)), float(np.median(wall))


def timed_wall(fn, calls):
    import torch
    t = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
        del out
    return float(np.median(t)), float(np.min(t))


def cut_bytes(nsel, nnz_out, span, width, ncomp):
    locate = I_B * (nsel + 1) + 16 * nsel
    mark = I_B * span + 2 * width
    scans = 16 * nsel + I_B * (nsel + 1) + 2 * width + 8 * width + 8 * ncomp
    fill = (I_B + 8) * nsel + 2 * (I_B + E_B) * nnz_out
    return {"locate": locate, "mark": mark, "scans": scans, "fill": fill, "total": locate + mark + scans + fill}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import scipy.sparse as sp
    import torch
    import hpcla_amd as hp

    assert torch.cuda.is_available(), "bench_submatrix needs a GPU"
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    nx = ny = args.grid
    n = nx * ny
    lib = hp._capi.load()
    s0 = torch.cuda.current_stream().cuda_stream
    nnz = lib.hpcla_poisson2d_nnz(nx, ny, 0, n)
    rp_d = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ci_d = torch.empty(nnz, dtype=torch.int64, device="cuda")
    va_d = torch.empty(nnz, dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_gen_poisson2d", nx, ny, 0, n, rp_d.data_ptr(), ci_d.data_ptr(), va_d.data_ptr(), s0)
    A = hp.HPCSparseMatrix_local_device(rp_d, ci_d, va_d, n, backend, col_window=(0, n - 1))
    S = sp.csr_matrix((va_d.cpu().numpy(), ci_d.cpu().numpy(), rp_d.cpu().numpy()), shape=(n, n))     # the user's host copy
    del rp_d, ci_d, va_d
    q0, q1, k = n // 4, 3 * n // 4, n // 2
    rowptr = S.indptr

    def plain_copy_ms(nbytes):
        half = max(int(nbytes) // 2, 16)
        src = torch.empty(half, dtype=torch.uint8, device="cuda")
        med, mn, _ = timed_events(lambda: torch.empty_like(src).copy_(src), args.calls, args.warmup)
        del src
        torch.cuda.empty_cache()
        return med, mn

    def host_cut(r0, r1, c0, c1):
        loc = S[r0:r1, c0:c1]
        return hp.HPCSparseMatrix_local(loc.indptr, loc.indices, loc.data, c1 - c0, backend)

    def host_column(kk):
        col = np.asarray(S[:, kk].todense()).ravel()
        return hp.HPCVector.from_global(col, backend)

    out = {"bench": "submatrix", "grid": args.grid, "nrows": n, "nnz": int(nnz), "index_bytes": I_B, "value_bytes": E_B,
           "calls": args.calls, "warmup": args.warmup, "host_calls": args.host_calls, "cuts": {}}

    def record(name, fn, nbytes, parts, host_fn, check):
        med, mn, wall = timed_events(fn, args.calls, args.warmup)
        cp_med, cp_min = plain_copy_ms(nbytes)
        rec = {"bytes": int(nbytes), "bytes_by_pass": parts, "median_ms": round(med, 4), "min_ms": round(mn, 4),
               "host_wall_median_ms": round(wall, 4), "GBps_by_model": round(nbytes / (med * 1e-3) / 1e9, 1),
               "plain_copy_same_bytes_median_ms": round(cp_med, 4), "ratio_to_plain_copy": round(med / cp_med, 2)}
        if host_fn is not None:
            h_med, h_min = timed_wall(host_fn, args.host_calls)
            rec["host_route_median_ms"], rec["host_route_min_ms"] = round(h_med, 2), round(h_min, 2)
            rec["speedup_vs_host_route"] = round(h_med / wall, 1)
        rec["matches_host_route"] = bool(check())
        out["cuts"][name] = rec
        torch.cuda.empty_cache()

    def same(B, H):
        return (np.array_equal(B.rowptr, H.rowptr) and np.array_equal(B.colval, H.colval)
                and np.array_equal(B.col_indices, H.col_indices) and torch.equal(B.nzval, H.nzval))

    for name, (r0, r1, c0, c1) in (("interior", (q0, q1, q0, q1)), ("slab", (q0, q1, 0, n))):
        B = A[r0:r1, c0:c1]
        span = int(rowptr[r1] - rowptr[r0])
        parts = cut_bytes(r1 - r0, B.nnz, span, c1 - c0, B.ncols_compressed)
        record(name, lambda: A[r0:r1, c0:c1], parts["total"], parts, lambda: host_cut(r0, r1, c0, c1),
               lambda: same(A[r0:r1, c0:c1], host_cut(r0, r1, c0, c1)))
        del B
    plan = hp.get_submatrix_plan(A, slice(q0, q1), slice(q0, q1))
    nsel, nnz_out = q1 - q0, plan.matrix.nnz
    ebytes = (I_B + 8) * nsel + 2 * E_B * nnz_out
    record("extract", lambda: plan.extract(A), ebytes, {"values": ebytes, "total": ebytes}, None,
           lambda: torch.equal(plan.extract(A).nzval, plan.matrix.nzval))
    cbytes = I_B * (n + 1) + E_B * n
    record("column", lambda: A[:, k], cbytes, {"column": cbytes, "total": cbytes}, lambda: host_column(k),
           lambda: torch.equal(A[:, k].v, host_column(k).v))

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_submatrix.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "MEASUREMENTS_submatrix.md"), "w") as f:
        f.write("# Range indexing of a sparse matrix: measurements\n\n")
        f.write(f"`python benchmarks/bench_submatrix.py --grid {args.grid} --calls {args.calls} --warmup {args.warmup} "
                f"--host-calls {args.host_calls}` on one MI355X: the 5-point matrix of a {args.grid} x {args.grid} grid "
                f"({n} rows, {int(nnz)} stored entries), Int32 / Float64.  Times are medians; the device time is between HIP events "
                "around the whole public call (kernels, the one synchronisation that returns the sizes, allocation of fresh "
                "outputs, read-back of `col_indices`).  The byte model is the one in the script's header; the plain copy moves the "
                "same number of bytes (half read, half written).  The host route is scipy's slice of the host CSR plus "
                "`HPCSparseMatrix_local` (host wall time).\n\n")
        f.write("| cut | bytes (model) | device ms | host wall ms | GB/s (model) | plain copy ms | ratio to copy | host route ms | "
                "speed-up vs host route | equal to host route |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for name, r in out["cuts"].items():
            f.write(f"| {name} | {r['bytes']} | {r['median_ms']} | {r['host_wall_median_ms']} | {r['GBps_by_model']} | "
                    f"{r['plain_copy_same_bytes_median_ms']} | {r['ratio_to_plain_copy']} | {r.get('host_route_median_ms', '-')} | "
                    f"{r.get('speedup_vs_host_route', '-')} | {r['matches_host_route']} |\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
