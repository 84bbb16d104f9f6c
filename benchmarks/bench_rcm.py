#!/usr/bin/env python3
"""Reverse Cuthill-McKee ordering on the device (csrc/rcm.hip, hp.rcm) on one GPU, Int32 indices, Float64 values.

Matrices: the 5-point matrix of a 2048 x 2048 and of a 4096 x 4096 grid and the 7-point matrix of a 128^3 grid, each
shuffled by a fixed random symmetric permutation (``hp.select(A, q, q)``), as a mesh generator or a file might deliver it.

For each, in ONE process, warm-up first, medians (and minima):
  rcm        hp.rcm of the shuffled matrix, host wall time around the call (it ends in a read-back), and its split into
             `graph` (count, fill, degrees, the sort by degree), `narrow` (launches of the one-workgroup kernel with their
             record read-backs) and `wide` (device-wide levels with their sorts and read-backs)
  host       the route the library had: structure to the host, scipy's reverse_cuthill_mckee, upload of p (host wall time)
  select     hp.select(A, p, p), HIP events
  spmv       A @ x of the shuffled, the reordered and the natural-order matrix, HIP events around --products products; the
             natural order is the bound a reordering can approach, not reach.  Which plans hold the 16-bit columns (cols16)
             and the pattern table is noted.
  pays after (rcm + select) / (spmv shuffled - spmv reordered) products
and hp.rcm of the natural-order matrix: a matrix already in a good order gains nothing.

Writes <out>/bench_rcm.json and <out>/MEASUREMENTS_rcm.md (default out: profiles/) and prints the JSON line.
usage: python benchmarks/bench_rcm.py [--cases 2048,4096,128] [--calls C] [--warmup W] [--products P] [--host-calls H] [--out DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmarks.bench_select import build, timed_events          # noqa: E402  (the same matrices, the same event timing)


def med(values, digits=3):
    return round(float(np.median(values)), digits), round(float(np.min(values)), digits)


def time_rcm(A, calls, warmup):
    """wall milliseconds of hp.rcm and of its parts: (total, graph, narrow, wide), each (median, min); the last result"""
    import torch
    from hpcla_amd.rcm import _rcm
    rows = []
    out = None
    for k in range(warmup + calls):
        t = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = _rcm(A, True, t)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        if k >= warmup:
            rows.append([1e3 * total, 1e3 * t["graph"], 1e3 * t["narrow"], 1e3 * t["wide"]])
    cols = list(zip(*rows))
    return [med(c) for c in cols], out


def time_spmv(A, x, products, calls, warmup):
    """milliseconds per product"""
    def run():
        y = None
        for _ in range(products):
            y = A @ x
        return y
    m, lo = timed_events(run, calls, warmup)
    return round(m / products, 5), round(lo / products, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048,4096,128")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--products", type=int, default=50)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import scipy.sparse as sp
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    import torch
    import hpcla_amd as hp

    assert torch.cuda.is_available(), "bench_rcm needs a GPU"
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    out = {"bench": "rcm", "calls": args.calls, "warmup": args.warmup, "products": args.products, "host_calls": args.host_calls,
           "frontier_cap": int(hp._capi.load().hpcla_rcm_frontier_cap()),
           "candidate_cap": int(hp._capi.load().hpcla_rcm_candidate_cap()), "cases": {}}
    for case in (int(c) for c in args.cases.split(",") if c):
        A, ci, rp = build(hp, backend, case)
        del ci, rp
        n = A.shape[0]
        g = torch.Generator(device="cuda")
        g.manual_seed(case)
        q = torch.randperm(n, generator=g, device="cuda")
        S = hp.select(A, q, q)                                             # the shuffled matrix
        rec = {"n": n, "nnz": A.nnz}
        (rec["rcm_ms"], rec["graph_ms"], rec["narrow_ms"], rec["wide_ms"]), (p, info) = time_rcm(S, args.calls, args.warmup)
        rec["info"] = dict(vars(info))
        rec["select_ms"] = timed_events(lambda: hp.select(S, p, p), args.calls, args.warmup)
        B = hp.select(S, p, p)
        xg = np.cos(np.arange(n, dtype=np.float64))
        x = hp.HPCVector.from_global(xg, backend)
        for name, M in (("shuffled", S), ("reordered", B), ("natural", A)):
            rec[f"spmv_{name}_ms"] = time_spmv(M, x, args.products, args.calls, args.warmup + 3)
            plan = hp.get_vector_plan(M, x)
            rec[f"plan_{name}"] = {"cols16": plan.cols16 is not None, "patterns": plan.patterns is not None}
        # the reordered product is the shuffled product permuted
        ys, yb = (S @ x).local_values(), (B @ hp.take(x, p)).local_values()
        rec["product_max_abs_diff"] = float(np.abs(yb - ys[p.cpu().numpy()]).max())
        gain = rec["spmv_shuffled_ms"][0] - rec["spmv_reordered_ms"][0]
        rec["spmv_shuffled_over_reordered"] = round(rec["spmv_shuffled_ms"][0] / rec["spmv_reordered_ms"][0], 2)
        rec["spmv_reordered_over_natural"] = round(rec["spmv_reordered_ms"][0] / rec["spmv_natural_ms"][0], 2)
        rec["products_to_pay"] = round((rec["rcm_ms"][0] + rec["select_ms"][0]) / gain, 1) if gain > 0 else None
        # a matrix already in a good order
        (t_nat, _, _, _), (_, info_nat) = time_rcm(A, max(2, args.calls // 2), 1)
        rec["natural_rcm_ms"] = t_nat
        rec["natural_info"] = dict(vars(info_nat))
        if args.host_calls:
            t = []
            ph = None
            for _ in range(args.host_calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                H = sp.csr_matrix((np.ones(S.nnz, dtype=np.int8), S.col_indices[S.colval_target().cpu().numpy()],
                                   S.rowptr_target.cpu().numpy()), shape=(n, n))
                ph = torch.from_numpy(reverse_cuthill_mckee(H, symmetric_mode=True).astype(np.int64)).cuda()
                torch.cuda.synchronize()
                t.append(1e3 * (time.perf_counter() - t0))
            rec["host_ms"] = med(t, 1)
            rec["host_over_rcm"] = round(rec["host_ms"][0] / rec["rcm_ms"][0], 1)
            rec["host_bandwidth_after"] = hp.bandwidth(hp.select(S, ph, ph))
            del H, ph
        out["cases"][str(case)] = rec
        print(f"# {case} {json.dumps(rec)}", file=sys.stderr, flush=True)
        del A, S, B, x, p, q
        hp.clear_plan_cache()
        torch.cuda.empty_cache()

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_rcm.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "MEASUREMENTS_rcm.md"), "w") as f:
        f.write("# Reverse Cuthill-McKee ordering: measurements\n\n")
        f.write(f"`python benchmarks/bench_rcm.py --cases {args.cases} --calls {args.calls} --warmup {args.warmup} --products "
                f"{args.products} --host-calls {args.host_calls}` on one MI355X, Int32 / Float64, `median (min)` in milliseconds.  "
                "Each matrix is shuffled by a fixed random symmetric permutation.  `rcm` is host wall time around `hp.rcm` (it ends "
                "in a read-back); `graph`, `narrow`, `wide` are its parts between the read-backs that end them.  `host` is the "
                "structure to the host, scipy's `reverse_cuthill_mckee` and the upload of `p`.  `select` and the products are "
                f"timed by HIP events, the products {args.products} at a time.  Caps: frontier {out['frontier_cap']}, candidates "
                f"{out['candidate_cap']}.\n\n")
        f.write("| case | rows | rcm | graph | narrow | wide | narrow launches, wide levels, levels | bandwidth before -> after (scipy) | "
                "host | host / rcm | select |\n|" + "---|" * 11 + "\n")

        def mm(r, k):
            return f"{r[k][0]} ({r[k][1]})" if k in r else "-"

        for name, r in out["cases"].items():
            i = r["info"]
            f.write(f"| {name} | {r['n']} | {mm(r, 'rcm_ms')} | {mm(r, 'graph_ms')} | {mm(r, 'narrow_ms')} | {mm(r, 'wide_ms')} | "
                    f"{i['narrow_launches']}, {i['wide_levels']}, {i['levels']} | {i['bandwidth_before']} -> {i['bandwidth_after']} "
                    f"({r.get('host_bandwidth_after', '-')}) | {mm(r, 'host_ms')} | {r.get('host_over_rcm', '-')} | {mm(r, 'select_ms')} |\n")
        f.write("\n| case | SpMV shuffled | SpMV reordered | SpMV natural | shuffled / reordered | reordered / natural | cols16, patterns: "
                "shuffled; reordered; natural | products that pay for rcm + select | max abs difference of the product |\n|" + "---|" * 9 + "\n")
        for name, r in out["cases"].items():
            plans = "; ".join(f"{r['plan_' + k]['cols16']}, {r['plan_' + k]['patterns']}" for k in ("shuffled", "reordered", "natural"))
            f.write(f"| {name} | {mm(r, 'spmv_shuffled_ms')} | {mm(r, 'spmv_reordered_ms')} | {mm(r, 'spmv_natural_ms')} | "
                    f"{r['spmv_shuffled_over_reordered']} | {r['spmv_reordered_over_natural']} | {plans} | {r['products_to_pay']} | "
                    f"{r['product_max_abs_diff']:.2e} |\n")
        f.write("\nA matrix already in a good order (the natural order, no shuffle):\n\n| case | rcm | bandwidth before -> after | levels |\n"
                "|---|---|---|---|\n")
        for name, r in out["cases"].items():
            i = r["natural_info"]
            f.write(f"| {name} | {mm(r, 'natural_rcm_ms')} | {i['bandwidth_before']} -> {i['bandwidth_after']} | {i['levels']} |\n")
        f.write("\nWhere it loses.  The 2-D walks are latency-bound: thousands of levels of a few thousand vertices, each a pass of ONE "
                "workgroup (narrow) or three launches, a sort and a read-back (wide), so the time follows the number of levels, not the "
                "bytes.  A level of more than `candidates / mean degree` vertices leaves the one-workgroup kernel.  The reordered grid is "
                "in diagonal (level) order: it regains the 16-bit columns but not the pattern table, so it stays behind the natural "
                "order.  A matrix already in a good order pays the full walk and gains nothing.\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
