#!/usr/bin/env python3
"""Index-set selection (csrc/select.hip, hp.select / hp.selection_plan / hp.take) on one GPU, Int32 indices, Float64 values.

Matrices: the 5-point matrix of a 2048 x 2048 and of a 4096 x 4096 grid, the 7-point matrix of a 128^3 grid.  Index sets,
passed as rows AND columns (a symmetric selection, as the solvers need):
  subset90   a sorted random 90 % of the indices (Dirichlet elimination)
  permute    a random permutation (a reordering)
  reverse    n - 1 .. 0

For each, measured in ONE process, warm-up first, HIP events around every call, median and min:
  select     the public call, and its three parts run through the C ABI on the same inputs: `sort` (the stable torch.sort of
             the column list), `structure` (look-up, count and mark, two scans, the read-back of the sizes), `fill`
  extract    plan.extract(A): the values alone, 24 bytes per kept entry (the int64 source position, the value read, the
             value written)
  take       VectorIndexPlan.take(v): 20 bytes per element (the int32 position, the value read, the value written)
  torch      a torch-only route to the same CSR: expand the selected rows' entries, map the columns through a table, ONE
             torch.sort of the composite key row * width + new column, gather, bincount and cumsum
  host       the only route the library had: scipy fancy indexing of a host copy plus HPCSparseMatrix_from_global (host wall
             time, --host-calls calls; the download of A is not counted)
`extract` and `take` are also given as a fraction of the streaming rate the README uses for assembly (--stream-tbps, 6.3).
The long-row case: a 5-point 512 x 512 matrix with one row of 8 * hpcla_select_tile() entries, permuted, against the same
selection of the matrix without that row.

Writes <out>/bench_select.json and <out>/MEASUREMENTS_select.md (default out: profiles/) and prints the JSON line.
usage: python benchmarks/bench_select.py [--cases 2048,4096,128] [--calls C] [--warmup W] [--host-calls H] [--out DIR]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_events(fn, calls, warmup):
    """(median, min) of the device time of fn, HIP events around every call"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev = []
    for _ in range(calls):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        dev.append(a.elapsed_time(e))
        del out
    return round(float(np.median(dev)), 4), round(float(np.min(dev)), 4)


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
    return round(float(np.median(t)), 2), round(float(np.min(t)), 2)


def build(hp, backend, case):
    """(A, global column ids of its entries, rowptr) on the device"""
    import torch
    lib = hp._capi.load()
    s0 = torch.cuda.current_stream().cuda_stream
    if case == 128:
        nx = ny = nz = 128
        n = nx * ny * nz
        nnz = lib.hpcla_poisson3d_nnz(nx, ny, nz, 0, n)
    else:
        nx = ny = case
        n = nx * ny
        nnz = lib.hpcla_poisson2d_nnz(nx, ny, 0, n)
    rp = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ci = torch.empty(nnz, dtype=torch.int64, device="cuda")
    va = torch.empty(nnz, dtype=torch.float64, device="cuda")
    if case == 128:
        hp._capi.call("hpcla_gen_poisson3d", nx, ny, nz, 0, n, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), s0)
    else:
        hp._capi.call("hpcla_gen_poisson2d", nx, ny, 0, n, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), s0)
    va += torch.arange(nnz, dtype=torch.float64, device="cuda") * 1e-9              # distinct values: a wrong entry shows
    A = hp.HPCSparseMatrix_local_device(rp, ci, va, n, backend, col_window=(0, n - 1))
    return A, ci, rp


def torch_route(rp, ci, vals, rows, cols, n):
    """The same CSR by torch alone: (rowptr, global new columns, values)."""
    import torch
    width = int(cols.numel())
    table = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    table[cols] = torch.arange(width, dtype=torch.int64, device="cuda")
    start = rp[rows]
    counts = rp[rows + 1] - start
    nsel = int(rows.numel())
    first = torch.cumsum(counts, 0) - counts
    out_row = torch.repeat_interleave(torch.arange(nsel, dtype=torch.int64, device="cuda"), counts)
    src = start[out_row] + (torch.arange(int(out_row.numel()), dtype=torch.int64, device="cuda") - first[out_row])
    newc = table[ci[src]]
    keep = newc >= 0
    key, perm = torch.sort(out_row[keep] * width + newc[keep])
    v = vals[src[keep][perm]]
    rowptr = torch.zeros(nsel + 1, dtype=torch.int64, device="cuda")
    rowptr[1:] = torch.cumsum(torch.bincount(torch.div(key, width, rounding_mode="floor"), minlength=nsel), 0)
    return rowptr, key % width, v


def parts_through_the_abi(hp, A, idx):
    """sort / structure / fill of select(A, idx, idx) as three callables over preallocated outputs"""
    import torch
    from hpcla_amd.indexing import _col_indices_dev
    from hpcla_amd.vectors import current_stream_ptr, dptr
    lib = hp._capi.load()
    n = A.shape[0]
    nsel = width = int(idx.numel())
    ci_src = _col_indices_dev(A)
    ncomp = int(ci_src.numel())
    colval = A.colval_target()
    work = torch.empty(lib.hpcla_select_work_bytes(nsel, ncomp, width), dtype=torch.uint8, device="cuda")
    rowptr_out = torch.empty(nsel + 1, dtype=torch.int32, device="cuda")
    ci_out = torch.empty(min(width, ncomp), dtype=torch.int64, device="cuda")
    sizes = [ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()]
    state = {}

    def sort():
        state["sorted"] = torch.sort(idx, stable=True)
        return state["sorted"]

    def structure():
        sc_, sp_ = state["sorted"]
        hp._capi.call("hpcla_select_structure_i32", dptr(A.rowptr_target), dptr(colval), n, A.nnz, dptr(ci_src), ncomp, dptr(idx),
                      nsel, dptr(sc_), dptr(sp_), width, width, 0, dptr(rowptr_out), dptr(ci_out), ctypes.byref(sizes[0]),
                      ctypes.byref(sizes[1]), ctypes.byref(sizes[2]), dptr(work), current_stream_ptr())

    sort()
    structure()
    nnz = int(sizes[0].value)
    colval_out = torch.empty(nnz, dtype=torch.int32, device="cuda")
    nzval_out = torch.empty(nnz, dtype=torch.float64, device="cuda")
    src_out = torch.empty(nnz, dtype=torch.int64, device="cuda")

    def fill():
        hp._capi.call("hpcla_select_fill_i32", 8, dptr(A.rowptr_target), dptr(colval), dptr(A.nzval), n, A.nnz, ncomp, dptr(idx), nsel,
                      dptr(rowptr_out), nnz, int(sizes[2].value), 0, dptr(work), dptr(colval_out), dptr(nzval_out), dptr(src_out),
                      current_stream_ptr())

    return sort, structure, fill


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2048,4096,128")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--stream-tbps", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import scipy.sparse as sp
    import torch
    import hpcla_amd as hp

    assert torch.cuda.is_available(), "bench_select needs a GPU"
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    lib = hp._capi.load()
    out = {"bench": "select", "calls": args.calls, "warmup": args.warmup, "host_calls": args.host_calls,
           "stream_TBps": args.stream_tbps, "cases": {}}
    stream = args.stream_tbps * 1e12

    def same(B, H):
        return bool(np.array_equal(B.rowptr, H.rowptr) and np.array_equal(B.colval, H.colval)
                    and np.array_equal(B.col_indices, H.col_indices) and torch.equal(B.nzval, H.nzval))

    state = {}
    for case in (int(c) for c in args.cases.split(",") if c):
        A, ci, rp = build(hp, backend, case)
        n = A.shape[0]
        S = sp.csr_matrix((A.nzval.cpu().numpy(), ci.cpu().numpy(), rp.cpu().numpy()), shape=(n, n)) if args.host_calls else None
        g = torch.Generator(device="cuda")
        g.manual_seed(case)
        perm = torch.randperm(n, generator=g, device="cuda")
        sets = {"subset90": torch.sort(perm[: (9 * n) // 10]).values, "permute": perm,
                "reverse": torch.arange(n - 1, -1, -1, dtype=torch.int64, device="cuda")}
        v = hp.HPCVector.from_global(np.cos(np.arange(n, dtype=np.float64)), backend)
        for name, idx in sets.items():
            rec = {"n": n, "nnz": A.nnz, "selected": int(idx.numel())}
            B = hp.select(A, idx, idx)
            rec["nnz_out"] = B.nnz
            rec["select_ms"] = timed_events(lambda: hp.select(A, idx, idx), args.calls, args.warmup)
            sort, structure, fill = parts_through_the_abi(hp, A, idx)
            rec["sort_ms"] = timed_events(sort, args.calls, args.warmup)
            rec["structure_ms"] = timed_events(structure, args.calls, args.warmup)
            rec["fill_ms"] = timed_events(fill, args.calls, args.warmup)
            del sort, structure, fill
            plan = hp.selection_plan(A, idx, idx)
            rec["extract_ms"] = timed_events(lambda: plan.extract(A), args.calls, args.warmup)
            rec["extract_fraction_of_stream"] = round(24.0 * B.nnz / stream / (rec["extract_ms"][0] * 1e-3), 3)
            assert torch.equal(plan.extract(A).nzval, B.nzval)
            del plan
            ip = hp.index_plan(idx, v.partition, backend)
            w = hp.HPCVector.zeros(ip.result_partition, backend)
            rec["take_ms"] = timed_events(lambda: ip.take(v, out=w), args.calls, args.warmup)
            rec["take_fraction_of_stream"] = round(20.0 * int(idx.numel()) / stream / (rec["take_ms"][0] * 1e-3), 3)
            del ip, w
            torch.cuda.empty_cache()
            rec["torch_ms"] = timed_events(lambda: torch_route(rp, ci, A.nzval, idx, idx, n), max(3, args.calls // 3), 1)
            t_rp, t_cols, t_vals = torch_route(rp, ci, A.nzval, idx, idx, n)
            rec["equals_torch_route"] = bool(torch.equal(t_rp, B.rowptr_target.to(torch.int64)) and torch.equal(t_vals, B.nzval)
                                             and torch.equal(t_cols, B._col_indices_dev[B._colval_target.to(torch.int64)]))
            rec["select_over_torch"] = round(rec["select_ms"][0] / rec["torch_ms"][0], 2)
            del t_rp, t_cols, t_vals
            torch.cuda.empty_cache()
            if args.host_calls:
                ih = idx.cpu().numpy()

                def host_route():
                    state["H"] = hp.HPCSparseMatrix_from_global(S[ih][:, ih], backend)
                    return state["H"]

                rec["host_ms"] = timed_wall(host_route, args.host_calls)
                rec["equals_host_route"] = same(B, state["H"])
                state.clear()
                rec["host_over_select"] = round(rec["host_ms"][0] / rec["select_ms"][0], 1)
            out["cases"][f"{case}:{name}"] = rec
            print(f"# {case}:{name} {json.dumps(rec)}", file=sys.stderr, flush=True)
            del B
            torch.cuda.empty_cache()
        del A, ci, rp, S, sets, perm, v
        torch.cuda.empty_cache()

    # the long-row case: one row of 8 tiles of kept entries
    tile = int(lib.hpcla_select_tile())
    nx = 512
    n = nx * nx
    idx = np.arange(n)
    i, j = idx % nx, idx // nx
    cand = np.stack([idx - nx, idx - 1, idx, idx + 1, idx + nx], axis=1)
    ok = np.stack([j > 0, i > 0, np.ones(n, bool), i < nx - 1, j < nx - 1], axis=1)
    base = sp.csr_matrix((np.where(cand[ok] == np.repeat(idx, ok.sum(axis=1)), 4.0, -1.0), cand[ok],
                          np.concatenate([[0], np.cumsum(ok.sum(axis=1))])), shape=(n, n))
    hub = sp.lil_matrix((n, n))
    hub[n // 2, np.random.default_rng(1).choice(n, 8 * tile, replace=False)] = 0.5
    long = sp.csr_matrix(base + hub.tocsr())
    p = torch.from_numpy(np.random.default_rng(2).permutation(n).astype(np.int64)).cuda()
    rec = {"n": n, "row_entries": int(np.diff(long.indptr).max())}
    for name, M in (("without_long_row", base), ("with_long_row", long)):
        AM = hp.HPCSparseMatrix_from_global(M, backend)
        rec[name + "_select_ms"] = timed_events(lambda: hp.select(AM, p, p), args.calls, args.warmup)
        sort, structure, fill = parts_through_the_abi(hp, AM, p)
        rec[name + "_fill_ms"] = timed_events(fill, args.calls, args.warmup)
        del AM, sort, structure, fill
    out["long_row"] = rec

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_select.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "MEASUREMENTS_select.md"), "w") as f:
        f.write("# Index-set selection: measurements\n\n")
        f.write(f"`python benchmarks/bench_select.py --cases {args.cases} --calls {args.calls} --warmup {args.warmup} --host-calls "
                f"{args.host_calls}` on one MI355X, Int32 / Float64; the index set is passed as rows and as columns.  Times are "
                "milliseconds between HIP events around the whole call, `median (min)`; `select` is the public call (the sort, the "
                "kernels, the one synchronisation that returns the sizes, allocation of fresh outputs), "
                "`sort` / `structure` / `fill` its parts through the C ABI.  `extract` moves 24 bytes per kept entry and `take` 20 "
                f"per element; their fractions are of {args.stream_tbps} TB/s.  `torch` is the composite-key `torch.sort` route, "
                "`host` scipy fancy indexing plus `HPCSparseMatrix_from_global` (host wall time).\n\n")
        f.write("| case | rows | kept entries | select | sort | structure | fill | extract | of stream | take | of stream | torch | "
                "select / torch | host | host / select | equal to torch, host |\n|" + "---|" * 16 + "\n")

        def mm(r, k):
            return f"{r[k][0]} ({r[k][1]})" if k in r else "-"

        for name, r in out["cases"].items():
            f.write(f"| {name} | {r['selected']} | {r['nnz_out']} | {mm(r, 'select_ms')} | {mm(r, 'sort_ms')} | {mm(r, 'structure_ms')} | "
                    f"{mm(r, 'fill_ms')} | {mm(r, 'extract_ms')} | {r['extract_fraction_of_stream']} | {mm(r, 'take_ms')} | "
                    f"{r['take_fraction_of_stream']} | {mm(r, 'torch_ms')} | {r['select_over_torch']} | {mm(r, 'host_ms')} | "
                    f"{r.get('host_over_select', '-')} | {r['equals_torch_route']}, {r.get('equals_host_route', '-')} |\n")
        r = out["long_row"]
        f.write(f"\nLong row: the 5-point matrix of a 512 x 512 grid, permuted, with and without one row of {r['row_entries']} entries "
                f"(the quadratic form): select {mm(r, 'with_long_row_select_ms')} against {mm(r, 'without_long_row_select_ms')}, fill "
                f"{mm(r, 'with_long_row_fill_ms')} against {mm(r, 'without_long_row_fill_ms')}.\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
