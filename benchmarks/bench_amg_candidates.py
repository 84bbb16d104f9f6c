#!/usr/bin/env python3
"""``hp.amg(A, B=rigid-body modes)`` against ``hp.amg(A)`` and ``"jacobi"`` in ``hp.cg``, one GPU, Float64, Int32 indices: 2-D
plane-strain elasticity (Q1 unit squares, E = 1, nu = 0.3, the left edge clamped: the matrix of tests/_amg_candidates_cases.py)
on 1024^2 and 2048^2 nodes, assembled on the device by ``hp.sparse_from_coo``.  b = fill_uniform.  All in one run, on one tree.

Per size:
  to 1e-8      per preconditioner, iterations and milliseconds of ``hp.cg(rtol=1e-8, check_every=32)``, HIP events around the call,
               median (min, max) of ``--solves`` calls; the true residual.
  cycle        ``M.apply(r)`` by events, median of ``--runs``, in milliseconds and in SpMVs of A (median of 50).
  setup        the first ``hp.amg`` call on the structure and each of ``--setups`` later ones; levels, operator complexity.
  fit          ``hpcla_amg_fit_f64`` alone on the first level's aggregates, median of ``--runs``, against the bytes it has to move
               (B, Tv, the member list and the coarse candidates once each) at 6.3 TB/s.

Prints one JSON line and writes <out>/bench_amg_candidates.json (default out: profiles/).
usage: python benchmarks/bench_amg_candidates.py [--nodes 1024,2048] [--runs R] [--solves S] [--setups N] [--out DIR]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 6.3


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def spread(values, digits=3):
    return [round(statistics.median(values), digits), round(min(values), digits), round(max(values), digits)]


def element_stiffness(E=1.0, nu=0.3):
    D = E / ((1 + nu) * (1 - 2 * nu)) * np.array([[1 - nu, nu, 0.0], [nu, 1 - nu, 0.0], [0.0, 0.0, (1 - 2 * nu) / 2]])
    g = 0.5 / np.sqrt(3.0)
    K = np.zeros((8, 8))
    for x in (0.5 - g, 0.5 + g):
        for y in (0.5 - g, 0.5 + g):
            dx, dy = np.array([-(1 - y), 1 - y, y, -y]), np.array([-(1 - x), -x, x, 1 - x])
            Bm = np.zeros((3, 8))
            Bm[0, 0::2], Bm[1, 1::2], Bm[2, 0::2], Bm[2, 1::2] = dx, dy, dy, dx
            K += 0.25 * Bm.T @ D @ Bm
    return K


def elasticity(hp, torch, backend, nodes):
    """(A, modes) on nodes x nodes nodes: the free unknowns 2 (j (nodes - 1) + i - 1) + c of the nodes with i >= 1."""
    dev, N = backend.torch_device, nodes
    i = torch.arange(N - 1, device=dev, dtype=torch.int64)
    first = (i[:, None] * N + i[None, :]).reshape(-1)                     # node j N + i of every element's corner
    corner = torch.tensor([0, 1, N + 1, N], device=dev, dtype=torch.int64)
    node = first[:, None] + corner[None, :]
    dof = (2 * node[:, :, None] + torch.arange(2, device=dev)[None, None, :]).reshape(-1, 8)
    free = torch.where((dof // 2) % N == 0, -1, 2 * ((dof // 2) // N * (N - 1) + (dof // 2) % N - 1) + dof % 2)
    rows, cols = free[:, :, None].expand(-1, 8, 8).reshape(-1), free[:, None, :].expand(-1, 8, 8).reshape(-1)
    vals = torch.from_numpy(element_stiffness()).to(dev).reshape(1, 64).expand(first.numel(), 64).reshape(-1)
    keep = (rows >= 0) & (cols >= 0)
    n = 2 * N * (N - 1)
    A = hp.sparse_from_coo(rows[keep].contiguous(), cols[keep].contiguous(), vals[keep].contiguous(), (n, n), backend)
    g = torch.arange(N * (N - 1), device=dev, dtype=torch.int64)
    x, y = (g % (N - 1) + 1).to(torch.float64), (g // (N - 1)).to(torch.float64)
    modes = torch.zeros((n, 3), device=dev, dtype=torch.float64)
    modes[0::2, 0] = 1.0
    modes[1::2, 1] = 1.0
    modes[0::2, 2] = -y
    modes[1::2, 2] = x
    return A, hp.HPCMatrix(A.row_partition, np.array([0, 3]), modes, backend)


def time_fit(hp, torch, lvl, runs):
    """The fit entry alone on a level's own candidates and aggregates."""
    n, k = lvl.candidates.shape
    n_agg = lvl.n_roots
    local = lvl.aggregates - int(lvl.aggregates.min().item())
    members = torch.sort(local, stable=True).indices
    mptr = torch.zeros(n_agg + 1, dtype=torch.int64, device=local.device)
    mptr[1:] = torch.cumsum(torch.bincount(local, minlength=n_agg), 0)
    tv, bc = torch.zeros((n, k), dtype=torch.float64, device=local.device), torch.zeros((n_agg * k, k), dtype=torch.float64,
                                                                                        device=local.device)
    info = torch.zeros(1, dtype=torch.int64, device=local.device)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda: hp._capi.call("hpcla_amg_fit_f64", lvl.candidates.data_ptr(), n, k, mptr.data_ptr(), members.data_ptr(), n, n_agg,
                                 tv.data_ptr(), bc.data_ptr(), info.data_ptr(), s)
    call()
    ms = [event_ms(torch, call)[0] for _ in range(max(runs, 5))]
    moved = 8 * (2 * n * k + n + n_agg * k * k + n_agg + 1)
    med = statistics.median(ms)
    return {"ms": spread(ms, 4), "bytes": moved, "aggregates": n_agg, "members_per_aggregate": round(n / n_agg, 2),
            "stream_ms": round(moved / (STREAM_TBS * 1e9), 4), "share_of_stream_rate": round(moved / (STREAM_TBS * 1e9) / med, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="1024,2048")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--setups", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=40000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from hpcla_amd import workloads as wl
    if not torch.cuda.is_available():
        raise SystemExit("bench_amg_candidates.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    record = {"device": torch.cuda.get_device_name(0), "rtol": 1e-8, "runs": args.runs, "solves": args.solves}
    for nodes in (int(v) for v in args.nodes.split(",")):
        A, B = elasticity(hp, torch, backend, nodes)
        n = int(A.shape[0])
        b = hp.HPCVector.zeros(A.row_partition, backend)
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, n, wl.SEED_RHS, torch.cuda.current_stream().cuda_stream)
        y = b.similar()
        hp.mul_(y, A, b)
        spmv = statistics.median(event_ms(torch, lambda: hp.mul_(y, A, b))[0] for _ in range(50))
        rec = {"rows": n, "nnz": int(A.nnz), "spmv_ms": round(spmv, 4), "setup": {}, "cycle": {}, "solve": {}}
        M = {"jacobi": "jacobi"}
        for name, kw in (("amg(A)", {}), ("amg(A, B=modes)", {"B": B})):
            first, M[name] = event_ms(torch, lambda: hp.amg(A, **kw))
            later = [round(event_ms(torch, lambda: hp.amg(A, **kw))[0], 2) for _ in range(args.setups)]
            rec["setup"][name] = {"first_call_ms": round(first, 2), "later_calls_each_ms": later, "levels": [l.n for l in M[name].levels],
                                  "operator_complexity": round(M[name].operator_complexity, 4),
                                  "galerkin": [l.galerkin for l in M[name].levels[:-1]]}
            z = b.similar()
            M[name].apply(b, out=z)
            ms = [event_ms(torch, lambda: M[name].apply(b, out=z))[0] for _ in range(args.runs)]
            rec["cycle"][name] = {"ms": spread(ms, 4), "spmvs_of_A": round(statistics.median(ms) / spmv, 2)}
        rec["fit"] = time_fit(hp, torch, M["amg(A, B=modes)"].levels[0], args.runs)
        ws = hp.PCGWorkspace(b)
        for name, m in M.items():
            times = []
            for _ in range(args.solves):
                t, (x, info) = event_ms(torch, lambda: hp.cg(A, b, rtol=1e-8, maxiter=args.maxiter, M=m, check_every=32, workspace=ws))
                times.append(t)
            true = hp.norm(b - A @ x) / hp.norm(b)
            rec["solve"][name] = {"iterations": info.iterations, "status": info.status, "ms": spread(times, 2),
                                  "true_residual": float(f"{true:.3e}")}
        record[f"{nodes}x{nodes} nodes"] = rec
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_amg_candidates.json"), "w") as f:
            json.dump(record, f, indent=1)
        print(json.dumps({f"{nodes}": rec}), flush=True)
        del A, B, b, y, ws, M
        hp.clear_plan_cache()
        hp.clear_matrix_plan_cache()
        hp.clear_transpose_plan_cache()
        torch.cuda.empty_cache()
    print(json.dumps(record))


if __name__ == "__main__":
    main()
