#!/usr/bin/env python3
"""``hp.assembly_plan``: what one reassembly costs on a structure that is already planned, one GPU, Float64, Int32 indices.

Inputs (generated on the device from index arithmetic and a seed):

  p1_2048, p1_4096   P1 triangles on an n x n grid of nodes, 9 contributions per element in natural element order, one unit
                     triplet per diagonal; ``_perm``: the same triplets in a random order (the gather's locality is the
                     caller's)
  q1_128             Q1 hexahedra on 128^3 nodes, 64 contributions per element
  hub / even         2^24 triplets on 1448^2 (2.1 M) entries: ``even`` 8 per entry, ``hub`` 10^6 of them on entry 0 and the rest
                     dealt over the other entries; equal bytes, both in one random order

Per input:

  reassembly   ``plan.assemble_(A, vals)``: HIP events around ``--launches`` calls, median of ``--windows`` windows after a
               warm-up, per call.
  bytes        what the step has to move when everything is moved once: 8 n_in values, 4 n_in of perm, 4 (nnz + 1) of seg_ptr,
               8 nnz stored; the time those bytes take at 6.3 TB/s (the streaming rate of cdna_hip_programming.md), and its
               share of the measured time.
  index_add    ``out.zero_(); out.index_add_(0, dest, vals)`` in the same run, with ``dest`` in the caller's order, and with the
               list pre-sorted by destination (values gathered beforehand, not timed): atomic, not reproducible -- the
               device yardstick.  Not run on ``hub``: one call with 10^6 adders on one address did not return in 7 minutes.
  host route   the only route without the plan: scipy ``coo_matrix(...).tocsr()`` on the host, then
               ``HPCSparseMatrix_from_global``; host clock, ending in a device synchronise; the triplets are on the host
               already (their download is not timed).  Skipped above ``--host-max`` triplets.
  plan build   events around ``hp.assembly_plan`` (second call), and around the stable ``torch.sort`` of its keys alone.

Prints one JSON line and writes <out>/bench_assemble.json and <out>/bench_assemble_tables.md (default out: profiles/).
usage: python benchmarks/bench_assemble.py [--cases p1_2048,...] [--launches K] [--windows W] [--host-max N] [--out DIR] [--small]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_BPS = 6.3e12
INDEX_ADD_MAX_LIST = 1 << 16      # index_add_ is not timed on an input with a longer list (see profiles/MEASUREMENTS_assemble.md)
ALL = ["p1_2048", "p1_2048_perm", "q1_128", "even", "hub", "p1_4096", "p1_4096_perm"]


def p1_triplets(torch, n, seed):
    """(rows, cols, vals, N): tests/_assemble_cases.py p1_triplets with a per-element coefficient, built on the device."""
    i = torch.arange(n - 1, device="cuda", dtype=torch.int64)
    a = (i[None, :] + n * i[:, None]).reshape(-1)
    b, c, d = a + 1, a + n, a + n + 1
    tri = torch.stack([torch.stack([a, b, c], 1), torch.stack([d, c, b], 1)], 1).reshape(-1, 3)
    del a, b, c, d
    elem = torch.tensor([1.0, -0.5, -0.5, -0.5, 0.5, 0.0, -0.5, 0.0, 0.5], device="cuda", dtype=torch.float64)
    g = torch.Generator(device="cuda").manual_seed(seed)
    k = 1.0 + torch.rand(tri.shape[0], device="cuda", dtype=torch.float64, generator=g)
    diag = torch.arange(n * n, device="cuda", dtype=torch.int64)
    rows = torch.cat([tri.repeat_interleave(3, dim=1).reshape(-1), diag])
    cols = torch.cat([tri.repeat(1, 3).reshape(-1), diag])
    vals = torch.cat([(k[:, None] * elem[None, :]).reshape(-1), torch.ones(n * n, device="cuda", dtype=torch.float64)])
    return rows, cols, vals, n * n


def q1_triplets(torch, n, seed):
    i = torch.arange(n - 1, device="cuda", dtype=torch.int64)
    base = (i[None, None, :] + n * i[None, :, None] + n * n * i[:, None, None]).reshape(-1)
    off = torch.tensor([0, 1, n, n + 1, n * n, n * n + 1, n * n + n, n * n + n + 1], device="cuda", dtype=torch.int64)
    conn = base[:, None] + off[None, :]
    g = torch.Generator(device="cuda").manual_seed(seed)
    e = torch.rand(8, 8, device="cuda", dtype=torch.float64, generator=g)
    e = (e + e.T).reshape(-1)
    k = 1.0 + torch.rand(conn.shape[0], device="cuda", dtype=torch.float64, generator=g)
    rows = conn.repeat_interleave(8, dim=1).reshape(-1)
    cols = conn.repeat(1, 8).reshape(-1)
    return rows, cols, (k[:, None] * e[None, :]).reshape(-1), n ** 3


def skew_triplets(torch, n_in, nnz, hub, seed):
    """n_in triplets on nnz entries of a sqrt(nnz)-wide matrix: ``hub`` of them on entry 0, the rest dealt evenly."""
    side = int(round(nnz ** 0.5))
    assert side * side == nnz
    t = torch.arange(n_in, device="cuda", dtype=torch.int64)
    key = torch.where(t < hub, torch.zeros_like(t), 1 + (t - hub) % (nnz - 1)) if hub else t % nnz
    g = torch.Generator(device="cuda").manual_seed(seed)
    key = key[torch.randperm(n_in, device="cuda", generator=g)]
    vals = torch.rand(n_in, device="cuda", dtype=torch.float64, generator=g) - 0.5
    return key // side, key % side, vals, side


def make_case(torch, name, small):
    if name.startswith("p1_"):
        n = int(name.split("_")[1]) // (16 if small else 1)
        rows, cols, vals, N = p1_triplets(torch, n, 7)
    elif name.startswith("q1_"):
        n = int(name.split("_")[1]) // (8 if small else 1)
        rows, cols, vals, N = q1_triplets(torch, n, 11)
    else:
        n_in, nnz, hub = (2 ** 16, 64 * 64, 10 ** 4) if small else (2 ** 24, 1448 * 1448, 10 ** 6)
        rows, cols, vals, N = skew_triplets(torch, n_in, nnz, hub if name == "hub" else 0, 13)
    if name.endswith("_perm"):
        g = torch.Generator(device="cuda").manual_seed(17)
        p = torch.randperm(rows.numel(), device="cuda", generator=g)
        rows, cols, vals = rows[p], cols[p], vals[p]
    return rows, cols, vals, N


def window_ms(torch, fn, launches, windows, warmup=3):
    """Median over ``windows`` of (the time of ``launches`` calls between two events) / launches.  A call that takes long (an
    index_add_ with a million adders on one address) gets fewer calls per window: a window is kept near half a second."""
    first = event_ms(torch, fn)[0]
    launches = max(1, min(launches, int(500.0 / max(first, 1e-3))))
    for _ in range(warmup if first < 100.0 else 0):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows if first < 1000.0 else 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / launches)
    return statistics.median(out), min(out), max(out)


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(ALL))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host-max", type=int, default=400_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small", action="store_true", help="small inputs (a rehearsal of the script)")
    args = ap.parse_args()
    import scipy.sparse as sp
    import torch
    import hpcla_amd as hp
    if not torch.cuda.is_available():
        raise SystemExit("bench_assemble.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    chunk = int(hp._capi.load().hpcla_assemble_chunk())
    record = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "windows": args.windows, "chunk": chunk,
              "stream_rate_Bps": STREAM_BPS}
    lines = ["| input | triplets | entries | longest list | reassembly ms, median (min, max) | bytes to move | ms at 6.3 TB/s | share |"
             " index_add_ caller's order ms | index_add_ sorted ms | host route s (scipy + from_global) | plan build ms | of which sort ms |"
             " reassemblies per plan build |", "|" + "---|" * 14]
    def say(text):                                               # progress on stderr: a long case is not a silent one
        print(f"[bench_assemble] {text}", file=sys.stderr, flush=True)

    for name in [c.strip() for c in args.cases.split(",") if c.strip()]:
        say(f"{name}: generating")
        rows, cols, vals, N = make_case(torch, name, args.small)
        n_in = int(rows.numel())
        hp.assembly_plan(rows[:1000], cols[:1000], (N, N), backend)                    # code objects, allocator
        build_first, plan = event_ms(torch, lambda: hp.assembly_plan(rows, cols, (N, N), backend))
        del plan
        build, plan = event_ms(torch, lambda: hp.assembly_plan(rows, cols, (N, N), backend))
        key = rows * N + cols
        torch.sort(key, stable=True)
        sort_ms = statistics.median(event_ms(torch, lambda: torch.sort(key, stable=True))[0] for _ in range(3))
        del key
        A = plan.assemble(vals)
        say(f"{name}: plan built in {build:.1f} ms, sort {sort_ms:.1f} ms")
        step = window_ms(torch, lambda: plan.assemble_(A, vals), args.launches, args.windows)
        say(f"{name}: reassembly {step[0]:.4f} ms")
        nnz = plan.nnz
        nbytes = 8 * n_in + 4 * n_in + 4 * (nnz + 1) + 8 * nnz
        floor_ms = nbytes / STREAM_BPS * 1e3
        # the device yardstick: atomic adds
        dest_sorted = torch.repeat_interleave(torch.arange(nnz, device="cuda", dtype=torch.int64),
                                              (plan._seg_ptr[1:] - plan._seg_ptr[:-1]).long())
        perm = plan._perm.long()
        dest_in = torch.empty_like(dest_sorted)
        dest_in[perm] = dest_sorted
        vals_sorted = vals[perm]
        out = torch.zeros(nnz, device="cuda", dtype=torch.float64)
        if plan.max_duplicates <= INDEX_ADD_MAX_LIST:
            ia_in = window_ms(torch, lambda: out.zero_().index_add_(0, dest_in, vals), args.launches, args.windows)
            ia_sorted = window_ms(torch, lambda: out.zero_().index_add_(0, dest_sorted, vals_sorted), args.launches, args.windows)
            worst = float((out - A.nzval).abs().max().item())
            say(f"{name}: index_add_ {ia_in[0]:.4f} ms in the caller's order, {ia_sorted[0]:.4f} ms sorted")
        else:                                                    # 10^6 adders on one address: one call did not return in 7 minutes
            ia_in = ia_sorted = worst = None
            say(f"{name}: index_add_ not run (a list of {plan.max_duplicates} contributions)")
        del dest_sorted, dest_in, vals_sorted, perm, out
        host = None
        if n_in <= args.host_max and not name.endswith("_perm"):           # the host route does not care about the order
            r_h, c_h, v_h = rows.cpu().numpy(), cols.cpu().numpy(), vals.cpu().numpy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S = sp.coo_matrix((v_h, (r_h, c_h)), shape=(N, N)).tocsr()
            t1 = time.perf_counter()
            A0 = hp.HPCSparseMatrix_from_global(S, backend)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            say(f"{name}: host route {t2 - t0:.2f} s")
            host = {"scipy_coo_to_csr_s": round(t1 - t0, 3), "from_global_s": round(t2 - t1, 3)}
            assert A0.nnz == nnz
            del r_h, c_h, v_h, S, A0
        rec = {"triplets": n_in, "entries": nnz, "longest_list": plan.max_duplicates,
               "reassembly_ms": [round(v, 4) for v in step], "bytes": nbytes, "ms_at_stream_rate": round(floor_ms, 4),
               "share_of_stream_rate": round(floor_ms / step[0], 3),
               "index_add_callers_order_ms": ia_in and [round(v, 4) for v in ia_in],
               "index_add_sorted_ms": ia_sorted and [round(v, 4) for v in ia_sorted],
               "max_abs_difference_to_index_add": worst, "host_route": host,
               "plan_build_ms": round(build, 2), "plan_build_first_call_ms": round(build_first, 2), "sort_ms": round(sort_ms, 2),
               "reassemblies_per_plan_build": round(build / step[0], 1)}
        record[name] = rec
        hs = "not run" if host is None else f"{host['scipy_coo_to_csr_s'] + host['from_global_s']:.2f} ({host['scipy_coo_to_csr_s']:.2f} + {host['from_global_s']:.2f})"
        ias = "not run | not run" if ia_in is None else f"{ia_in[0]:.4f} | {ia_sorted[0]:.4f}"
        lines.append(f"| {name} | {n_in} | {nnz} | {plan.max_duplicates} | {step[0]:.4f} ({step[1]:.4f}, {step[2]:.4f}) | {nbytes} | "
                     f"{floor_ms:.4f} | {floor_ms / step[0]:.3f} | {ias} | {hs} | {build:.1f} | {sort_ms:.1f} | "
                     f"{build / step[0]:.0f} |")
        del rows, cols, vals, A, plan
        hp.clear_plan_cache()
        torch.cuda.empty_cache()
        os.makedirs(args.out, exist_ok=True)                     # after every case: a cut-off run keeps what it measured
        with open(os.path.join(args.out, "bench_assemble.json"), "w") as f:
            json.dump(record, f, indent=1)
        with open(os.path.join(args.out, "bench_assemble_tables.md"), "w") as f:
            f.write("\n".join(lines) + "\n")
    if "hub" in record and "even" in record:
        record["hub_over_even"] = round(record["hub"]["reassembly_ms"][0] / record["even"]["reassembly_ms"][0], 3)
        with open(os.path.join(args.out, "bench_assemble.json"), "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
