#!/usr/bin/env python3
"""One iteration of the block eigensolver (``hp.lobpcg``) on the standard problem against one on a pencil ``A x = lambda B x``,
with ``B`` as positive weights (a diagonal ``B``: ``B W`` comes out of the residual kernel) and as a sparse matrix (a second
SpMM per iteration), on the 1024 x 1024 5-point matrix (1 048 576 rows) at ``k`` = 8.  One GPU, Float64, Int32 indices.

``B`` as weights is ``uniform(0.5, 1.5)``; the sparse ``B`` is ``hp.add_scaled_identity(A, 8.0)``, which is symmetric positive
definite (its eigenvalues lie in (8, 16)) and has A's five entries per row, so its SpMM costs what A's does.

The time per iteration of a variant is ``hp.lobpcg(A, k, tol=0, maxiter=m, B=...)`` at m = ``--long`` minus the same at
m = ``--short``, over ``long - short``: the start (X0, the first products and projection) cancels and what remains is the
residual kernel, the SpMM(s), the Gram pass, the read-back, the host's Rayleigh-Ritz step, the upload and the combine(s),
exactly as a caller pays for them.  Every figure is a median of ``--runs`` samples (default 9) after ``--warmup`` untimed ones
with (min, max) as the spread, the three variants ALTERNATING sample by sample; HIP events on the stream around the work,
which contain every read-back.

Next to the times the byte counts per local row and iteration from the docstrings (linearalgebrampi.jl_amd/lobpcg.py,
csrc/lobpcg.hip), the SpMM's own traffic aside, and what the added bytes would cost at the achievable HBM stream rate
(``--stream-tbs``, default 6.3 TB/s).

Prints one JSON line and writes <out>/bench_lobpcg_gen.json and <out>/bench_lobpcg_gen_tables.md (default out: profiles/).
usage: python benchmarks/bench_lobpcg_gen.py [--runs R] [--warmup W] [--out DIR] [--small-only]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 8


def bytes_per_row(k, form):
    """Bytes per local row and iteration next to the SpMMs' own traffic, from the docstrings: residual, the copies of the
    products into the buffer, the Gram pass (every column once per 64-column panel of the right operand), the combine(s)."""
    if form == "none":
        return {"residual": 8 * 2 * k + 16 * k, "copies": 16 * k, "gram": 8 * 6 * k, "combine": 16 * 3 * k + 32 * k}
    out = {"residual": 8 * (2 * k + (1 if form == "weights" else 0)) + 16 * k + (8 * k if form == "weights" else 0),
           "copies": 16 * k * (2 if form == "sparse" else 1), "gram": 8 * 9 * k,
           "combine": 16 * 3 * k + 32 * k + 8 * 3 * k + 16 * k}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--short", type=int, default=2)
    ap.add_argument("--long", type=int, default=12)
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small-only", action="store_true", help="256 x 256 only (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from benchmarks.bench_pcg import timed_table
    from benchmarks.extra_workloads import device_stencil
    if not torch.cuda.is_available():
        raise SystemExit("bench_lobpcg_gen.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    dims = (256, 256) if args.small_only else (1024, 1024)
    n = int(np.prod(dims))
    k = K
    A = device_stencil(hp, torch, backend, dims, 0, n)
    weights = hp.HPCVector.from_global(np.random.default_rng(1).uniform(0.5, 1.5, n), backend)
    Bs = hp.add_scaled_identity(A, 8.0)
    X0 = hp.HPCMatrix.from_global(np.random.default_rng(0).uniform(-1.0, 1.0, (n, k)), backend)
    operands = {"none": None, "weights": weights, "sparse": Bs}
    spaces = {name: hp.LobpcgWorkspace(A, k, B) for name, B in operands.items()}
    span = args.long - args.short

    def solve(name, m):
        return lambda: hp.lobpcg(A, k=k, X0=X0, tol=0.0, maxiter=m, workspace=spaces[name], B=operands[name])

    # before anything is timed: the three variants run the iterations asked for and stay finite
    for name in operands:
        vals, _, info = solve(name, args.long)()
        assert (info.status, info.iterations) == ("maxiter", args.long + 1) and np.all(np.isfinite(vals)), (name, info.status)
    per = {name: {"short": [], "long": []} for name in operands}
    for _ in range(args.warmup):
        for name in operands:
            solve(name, args.short)(), solve(name, args.long)()
    torch.cuda.synchronize()
    for _ in range(args.runs):                                   # alternating: short and long solve of every variant in turn
        for name in operands:
            t = timed_table(torch, {"short": solve(name, args.short), "long": solve(name, args.long)}, 1, 0, 1)
            per[name]["short"].append(t["short"][0])
            per[name]["long"].append(t["long"][0])
    stat = lambda v: (float(np.median(v)), float(min(v)), float(max(v)))
    fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f}, {t[2]:.4f})"
    record = {"runs": args.runs, "warmup": args.warmup, "short": args.short, "long": args.long, "stream_tbs": args.stream_tbs,
              "gpu": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
              "rows": n, "nnz": int(A.nnz), "nnz_B": int(Bs.nnz), "k": k, "unit": "ms, median (min, max)", "iteration": {}}
    lines = [f"GPU: {record['gpu']} ({record['arch']})", "", f"### {dims[0]}x{dims[1]} ({n} rows, {int(A.nnz)} stored entries), k = {k}", "",
             "| B | ms / iteration | spread | B/row next to the SpMMs (residual + copies + Gram + combine) | added B/row | added ms at the stream rate | added ms measured |",
             "|---|---|---|---|---|---|---|"]
    base_bytes = sum(bytes_per_row(k, "none").values())
    base = None
    for name in operands:
        it = stat([(b - a) / span for a, b in zip(per[name]["short"], per[name]["long"])])
        parts = bytes_per_row(k, name)
        total = sum(parts.values())
        base = it if base is None else base
        model = (total - base_bytes) * n / (args.stream_tbs * 1e12) * 1e3
        record["iteration"][name] = {"ms": [round(v, 5) for v in it], "solve_short_ms": [round(v, 4) for v in stat(per[name]["short"])],
                                     "solve_long_ms": [round(v, 4) for v in stat(per[name]["long"])], "bytes_per_row": parts,
                                     "bytes_per_row_total": total, "added_bytes_per_row": total - base_bytes,
                                     "added_ms_at_stream_rate": round(model, 5), "added_ms_measured": round(it[0] - base[0], 5)}
        lines.append(f"| {name} | {fmt(it)} | {(it[2] - it[1]) / it[0]:.3f} | {total} ({' + '.join(str(v) for v in parts.values())}) | "
                     f"{total - base_bytes} | {model:.4f} | {it[0] - base[0]:.4f} |")
    hp.clear_plan_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_lobpcg_gen.json"), "w") as fjson:
        json.dump(record, fjson, indent=1)
    with open(os.path.join(args.out, "bench_lobpcg_gen_tables.md"), "w") as fmd:
        fmd.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
