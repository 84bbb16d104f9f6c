#!/usr/bin/env python3
"""The tall-skinny Householder QR (``hp.qr``) against its byte bound and against the same job composed from what the package
offered before it, at 4 194 304 rows and ``k`` = 4, 16 and 32.  One GPU, Float64.

(a) ``hp.qr(X)``: Q and R.  Bytes: ``32 n k`` (read X, write the reflectors, read them, write Q).
(b) ``hp.qr(X, mode="r")``: R alone.  Bytes: ``8 n k``.
(c) CholQR2 from the parent's operators: ``G = hp.transpose(X) @ X`` read back, a host Cholesky, ``torch.matmul`` with the
    inverse factor -- done twice.  It needs a well-conditioned input: the timed block is ``U0 diag(s) V'`` with ``U0`` a device
    normal block scaled by ``1 / sqrt(n)`` (nearly orthonormal columns), ``s = logspace(0, -3, k)``: kappa about 1e3.
Each is timed as a caller pays for it -- allocations, the read-back of R and the host's part included -- with HIP events on
the stream; every figure is a median of ``--runs`` samples after ``--warmup`` untimed ones with (min, max), the three variants
ALTERNATING sample by sample.  The effective bandwidth is the byte count over the time, against the achievable HBM stream
rate (``--stream-tbs``, default 6.3 TB/s).

The second table is the orthogonality ``max |Q'Q - I|`` each method reaches on ``X = U diag(s) V'`` (orthonormal U, V from
seeded normal matrices, 65 537 rows) at kappa = 1e3, 1e8 and 1e12.

Prints one JSON line and writes <out>/bench_qr.json and <out>/bench_qr_tables.md (default out: profiles/).
usage: python benchmarks/bench_qr.py [--runs R] [--warmup W] [--out DIR] [--small-only]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (4, 16, 32)
KAPPAS = (1e3, 1e8, 1e12)


def make(n, k, kappa, seed):
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, k)))
    V, _ = np.linalg.qr(rng.standard_normal((k, k)))
    return (U * np.logspace(0, -np.log10(kappa), k)) @ V.T


def cholqr2(hp, torch, X):
    """(Q's local block, R) by two rounds of Gram matrix, host Cholesky and a product with the inverse factor."""
    R = np.eye(X.shape[1])
    cur = X
    for _ in range(2):
        G = (hp.transpose(cur) @ cur).local_values()
        Rc = np.linalg.cholesky((G + G.T) / 2).T
        Q = torch.matmul(cur.A, torch.from_numpy(np.linalg.inv(Rc)).to(cur.A.device))
        cur = hp.HPCMatrix(X.row_partition, X.col_partition, Q, X.backend)
        R = Rc @ R
    return cur, R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small-only", action="store_true", help="65 536 rows only (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from benchmarks.bench_pcg import timed_table
    if not torch.cuda.is_available():
        raise SystemExit("bench_qr.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    n = 65536 if args.small_only else 4194304
    eps = float(np.finfo(np.float64).eps)
    record = {"runs": args.runs, "warmup": args.warmup, "stream_tbs": args.stream_tbs, "gpu": torch.cuda.get_device_name(0),
              "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "rows": n,
              "unit": "ms, median (min, max)", "time": {}, "orth": {}}
    fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f}, {t[2]:.4f})"
    t_lines = ["| k | variant | ms | bytes / row | TB/s | of stream | model at stream rate, ms | orth of the timed result |",
               "|---|---|---|---|---|---|---|---|"]
    for k in KS:
        g = torch.Generator(device="cuda").manual_seed(k)
        U0 = torch.randn((n, k), generator=g, dtype=torch.float64, device="cuda") / np.sqrt(n)
        V = np.linalg.qr(np.random.default_rng(k).standard_normal((k, k)))[0]
        M = torch.from_numpy(np.logspace(0, -3, k)[:, None] * V.T).cuda()
        X = hp.HPCMatrix(hp.uniform_partition(n, 1), hp.uniform_partition(k, 1), U0 @ M, backend)
        del U0
        orth_of = lambda Q: float((Q.A.T @ Q.A - torch.eye(k, dtype=torch.float64, device="cuda")).abs().max())
        Qa, Ra = hp.qr(X)
        Qc, Rc = cholqr2(hp, torch, X)
        d = np.where(np.diag(Rc) < 0, -1.0, 1.0)
        agree = float(np.linalg.norm(d[:, None] * Rc - Ra) / np.linalg.norm(Ra))
        orths = {"qr": orth_of(Qa), "qr_r": None, "cholqr2": orth_of(Qc)}
        del Qa, Qc
        table = timed_table(torch, {"qr": lambda: hp.qr(X), "qr_r": lambda: hp.qr(X, mode="r"),
                                    "cholqr2": lambda: cholqr2(hp, torch, X)}, args.runs, args.warmup, 1)
        record["time"][k] = {"r_cholqr2_vs_qr": agree}
        for name, bpr in (("qr", 32 * k), ("qr_r", 8 * k), ("cholqr2", 32 * k)):
            t = table[name]
            tbs = bpr * n / (t[0] * 1e-3) / 1e12
            model = bpr * n / (args.stream_tbs * 1e12) * 1e3
            record["time"][k][name] = {"ms": [round(v, 5) for v in t], "bytes_per_row": bpr, "tbs": round(tbs, 3),
                                       "fraction_of_stream": round(tbs / args.stream_tbs, 3), "model_ms": round(model, 5),
                                       "orth": orths[name]}
            o = "-" if orths[name] is None else f"{orths[name]:.1e}"
            t_lines.append(f"| {k} | {name} | {fmt(t)} | {bpr} | {tbs:.3f} | {tbs / args.stream_tbs:.3f} | {model:.4f} | {o} |")
        record["time"][k]["qr_over_cholqr2"] = round(table["qr"][0] / table["cholqr2"][0], 4)
        del X
        torch.cuda.empty_cache()

    o_lines = ["| k | kappa | hp.qr | CholQR2 | numpy.linalg.qr | 16 k eps |", "|---|---|---|---|---|---|"]
    no = 65537
    for k in (16, 32):
        for kappa in KAPPAS:
            Xn = make(no, k, kappa, 1)
            Xh = hp.HPCMatrix.from_global(Xn, backend)
            Qg = hp.qr(Xh)[0].gather()
            o_qr = float(np.abs(Qg.T @ Qg - np.eye(k)).max())
            try:
                Qc = cholqr2(hp, torch, Xh)[0].gather()
                o_c = float(np.abs(Qc.T @ Qc - np.eye(k)).max())
            except np.linalg.LinAlgError:
                o_c = None
            Qn = np.linalg.qr(Xn)[0]
            o_np = float(np.abs(Qn.T @ Qn - np.eye(k)).max())
            record["orth"][f"{k},{kappa:g}"] = {"qr": o_qr, "cholqr2": o_c, "numpy": o_np, "limit": 16 * k * eps}
            o_lines.append(f"| {k} | {kappa:g} | {o_qr:.1e} | {'Cholesky fails' if o_c is None else format(o_c, '.1e')} | {o_np:.1e} | {16 * k * eps:.1e} |")
    lines = [f"GPU: {record['gpu']} ({record['arch']})", "", f"### {n} rows", ""] + t_lines + ["", f"### orthogonality, {no} rows", ""] + o_lines + [""]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_qr.json"), "w") as fjson:
        json.dump(record, fjson, indent=1)
    with open(os.path.join(args.out, "bench_qr_tables.md"), "w") as fmd:
        fmd.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
