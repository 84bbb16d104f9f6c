#!/usr/bin/env python3
"""One iteration of the block eigensolver (``hp.lobpcg``) against the same iteration composed from what the package offered
before it, and its two kernels alone against their byte counts, on the 2048 x 2048 5-point matrix (4 194 304 rows) at
``k`` = 4 and 16.  One GPU, Float64, Int32 indices.

(a) The fused iteration: ``hp.lobpcg(A, k, tol=0, maxiter=m)`` at m = ``--short`` and ``--long``; the time per iteration is
    the difference of the two over ``long - short``, so the start (X0, the first product and projection) cancels and what
    remains is the residual kernel, the SpMM, the Gram pass, the read-back, the host's Rayleigh-Ritz step, the upload and the
    combine kernel, exactly as a caller pays for them.
    The composed iteration, on a state taken after the start: ``W = AX - X * theta`` and its column norms in torch,
    ``A @ W``, ``hp.transpose(S_i) @ S_j`` and ``hp.transpose(S_i) @ AS_j`` for the six block pairs i <= j of each Gram matrix
    (each read back, as the host needs them), the same host Rayleigh-Ritz step, and ``S C`` / ``AS C`` by ``torch.matmul``.
    Before anything is timed the composed iteration's Ritz values are compared with ``hp.lobpcg(maxiter=1)``'s.
(b) The residual kernel (second copy of W on, no minv: read 16k, write 16k bytes per row) and the combine kernel (c_rest = 2k,
    S and AS: read 48k, write 32k) alone, ``--launches`` launches per sample, against the achievable HBM stream rate
    (``--stream-tbs``, default 6.3 TB/s).

Every figure is a median of ``--runs`` samples (default 9) after ``--warmup`` untimed ones with (min, max) as the spread, the
variants ALTERNATING sample by sample; HIP events on the stream around the work, which contain every read-back.

Prints one JSON line and writes <out>/bench_lobpcg.json and <out>/bench_lobpcg_tables.md (default out: profiles/).
usage: python benchmarks/bench_lobpcg.py [--runs R] [--warmup W] [--out DIR] [--small-only]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (4, 16)


class Composed:
    """The iteration from A @ W, hp.transpose(.) @ . per block pair and torch, on the state (X, AX, P, AP, theta)."""

    def __init__(self, hp, torch, A, k, X0):
        self.hp, self.torch, self.A, self.k = hp, torch, A, k
        self.rr = sys.modules[hp.lobpcg.__module__].rayleigh_ritz
        X = X0.A.clone()
        AX = (A @ X0).A.clone()
        theta, C, _ = self.rr(self.gram([X], [AX]), self.gram([X], [X]), k, "SA")
        Cd = torch.from_numpy(C).cuda()
        self.X, self.AX = X @ Cd, AX @ Cd
        self.P, self.AP = torch.zeros_like(X), torch.zeros_like(X)
        self.theta = torch.from_numpy(theta).cuda()

    def block(self, t):
        return self.hp.HPCMatrix(self.A.row_partition, self.hp.uniform_partition(self.k, 1), t, self.A.backend)

    def gram(self, left, right):
        """The symmetric block matrix [left_i' right_j] from the pairs i <= j, each product read back."""
        hp, k, m = self.hp, self.k, len(left)
        G = np.zeros((m * k, m * k))
        for i in range(m):
            for j in range(i, m):
                g = (hp.transpose(self.block(left[i])) @ self.block(right[j])).local_values()
                G[i * k:(i + 1) * k, j * k:(j + 1) * k] = g
                G[j * k:(j + 1) * k, i * k:(i + 1) * k] = g.T
        return G

    def __call__(self):
        torch, k = self.torch, self.k
        W = self.AX - self.X * self.theta
        rn = torch.sqrt((W * W).sum(dim=0)).cpu().numpy()
        AW = (self.A @ self.block(W)).A
        S, AS = [self.X, W, self.P], [self.AX, AW, self.AP]
        theta, C, _ = self.rr(self.gram(S, AS), self.gram(S, S), k, "SA")
        Cd = torch.from_numpy(C).cuda()
        Sc, ASc = torch.cat(S, dim=1), torch.cat(AS, dim=1)
        Pn, APn = Sc[:, k:] @ Cd[k:], ASc[:, k:] @ Cd[k:]
        Xn, AXn = Sc[:, :k] @ Cd[:k] + Pn, ASc[:, :k] @ Cd[:k] + APn
        return theta, rn, (Xn, AXn, Pn, APn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--short", type=int, default=2)
    ap.add_argument("--long", type=int, default=12)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small-only", action="store_true", help="256 x 256 only (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from benchmarks.bench_pcg import timed_table
    from benchmarks.extra_workloads import device_stencil
    if not torch.cuda.is_available():
        raise SystemExit("bench_lobpcg.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    lib = hp._capi.load()
    stream = torch.cuda.current_stream().cuda_stream
    dims = (256, 256) if args.small_only else (2048, 2048)
    n = int(np.prod(dims))
    A = device_stencil(hp, torch, backend, dims, 0, n)
    record = {"runs": args.runs, "warmup": args.warmup, "short": args.short, "long": args.long, "launches": args.launches,
              "stream_tbs": args.stream_tbs, "gpu": torch.cuda.get_device_name(0),
              "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "rows": n, "nnz": int(A.nnz),
              "unit": "ms, median (min, max)", "iteration": {}, "kernels": {}}
    it_lines = ["| k | fused, ms / iteration | composed, ms / iteration | fused / composed | spread fused | spread composed | Ritz values, composed vs fused |",
                "|---|---|---|---|---|---|---|"]
    k_lines = ["| k | kernel | ms | B/row | TB/s | of stream | model at stream rate, ms |", "|---|---|---|---|---|---|---|"]
    fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f}, {t[2]:.4f})"
    for k in KS:
        X0 = hp.HPCMatrix.from_global(np.random.default_rng(0).uniform(-1.0, 1.0, (n, k)), backend)
        ws = hp.LobpcgWorkspace(A, k)
        composed = Composed(hp, torch, A, k, X0)
        vals1, _, info1 = hp.lobpcg(A, k=k, X0=X0, tol=0.0, maxiter=1, workspace=ws)
        theta_c, _, _ = composed()
        agree = float(np.abs(theta_c - vals1).max() / info1.anorm)
        assert agree <= 1e-10, agree
        span = args.long - args.short
        solve = lambda m: (lambda: hp.lobpcg(A, k=k, X0=X0, tol=0.0, maxiter=m, workspace=ws))
        per = {"short": [], "long": [], "composed": []}
        for _ in range(args.warmup):
            solve(args.short)(), solve(args.long)(), composed()
        torch.cuda.synchronize()
        for _ in range(args.runs):                               # alternating: short solve, long solve, composed iterations
            t = timed_table(torch, {"short": solve(args.short), "long": solve(args.long)}, 1, 0, 1)
            per["short"].append(t["short"][0])
            per["long"].append(t["long"][0])
            per["composed"].append(timed_table(torch, {"c": lambda: [composed() for _ in range(span)]}, 1, 0, span)["c"][0])
        fused = [(b - a) / span for a, b in zip(per["short"], per["long"])]
        stat = lambda v: (float(np.median(v)), float(min(v)), float(max(v)))
        f, c = stat(fused), stat(per["composed"])
        record["iteration"][k] = {"fused_ms": [round(v, 5) for v in f], "composed_ms": [round(v, 5) for v in c],
                                  "fused_over_composed": round(f[0] / c[0], 4), "solve_short_ms": [round(v, 4) for v in stat(per["short"])],
                                  "solve_long_ms": [round(v, 4) for v in stat(per["long"])], "ritz_values_deviation": agree}
        it_lines.append(f"| {k} | {fmt(f)} | {fmt(c)} | {f[0] / c[0]:.4f} | {(f[2] - f[1]) / f[0]:.3f} | {(c[2] - c[1]) / c[0]:.3f} | {agree:.1e} |")

        # -- (b) the kernels alone
        Q, Wp = ws.Q, ws.Wp
        lib.hpcla_fill_uniform_f64(Q.data_ptr(), 0, Q.numel(), 0xBEEF, stream)
        C_h = np.zeros((48, 16))
        C_h[:3 * k, :k] = np.linalg.qr(np.random.default_rng(k).uniform(-1.0, 1.0, (3 * k, 3 * k)))[0][:, :k] / 2   # bounded under repetition
        up = torch.from_numpy(np.concatenate([np.ones(16), C_h.reshape(-1)])).cuda()
        P = lambda t, col=0: t[:, col:].data_ptr()

        def residual():
            for _ in range(args.launches):
                assert lib.hpcla_lobpcg_residual_f64(None, P(Q), 6 * k, P(Q, 3 * k), 6 * k, up.data_ptr(), None, P(Q, k), 6 * k,
                                                     Wp.data_ptr(), ws.pitch, n, k, ws.small.data_ptr(), ws.rwork.data_ptr(), stream) == 0

        def combine():
            for _ in range(args.launches):
                assert lib.hpcla_lobpcg_combine_f64(P(Q), 6 * k, P(Q, 3 * k), 6 * k, up[16:].data_ptr(), k, 2 * k, n, stream) == 0

        table = timed_table(torch, {"residual": residual, "combine": combine}, args.runs, args.warmup, args.launches)
        record["kernels"][k] = {}
        for name, bpr in (("residual", 32 * k), ("combine", 80 * k)):
            t = table[name]
            tbs = bpr * n / (t[0] * 1e-3) / 1e12
            model = bpr * n / (args.stream_tbs * 1e12) * 1e3
            record["kernels"][k][name] = {"ms": [round(v, 5) for v in t], "bytes_per_row": bpr, "tbs": round(tbs, 3),
                                          "fraction_of_stream": round(tbs / args.stream_tbs, 3), "model_ms": round(model, 5)}
            k_lines.append(f"| {k} | {name} | {fmt(t)} | {bpr} | {tbs:.3f} | {tbs / args.stream_tbs:.3f} | {model:.4f} |")
        del ws, composed, X0, Q, Wp
        torch.cuda.empty_cache()
    hp.clear_plan_cache()
    lines = [f"GPU: {record['gpu']} ({record['arch']})", "", f"### {dims[0]}x{dims[1]} ({n} rows, {int(A.nnz)} stored entries)", ""]
    lines += it_lines + [""] + k_lines + [""]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_lobpcg.json"), "w") as fjson:
        json.dump(record, fjson, indent=1)
    with open(os.path.join(args.out, "bench_lobpcg_tables.md"), "w") as fmd:
        fmd.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
