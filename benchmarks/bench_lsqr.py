#!/usr/bin/env python3
"""The least-squares solver (``hp.lsqr``) against the same algorithm composed from the public operators, on a tall operator of
config 4's per-GPU shape: the device-generated 7-point Laplacian of a 512 x 512 x 64 slab (n = 16 777 216) with a diagonal block
of the same size, 0.5 (1 + u_i), stacked under it (2n x n), and on the 64^3 form.  One GPU, Float64, Int32 indices.

Every figure is ms per iteration of a WHOLE call of 100 iterations (``rtol = ntol = 0``: no stop rule fires, the work is fixed):
HIP events on the stream around the call, which therefore contain the set-up, the iterations and every read-back.  ``--runs``
timed calls (default 21) after ``--warmup`` untimed ones, the variants ALTERNATING call by call so that a drift of the card
hits all of them alike; median, with the minimum and maximum next to it.

  fused      hp.lsqr(check_every=8): 2 SpMV + 5 launches per iteration (24 m + 64 n vector bytes), one 16-byte read-back per 8.
  composed   the textbook recurrence (normalised u and v) from mul_, norm, xpay_ / axpy_ and ``v / a`` with host scalars, as a
             caller of the parent commit writes it (nothing under it changes in this commit, so it stands for the parent):
             48 m + 96 n vector bytes and two host read-backs of a norm per iteration.
  floor      one ``mul_`` on A plus one on its materialised transpose per "iteration": what both forms stand on.

Prints one JSON line and writes <out>/bench_lsqr.json and <out>/bench_lsqr_tables.md (default out: profiles/).
usage: python benchmarks/bench_lsqr.py [--runs R] [--warmup W] [--iters K] [--out DIR] [--small-only]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED_DIAG = 0xD1A6


def tall_operator(hp, torch, backend, dims):
    """[L; D]: the 7-point Laplacian generated on the device with the diagonal D = 0.5 (1 + u) stacked under it."""
    n = int(np.prod(dims))
    lib = hp._capi.load()
    s0 = torch.cuda.current_stream().cuda_stream
    nnz = lib.hpcla_poisson3d_nnz(dims[0], dims[1], dims[2], 0, n)
    rp = torch.empty(2 * n + 1, dtype=torch.int64, device="cuda")
    ci = torch.empty(nnz + n, dtype=torch.int64, device="cuda")
    va = torch.empty(nnz + n, dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_gen_poisson3d", dims[0], dims[1], dims[2], 0, n, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), s0)
    rp[n + 1:] = nnz + torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
    ci[nnz:] = torch.arange(n, dtype=torch.int64, device="cuda")
    hp._capi.call("hpcla_fill_uniform_f64", va[nnz:].data_ptr(), 0, n, SEED_DIAG, s0)
    va[nnz:] = 0.5 * (1.0 + va[nnz:])
    return hp.HPCSparseMatrix_local_device(rp, ci, va, n, backend, col_window=(0, n - 1))


class Composed:
    """Textbook LSQR from the public operators with host scalars (stop rules left out: rtol = ntol = 0)."""

    def __init__(self, hp, A, At, b):
        self.hp, self.A, self.At, self.b = hp, A, At, b
        self.x = hp.HPCVector.zeros(A.col_partition, b.backend)
        self.w, self.tv = self.x.similar(), self.x.similar()
        self.tu = b.similar()

    def __call__(self, iters):
        hp = self.hp
        mul_, norm = hp.mul_, hp.norm
        A, At, x, w, tu, tv = self.A, self.At, self.x, self.w, self.tu, self.tv
        x.v.zero_()
        beta = norm(self.b)
        u = self.b / beta
        mul_(tv, At, u)
        alpha = norm(tv)
        v = tv / alpha
        w.v.copy_(v.v)
        phibar, rhobar = beta, alpha
        hist = [beta]
        for _ in range(iters):
            mul_(tu, A, v)
            u.xpay_(tu, -alpha)                                   # u = A v - alpha u
            beta = norm(u)
            u = u / beta
            mul_(tv, At, u)
            v.xpay_(tv, -beta)                                    # v = At u - beta v
            alpha = norm(v)
            v = v / alpha
            rho = math.sqrt(rhobar * rhobar + beta * beta)
            c, s = rhobar / rho, beta / rho
            theta, rhobar = s * alpha, -c * alpha
            phi, phibar = c * phibar, s * phibar
            x.axpy_(phi / rho, w)
            w.xpay_(v, -(theta / rho))                            # w = v - (theta / rho) w
            hist.append(abs(phibar))
        return hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small-only", action="store_true", help="64^3 only (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from hpcla_amd import workloads as wl
    from benchmarks.bench_pcg import timed_table
    if not torch.cuda.is_available():
        raise SystemExit("bench_lsqr.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    K = args.iters
    record = {"iters_per_call": K, "runs": args.runs, "warmup": args.warmup, "unit": "ms per iteration, median (min, max)"}
    lines = []
    for label, dims in ([] if args.small_only else [("512x512x64", (512, 512, 64))]) + [("64x64x64", (64, 64, 64))]:
        n = int(np.prod(dims))
        A = tall_operator(hp, torch, backend, dims)
        print(f"bench_lsqr: {label}: operator built, transposing", file=sys.stderr, flush=True)
        At = hp.transpose(A).materialize()
        print(f"bench_lsqr: {label}: transpose materialised", file=sys.stderr, flush=True)
        b = hp.HPCVector.zeros(A.row_partition, backend)
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, 2 * n, wl.SEED_RHS, torch.cuda.current_stream().cuda_stream)
        ws = hp.LSQRWorkspace(A, b, K + 2)
        composed = Composed(hp, A, At, b)
        yu, yv = b.similar(), ws.x.similar()

        def fused():
            _, info = hp.lsqr(A, b, rtol=0.0, atol=0.0, ntol=0.0, maxiter=K, check_every=8, workspace=ws)
            assert info.iterations == K and info.status == "maxiter", info.status
            return info

        def floor():
            for _ in range(K):
                hp.mul_(yu, A, yv)
                hp.mul_(yv, At, yu)

        yv.v.zero_()
        # the same recurrence before anything is timed: the heads of the two residual histories agree
        h_f = fused().residual_norms[:5]
        h_c = composed(4)
        agree = max(abs(f - c) / c for f, c in zip(h_f, h_c))
        assert agree <= 1e-10, (h_f, h_c)
        print(f"bench_lsqr: {label}: fused and composed agree ({agree:.1e}), timing", file=sys.stderr, flush=True)

        table = timed_table(torch, {"hp.lsqr": fused, "composed": lambda: composed(K), "SpMV A + SpMV At": floor},
                            args.runs, args.warmup, K)
        f, c = table["hp.lsqr"], table["composed"]
        spread = max(f[2] - f[1], c[2] - c[1])
        rec = {"rows": 2 * n, "cols": n, "nnz": int(A.nnz), "head_deviation_fused_vs_composed": float(agree),
               "table": {k: [round(x, 5) for x in v] for k, v in table.items()},
               "fused_over_composed": round(f[0] / c[0], 4),
               "composed_minus_fused_ms": round(c[0] - f[0], 5), "larger_min_max_spread_ms": round(spread, 5),
               "fused_below_composed_by_more_than_the_spread": bool(c[0] - f[0] > spread)}
        record[label] = rec
        lines += [f"### {label} ({2 * n} x {n}, {int(A.nnz)} stored entries)", "",
                  f"| call ({K} iterations) | ms / iteration, median | min | max |", "|---|---|---|---|"]
        lines += [f"| {k} | {v[0]:.4f} | {v[1]:.4f} | {v[2]:.4f} |" for k, v in table.items()]
        lines += ["", f"fused / composed: {rec['fused_over_composed']:.4f}; composed - fused = {rec['composed_minus_fused_ms']:.4f} ms "
                      f"against a larger min-max spread of {rec['larger_min_max_spread_ms']:.4f} ms", ""]
        del A, At, b, ws, composed, yu, yv
        hp.clear_plan_cache()
        hp.clear_transpose_plan_cache()
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_lsqr.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out, "bench_lsqr_tables.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
