#!/usr/bin/env python3
"""The BiCGStab solver (``hp.bicgstab``) against the same algorithm composed from the public operators, on config 4's per-GPU
shape -- a 512 x 512 x 64 slab (16 777 216 rows) -- with a 7-point convection-diffusion operator (the Laplacian's pattern,
west / east / south / north / down / up entries -1.5, -0.5, -1.3, -0.7, -1.2, -0.8, diagonal 6: not symmetric), and on 64^3.
One GPU, Float64, Int32 indices.

Every figure is ms per iteration of a WHOLE call of 100 iterations (``rtol=0``: the stop rule never fires, the work is fixed):
HIP events on the stream around the call, which therefore contain the set-up, the iterations and every read-back.  ``--runs``
timed calls (default 21) after ``--warmup`` untimed ones, the variants ALTERNATING call by call so that a drift of the card
hits all of them alike; median, with the minimum and maximum next to it.

  fused      hp.bicgstab(M=None / "jacobi", check_every=8): 2 SpMV + 8 launches per iteration, one 16-byte read-back per 8.
  composed   the same recurrence from mul_, dot, axpy_ / xpay_ and copies with host scalars, as a caller of the parent commit
             writes it (nothing under it changes in this commit, so it stands for the parent): five host read-backs per
             iteration; Jacobi applies ``1 ./ diag(A)`` as a diagonal sparse matrix through mul_.
  2 x SpMV   two plain ``mul_`` per "iteration" on the same matrix: the floor both forms stand on.

Prints one JSON line and writes <out>/bench_bicgstab.json and <out>/bench_bicgstab_tables.md (default out: profiles/).
usage: python benchmarks/bench_bicgstab.py [--runs R] [--warmup W] [--iters K] [--out DIR] [--small-only]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OFFDIAG = (-1.5, -0.5, -1.3, -0.7, -1.2, -0.8)     # column offsets -1, +1, -nx, +nx, -nx ny, +nx ny


def convection_diffusion(hp, torch, backend, dims):
    """The 7-point Laplacian generated on the device (as benchmarks/extra_workloads.py does), its off-diagonal values replaced."""
    n = int(np.prod(dims))
    lib = hp._capi.load()
    s0 = torch.cuda.current_stream().cuda_stream
    nnz = lib.hpcla_poisson3d_nnz(dims[0], dims[1], dims[2], 0, n)
    rp = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ci = torch.empty(nnz, dtype=torch.int64, device="cuda")
    va = torch.empty(nnz, dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_gen_poisson3d", dims[0], dims[1], dims[2], 0, n, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), s0)
    off = ci - torch.repeat_interleave(torch.arange(n, device="cuda"), rp[1:] - rp[:-1])
    plane = dims[0] * dims[1]
    for o, val in zip((-1, 1, -dims[0], dims[0], -plane, plane), OFFDIAG):
        va[off == o] = val
    del off
    return hp.HPCSparseMatrix_local_device(rp, ci, va, n, backend, col_window=(0, n - 1))


def diagonal_matrix(hp, torch, backend, d):
    n = d.numel()
    rp = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    return hp.HPCSparseMatrix_local_device(rp, rp[:-1].clone(), d.clone(), n, backend, col_window=(0, n - 1))


class Composed:
    """BiCGStab from the public operators with host scalars (gates left out: rtol = 0 on a well-posed operator)."""

    def __init__(self, hp, A, b, Dinv=None):
        self.hp, self.A, self.b, self.Dinv = hp, A, b, Dinv
        self.x, self.r, self.rhat, self.p, self.v, self.s, self.t = (b.similar() for _ in range(7))
        self.ph, self.sh = (b.similar(), b.similar()) if Dinv is not None else (self.p, self.s)

    def __call__(self, iters):
        hp = self.hp
        mul_, dot = hp.mul_, hp.dot
        x, r, rhat, p, v, s, t, ph, sh = self.x, self.r, self.rhat, self.p, self.v, self.s, self.t, self.ph, self.sh
        x.v.zero_()
        r.v.copy_(self.b.v)
        rhat.v.copy_(r.v)
        p.v.copy_(r.v)
        rho = dot(rhat, r)
        hist = [rho]
        for _ in range(iters):
            if self.Dinv is not None:
                mul_(ph, self.Dinv, p)
            mul_(v, self.A, ph)
            alpha = rho / dot(rhat, v)
            s.v.copy_(r.v)
            s.axpy_(-alpha, v)
            if self.Dinv is not None:
                mul_(sh, self.Dinv, s)
            mul_(t, self.A, sh)
            omega = dot(t, s) / dot(t, t)
            x.axpy_(alpha, ph)
            x.axpy_(omega, sh)
            r.v.copy_(s.v)
            r.axpy_(-omega, t)
            rho_new, rr = dot(rhat, r), dot(r, r)
            hist.append(rr)
            beta = (rho_new / rho) * (alpha / omega)
            p.axpy_(-omega, v)
            p.xpay_(r, beta)
            rho = rho_new
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
        raise SystemExit("bench_bicgstab.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    K = args.iters
    record = {"iters_per_call": K, "runs": args.runs, "warmup": args.warmup, "unit": "ms per iteration, median (min, max)"}
    lines = []
    for label, dims in ([] if args.small_only else [("512x512x64", (512, 512, 64))]) + [("64x64x64", (64, 64, 64))]:
        n = int(np.prod(dims))
        A = convection_diffusion(hp, torch, backend, dims)
        b = hp.HPCVector.zeros(A.row_partition, backend)
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, n, wl.SEED_RHS, torch.cuda.current_stream().cuda_stream)
        dinv = hp.diag(A, reciprocal=True)
        Dinv = diagonal_matrix(hp, torch, backend, dinv.v)
        ws = hp.BiCGStabWorkspace(b, K + 2)
        composed = {"none": Composed(hp, A, b), "jacobi": Composed(hp, A, b, Dinv)}
        y = b.similar()

        def fused(M=None):
            _, info = hp.bicgstab(A, b, rtol=0.0, atol=0.0, maxiter=K, M=M, check_every=8, workspace=ws)
            assert info.iterations == K and info.status == "maxiter", info.status
            return info

        def two_spmv():
            for _ in range(K):
                hp.mul_(y, A, b)
                hp.mul_(y, A, b)

        # the same recurrence before anything is timed: the heads of the two histories agree
        agree = {}
        for name, M in (("none", None), ("jacobi", dinv)):
            h_f = fused(M).residual_norms[:5]
            h_c = [float(np.sqrt(v)) for v in composed[name](4)]
            agree[name] = max(abs(f - c) / c for f, c in zip(h_f, h_c))
            assert agree[name] <= 1e-10, (name, h_f, h_c)

        table = timed_table(torch, {"hp.bicgstab M=None": lambda: fused(),
                                    "composed M=None": lambda: composed["none"](K),
                                    "hp.bicgstab M=jacobi": lambda: fused(dinv),
                                    "composed M=jacobi": lambda: composed["jacobi"](K),
                                    "2 x SpMV": two_spmv}, args.runs, args.warmup, K)
        rec = {"rows": n, "nnz": int(A.nnz), "head_deviation_fused_vs_composed": {k: float(v) for k, v in agree.items()},
               "table": {k: [round(x, 5) for x in v] for k, v in table.items()},
               "fused_over_composed_none": round(table["hp.bicgstab M=None"][0] / table["composed M=None"][0], 4),
               "fused_over_composed_jacobi": round(table["hp.bicgstab M=jacobi"][0] / table["composed M=jacobi"][0], 4)}
        record[label] = rec
        lines += [f"### {label} ({n} rows, {int(A.nnz)} stored entries)", "",
                  "| call (100 iterations) | ms / iteration, median | min | max |", "|---|---|---|---|"]
        lines += [f"| {k} | {v[0]:.4f} | {v[1]:.4f} | {v[2]:.4f} |" for k, v in table.items()]
        lines += ["", f"fused / composed: {rec['fused_over_composed_none']:.4f} (M=None), "
                      f"{rec['fused_over_composed_jacobi']:.4f} (M=jacobi)", ""]
        del A, b, ws, composed, Dinv, dinv, y
        hp.clear_plan_cache()
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_bicgstab.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out, "bench_bicgstab_tables.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
