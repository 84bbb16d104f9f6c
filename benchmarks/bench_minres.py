#!/usr/bin/env python3
"""The MINRES solver (``hp.minres``) against the same algorithm composed from the public operators, on a symmetric indefinite
operator: the device-generated 5-point Laplacian of a 4096 x 4096 grid with 2.0 subtracted from its diagonal (n = 16 777 216,
eigenvalues in (-2, 6)), and on the 256 x 256 form.  One GPU, Float64, Int32 indices, no preconditioner.

Every figure is ms per iteration of a WHOLE call of 100 iterations (``rtol = 0``: the stop rule never fires, the work is fixed):
HIP events on the stream around the call, which therefore contain the set-up, the iterations and every read-back.  ``--runs``
timed calls (default 21) after ``--warmup`` untimed ones, the variants ALTERNATING call by call so that a drift of the card
hits all of them alike; median, with the minimum and maximum next to it.

  fused      hp.minres(check_every=8): SpMV with the y.t partials + 3 launches per iteration (80 vector bytes per row), one
             16-byte read-back per 8.
  composed   the textbook recurrence (normalised v) from mul_, dot, norm, xpay_ / axpy_ and ``v / a`` with host scalars, as a
             caller of the parent commit writes it (nothing under it changes in this commit, so it stands for the parent):
             176 vector bytes per row and two host read-backs per iteration.
  floor      one ``mul_dot_`` (the SpMV with the dot partials) per "iteration": what the fused form stands on; and next to it
             the byte model, that SpMV plus 80 bytes per row at the rate ``axpy_`` (24 bytes per row) reaches in the same run.

Prints one JSON line and writes <out>/bench_minres.json and <out>/bench_minres_tables.md (default out: profiles/).
usage: python benchmarks/bench_minres.py [--runs R] [--warmup W] [--iters K] [--out DIR] [--small-only]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHIFT = 2.0
FUSED_BYTES, COMPOSED_BYTES, AXPY_BYTES = 80, 176, 24


def shifted_operator(hp, torch, backend, nx, ny):
    """The 5-point Laplacian generated on the device, SHIFT subtracted from its diagonal."""
    n = nx * ny
    lib = hp._capi.load()
    s0 = torch.cuda.current_stream().cuda_stream
    nnz = lib.hpcla_poisson2d_nnz(nx, ny, 0, n)
    rp = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ci = torch.empty(nnz, dtype=torch.int64, device="cuda")
    va = torch.empty(nnz, dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_gen_poisson2d", nx, ny, 0, n, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), s0)
    row_of = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device="cuda"), rp[1:] - rp[:-1])
    va -= SHIFT * (ci == row_of)
    del row_of
    return hp.HPCSparseMatrix_local_device(rp, ci, va, n, backend, col_window=(0, n - 1))


class Composed:
    """Textbook MINRES from the public operators with host scalars (the stop rule left out: rtol = 0)."""

    def __init__(self, hp, A, b):
        self.hp, self.A, self.b = hp, A, b
        self.x = hp.HPCVector.zeros(b.partition, b.backend)
        self.bufs = [b.similar() for _ in range(5)]

    def __call__(self, iters):
        hp = self.hp
        mul_, dot, norm = hp.mul_, hp.dot, hp.norm
        A, x = self.A, self.x
        r1, r2, t, w1, w2 = self.bufs
        x.v.zero_()
        w1.v.zero_()
        w2.v.zero_()
        r2.v.copy_(self.b.v)
        beta = norm(r2)
        oldb, cs, sn, dbar, epsln, phibar = 0.0, -1.0, 0.0, 0.0, 0.0, beta
        hist = [beta]
        for j in range(1, iters + 1):
            v = r2 / beta
            mul_(t, A, v)
            if j >= 2:
                t.axpy_(-(beta / oldb), r1)
            alfa = dot(v, t)
            t.axpy_(-(alfa / beta), r2)
            r1, r2, t = r2, t, r1
            oldb, beta = beta, norm(r2)
            oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
            epsln, dbar = sn * beta, -cs * beta
            gamma = math.sqrt(gbar * gbar + beta * beta)
            cs, sn = gbar / gamma, beta / gamma
            phi, phibar = cs * phibar, sn * phibar
            w1.xpay_(v, -oldeps)                                  # w = ((v - oldeps w1) - delta w2) / gamma
            w1.axpy_(-delta, w2)
            w1, w2 = w2, w1 / gamma
            x.axpy_(phi, w2)
            hist.append(abs(phibar))
        return hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small-only", action="store_true", help="256 x 256 only (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from hpcla_amd import workloads as wl
    from benchmarks.bench_pcg import timed_table
    if not torch.cuda.is_available():
        raise SystemExit("bench_minres.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    K = args.iters
    record = {"iters_per_call": K, "runs": args.runs, "warmup": args.warmup, "unit": "ms per iteration, median (min, max)",
              "measured_on": {"name": torch.cuda.get_device_name(0),
                              "arch": torch.cuda.get_device_properties(0).gcnArchName,
                              "compute_units": torch.cuda.get_device_properties(0).multi_processor_count},
              "vector_bytes_per_row": {"fused": FUSED_BYTES, "composed": COMPOSED_BYTES}}
    lines = []
    for label, (nx, ny) in ([] if args.small_only else [("4096x4096", (4096, 4096))]) + [("256x256", (256, 256))]:
        n = nx * ny
        A = shifted_operator(hp, torch, backend, nx, ny)
        b = hp.HPCVector.zeros(A.row_partition, backend)
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, n, wl.SEED_RHS, torch.cuda.current_stream().cuda_stream)
        ws = hp.MinresWorkspace(b, K + 2)
        composed = Composed(hp, A, b)
        yu, yv = b.similar(), b.copy()
        out = torch.zeros(1, dtype=torch.float64, device="cuda")

        def fused():
            _, info = hp.minres(A, b, rtol=0.0, atol=0.0, maxiter=K, check_every=8, workspace=ws)
            assert info.iterations == K and info.status == "maxiter", info.status
            return info

        def floor():
            for _ in range(K):
                hp.mul_dot_(yu, A, yv, out)

        def stream():
            for _ in range(K):
                yu.axpy_(0.5, yv)

        # the same recurrence before anything is timed: the heads of the two residual histories agree
        h_f = fused().residual_norms[:5]
        h_c = composed(4)
        agree = max(abs(f - c) / c for f, c in zip(h_f, h_c))
        assert agree <= 1e-10, (h_f, h_c)
        print(f"bench_minres: {label}: fused and composed agree ({agree:.1e}), timing", file=sys.stderr, flush=True)

        table = timed_table(torch, {"hp.minres": fused, "composed": lambda: composed(K), "SpMV with dot": floor,
                                    "axpy_": stream}, args.runs, args.warmup, K)
        f, c = table["hp.minres"], table["composed"]
        spread = max(f[2] - f[1], c[2] - c[1])
        model = table["SpMV with dot"][0] + table["axpy_"][0] * FUSED_BYTES / AXPY_BYTES
        rec = {"rows": n, "nnz": int(A.nnz), "head_deviation_fused_vs_composed": float(agree),
               "table": {k: [round(x, 5) for x in v] for k, v in table.items()},
               "byte_model_floor_ms": round(model, 5), "fused_over_byte_model_floor": round(f[0] / model, 4),
               "fused_over_composed": round(f[0] / c[0], 4),
               "composed_minus_fused_ms": round(c[0] - f[0], 5), "larger_min_max_spread_ms": round(spread, 5),
               "difference_over_spread": round((c[0] - f[0]) / spread, 1),
               "fused_below_composed_by_more_than_the_spread": bool(c[0] - f[0] > spread)}
        record[label] = rec
        lines += [f"### {label} ({n} rows, {int(A.nnz)} stored entries, diagonal 4 - {SHIFT})", "",
                  f"| call ({K} iterations) | ms / iteration, median | min | max |", "|---|---|---|---|"]
        lines += [f"| {k} | {v[0]:.4f} | {v[1]:.4f} | {v[2]:.4f} |" for k, v in table.items()]
        lines += ["", f"byte-model floor (SpMV with dot + {FUSED_BYTES} B per row at axpy_'s rate): {model:.4f} ms; fused / floor: "
                      f"{rec['fused_over_byte_model_floor']:.4f}",
                  f"fused / composed: {rec['fused_over_composed']:.4f}; composed - fused = {rec['composed_minus_fused_ms']:.4f} ms "
                  f"against a larger min-max spread of {rec['larger_min_max_spread_ms']:.4f} ms ({rec['difference_over_spread']:.1f} times)", ""]
        del A, b, ws, composed, yu, yv
        hp.clear_plan_cache()
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_minres.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out, "bench_minres_tables.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
