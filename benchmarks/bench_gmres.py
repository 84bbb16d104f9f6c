#!/usr/bin/env python3
"""The restarted GMRES solver (``hp.gmres``) against the same algorithm composed from the public operators, on config 4's
per-GPU shape -- a 512 x 512 x 64 slab (16 777 216 rows) -- with the 7-point convection-diffusion operator of
benchmarks/bench_bicgstab.py, and on 64^3.  One GPU, Float64, Int32 indices.

(a) against a user's composition.  The orthogonalisation step alone at c = 1, 8, 9, 16, 30 basis columns (twice-applied
    classical Gram-Schmidt, no SpMV): the fused step is gmres_dots, gmres_update, gmres_dots, gmres_update with the small
    step, gmres_next through the C entries; the composed one is 2c ``hp.dot``, 2c ``axpy_``, ``hp.norm`` and ``w / hn`` with
    host scalars, as a caller of the parent commit writes it (nothing under it changes in this commit, so it stands for the
    parent).  And the whole solve: ``hp.gmres(restart=30, rtol=0, maxiter=K)`` against the composed GMRES(30) with host Givens
    rotations, M = None and Jacobi (composed: ``1 ./ diag(A)`` as a diagonal sparse matrix through mul_), next to K plain SpMVs.
(b) against the stream rate.  Bytes per row of the fused step from the table in DESIGN.md, 32 c + 48 + 16 ceil(c / 8), over
    its time, as a fraction of the achievable HBM stream rate (``--stream-tbs``, default 6.3 TB/s).

Every figure is a median of ``--runs`` timed calls (default 11) after ``--warmup`` untimed ones, the variants ALTERNATING call
by call; HIP events on the stream around the call, which contain every read-back.  Step figures are ms per step of a call of
``--steps`` steps (default 20); solve figures are ms per inner step of a call of K = ``--iters`` steps (default 120).

Prints one JSON line and writes <out>/bench_gmres.json and <out>/bench_gmres_tables.md (default out: profiles/).
usage: python benchmarks/bench_gmres.py [--runs R] [--warmup W] [--iters K] [--steps S] [--out DIR] [--small-only]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS = (1, 8, 9, 16, 30)
RESTART = 30


def step_bytes_per_row(c, precond=False):
    """DESIGN.md, the GMRES byte table: dots, update, dots, update, next."""
    return 32 * c + 48 + 16 * ((c + 7) // 8) + (16 if precond else 0)


class FusedStep:
    """The orthogonalisation step at a fixed c through the C entries (state running, thr < 0: no gate fires)."""

    def __init__(self, hp, torch, ws, c):
        self.hp, self.ws, self.c = hp, ws, c
        self.n, self.P = ws.x.local_length, (lambda t: t.data_ptr())
        self.h1, self.h2, self.hn = ws.small_array("h1"), ws.small_array("h2"), ws.small_array("hn")
        self.stream = torch.cuda.current_stream().cuda_stream

    def __call__(self, steps):
        call, ws, c, P, n, s = self.hp._capi.call, self.ws, self.c, self.P, self.n, self.stream
        V, w, st, work = P(ws.V), P(ws.w.v), P(ws.state), P(ws.work)
        for _ in range(steps):
            call("hpcla_gmres_dots_f64", None, V, ws.ldv, c, w, n, st, P(self.h1), work, s)
            call("hpcla_gmres_update_f64", None, V, ws.ldv, c, P(self.h1), w, n, 1, ws.restart, None, None, st, work, s)
            call("hpcla_gmres_dots_f64", None, V, ws.ldv, c, w, n, st, P(self.h2), work, s)
            call("hpcla_gmres_update_f64", None, V, ws.ldv, c, P(self.h2), w, n, 1, ws.restart, P(ws.small), P(ws.hist), st, work, s)
            call("hpcla_gmres_next_f64", w, P(self.hn), None, V + 8 * c * ws.ldv, None, n, st, s)


class ComposedStep:
    """The same step from hp.dot / axpy_ / hp.norm / division with host scalars."""

    def __init__(self, hp, cols, w):
        self.hp, self.cols, self.w = hp, cols, w

    def __call__(self, steps):
        hp, w = self.hp, self.w
        for _ in range(steps):
            for _pass in range(2):
                h = [hp.dot(v, w) for v in self.cols]
                for hi, v in zip(h, self.cols):
                    w.axpy_(-hi, v)
            hn = hp.norm(w)
            _ = w / hn


class ComposedGMRES:
    """GMRES(m) with CGS2 from the public operators, host Givens rotations (gates left out: rtol = 0, a well-posed operator)."""

    def __init__(self, hp, A, b, m, Dinv=None):
        self.hp, self.A, self.b, self.m, self.Dinv = hp, A, b, m, Dinv
        self.V = [b.similar() for _ in range(m + 1)]
        self.x, self.w, self.z = b.similar(), b.similar(), b.similar()

    def _K(self, v):
        if self.Dinv is None:
            return v
        self.hp.mul_(self.z, self.Dinv, v)
        return self.z

    def __call__(self, iters):
        hp, m, V, x, w = self.hp, self.m, self.V, self.x, self.w
        x.v.zero_()
        hist, k = [], 0
        while k < iters:
            hp.mul_(w, self.A, x)
            w.v.mul_(-1.0).add_(self.b.v)
            beta = hp.norm(w)
            if not hist:
                hist.append(beta)
            V[0].v.copy_((w / beta).v)
            cs, sn, R, g = np.zeros(m), np.zeros(m), np.zeros((m, m)), np.zeros(m + 1)
            g[0] = beta
            c = 0
            while c < m and k < iters:
                j, c, k = c, c + 1, k + 1
                hp.mul_(w, self.A, self._K(V[j]))
                col = np.zeros(c + 1)
                for _pass in range(2):
                    h = [hp.dot(V[i], w) for i in range(c)]
                    for i in range(c):
                        w.axpy_(-h[i], V[i])
                    col[:c] += h
                col[c] = hn = hp.norm(w)
                for i in range(j):
                    col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], -sn[i] * col[i] + cs[i] * col[i + 1]
                d = math.hypot(col[j], col[j + 1])
                cs[j], sn[j] = col[j] / d, col[j + 1] / d
                R[:j, j], R[j, j] = col[:j], d
                g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
                hist.append(abs(g[j + 1]))
                if c < m:
                    V[c].v.copy_((w / hn).v)
            y = np.linalg.solve(np.triu(R[:c, :c]), g[:c])
            w.v.zero_()
            for i in range(c):
                w.axpy_(float(y[i]), V[i])
            x.axpy_(1.0, self._K(w))
        return hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=120)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small-only", action="store_true", help="64^3 only (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from hpcla_amd import workloads as wl
    from benchmarks.bench_bicgstab import convection_diffusion, diagonal_matrix
    from benchmarks.bench_pcg import timed_table
    if not torch.cuda.is_available():
        raise SystemExit("bench_gmres.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    K, S = args.iters, args.steps
    record = {"iters_per_solve": K, "steps_per_call": S, "runs": args.runs, "warmup": args.warmup, "restart": RESTART,
              "stream_tbs": args.stream_tbs, "unit": "ms per inner step, median (min, max)"}
    lines = []
    for label, dims in ([] if args.small_only else [("512x512x64", (512, 512, 64))]) + [("64x64x64", (64, 64, 64))]:
        n = int(np.prod(dims))
        A = convection_diffusion(hp, torch, backend, dims)
        b = hp.HPCVector.zeros(A.row_partition, backend)
        stream = torch.cuda.current_stream().cuda_stream
        hp._capi.call("hpcla_fill_uniform_f64", b.v.data_ptr(), 0, n, wl.SEED_RHS, stream)
        dinv = hp.diag(A, reciprocal=True)
        Dinv = diagonal_matrix(hp, torch, backend, dinv.v)
        ws = hp.GMRESWorkspace(b, RESTART)
        y = b.similar()

        # -- (a), (b): the orthogonalisation step at fixed c, on a basis of uniform columns
        hp._capi.call("hpcla_fill_uniform_f64", ws.V.data_ptr(), 0, ws.V.numel(), wl.SEED_RHS + 1, stream)
        ws.V.mul_(0.2 / math.sqrt(n))                                # largest eigenvalue of V V^T about 0.3: repeated steps stay bounded
        ws.work.zero_()
        ws.work[-2:-1].fill_(-1.0)                                   # thr < 0: gate C cannot fire while g decays over repeated steps
        ws.small.zero_()
        ws.small_array("g").fill_(1.0)
        ws.w.v.copy_(b.v)
        cols = [hp.HPCVector(b.structural_hash, b.partition, ws.V[i * ws.ldv:i * ws.ldv + n], backend) for i in range(RESTART)]
        wc = b.copy()
        variants = {}
        for c in COLUMNS:
            variants[f"fused c={c}"] = (lambda f=FusedStep(hp, torch, ws, c): f(S))
            variants[f"composed c={c}"] = (lambda f=ComposedStep(hp, cols[:c], wc): f(S))
        steps = timed_table(torch, variants, args.runs, args.warmup, S)
        assert ws.state[:2].cpu().tolist() == [0, 0], "a gate fired inside the timed steps"
        step_rows = {}
        for c in COLUMNS:
            f, cmp_ = steps[f"fused c={c}"], steps[f"composed c={c}"]
            tbs = step_bytes_per_row(c) * n / (f[0] * 1e-3) / 1e12
            step_rows[c] = {"fused_ms": [round(v, 5) for v in f], "composed_ms": [round(v, 5) for v in cmp_],
                            "fused_over_composed": round(f[0] / cmp_[0], 4), "bytes_per_row": step_bytes_per_row(c),
                            "composed_bytes_per_row": 80 * c + 24, "fused_tbs": round(tbs, 3),
                            "fraction_of_stream": round(tbs / args.stream_tbs, 3)}

        # -- (a): the whole solve
        composed = {"none": ComposedGMRES(hp, A, b, RESTART), "jacobi": ComposedGMRES(hp, A, b, RESTART, Dinv)}

        def fused(M=None):
            _, info = hp.gmres(A, b, rtol=0.0, atol=0.0, restart=RESTART, maxiter=K, M=M, check_every=8, workspace=ws)
            assert info.iterations == K and info.status == "maxiter", info.status
            return info

        def spmvs():
            for _ in range(K):
                hp.mul_(y, A, b)

        agree = {}                                                   # the same recurrence before anything is timed
        for name, M in (("none", None), ("jacobi", dinv)):
            h_f = fused(M).residual_norms[:9]
            h_c = composed[name](8)
            agree[name] = max(abs(f - c_) / c_ for f, c_ in zip(h_f, h_c))
            assert agree[name] <= 1e-10, (name, h_f, h_c)
        table = timed_table(torch, {"hp.gmres M=None": lambda: fused(), "composed M=None": lambda: composed["none"](K),
                                    "hp.gmres M=jacobi": lambda: fused(dinv), "composed M=jacobi": lambda: composed["jacobi"](K),
                                    "1 x SpMV": spmvs}, max(3, args.runs // 2), 1, K)
        rec = {"rows": n, "nnz": int(A.nnz), "head_deviation_fused_vs_composed": {k: float(v) for k, v in agree.items()},
               "step": step_rows, "solve": {k: [round(x, 5) for x in v] for k, v in table.items()},
               "fused_over_composed_none": round(table["hp.gmres M=None"][0] / table["composed M=None"][0], 4),
               "fused_over_composed_jacobi": round(table["hp.gmres M=jacobi"][0] / table["composed M=jacobi"][0], 4)}
        record[label] = rec
        lines += [f"### {label} ({n} rows, {int(A.nnz)} stored entries)", "",
                  "| c | fused step, ms | composed step, ms | fused / composed | B/row fused | B/row composed | fused TB/s | of stream |",
                  "|---|---|---|---|---|---|---|---|"]
        lines += [f"| {c} | {r['fused_ms'][0]:.4f} | {r['composed_ms'][0]:.4f} | {r['fused_over_composed']:.4f} | {r['bytes_per_row']} | "
                  f"{r['composed_bytes_per_row']} | {r['fused_tbs']:.3f} | {r['fraction_of_stream']:.3f} |" for c, r in step_rows.items()]
        lines += ["", f"| call ({K} inner steps, restart {RESTART}) | ms / step, median | min | max |", "|---|---|---|---|"]
        lines += [f"| {k} | {v[0]:.4f} | {v[1]:.4f} | {v[2]:.4f} |" for k, v in table.items()]
        lines += ["", f"fused / composed: {rec['fused_over_composed_none']:.4f} (M=None), "
                      f"{rec['fused_over_composed_jacobi']:.4f} (M=jacobi)", ""]
        del A, b, ws, composed, Dinv, dinv, y, cols, wc, variants
        hp.clear_plan_cache()
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_gmres.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out, "bench_gmres_tables.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
