#!/usr/bin/env python3
"""A cycle of the truncated SVD (``hp.svds``) against the same steps composed from the public operators, on the stacked Poisson
matrix of ``benchmarks/bench_lsqr.py``: the device-generated 7-point Laplacian of a 512 x 512 x 64 slab (n = 16 777 216) with a
diagonal block of the same size stacked under it (2n x n).  One GPU, Float64, Int32 indices.

A first cycle of Golub-Kahan steps with full two-sided reorthogonalisation at ``ncv`` = 20 and 64, from the same normalised start:

  fused      ``hpcla_svds_steps_f64_i32`` for columns 0 .. ncv-1 in ONE call (per column: SpMV on A, dots, update, dots, the
             second pass of the left side, next; SpMV on the transpose, the same on the right side; no read-back).
  composed   the same steps from ``mul_``, ``hp.dot``, ``axpy_``, ``hp.norm`` and a division with host scalars: one host call
             per kernel and a read-back per reduction, 4 c + 2 of them in the step that orthogonalises against c columns on each
             side, as a caller of the parent commit writes it (nothing under it changes in this commit, so it stands for the
             parent).
  floor      one ``mul_`` on A plus one on its materialised transpose per step: what both forms stand on.  The share of a fused
             step that goes to orthogonalisation is reported as 1 - floor / fused.

Reported per step: the cycle's time over ncv.  Every figure is a median of ``--runs`` timed calls (default 7) after ``--warmup``
untimed ones, the variants ALTERNATING call by call; HIP events on the stream around the call, which contain every read-back.
Before anything is timed the first cycle's projected matrix of the fused form is compared with the composed form's.

Prints one JSON line and writes <out>/bench_svds.json and <out>/bench_svds_tables.md (default out: profiles/).
usage: python benchmarks/bench_svds.py [--runs R] [--warmup W] [--out DIR] [--small-only]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCVS = (20, 64)


class FusedCycle:
    """Columns 0 .. m-1 of a first cycle in one library call, from a normalised start in column 0 of V."""

    def __init__(self, hp, torch, A, At, ws):
        from hpcla_amd.sparse import get_vector_plan
        plan, plan_t = get_vector_plan(A, ws.v), get_vector_plan(At, ws.u)
        assert not plan.is_i64 and not plan_t.is_i64
        self.hp, self.ws, self.torch = hp, ws, torch
        self.blocks = plan.matrix_block(A) + plan_t.matrix_block(At)
        self.comm = A.backend.rccl

    def __call__(self):
        ws, P = self.ws, (lambda t: t.data_ptr())
        self.hp._capi.call("hpcla_svds_steps_f64_i32", self.comm, *self.blocks, P(ws.U), ws.ldu, P(ws.V), ws.ldv, P(ws.u.v),
                           P(ws.v.v), P(ws.small), P(ws.work), ws.ncv, 0, ws.ncv, 1, self.torch.cuda.current_stream().cuda_stream)


class ComposedCycle:
    """The same cycle from mul_, hp.dot, axpy_, hp.norm and a division (straight into the next column) with host scalars."""

    def __init__(self, hp, torch, A, At, Ucols, Vcols, u, v):
        self.hp, self.A, self.At, self.U, self.V, self.u, self.v = hp, A, At, Ucols, Vcols, u, v
        self.stream = torch.cuda.current_stream().cuda_stream

    def _half(self, w, W, c):
        hp = self.hp
        total = np.zeros(c)
        for _pass in range(2):
            h = [hp.dot(W[i], w) for i in range(c)]
            for i in range(c):
                w.axpy_(-h[i], W[i])
            total += h
        return total, hp.norm(w)

    def __call__(self):
        hp, U, V, u, v = self.hp, self.U, self.V, self.u, self.v
        m = len(U)
        B, beta = np.zeros((m, m)), np.zeros(m)
        for j in range(m):
            hp.mul_(u, self.A, V[j])
            B[:j, j], B[j, j] = self._half(u, U, j)
            hp._capi.call("hpcla_divide_f64", u.v.data_ptr(), float(B[j, j]), U[j].v.data_ptr(), u.local_length, self.stream)
            hp.mul_(v, self.At, U[j])
            _, beta[j] = self._half(v, V, j + 1)
            hp._capi.call("hpcla_divide_f64", v.v.data_ptr(), float(beta[j]), V[j + 1].v.data_ptr(), v.local_length, self.stream)
        return B, beta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small-only", action="store_true", help="64^3 only (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from benchmarks.bench_lsqr import tall_operator
    from benchmarks.bench_pcg import timed_table
    if not torch.cuda.is_available():
        raise SystemExit("bench_svds.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    record = {"runs": args.runs, "warmup": args.warmup, "gpu": torch.cuda.get_device_name(0),
              "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "unit": "ms per step, median (min, max)"}
    lines = [f"GPU: {record['gpu']} ({record['arch']})", ""]
    for label, dims in ([("64x64x64", (64, 64, 64))] if args.small_only else [("512x512x64", (512, 512, 64))]):
        n = int(np.prod(dims))
        A = tall_operator(hp, torch, backend, dims)
        print(f"bench_svds: {label}: operator built, transposing", file=sys.stderr, flush=True)
        At = hp.transpose(A).materialize()
        print(f"bench_svds: {label}: transpose materialised", file=sys.stderr, flush=True)
        v0 = hp.HPCVector.from_global(np.random.default_rng(0).uniform(-1.0, 1.0, n), backend, partition=A.col_partition)
        rec = {"rows": 2 * n, "cols": n, "nnz": int(A.nnz), "cycle": {}}
        lines += [f"### {label}: {2 * n} x {n}, {int(A.nnz)} stored entries", "",
                  "| ncv | fused, ms / step | composed, ms / step | fused / composed | two SpMVs, ms / step | orthogonalisation share "
                  "of a fused step | first-cycle B, fused vs composed |", "|---|---|---|---|---|---|---|"]
        for m in NCVS:
            ws = hp.SvdsWorkspace(A, m)
            assert ws.ldu == 2 * n and ws.ldv == n
            col = lambda like, buf, ld, i: hp.HPCVector(like.structural_hash, like.partition, buf[i * ld:i * ld + like.local_length],
                                                        backend)
            Ucols = [col(ws.u, ws.U, ws.ldu, i) for i in range(m)]
            Vcols = [col(ws.v, ws.V, ws.ldv, i) for i in range(m + 1)]
            Vcols[0].v.copy_((v0 / hp.norm(v0)).v)
            fused = FusedCycle(hp, torch, A, At, ws)
            composed = ComposedCycle(hp, torch, A, At, Ucols, Vcols, ws.u.similar(), ws.v.similar())
            yu, yv = ws.u.similar(), ws.v.similar()

            def floor():
                for _ in range(m):
                    hp.mul_(yu, A, Vcols[0])
                    hp.mul_(yv, At, yu)

            ws.small.zero_()
            ws.work.zero_()
            fused()                                              # the same recurrence before anything is timed
            torch.cuda.synchronize()
            assert ws.state[:2].cpu().tolist() == [0, 0], "a gate fired"
            B_f = np.triu(ws.small_array("B").cpu().numpy().reshape(m, m).T)
            b_f = ws.small_array("beta").cpu().numpy()
            B_c, b_c = composed()
            agree = float(max(np.abs(B_f - B_c).max(), np.abs(b_f - b_c).max()) / np.abs(B_c).max())
            assert agree <= 1e-10, agree
            table = timed_table(torch, {"fused": fused, "composed": composed, "floor": floor}, args.runs, args.warmup, m)
            assert ws.state[:2].cpu().tolist() == [0, 0], "a gate fired inside the timed cycles"
            share = 1.0 - table["floor"][0] / table["fused"][0]
            rec["cycle"][m] = {"fused_ms_per_step": [round(x, 5) for x in table["fused"]],
                               "composed_ms_per_step": [round(x, 5) for x in table["composed"]],
                               "two_spmv_ms_per_step": [round(x, 5) for x in table["floor"]],
                               "fused_over_composed": round(table["fused"][0] / table["composed"][0], 4),
                               "orthogonalisation_share_of_fused": round(share, 4), "first_cycle_B_deviation": agree}
            fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f}, {t[2]:.4f})"
            lines += [f"| {m} | {fmt(table['fused'])} | {fmt(table['composed'])} | {rec['cycle'][m]['fused_over_composed']:.4f} | "
                      f"{fmt(table['floor'])} | {share:.3f} | {agree:.1e} |"]
            del ws, Ucols, Vcols, fused, composed, yu, yv
            torch.cuda.empty_cache()
        lines.append("")
        record[label] = rec
        del A, At, v0
        hp.clear_plan_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_svds.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out, "bench_svds_tables.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
