#!/usr/bin/env python3
"""The eigensolver's (``hp.eigsh``) two device pieces against what was available before it, on the 4096 x 4096 5-point matrix
(16 777 216 rows).  One GPU, Float64, Int32 indices.

(a) A cycle of Lanczos steps at ``ncv`` = 20 and 64: ``hpcla_eigsh_steps_f64_i32`` for columns 0 .. ncv-1 in one call (SpMV,
    dots, update, dots, the Lanczos second pass, next; no read-back) against the same steps composed from ``mul_``, ``hp.dot``,
    ``axpy_``, ``hp.norm`` and ``w / hn`` with host scalars, as a caller of the parent commit writes them (nothing under them
    changes in this commit, so they stand for the parent).  Reported per step: the cycle's time over ncv.  Byte model per row
    of the step at c columns next to the SpMV: 32 c + 48 + 16 ceil(c / 8); composed 80 c + 24.
(b) The restart's rotate kernel, in place with the moved column, at (m, p) = (20, 12) and (64, 35): against its byte model
    8 (m + p) + 16 per row at the achievable HBM stream rate (``--stream-tbs``, default 6.3 TB/s), and against ``torch.matmul``
    on the same basis plus the copy back into it (``tmp = S^T V[0:m]; V[0:p] = tmp; V[p] = V[m]``), the alternative available
    before.  S has orthonormal columns, so repeated rotations of the same basis stay bounded.

Every figure is a median of ``--runs`` timed calls (default 7) after ``--warmup`` untimed ones, the variants ALTERNATING call by
call; HIP events on the stream around the call, which contain every read-back.

Prints one JSON line and writes <out>/bench_eigsh.json and <out>/bench_eigsh_tables.md (default out: profiles/).
usage: python benchmarks/bench_eigsh.py [--runs R] [--warmup W] [--out DIR] [--small-only]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCVS = (20, 64)
ROTATIONS = ((20, 12), (64, 35))


def step_bytes_per_row(c):
    """DESIGN.md, the step's byte table next to the SpMV: dots, update, dots, update, next."""
    return 32 * c + 48 + 16 * ((c + 7) // 8)


class FusedCycle:
    """Columns 0 .. m-1 of a first cycle in one library call, from a normalised start in column 0."""

    def __init__(self, hp, torch, A, ws):
        from hpcla_amd.sparse import get_vector_plan
        plan = get_vector_plan(A, ws.w)
        assert not plan.is_i64
        self.hp, self.ws, self.torch = hp, ws, torch
        blk = plan.matrix_block(A)
        self.spmv = (blk[0], A.backend.rccl, *blk[1:])

    def __call__(self):
        ws, P = self.ws, (lambda t: t.data_ptr())
        self.hp._capi.call("hpcla_eigsh_steps_f64_i32", *self.spmv, P(ws.V), ws.ldv, P(ws.w.v), P(ws.small), P(ws.work), ws.ncv, 0,
                           ws.ncv, 1, self.torch.cuda.current_stream().cuda_stream)


class ComposedCycle:
    """The same cycle from mul_, hp.dot, axpy_, hp.norm and a division (straight into the next column) with host scalars."""

    def __init__(self, hp, torch, A, cols, w):
        self.hp, self.A, self.V, self.w = hp, A, cols, w
        self.stream = torch.cuda.current_stream().cuda_stream

    def __call__(self):
        hp, V, w = self.hp, self.V, self.w
        m = len(V) - 1
        T, beta = np.zeros((m, m)), np.zeros(m)
        for j in range(m):
            hp.mul_(w, self.A, V[j])
            for _pass in range(2):
                h = [hp.dot(V[i], w) for i in range(j + 1)]
                for i in range(j + 1):
                    w.axpy_(-h[i], V[i])
                T[:j + 1, j] += h
            beta[j] = hn = hp.norm(w)
            hp._capi.call("hpcla_divide_f64", w.v.data_ptr(), float(hn), V[j + 1].v.data_ptr(), w.local_length, self.stream)
        return T, beta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--small-only", action="store_true", help="256 x 256 only (a rehearsal of the script)")
    args = ap.parse_args()
    import torch
    import hpcla_amd as hp
    from benchmarks.bench_pcg import timed_table
    from benchmarks.extra_workloads import device_stencil
    if not torch.cuda.is_available():
        raise SystemExit("bench_eigsh.py measures on the GPU; none is visible")
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    lib = hp._capi.load()
    record = {"runs": args.runs, "warmup": args.warmup, "stream_tbs": args.stream_tbs, "gpu": torch.cuda.get_device_name(0),
              "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
              "unit": "ms, median (min, max)"}
    lines = [f"GPU: {record['gpu']} ({record['arch']})", ""]
    for label, dims in ([("256x256", (256, 256))] if args.small_only else [("4096x4096", (4096, 4096))]):
        n = int(np.prod(dims))
        A = device_stencil(hp, torch, backend, dims, 0, n)
        v0 = hp.HPCVector.from_global(np.random.default_rng(0).uniform(-1.0, 1.0, n), backend)
        rec = {"rows": n, "nnz": int(A.nnz), "cycle": {}, "rotate": {}}

        # -- (a) a first cycle of ncv steps, fused and composed, from the same start
        lines += [f"### {label} ({n} rows, {int(A.nnz)} stored entries)", "",
                  "| ncv | fused, ms / step | composed, ms / step | fused / composed | B/row fused (mean over c) | B/row composed | first-cycle T, fused vs composed |",
                  "|---|---|---|---|---|---|---|"]
        for m in NCVS:
            ws = hp.EigshWorkspace(v0, m)
            start = v0 / hp.norm(v0)
            cols = [hp.HPCVector(v0.structural_hash, v0.partition, ws.V[i * ws.ldv:i * ws.ldv + n], backend) for i in range(m + 1)]
            cols[0].v.copy_(start.v)
            fused, composed = FusedCycle(hp, torch, A, ws), ComposedCycle(hp, torch, A, cols, v0.similar())
            ws.small.zero_()
            ws.work.zero_()
            fused()                                              # the same recurrence before anything is timed
            torch.cuda.synchronize()
            assert ws.state[:2].cpu().tolist() == [0, 0], "a gate fired"
            T_f = np.triu(ws.small_array("T").cpu().numpy().reshape(m, m).T)
            T_c, _ = composed()
            agree = float(np.abs(T_f - T_c).max() / np.abs(T_c).max())
            assert agree <= 1e-10, agree
            table = timed_table(torch, {"fused": fused, "composed": composed}, args.runs, args.warmup, m)
            assert ws.state[:2].cpu().tolist() == [0, 0], "a gate fired inside the timed cycles"
            mean_b = sum(step_bytes_per_row(c) for c in range(1, m + 1)) / m
            mean_c = sum(80 * c + 24 for c in range(1, m + 1)) / m
            rec["cycle"][m] = {"fused_ms_per_step": [round(v, 5) for v in table["fused"]],
                               "composed_ms_per_step": [round(v, 5) for v in table["composed"]],
                               "fused_over_composed": round(table["fused"][0] / table["composed"][0], 4),
                               "mean_bytes_per_row_fused": round(mean_b, 1), "mean_bytes_per_row_composed": round(mean_c, 1),
                               "first_cycle_T_deviation": agree}
            lines += [f"| {m} | {table['fused'][0]:.4f} ({table['fused'][1]:.4f}, {table['fused'][2]:.4f}) | {table['composed'][0]:.4f} "
                      f"({table['composed'][1]:.4f}, {table['composed'][2]:.4f}) | {rec['cycle'][m]['fused_over_composed']:.4f} | "
                      f"{mean_b:.0f} | {mean_c:.0f} | {agree:.1e} |"]
            del ws, cols, fused, composed, start
            torch.cuda.empty_cache()

        # -- (b) the rotate kernel against its byte model and against torch.matmul plus the copy back
        lines += ["", "| (m, p) | rotate, ms | B/row | TB/s | of stream | model at stream rate, ms | torch.matmul + copy back, ms | rotate / matmul |",
                  "|---|---|---|---|---|---|---|---|"]
        stream = torch.cuda.current_stream().cuda_stream
        for m, p in ROTATIONS:
            ldv = n + (n & 1)
            V = torch.empty((m + 1) * ldv, dtype=torch.float64, device="cuda")
            hp._capi.call("hpcla_fill_uniform_f64", V.data_ptr(), 0, V.numel(), 0xBEEF, stream)
            V.mul_(1.0 / math.sqrt(n))
            S_h = np.linalg.qr(np.random.default_rng(m).uniform(-1.0, 1.0, (m, m)))[0][:, :p]
            S = torch.from_numpy(np.ascontiguousarray(S_h.T).reshape(-1)).cuda()         # column j contiguous
            St = torch.from_numpy(np.ascontiguousarray(S_h.T)).cuda()                    # p x m
            Vm = V.view(m + 1, ldv)
            tmp = torch.empty((p, ldv), dtype=torch.float64, device="cuda")

            def rotate():
                assert lib.hpcla_eigsh_rotate_f64(V.data_ptr(), ldv, m, p, S.data_ptr(), 1, None, 0, 0, n, stream) == 0

            def matmul():
                torch.matmul(St, Vm[:m], out=tmp)
                Vm[:p].copy_(tmp)
                Vm[p].copy_(Vm[m])

            table = timed_table(torch, {"rotate": rotate, "matmul": matmul}, args.runs, args.warmup, 1)
            bpr = 8 * (m + p) + 16
            tbs = bpr * n / (table["rotate"][0] * 1e-3) / 1e12
            model_ms = bpr * n / (args.stream_tbs * 1e12) * 1e3
            rec["rotate"][f"{m},{p}"] = {"rotate_ms": [round(v, 5) for v in table["rotate"]],
                                         "matmul_copy_ms": [round(v, 5) for v in table["matmul"]], "bytes_per_row": bpr,
                                         "rotate_tbs": round(tbs, 3), "fraction_of_stream": round(tbs / args.stream_tbs, 3),
                                         "model_ms": round(model_ms, 5),
                                         "rotate_over_matmul": round(table["rotate"][0] / table["matmul"][0], 4)}
            lines += [f"| ({m}, {p}) | {table['rotate'][0]:.4f} ({table['rotate'][1]:.4f}, {table['rotate'][2]:.4f}) | {bpr} | {tbs:.3f} | "
                      f"{tbs / args.stream_tbs:.3f} | {model_ms:.4f} | {table['matmul'][0]:.4f} ({table['matmul'][1]:.4f}, "
                      f"{table['matmul'][2]:.4f}) | {table['rotate'][0] / table['matmul'][0]:.4f} |"]
            del V, Vm, tmp, S, St
            torch.cuda.empty_cache()
        lines.append("")
        record[label] = rec
        del A, v0
        hp.clear_plan_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_eigsh.json"), "w") as f:
        json.dump(record, f, indent=1)
    with open(os.path.join(args.out, "bench_eigsh_tables.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
