"""Worker for tests/test_gpu_minres.py::test_minres_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the
GPU.  The 24 x 20 saddle-point case (tests/_minres_cases.py: 960 rows, 320 per rank on three), without a preconditioner and, in
its scaled form, with the Jacobi weights, ``check_every=8``:
  * every rank reports the same ``CGInfo`` (the solve ends: no rank leaves the chunk loop alone);
  * the head of the history is within HIST_RTOL of the restatement, the iteration count within the window of
    ``_minres_cases.EXPECTED`` (the four summation orders, 2 more either way);
  * the gathered x is within 10 times the restatement's own error of numpy.linalg.solve, its true residual in the tested norm
    within twice the limit, and it agrees with a one-rank run (a serial backend on the same GPU) to that same answer margin;
  * ``check_every=3`` gives the same bits as 8;
  * diag(1, 0, 0, ...) with b = (1, 0, ...), one row per rank or more: one iteration, residual norms (1, 0) exactly -- the
    history pair is formed from global scalars and must not be summed over the ranks.
Exit code 0 = all passed on this rank."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main():
    import torch
    import torch.distributed as dist
    import hpcla_amd as hp
    from oracle import oracle as orc
    from tests import _minres_cases as mc
    from tests import _pcg_cases as pc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    serial = hp.backend_rocm_serial(np.float64, np.int32)
    tag = f"[minres rank {rank}/{nranks}]"

    def on_ranks(rowptr, colidx, vals, bg):
        n = len(bg)
        part = hp.uniform_partition(n, nranks)
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[lo]), int(rowptr[hi])
        A = hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], n, backend)
        return A, hp.HPCVector.from_global(bg, backend)

    def same_everywhere(info):
        mine = (info.converged, info.iterations, info.status, info.residual_norms)
        every = [None] * nranks
        dist.all_gather_object(every, mine)
        assert all(e == mine for e in every), (tag, "ranks disagree", [e[:3] for e in every])

    cases = mc.all_cases(orc)
    for key in (("saddle", mc.RANK_SIZE, False), ("scaled_saddle", mc.RANK_SIZE, True)):
        rowptr, colidx, vals, bg, dinv = cases[key]
        M = "jacobi" if dinv is not None else None
        dense = mc.dense_of(rowptr, colidx, vals)
        x_ref = np.linalg.solve(dense, bg)
        x_res, its_ref, _, hist_ref = mc.minres(rowptr, colidx, vals, bg, dinv=dinv)
        err_ref = np.linalg.norm(x_res - x_ref) / np.linalg.norm(x_ref)
        A, b = on_ranks(rowptr, colidx, vals, bg)
        assert A.nrows_local == len(bg) // nranks, (tag, A.nrows_local)
        x, info = hp.minres(A, b, M=M, check_every=8)
        same_everywhere(info)
        want, lo, hi = mc.EXPECTED[key]
        assert (info.status, info.converged) == ("converged", True), (tag, key, info.status)
        assert lo - 2 <= info.iterations <= hi + 2, (tag, key, info.iterations)
        assert len(info.residual_norms) == info.iterations + 1, (tag, key)
        head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:mc.HEAD], hist_ref[:mc.HEAD]))
        xg = x.gather()
        err = np.linalg.norm(xg - x_ref) / np.linalg.norm(x_ref)
        true = mc.m_norm(bg - dense @ xg, dinv) / (1e-8 * mc.m_norm(bg, dinv))
        x1, info1 = hp.minres(hp.HPCSparseMatrix_local(rowptr, colidx, vals, len(bg), serial), hp.HPCVector.from_global(bg, serial),
                              M=M, check_every=8)
        x1 = x1.local_values()
        err1 = np.linalg.norm(x1 - x_ref) / np.linalg.norm(x_ref)
        across = np.linalg.norm(xg - x1) / np.linalg.norm(x_ref)
        print(f"{tag} {key}: converged at {info.iterations} (restatement {its_ref}, one rank {info1.iterations}), head deviation "
              f"{head:.2e}, against solve {err:.2e} (restatement {err_ref:.2e}), true residual {true:.3f} of the limit, against "
              f"one rank {across:.2e}", file=sys.stderr)
        assert head <= mc.HIST_RTOL, (tag, key, head)
        assert err <= 10 * err_ref and err1 <= 10 * err_ref and true <= 2.0, (tag, key, err, err1, err_ref, true)
        assert across <= 10 * err_ref, (tag, key, across)             # the answer margin; only the summation order differs
        x3, info3 = hp.minres(A, b, M=M, check_every=3)
        assert info3 == info and np.array_equal(pc.bits(x3.gather()), pc.bits(xg)), (tag, key, "chunk")
        hp.clear_plan_cache()

    # a globally reduced scalar is not summed again across ranks
    k = nranks + 1
    d = np.zeros(k)
    d[0] = 1.0
    A, b = on_ranks(*pc.diag_matrix(d), d.copy())
    x, info = hp.minres(A, b)
    same_everywhere(info)
    assert (info.iterations, info.status, info.residual_norms) == (1, "converged", [1.0, 0.0]), (tag, info)
    xg = x.gather()
    assert xg[0] == 1.0 and not xg[1:].any(), (tag, xg)
    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
