"""Worker for tests/test_gpu_ilu0.py::test_ilu0_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the GPU.
The 24 x 20 convection-diffusion case (tests/_bicgstab_cases.py):
  * on the uniform partition each rank's factors equal the restatement of its own block (tests/_ilu_cases.py: structure exactly,
    values within ILU_RTOL; the columns other ranks own are dropped);
  * ``hp.gmres`` and ``hp.bicgstab`` with ``M=hp.ilu0(A)`` converge within +-2 iterations of the restatements run with the
    blockwise operator, every rank reports the same count and status, the gathered x meets the true-residual bound, and
    ``check_every=3`` gives the bits of 8;
  * a partition that gives the last rank no rows builds and applies;
  * a zero diagonal in one rank's rows raises on every rank, with the global row.
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
    from tests import _bicgstab_cases as bc
    from tests import _ilu_cases as ic
    from tests import _pcg_cases as pc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[ilu0 rank {rank}/{nranks}]"
    rowptr, colidx, vals, bg = bc.convection_diffusion(orc, 24, 20)
    n = len(bg)

    def local_matrix(part, values=vals):
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[lo]), int(rowptr[hi])
        return hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], values[a:b_], n, backend,
                                        col_partition=np.asarray(part, dtype=np.int64))

    def check_factors(M, part, what):
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[lo]), int(rowptr[hi])
        wp, wc, wv = ic.block_csr(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], lo)
        bp, bcols, f, start = M.factors()
        assert start == lo and np.array_equal(bp, wp) and np.array_equal(bcols, wc), (tag, what)
        if len(wv):
            want = ic.sweep_factors(wp, wc, wv, 3, lo)
            dev = float(np.max(np.abs(f - want) / np.abs(want)))
            print(f"{tag} {what}: {hi - lo} rows, largest relative deviation of an entry {dev:.2e}", file=sys.stderr)
            assert dev <= ic.ILU_RTOL, (tag, what, dev)

    def same_on_every_rank(values):
        mine = torch.tensor(values, dtype=torch.int64)
        every = [torch.empty_like(mine) for _ in range(nranks)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, mine) for e in every), (tag, every)

    # -- the uniform partition: the factors, then both solves
    part = hp.uniform_partition(n, nranks)
    A = local_matrix(part)
    M = hp.ilu0(A)
    check_factors(M, part, "uniform")
    b = hp.HPCVector.from_global(bg, backend)
    K = ic.operator(ic.ilu_blocks(rowptr, colidx, vals, [int(v) for v in part]))
    for solver, restated in ((hp.gmres, ic.gmres_op), (hp.bicgstab, ic.bicgstab_op)):
        _, its_ref, status_ref, _ = restated(rowptr, colidx, vals, bg, K, rtol=1e-8)
        x, info = solver(A, b, M=M, rtol=1e-8, check_every=8)
        assert status_ref == "converged" and info.converged, (tag, solver.__name__, info.status)
        same_on_every_rank([info.iterations, int(info.converged)])
        print(f"{tag} {solver.__name__}: iterations {info.iterations} (restatement with the blocked operator {its_ref})", file=sys.stderr)
        assert abs(info.iterations - its_ref) <= 2, (tag, solver.__name__, info.iterations, its_ref)
        xg = x.gather()
        true = np.linalg.norm(bg - pc.matvec(rowptr, colidx, vals, xg)) / np.linalg.norm(bg)
        assert true <= pc.TRUE_RES_RTOL, (tag, solver.__name__, true)
        x3, info3 = solver(A, b, M=M, rtol=1e-8, check_every=3)
        assert info3 == info and np.array_equal(pc.bits(x3.gather()), pc.bits(xg)), tag + " chunk"

    # -- the last rank holds no rows
    cut = hp.uniform_partition(n, nranks - 1)
    part0 = np.concatenate([cut, [n]]).astype(np.int64)
    A0 = local_matrix(part0)
    M0 = hp.ilu0(A0)
    check_factors(M0, part0, "empty last rank")
    assert (M0.n == 0) == (rank == nranks - 1), tag
    z0 = M0.apply(hp.HPCVector.zeros(part0, backend))
    assert not z0.local_values().any(), tag

    # -- a zero diagonal in the rows of the last rank that has some: every rank raises, with the global row
    bad_row = int(part[nranks - 1]) + 7
    bad = vals.copy()
    bad[int(rowptr[bad_row]) + int(np.flatnonzero(colidx[rowptr[bad_row]:rowptr[bad_row + 1]] == bad_row)[0])] = 0.0
    try:
        hp.ilu0(local_matrix(part, bad))
        raise AssertionError(tag + " no error")
    except ValueError as e:
        assert str(e) == f"ilu0: the diagonal of row {bad_row} is zero or NaN", (tag, str(e))
    check_factors(hp.ilu0(A), part, "after the error")

    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
