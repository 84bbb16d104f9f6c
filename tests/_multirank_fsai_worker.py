"""Worker for tests/test_gpu_fsai.py::test_fsai_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the GPU.
The 24 x 20 scaled Poisson case (tests/_pcg_cases.py):
  * on the uniform partition each rank's G equals the rank-local restatement (tests/_fsai_cases.py: structure exactly, values
    within FSAI_RTOL; the columns other ranks own are ignored), and ``max_row`` is the same on every rank;
  * ``hp.cg(A, b, M=hp.fsai(A))`` converges within +-2 iterations of ``pcg_op`` run with the blocked G, every rank reports the
    same count and status, the gathered x meets the true-residual bound, and ``check_every=3`` gives the bits of 8;
  * a partition that gives the last rank no rows builds, with the same checks on G;
  * a matrix that is not positive definite in one rank's rows raises on every rank, with the global row.
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
    from tests import _fsai_cases as fc
    from tests import _pcg_cases as pc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[fsai rank {rank}/{nranks}]"
    rowptr, colidx, vals, bg = pc.scaled_poisson(orc, 24, 20)
    n = len(bg)

    def local_matrix(part, values=vals):
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[lo]), int(rowptr[hi])
        return hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], values[a:b_], n, backend,
                                        col_partition=np.asarray(part, dtype=np.int64)), lo, hi, a, b_

    def check_G(F, part, what):
        A_lo, A_hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[A_lo]), int(rowptr[A_hi])
        wp, wc, wv = fc.fsai_cholesky(rowptr[A_lo:A_hi + 1] - a, colidx[a:b_], vals[a:b_], A_lo)
        G = F.G
        gp = G.rowptr_target.cpu().numpy().astype(np.int64)
        gc = G.col_indices[G.colval.astype(np.int64)] if G.nnz else np.zeros(0, dtype=np.int64)
        gv = G.nzval.cpu().numpy()
        assert np.array_equal(gp, wp) and np.array_equal(gc, wc), (tag, what)
        assert np.all((gc >= A_lo) & (gc < A_hi)), (tag, what)
        if len(wv):
            dev = float(np.max(np.abs(gv - wv) / np.abs(wv)))
            print(f"{tag} {what}: {A_hi - A_lo} rows, largest relative deviation of an entry {dev:.2e}", file=sys.stderr)
            assert dev <= fc.FSAI_RTOL, (tag, what, dev)
        assert np.array_equal(G.row_partition, part) and np.array_equal(F.Gt.row_partition, part), (tag, what)
        mine = torch.tensor([F.max_row], dtype=torch.int64)
        every = [torch.empty_like(mine) for _ in range(nranks)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, mine) for e in every) and F.max_row == 3, (tag, what, every)

    # -- the uniform partition: G, then the solve
    part = hp.uniform_partition(n, nranks)
    A, lo, hi, _, _ = local_matrix(part)
    F = hp.fsai(A)
    check_G(F, part, "uniform")
    b = hp.HPCVector.from_global(bg, backend)
    Gb = fc.fsai_blocks(rowptr, colidx, vals, [int(v) for v in part])
    _, its_ref, status_ref, h_ref = fc.pcg_op(rowptr, colidx, vals, bg, Gb, rtol=1e-8)
    x, info = hp.cg(A, b, M=F, rtol=1e-8, check_every=8)
    assert status_ref == "converged" and info.converged and info.status == "converged", (tag, info.status)
    mine = torch.tensor([info.iterations, 1], dtype=torch.int64)
    every = [torch.empty_like(mine) for _ in range(nranks)]
    dist.all_gather(every, mine)
    assert all(torch.equal(e, mine) for e in every), (tag, every)
    head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:pc.HEAD], h_ref[:pc.HEAD]))
    print(f"{tag} iterations {info.iterations} (pcg_op with the blocked G {its_ref}), head deviation {head:.2e}", file=sys.stderr)
    assert abs(info.iterations - its_ref) <= 2, (tag, info.iterations, its_ref)
    assert head <= pc.CG_RTOL, (tag, head)
    xg = x.gather()
    true = np.linalg.norm(bg - pc.matvec(rowptr, colidx, vals, xg)) / np.linalg.norm(bg)
    assert true <= pc.TRUE_RES_RTOL, (tag, true)
    x3, info3 = hp.cg(A, b, M=F, rtol=1e-8, check_every=3)
    assert info3 == info and np.array_equal(pc.bits(x3.gather()), pc.bits(xg)), tag + " chunk"

    # -- the last rank holds no rows
    cut = hp.uniform_partition(n, nranks - 1)
    part0 = np.concatenate([cut, [n]]).astype(np.int64)
    A0, _, _, _, _ = local_matrix(part0)
    F0 = hp.fsai(A0)
    check_G(F0, part0, "empty last rank")
    assert (F0.G.nrows_local == 0) == (rank == nranks - 1), tag

    # -- not positive definite in the rows of the last rank that has some: every rank raises, with the global row
    bad_row = int(part[nranks - 1]) + 7
    bad = vals.copy()
    bad[int(rowptr[bad_row]) + int(np.flatnonzero(colidx[rowptr[bad_row]:rowptr[bad_row + 1]] == bad_row)[0])] = -1.0
    Ab, _, _, _, _ = local_matrix(part, bad)
    try:
        hp.fsai(Ab)
        raise AssertionError(tag + " no error")
    except ValueError as e:
        assert str(e) == f"fsai: A is not positive definite on the pattern of row {bad_row}", (tag, str(e))
    check_G(hp.fsai(A), part, "after the error")

    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
