"""Worker for tests/test_gpu_lobpcg.py::test_lobpcg_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the
GPU.  The 5-point matrix on the square 16 x 16 grid (tests/_lobpcg_cases.py), ``k = 4``, ``"SA"`` and ``"LA"``, on the uniform
row partition and on one whose last rank holds no rows (that rank still takes part in every all-reduce and exchange):
  * ``vals``, ``residual_norms``, ``history``, ``anorm``, ``iterations`` and ``status`` are bit-identical on every rank (only
    rank 0 decides, and its theta and C are the ones every rank combines with);
  * ``vals`` is within 1e-12 anorm of the one-rank run (a serial backend on the same GPU) and holds the double eigenvalue twice;
  * the gathered X meets the true-residual bound 2 tol anorm and is orthonormal to 1e-12; the count stays under the cap.
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
    from tests import _lobpcg_cases as lc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    serial = hp.backend_rocm_serial(np.float64, np.int32)
    tag = f"[lobpcg rank {rank}/{nranks}]"

    name, k = lc.RANK_CASE
    dense = lc.dense_matrices(orc)[name]
    rowptr, colidx, vals, n = lc.csr_of(dense)
    A1 = hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, serial)
    uniform = hp.uniform_partition(n, nranks)
    empty_last = np.concatenate([hp.uniform_partition(n, nranks - 1), [n]]).astype(np.int64)      # the last rank holds no rows
    codes = {"converged": 1, "maxiter": 3, "breakdown": 2}
    for label, part in (("uniform", uniform), ("empty last rank", empty_last)):
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[lo]), int(rowptr[hi])
        A = hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], n, backend, col_partition=part)
        assert np.array_equal(A.row_partition, part), (tag, A.row_partition)
        for which in ("SA", "LA"):
            got1, _, info1 = hp.lobpcg(A1, k=k, which=which, tol=lc.TOL)
            got, X, info = hp.lobpcg(A, k=k, which=which, tol=lc.TOL)
            assert info1.converged and info.converged and info.status == "converged", (tag, info.status)
            mine = torch.from_numpy(np.concatenate([got, info.residual_norms, [info.anorm, info.iterations, codes[info.status]],
                                                    info.history]))
            size = torch.tensor([mine.numel()])
            sizes = [torch.empty_like(size) for _ in range(nranks)]
            dist.all_gather(sizes, size)
            assert all(int(s) == mine.numel() for s in sizes), (tag, sizes)
            every = [torch.empty_like(mine) for _ in range(nranks)]
            dist.all_gather(every, mine)
            assert all(torch.equal(e.view(torch.int64), mine.view(torch.int64)) for e in every), (tag, label, which)
            dv = np.abs(got - got1).max() / info1.anorm
            Xg = X.gather()
            res = np.linalg.norm(dense @ Xg - Xg * got, axis=0).max() / (lc.TOL * info.anorm)
            orth = np.abs(Xg.T @ Xg - np.eye(k)).max()
            exact = lc.poisson16_exact(k, which)
            print(f"{tag} {label} {which}: {info.iterations} iterations (one rank {info1.iterations}), values {dv:.1e} anorm from one "
                  f"rank's, true residual {res:.2f} tol anorm, orthogonality {orth:.1e}", file=sys.stderr)
            assert dv <= 1e-12, (tag, dv)
            assert np.abs(got - exact).max() <= 2 * lc.TOL * 8.0 and abs(got[1] - got[2]) <= 2 * lc.TOL * 8.0, (tag, got)
            assert res <= 2.0 and orth <= lc.ORTH_TOL, (tag, res, orth)
            assert info.iterations <= 1.5 * info1.iterations + 5, (tag, info.iterations, info1.iterations)
            assert Xg.shape == (n, k) and X.local_values().shape == (hi - lo, k), tag
            torch.cuda.synchronize()
        hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
