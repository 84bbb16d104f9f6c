"""Worker for tests/test_gpu_eigsh.py::test_eigsh_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the
GPU.  The plain 5-point matrix on 24 x 20 (tests/_eigsh_cases.py), ``k = 4``, ``ncv = 20`` -- c passes 8 and 16, so the
all-reduces of the Gram-Schmidt sums are multi-slice -- for ``"LA"`` and ``"SA"``:
  * every rank reports the same ``iterations``, ``restarts`` and ``status`` (only rank 0 decides: no rank leaves the loop alone);
  * ``vals`` is within VAL_RTOL * anorm of the one-rank run (a serial backend on the same GPU), the step count within one cycle;
  * the gathered X meets the true-residual bound 2 tol anorm and is orthonormal to 1e-12.
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
    from tests import _eigsh_cases as ec
    from tests import _pcg_cases as pc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    serial = hp.backend_rocm_serial(np.float64, np.int32)
    tag = f"[eigsh rank {rank}/{nranks}]"

    _, (nx, ny), k, m = ec.RANK_CASE
    rowptr, colidx, vals = ec.plain_poisson(orc, nx, ny)
    n = len(rowptr) - 1
    part = hp.uniform_partition(n, nranks)
    lo, hi = int(part[rank]), int(part[rank + 1])
    a, b_ = int(rowptr[lo]), int(rowptr[hi])
    A = hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], n, backend)
    A1 = hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, serial)
    codes = {"converged": 1, "maxiter": 0, "breakdown": 2, "invariant": 4}
    for which in ("LA", "SA"):
        got1, _, info1 = hp.eigsh(A1, k=k, which=which, ncv=m, tol=ec.TOL)
        got, X, info = hp.eigsh(A, k=k, which=which, ncv=m, tol=ec.TOL)
        assert info1.converged and info.converged and info.status == "converged", (tag, info.status)
        mine = torch.tensor([info.iterations, info.restarts, codes[info.status]], dtype=torch.int64)
        every = [torch.empty_like(mine) for _ in range(nranks)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, mine) for e in every), (tag, every)
        dv = np.abs(got - got1).max() / info1.anorm
        Xg = X.gather()
        AX = np.stack([pc.matvec(rowptr, colidx, vals, Xg[:, i]) for i in range(k)], axis=1)
        res = np.linalg.norm(AX - Xg * got, axis=0).max() / (ec.TOL * info.anorm)
        orth = np.abs(Xg.T @ Xg - np.eye(k)).max()
        print(f"{tag} {which}: {info.iterations} steps (one rank {info1.iterations}), values {dv:.1e} anorm from one rank's, true "
              f"residual {res:.2f} tol anorm, orthogonality {orth:.1e}", file=sys.stderr)
        assert dv <= ec.VAL_RTOL, (tag, dv)
        assert abs(info.iterations - info1.iterations) <= m - (k + (m - k) // 2), (tag, info.iterations, info1.iterations)
        assert res <= 2.0 and orth <= 1e-12, (tag, res, orth)
        assert Xg.shape == (n, k) and info.residual_norms.shape == (k,), tag
        torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
