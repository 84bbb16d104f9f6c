"""Worker for tests/test_gpu_gmres.py::test_gmres_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the
GPU.  Two convection-diffusion cases (tests/_gmres_cases.py) under Jacobi, ``check_every=8``:
  * 16 x 16 at ``restart = 30``: c passes 8, 16 and 24, so the all-reduces of the Gram-Schmidt sums are multi-slice;
  * 24 x 20 at ``restart = 8``: restarts inside the chunks, and a finish call with an open cycle.
For each:
  * every rank reports the same ``iterations`` and ``status`` (the solve ends: no rank leaves the chunk loop alone);
  * the head of the history is within HIST_RTOL of the one-rank run (a serial backend on the same GPU), the count within +-2;
  * the gathered x meets the stop rule's true-residual bound, and ``check_every=3`` gives the same bits as 8.
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
    from tests import _gmres_cases as gc
    from tests import _pcg_cases as pc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    serial = hp.backend_rocm_serial(np.float64, np.int32)
    tag = f"[gmres rank {rank}/{nranks}]"

    for (nx, ny), m in (((16, 16), 30), ((24, 20), 8)):
        rowptr, colidx, vals, bg = bc.convection_diffusion(orc, nx, ny)
        n = len(bg)
        part = hp.uniform_partition(n, nranks)
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[lo]), int(rowptr[hi])
        A = hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], n, backend)
        b = hp.HPCVector.from_global(bg, backend)
        A1 = hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, serial)
        b1 = hp.HPCVector.from_global(bg, serial)

        x1, info1 = hp.gmres(A1, b1, M="jacobi", rtol=1e-8, restart=m, check_every=8)
        x, info = hp.gmres(A, b, M="jacobi", rtol=1e-8, restart=m, check_every=8)
        assert info1.converged and info.converged and info.status == "converged", (tag, info.status)
        mine = torch.tensor([info.iterations, {"converged": 1, "maxiter": 0, "breakdown": 2}[info.status]], dtype=torch.int64)
        every = [torch.empty_like(mine) for _ in range(nranks)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, mine) for e in every), (tag, every)
        assert len(info.residual_norms) == info.iterations + 1, tag
        head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:gc.HEAD], info1.residual_norms[:gc.HEAD]))
        print(f"{tag} {nx}x{ny} restart {m}: iterations {info.iterations} (one rank {info1.iterations}), head deviation {head:.2e}",
              file=sys.stderr)
        assert head <= gc.HIST_RTOL, (tag, head)
        assert abs(info.iterations - info1.iterations) <= 2, (tag, info.iterations, info1.iterations)
        xg = x.gather()
        true = np.linalg.norm(bg - pc.matvec(rowptr, colidx, vals, xg)) / np.linalg.norm(bg)
        assert true <= 2e-8, (tag, true)
        x3, info3 = hp.gmres(A, b, M="jacobi", rtol=1e-8, restart=m, check_every=3)
        assert info3 == info and np.array_equal(pc.bits(x3.gather()), pc.bits(xg)), tag + " chunk"
        torch.cuda.synchronize()
        hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
