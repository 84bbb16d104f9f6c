"""Worker for tests/test_gpu_bicgstab.py::test_bicgstab_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share
the GPU.  The 24 x 20 convection-diffusion case (tests/_bicgstab_cases.py), Jacobi, ``check_every=8``:
  * every rank reports the same ``iterations`` and ``status`` (the solve ends: no rank leaves the chunk loop alone);
  * the head of the history is within HIST_RTOL of the one-rank run (a serial backend on the same GPU), the count within +-2;
  * the gathered x meets the stop rule's true-residual bound, and ``check_every=3`` gives the same bits as 8;
  * half-step stops: the 16 x 16 case with ``rtol = 0.7`` (gate S at iteration 8 with ||s|| > 0) reports the one-rank run's
    history within HALF_HIST_RTOL and a last entry within the stop rule -- the already global sum of squares must not be
    summed over the ranks once more; the diagonal case under Jacobi stops at iteration 1 within the stop rule.
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
    from tests import _pcg_cases as pc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    serial = hp.backend_rocm_serial(np.float64, np.int32)
    tag = f"[bicgstab rank {rank}/{nranks}]"
    rowptr, colidx, vals, bg = bc.convection_diffusion(orc, 24, 20)
    n = len(bg)
    part = hp.uniform_partition(n, nranks)
    lo, hi = int(part[rank]), int(part[rank + 1])
    a, b_ = int(rowptr[lo]), int(rowptr[hi])
    A = hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], n, backend)
    b = hp.HPCVector.from_global(bg, backend)
    A1 = hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, serial)
    b1 = hp.HPCVector.from_global(bg, serial)

    x1, info1 = hp.bicgstab(A1, b1, M="jacobi", rtol=1e-8, check_every=8)
    x, info = hp.bicgstab(A, b, M="jacobi", rtol=1e-8, check_every=8)
    assert info1.converged and info.converged and info.status == "converged", (tag, info.status)
    mine = torch.tensor([info.iterations, {"converged": 1, "maxiter": 0, "breakdown": 2}[info.status]], dtype=torch.int64)
    every = [torch.empty_like(mine) for _ in range(nranks)]
    dist.all_gather(every, mine)
    assert all(torch.equal(e, mine) for e in every), (tag, every)
    head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:bc.HEAD], info1.residual_norms[:bc.HEAD]))
    print(f"{tag} iterations {info.iterations} (one rank {info1.iterations}), head deviation {head:.2e}", file=sys.stderr)
    assert head <= bc.HIST_RTOL, (tag, head)
    assert abs(info.iterations - info1.iterations) <= 2, (tag, info.iterations, info1.iterations)
    xg = x.gather()
    true = np.linalg.norm(bg - pc.matvec(rowptr, colidx, vals, xg)) / np.linalg.norm(bg)
    assert true <= 2e-8, (tag, true)
    x3, info3 = hp.bicgstab(A, b, M="jacobi", rtol=1e-8, check_every=3)
    assert info3 == info and np.array_equal(pc.bits(x3.gather()), pc.bits(xg)), tag + " chunk"

    def on_ranks(rowptr, colidx, vals, bg):
        n = len(bg)
        part = hp.uniform_partition(n, nranks)
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[lo]), int(rowptr[hi])
        return (hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], n, backend),
                hp.HPCVector.from_global(bg, backend),
                hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, serial), hp.HPCVector.from_global(bg, serial))

    hp.clear_plan_cache()
    for label, case, rtol, its_want in (("half step", bc.convection_diffusion(orc, *bc.HALF_SIZE), bc.HALF_RTOL, bc.HALF_ITERATIONS),
                                        ("diagonal", pc.diagonal_case(orc), 1e-8, 1)):
        Ah, bh, Ah1, bh1 = on_ranks(*case)
        bnorm = float(np.linalg.norm(case[3]))
        _, i1 = hp.bicgstab(Ah1, bh1, M="jacobi", rtol=rtol)
        _, iN = hp.bicgstab(Ah, bh, M="jacobi", rtol=rtol)
        assert (i1.iterations, i1.status) == (its_want, "converged") == (iN.iterations, iN.status), (tag, label, i1, iN)
        assert len(iN.residual_norms) == len(i1.residual_norms) == its_want + 1, (tag, label)
        last = iN.residual_norms[-1]
        print(f"{tag} {label}: last entry / |b| = {last / bnorm:.3e} (one rank {i1.residual_norms[-1] / bnorm:.3e})", file=sys.stderr)
        assert last <= rtol * bnorm, (tag, label, last, rtol * bnorm)
        if label == "half step":                                 # the diagonal case's s is rounding noise: only the bound holds
            dev = max(abs(g - w) / w for g, w in zip(iN.residual_norms, i1.residual_norms))
            assert last > 0.0 and dev <= bc.HALF_HIST_RTOL, (tag, label, dev)
        else:
            assert abs(iN.residual_norms[0] - i1.residual_norms[0]) <= bc.HIST_RTOL * i1.residual_norms[0], (tag, label)
        hp.clear_plan_cache()
    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
