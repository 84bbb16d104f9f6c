"""Worker for tests/test_gpu_multirank.py::test_rccl_plans_across_ranks: ONE process per rank (launch.spawn_ranks), one GPU
per rank.  The two exchanges whose halo plans are never attached to the peer windows, so they run over RCCL only: dense
A*x (every rank sends its slice of x to all others) and the value exchange of sparse A * sparse B.  Integer-valued inputs:
every product is exact in any summation order and must equal numpy's int64 product bit for bit.  Each product runs twice,
the second time on the cached plan and its ghost pointer; x sits on a partition whose last rank holds nothing.
Exit code 0 = all passed on this rank."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main():
    import scipy.sparse as sp
    import torch
    import torch.distributed as dist
    import hpcla_amd as hp

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    rng = np.random.default_rng(913)                   # same stream on every rank: identical global inputs
    for Ti in (np.int32, np.int64):
        backend = hp.backend_rocm_mpi(np.float64, Ti)
        tag = f"[rccl plans rank {rank}/{nranks} {np.dtype(Ti).name}]"
        # dense A * x
        m, n = 301, 517
        Ag = rng.integers(-5, 6, size=(m, n)).astype(np.float64)
        xg = rng.integers(-5, 6, size=n).astype(np.float64)
        xpart = np.array([0] + [(n * (r + 1)) // (nranks - 1) for r in range(nranks - 1)] + [n], dtype=np.int64)
        A = hp.HPCMatrix.from_global(Ag, backend)
        x = hp.HPCVector.from_global(xg, backend, partition=xpart)
        want = (Ag.astype(np.int64) @ xg.astype(np.int64)).astype(np.float64)
        lo, hi = int(A.row_partition[rank]), int(A.row_partition[rank + 1])
        for rep in range(2):
            y = A @ x
            assert np.array_equal(y.local_values(), want[lo:hi]), f"{tag} dense A*x differs (call {rep})"
        # sparse A * sparse B
        p, q = 2_003, 1_511
        S, T = (sp.random(r, c, density=0.004, format="csr", random_state=np.random.RandomState(int(rng.integers(1 << 30))))
                for r, c in ((4 * m, p), (p, q)))
        S.data = rng.integers(-9, 10, S.nnz).astype(np.float64)
        T.data = rng.integers(-9, 10, T.nnz).astype(np.float64)
        As = hp.HPCSparseMatrix_from_global(S, backend)
        Bs = hp.HPCSparseMatrix_from_global(T, backend)
        want = (S.astype(np.int64) @ T.astype(np.int64)).toarray().astype(np.float64)
        lo, hi = int(As.row_partition[rank]), int(As.row_partition[rank + 1])
        for rep in range(2):
            C = As @ Bs
            got = sp.csr_matrix((C.nzval.cpu().numpy(), C.col_indices[C.colval.astype(np.int64)], C.rowptr.astype(np.int64)),
                                shape=(hi - lo, q)).toarray()
            assert np.array_equal(got, want[lo:hi]), f"{tag} sparse A*B differs (call {rep})"
        hp.check_exchange_health(backend, always=True)
        hp.clear_dense_plan_cache()
        hp.clear_matrix_plan_cache()
        hp.clear_plan_cache()
        print(f"{tag} ok", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
