"""Worker for tests/test_gpu_dense_sparse.py: ONE process per rank (launch.spawn_ranks), one GPU per rank (the reverse
exchange and copy(transpose(X)) go through RCCL).  transpose(X) * A and X * A through the host layer:
  * A's row partition with an empty rank; m not divisible by the rank count;
  * integer inputs: every slice bit-equal to the 1-rank product (= numpy's int64 product);
  * random inputs: within 1e-12 |X|^T |A| of the exact product; the gathered result bit-identical on every rank and on a
    second call;
  * result partitions: transpose(X) * A rows = X.col_partition, X * A rows = X.row_partition, columns =
    uniform_partition(n, nranks); transpose(X).materialize() rows = X.col_partition, columns = X.row_partition.
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
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[dense*sparse rank {rank}/{nranks}]"
    rng = np.random.default_rng(4242)                  # same stream on every rank: identical global inputs
    p, n = 20_011, 15_013
    # the last rank holds no rows of A; the others split the rest unevenly
    pa = np.array([0] + [(p * (r + 1)) // (nranks - 1) - 13 * r for r in range(nranks - 2)] + [p, p], dtype=np.int64)
    for m in (16, 7, 1):
        for kind in ("int", "rand"):
            S = sp.random(p, n, density=0.0006, format="csr", random_state=np.random.RandomState(int(rng.integers(1 << 30))))
            if kind == "int":
                S.data = rng.integers(-9, 10, S.nnz).astype(np.float64)
                Xg = rng.integers(-8, 9, size=(p, m)).astype(np.float64)
                Zg = rng.integers(-8, 9, size=(m, p)).astype(np.float64)
            else:
                S.data = rng.uniform(-1, 1, S.nnz)
                Xg, Zg = rng.uniform(-1, 1, (p, m)), rng.uniform(-1, 1, (m, p))
            A = hp.HPCSparseMatrix_from_global(S, backend, row_partition=pa)
            X = hp.HPCMatrix.from_global(Xg, backend, row_partition=pa)
            Z = hp.HPCMatrix.from_global(Zg, backend)
            C = hp.transpose(X) @ A
            D = Z @ A
            np.testing.assert_array_equal(C.row_partition, X.col_partition)
            np.testing.assert_array_equal(D.row_partition, Z.row_partition)
            for R in (C, D):
                np.testing.assert_array_equal(R.col_partition, hp.uniform_partition(n, nranks))
            Zt = hp.transpose(Z).materialize()
            np.testing.assert_array_equal(Zt.row_partition, Z.col_partition)
            np.testing.assert_array_equal(Zt.col_partition, Z.row_partition)
            assert np.array_equal(Zt.gather(), Zg.T), tag
            Cg, Dg = C.gather(), D.gather()
            Ad = S.toarray()
            if kind == "int":
                wc = (Xg.T.astype(np.int64) @ Ad.astype(np.int64)).astype(np.float64)
                wd = (Zg.astype(np.int64) @ Ad.astype(np.int64)).astype(np.float64)
                assert np.array_equal(Cg, wc), f"{tag} m={m}: transpose(X)*A"
                assert np.array_equal(Dg, wd), f"{tag} m={m}: X*A"
                lo, hi = int(C.row_partition[rank]), int(C.row_partition[rank + 1])
                assert np.array_equal(C.local_values(), wc[lo:hi]), tag
            else:
                bc = 1e-12 * (np.abs(Xg).T @ np.abs(Ad))
                bd = 1e-12 * (np.abs(Zg) @ np.abs(Ad))
                assert np.all(np.abs(Cg - Xg.T @ Ad) <= bc), f"{tag} m={m}: bound"
                assert np.all(np.abs(Dg - Zg @ Ad) <= bd), f"{tag} m={m}: bound"
                assert np.array_equal((hp.transpose(X) @ A).gather(), Cg), f"{tag} m={m}: second call"
                # identical on every rank
                for got in (Cg, Dg):
                    t = torch.from_numpy(np.ascontiguousarray(got))
                    outs = [torch.empty_like(t) for _ in range(nranks)]
                    dist.all_gather(outs, t)
                    assert all(torch.equal(o, t) for o in outs), f"{tag} m={m}: ranks disagree"
    hp.clear_spmm_cache()
    hp.clear_dense_plan_cache()
    hp.clear_plan_cache()
    dist.barrier()
    dist.destroy_process_group()
    print(f"{tag}: OK")


if __name__ == "__main__":
    main()
