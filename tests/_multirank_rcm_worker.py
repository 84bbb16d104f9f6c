"""Worker for tests/test_gpu_rcm.py::test_rcm_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the GPU.
``hp.rcm`` is rank-local: on uneven row partitions, one of them with an empty rank,
  * every rank's ``p`` equals the restatement (tests/_rcm_cases.py) on its owned block plus its row start, ``info`` included,
    for both ``symmetric`` settings;
  * ``hp.select(A, p, p)`` keeps A's partition and its rows are scipy's ``A[pg][:, pg]`` for the concatenated ``pg``;
    ``hp.bandwidth`` of both is numpy's, the same number on every rank;
  * a non-square matrix and unequal partitions raise ValueError on every rank.
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
    from tests import _rcm_cases as rc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[rcm rank {rank}/{nranks}]"
    for name, symmetric in (("grid33x31", True), ("delaunay2000", True), ("nonsymmetric", False), ("nonsymmetric", True)):
        C = rc.matrix(name)
        n = C.shape[0]
        parts = [np.array([0, 400, n] if nranks == 2 else [0, 400, 400, n], dtype=np.int64),       # 3 ranks: rank 1 holds no rows
                 np.array([0, 7, n] if nranks == 2 else [0, 7, 619, n], dtype=np.int64)]
        for part in parts:
            what = f"{tag} {name} symmetric={symmetric} partition {part.tolist()}"
            lo, hi = int(part[rank]), int(part[rank + 1])
            R = C[lo:hi]
            A = hp.HPCSparseMatrix_local(R.indptr, R.indices, R.data, n, backend, col_partition=part)
            assert np.array_equal(A.row_partition, part) and np.array_equal(A.col_partition, part), what
            p, info = hp.rcm(A, symmetric=symmetric)
            want, facts, _ = rc.expected(name, symmetric, lo, hi)
            got = p.cpu().numpy()
            assert p.dtype == torch.int64 and np.array_equal(got, want + lo), what
            for f in ("components", "levels", "bandwidth_before", "bandwidth_after"):
                assert getattr(info, f) == facts[f], (what, f, getattr(info, f), facts[f])
            assert A.structural_hash is None, what
            pg = np.concatenate([rc.expected(name, symmetric, int(part[r]), int(part[r + 1]))[0] + int(part[r]) for r in range(nranks)])
            assert rc.is_permutation(pg, n), what
            B = hp.select(A, p, p)
            assert np.array_equal(B.row_partition, part) and np.array_equal(B.col_partition, part), what
            E = sp.csr_matrix(C[pg][:, pg])[lo:hi]
            E.sort_indices()
            assert np.array_equal(B.rowptr, E.indptr) and np.array_equal(B.col_indices[B.colval], E.indices), what
            assert np.array_equal(B.nzval.cpu().numpy(), E.data), what
            assert hp.bandwidth(A) == rc.bandwidth_of_matrix(C), what
            assert hp.bandwidth(B) == rc.bandwidth_of_matrix(C[pg][:, pg]), what
    # -- errors: the same ValueError on every rank ---------------------------------------------------------------------------------
    C = rc.matrix("grid33x31")
    n = C.shape[0]
    part = np.array([0, 400, n] if nranks == 2 else [0, 400, 700, n], dtype=np.int64)
    lo, hi = int(part[rank]), int(part[rank + 1])
    R = C[lo:hi]
    A = hp.HPCSparseMatrix_local(R.indptr, R.indices, R.data, n, backend)          # the default column partition: uniform
    assert not np.array_equal(A.row_partition, A.col_partition), tag
    for call in (lambda: hp.rcm(A), lambda: hp.rcm(A, symmetric=False)):
        try:
            call()
            raise AssertionError(f"{tag}: unequal partitions did not raise")
        except ValueError as exc:
            assert str(exc) == "rcm: A's rows and columns must be partitioned alike", (tag, str(exc))
    R = C[lo:hi, :1000]
    N = hp.HPCSparseMatrix_local(R.indptr, R.indices, R.data, 1000, backend)
    try:
        hp.rcm(N)
        raise AssertionError(f"{tag}: a non-square matrix did not raise")
    except ValueError as exc:
        assert str(exc) == f"rcm: the matrix must be square, got {n} x 1000", (tag, str(exc))
    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
