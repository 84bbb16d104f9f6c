"""Worker for tests/test_gpu_svds.py::test_svds_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the GPU.
The tall 24 x 20 case (tests/_svds_cases.py; 960 x 480, so the local row and column lengths differ on every rank), ``k = 4``,
``ncv = 20`` -- the column counts pass 8 and 16, so the all-reduces of the Gram-Schmidt sums are multi-slice.  The transpose is
seeded into the matrix's cache from the host CSR (the value exchange of ``transpose(A).materialize()`` needs RCCL, one GPU per
rank; the SpMVs of both plans use the peer windows):
  * every rank reports the same ``s`` bits and the same ``info`` (only rank 0 decides: no rank leaves the loop alone);
  * ``s`` is within VAL_RTOL * anorm of numpy.linalg.svd of the dense matrix, the step count within one cycle of the one-rank
    restatement's;
  * the gathered U and V meet the true-residual bound 2 tol anorm, A v - s u <= 1e-12 anorm, and are orthonormal to 1e-12.
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
    from tests import _lsqr_cases as lc
    from tests import _pcg_cases as pc
    from tests import _svds_cases as sc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[svds rank {rank}/{nranks}]"

    name, k, m = sc.RANK_CASE
    rowptr, colidx, vals, ncols = sc.matrix(orc, name)
    nrows = len(rowptr) - 1
    part = hp.uniform_partition(nrows, nranks)
    lo, hi = int(part[rank]), int(part[rank + 1])
    a, b_ = int(rowptr[lo]), int(rowptr[hi])
    A = hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], ncols, backend)
    rt, ct, vt = lc.transpose_csr(rowptr, colidx, vals, ncols)
    lo_t, hi_t = int(A.col_partition[rank]), int(A.col_partition[rank + 1])
    a, b_ = int(rt[lo_t]), int(rt[hi_t])
    At = hp.HPCSparseMatrix_local(rt[lo_t:hi_t + 1] - a, ct[a:b_], vt[a:b_], nrows, backend, col_partition=A.row_partition)
    assert np.array_equal(At.row_partition, A.col_partition) and np.array_equal(At.col_partition, A.row_partition)
    A.cached_transpose, At.cached_transpose = At, A
    assert A.nrows_local != int(np.diff(A.col_partition)[rank]), (tag, "local lengths should differ")

    ref = sc.svds(rowptr, colidx, vals, ncols, k=k, ncv=m)[3]
    U, s, V, info = hp.svds(A, k=k, ncv=m, tol=sc.TOL)
    assert info.converged and info.status == "converged", (tag, info.status)
    mine = (pc.bits(s).tolist(), info.converged, info.status, info.iterations, info.restarts,
            pc.bits(info.residual_norms).tolist(), info.history, info.anorm)
    every = [None] * nranks
    dist.all_gather_object(every, mine)
    assert all(e == mine for e in every), (tag, "ranks disagree", [e[1:5] for e in every])
    Ug, Vg = U.gather(), V.gather()
    assert Ug.shape == (nrows, k) and Vg.shape == (ncols, k) and info.residual_norms.shape == (k,), tag
    f = sc.figures(rowptr, colidx, vals, ncols, Ug, s, Vg, info, sc.dense_singular_values(rowptr, colidx, vals, ncols))
    print(f"{tag}: {info.iterations} steps (restatement {ref['iterations']}), value error {f['err']:.1e} anorm, true residual "
          f"{f['res']:.2f} tol anorm, A v - s u {f['left']:.1e} anorm, orthogonality {f['orth']:.1e}", file=sys.stderr)
    assert f["err"] <= sc.VAL_RTOL, (tag, f)
    assert abs(info.iterations - ref["iterations"]) <= m - (k + (m - k) // 2), (tag, info.iterations, ref["iterations"])
    assert f["res"] <= 2.0 and f["left"] <= 1e-12 and f["orth"] <= 1e-12 and f["est"] <= 1e-12 and f["sign"] > 0, (tag, f)
    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
