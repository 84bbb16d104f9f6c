"""Worker for tests/test_gpu_lobpcg_gen.py::test_lobpcg_gen_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks
share the GPU.  The 2-D finite-element pencil on the 16 x 16 grid (tests/_lobpcg_gen_cases.py), ``k = 4``, ``"SA"``, with the
consistent mass matrix as a sparse ``B`` and the lumped one as an HPCVector of weights, on the uniform row partition and on one
whose last rank holds no rows (that rank still takes part in every all-reduce and exchange):
  * ``vals``, ``residual_norms``, ``residual_scales``, ``history``, ``anorm``, ``iterations`` and ``status`` are bit-identical on
    every rank (only rank 0 decides, and its theta and C are the ones every rank combines with);
  * ``vals`` is within 1e-12 anorm of the one-rank run (a serial backend on the same GPU);
  * the gathered X meets the bounds of the one-rank tests (eigenvalues, true residuals, B-orthonormality, all against dense
    numpy), and the count stays under the cap.
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
    from tests import _lobpcg_cases as lc
    from tests import _lobpcg_gen_cases as gc
    from tests import _pcg_cases as pc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    serial = hp.backend_rocm_serial(np.float64, np.int32)
    tag = f"[lobpcg_gen rank {rank}/{nranks}]"

    name, k, which = gc.RANK_CASE
    K, M = gc.pencils()[name]
    n = K.shape[0]
    weights = gc.lumped(M)

    def rows_of(dense, be, part=None):
        rowptr, colidx, vals, _ = lc.csr_of(dense)
        if part is None:
            return hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, be)
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[lo]), int(rowptr[hi])
        return hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], n, be, col_partition=part)

    A1 = rows_of(K, serial)
    one_rank = {"sparse": hp.lobpcg(A1, k=k, which=which, tol=gc.TOL, B=rows_of(M, serial)),
                "vector": hp.lobpcg(A1, k=k, which=which, tol=gc.TOL, B=hp.HPCVector.from_global(weights, serial))}
    dense_b = {"sparse": M, "vector": np.diag(weights)}
    uniform = hp.uniform_partition(n, nranks)
    empty_last = np.concatenate([hp.uniform_partition(n, nranks - 1), [n]]).astype(np.int64)      # the last rank holds no rows
    codes = {"converged": 1, "maxiter": 3, "breakdown": 2}
    for label, part in (("uniform", uniform), ("empty last rank", empty_last)):
        A = rows_of(K, backend, part)
        assert np.array_equal(A.row_partition, part), (tag, A.row_partition)
        for kind in ("sparse", "vector"):
            B = rows_of(M, backend, part) if kind == "sparse" else hp.HPCVector.from_global(weights, backend, partition=part)
            got1, _, info1 = one_rank[kind]
            got, X, info = hp.lobpcg(A, k=k, which=which, tol=gc.TOL, B=B)
            assert info1.converged and info.converged and info.status == "converged", (tag, info.status)
            mine = torch.from_numpy(np.concatenate([got, info.residual_norms, info.residual_scales,
                                                    [info.anorm, info.iterations, codes[info.status]], info.history]))
            size = torch.tensor([mine.numel()])
            sizes = [torch.empty_like(size) for _ in range(nranks)]
            dist.all_gather(sizes, size)
            assert all(int(s) == mine.numel() for s in sizes), (tag, sizes)
            every = [torch.empty_like(mine) for _ in range(nranks)]
            dist.all_gather(every, mine)
            assert all(torch.equal(e.view(torch.int64), mine.view(torch.int64)) for e in every), (tag, label, kind)
            dv = np.abs(got - got1).max() / info1.anorm
            Xg = X.gather()
            Bd = dense_b[kind]
            want, bmin = gc.reference(K, Bd, k, which)
            err, res, orth = gc.figures(K, Bd, want, bmin, got, Xg)
            print(f"{tag} {label} {kind}: {info.iterations} iterations (one rank {info1.iterations}), values {dv:.1e} anorm from one "
                  f"rank's, eigenvalue error {err:.1e} of its bound, true residual {res:.2f} tol scale, B-orthonormality {orth:.1e}",
                  file=sys.stderr)
            assert dv <= 1e-12, (tag, dv)
            assert err <= 1.0 and res <= pc.TRUE_RES_FACTOR and orth <= lc.ORTH_TOL, (tag, err, res, orth)
            assert np.all(info.residual_norms <= gc.TOL * info.residual_scales), tag
            assert info.iterations <= 1.5 * info1.iterations + 5, (tag, info.iterations, info1.iterations)
            assert Xg.shape == (n, k) and X.local_values().shape == (int(part[rank + 1]) - int(part[rank]), k), tag
            torch.cuda.synchronize()
        hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
