"""Worker for tests/test_gpu_lsqr.py::test_lsqr_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the GPU.
The tall and the wide 24 x 20 case (tests/_lsqr_cases.py; 960 x 480 and 480 x 960, so the local row and column lengths differ on
every rank), damp 0 and 0.3, ``check_every=8``.  The transposes are seeded into the matrices' cache from the host CSR (the
value exchange of ``transpose(A).materialize()`` needs RCCL, one GPU per rank; the SpMVs of both plans use the peer windows):
  * every rank reports the same ``LSQRInfo`` (the solve ends: no rank leaves the chunk loop alone);
  * iterations within +-2 of the restatement's, status equal, the heads of both histories within HIST_RTOL of it;
  * the gathered x is within 1e-6 of numpy.linalg.lstsq on the dense augmented system;
  * diag(1, 0, 0, ...) with b = (1, 1, 0, ...), one row per rank or more: one iteration, "least_squares", and the second
    residual norm stays 1.0 to 1e-15 -- the history pair is formed from global scalars and must not be summed over the ranks.
Exit code 0 = all passed on this rank."""
import math
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

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[lsqr rank {rank}/{nranks}]"

    def on_ranks(rowptr, colidx, vals, ncols, bg):
        m = len(bg)
        part = hp.uniform_partition(m, nranks)
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(rowptr[lo]), int(rowptr[hi])
        A = hp.HPCSparseMatrix_local(rowptr[lo:hi + 1] - a, colidx[a:b_], vals[a:b_], ncols, backend)
        # transpose(A).materialize() moves the values between ranks through RCCL, which ranks sharing one GPU do not have: this
        # rank's rows of the transpose come from the host CSR instead and are put where materialize() caches them
        rt, ct, vt = lc.transpose_csr(rowptr, colidx, vals, ncols)
        lo_t, hi_t = int(A.col_partition[rank]), int(A.col_partition[rank + 1])
        a, b_ = int(rt[lo_t]), int(rt[hi_t])
        At = hp.HPCSparseMatrix_local(rt[lo_t:hi_t + 1] - a, ct[a:b_], vt[a:b_], m, backend, col_partition=A.row_partition)
        assert np.array_equal(At.row_partition, A.col_partition) and np.array_equal(At.col_partition, A.row_partition)
        A.cached_transpose, At.cached_transpose = At, A
        return A, hp.HPCVector.from_global(bg, backend)

    def same_everywhere(info):
        mine = (info.converged, info.iterations, info.status, info.residual_norms, info.normal_residual_norms, info.anorm)
        every = [None] * nranks
        dist.all_gather_object(every, mine)
        assert all(e == mine for e in every), (tag, "ranks disagree", [e[:3] for e in every])

    for kind, make in lc.CASES.items():
        case = make(orc, *lc.RANK_SIZE)
        dense = lc.dense_of(*case[:4])
        A, b = on_ranks(*case)
        assert A.nrows_local != int(np.diff(A.col_partition)[rank]), (tag, "local lengths should differ")
        for damp in lc.DAMPS:
            _, its_ref, status_ref, hr, hn, _ = lc.lsqr(*case, damp=damp)
            x, info = hp.lsqr(A, b, damp=damp, check_every=8)
            same_everywhere(info)
            assert info.status == status_ref and info.converged, (tag, kind, damp, info.status, status_ref)
            assert abs(info.iterations - its_ref) <= 2, (tag, kind, damp, info.iterations, its_ref)
            assert len(info.residual_norms) == len(info.normal_residual_norms) == info.iterations + 1, (tag, kind, damp)
            head = max(abs(g - w) / w for got, want in ((info.residual_norms, hr), (info.normal_residual_norms, hn))
                       for g, w in zip(got[:lc.HEAD], want[:lc.HEAD]))
            xg = x.gather()
            Ab, bb = lc.augmented(dense, case[4], damp)
            x_ref = np.linalg.lstsq(Ab, bb, rcond=None)[0]
            err = np.linalg.norm(xg - x_ref) / np.linalg.norm(x_ref)
            print(f"{tag} {kind} damp {damp}: {info.status} at {info.iterations} (restatement {its_ref}), head deviation {head:.2e}, "
                  f"against lstsq {err:.2e}", file=sys.stderr)
            assert head <= lc.HIST_RTOL, (tag, kind, damp, head)
            assert err <= 1e-6, (tag, kind, damp, err)
        hp.clear_plan_cache()

    # a globally reduced scalar is not summed again across ranks
    k = nranks + 1
    d = np.zeros(k)
    d[0] = 1.0
    bg = np.zeros(k)
    bg[:2] = 1.0
    A, b = on_ranks(np.arange(k + 1, dtype=np.int64), np.arange(k, dtype=np.int64), d, k, bg)
    x, info = hp.lsqr(A, b)
    same_everywhere(info)
    assert (info.iterations, info.status) == (1, "least_squares"), (tag, info)
    assert abs(info.residual_norms[0] - math.sqrt(2.0)) <= 1e-15 and abs(info.residual_norms[1] - 1.0) <= 1e-15, (tag, info)
    assert info.normal_residual_norms[1] <= 1e-15, (tag, info)
    xg = x.gather()
    assert abs(xg[0] - 1.0) <= 1e-15 and not xg[1:].any(), (tag, xg)
    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
