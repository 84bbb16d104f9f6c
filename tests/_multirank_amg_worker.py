"""Worker for tests/test_gpu_amg.py::test_amg_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the GPU.
The 32 x 32 five-point grid (tests/_amg_cases.py) on the uniform partition:
  * the rank-local part of a level's setup (``amg.aggregate_level``: weights, strength graph, independent set, join, numbering;
    it exchanges sizes only): each rank's aggregate ids, its root count and the coarse partition equal the blocked restatement
    (aggregates never cross a rank), for theta = 0 and 0.25, the weights within the one-rank tests' 1e-13;
  * a diagonal that is not positive in one rank's rows raises the same error on every rank, with the global row, and a good call
    passes afterwards;
  * ``hp.amg(A)`` itself is refused on every rank with NotImplementedError: the setup's products and transposes move values
    between ranks through RCCL, which ranks sharing a GPU do not have (tests/_multirank_lsqr_worker.py has the same limit for
    ``transpose(A).materialize()``), so the hierarchy and the solve across ranks are not offered in this version.
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
    from tests import _amg_cases as ac
    amg_mod = sys.modules[hp.amg.__module__]

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[amg rank {rank}/{nranks}]"
    Ah = ac.cases()["grid32x32"]
    n = Ah.shape[0]
    part = hp.uniform_partition(n, nranks)

    def local_matrix(values=Ah.data):
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(Ah.indptr[lo]), int(Ah.indptr[hi])
        return hp.HPCSparseMatrix_local(Ah.indptr[lo:hi + 1] - a, Ah.indices[a:b_], values[a:b_], n, backend,
                                        col_partition=np.asarray(part, dtype=np.int64))

    blocks = [int(v) for v in part]
    lo, hi = int(part[rank]), int(part[rank + 1])

    def check_aggregation(theta, what):
        agg, counts, _, rounds, _ = ac.aggregate(Ah, blocks, theta)
        lvl = amg_mod.aggregate_level(local_matrix(), theta=theta)
        assert np.array_equal(lvl.aggregates.cpu().numpy(), agg[lo:hi]), (tag, what)
        assert lvl.n_roots == int(counts[rank]), (tag, what)
        assert np.array_equal(lvl.coarse_partition, np.concatenate([[0], np.cumsum(counts)])), (tag, what)
        s_ref, w_ref, rho_ref = ac.weights(Ah)
        assert abs(lvl.rho - rho_ref) <= 1e-13 * rho_ref and abs(lvl.w - w_ref) <= 1e-13 * w_ref, (tag, what)
        assert np.all(np.abs(lvl.s.local_values() - s_ref[lo:hi]) <= 1e-13 * np.abs(s_ref).max()), (tag, what)
        assert 1 <= lvl.rounds <= rounds, (tag, what)               # a rank's own graph takes no more rounds than all blocks

    check_aggregation(0.0, "theta 0")
    check_aggregation(0.25, "theta 0.25")

    # -- a diagonal that is not positive in the rows of the last rank: every rank raises, with the global row
    bad_row = int(part[nranks - 1]) + 7
    bad = Ah.data.copy()
    bad[int(Ah.indptr[bad_row]) + int(np.flatnonzero(Ah.indices[Ah.indptr[bad_row]:Ah.indptr[bad_row + 1]] == bad_row)[0])] = -1.0
    try:
        amg_mod.aggregate_level(local_matrix(bad))
        raise AssertionError(tag + " no error")
    except ValueError as e:
        assert str(e) == f"amg: the diagonal of row {bad_row} is not positive (level of {n} rows)", (tag, str(e))
    check_aggregation(0.0, "after the error")

    # -- the hierarchy: refused on every rank
    try:
        hp.amg(local_matrix())
        raise AssertionError(tag + " no refusal")
    except NotImplementedError as e:
        assert str(e).startswith("amg: one rank only"), (tag, str(e))

    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
