"""Worker for tests/test_gpu_assemble.py::test_assembly_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks
share the GPU.  Element-partitioned P1 triplets (tests/_assemble_cases.py), so the rows on the seam between two ranks' element
shares receive from a neighbour; uneven row partitions, one of them with a rank that holds no rows:
  * each rank's slice (rowptr, global columns, value bits) against the restatement applied to that rank's value list in the
    stated order: its own triplets in input order, then the received ones in ascending sender rank;
  * against the one-rank result (a serial backend on the same GPU): bit for bit on the dyadic P1 values, within
    (L - 1) eps sum|v| per entry for a random coefficient;
  * traffic shapes: a rank that contributes nothing, a rank that receives from all others, and triplets that all stay at
    home (n_routed == 0 everywhere: no halo plan);
  * assemble_ twice in a row with different values (a ghost buffer read too early would show), the vector form, and an
    out-of-range index on one rank that every rank must raise on.
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
    from tests import _assemble_cases as ac

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    serial = hp.backend_rocm_serial(np.float64, np.int32)
    tag = f"[assemble rank {rank}/{nranks}]"
    nx, ny = 33, 31
    N = nx * ny
    ne = 2 * (nx - 1) * (ny - 1)
    eps = np.finfo(np.float64).eps
    coeff = 1.0 + 0.5 * np.sin(np.arange(ne, dtype=np.float64))
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))

    def triplets(ncontrib, k):
        """Every rank's triplets: the first ``ncontrib`` ranks share the elements, the others contribute nothing."""
        return [ac.element_partition_triplets(nx, ny, ncontrib, r, k) if r < ncontrib else empty for r in range(nranks)]

    def check(plan, A, trips, part, what):
        lo, hi = int(part[rank]), int(part[rank + 1])
        r, c, v = ac.rank_value_list(trips, part, rank)
        rowptr, cols, vals = ac.assemble_ref(r, c, v, (N, N), lo, hi)
        assert np.array_equal(A.row_partition, part), what
        assert np.array_equal(A.rowptr, rowptr), what
        assert np.array_equal(A.col_indices[A.colval.astype(np.int64)] if len(vals) else np.zeros(0, dtype=np.int64), cols), what
        assert np.array_equal(ac.bits(A.nzval.cpu().numpy()), ac.bits(vals)), what + ": bits differ from the rank's restatement"
        own = trips[rank][0]
        assert plan.n_routed == int(((own < lo) | (own >= hi)).sum()) and plan.n_received == len(r) - (len(own) - plan.n_routed), what
        return rowptr, cols, vals

    parts = [np.array([0] + [N] * nranks, dtype=np.int64),                 # rank 0 holds every row and receives from all others
             np.array([0, 500, N] if nranks == 2 else [0, 300, 700, N], dtype=np.int64)]
    for pi, part in enumerate(parts):
        lo, hi = int(part[rank]), int(part[rank + 1])
        for ncontrib in (nranks, nranks - 1):                                # everyone contributes; the last rank contributes nothing
            what = f"{tag} part {pi} contributors {ncontrib}"
            dyadic, rnd = triplets(ncontrib, None), triplets(ncontrib, coeff)
            mine = dyadic[rank]
            plan = hp.assembly_plan(mine[0], mine[1], (N, N), backend, row_partition=part)
            A = plan.assemble(mine[2])
            check(plan, A, dyadic, part, what)
            # the one-rank result of the same triplets, rank after rank
            allr, allc = np.concatenate([t[0] for t in dyadic]), np.concatenate([t[1] for t in dyadic])
            plan1 = hp.assembly_plan(allr, allc, (N, N), serial)
            A1 = plan1.assemble(np.concatenate([t[2] for t in dyadic]))
            p0, p1 = int(A1.rowptr[lo]), int(A1.rowptr[hi])
            assert np.array_equal(A.rowptr, A1.rowptr[lo:hi + 1] - p0), what
            one = A1.nzval.cpu().numpy()[p0:p1]
            assert np.array_equal(ac.bits(A.nzval.cpu().numpy() + 0.0), ac.bits(one + 0.0)), what + ": dyadic values differ across partitions"
            # a random coefficient, in place, twice in a row: the second call's values must be the ones that stay
            v_rnd = rnd[rank][2]
            plan.assemble_(A, v_rnd * 3.0)
            plan.assemble_(A, v_rnd)
            rowptr, cols, vals = check(plan, A, rnd, part, what + " in place")
            one = plan1.assemble(np.concatenate([t[2] for t in rnd])).nzval.cpu().numpy()[p0:p1]
            L = plan1.assemble(np.ones(len(allr))).nzval.cpu().numpy()[p0:p1]
            S = plan1.assemble(np.abs(np.concatenate([t[2] for t in rnd]))).nzval.cpu().numpy()[p0:p1]
            assert np.all(np.abs(vals - one) <= (L - 1) * eps * S), what + ": beyond (L - 1) eps sum|v| of the one-rank result"
            B = plan.assemble(mine[2])                                       # and the first values again, in a new matrix
            assert B.rowptr_target is A.rowptr_target and B._ensure_hash() is A._ensure_hash(), what
            check(plan, B, dyadic, part, what + " again")
            if pi == 0:
                others = sum(len(t[0]) for t in dyadic) - len(mine[0])
                assert (plan.n_routed, plan.n_received) == ((0, others) if rank == 0 else (len(mine[0]), 0)), what
            # the vector form over the same rows
            vp = hp.assembly_plan(mine[0], None, (N,), backend, row_partition=part)
            b = vp.assemble(v_rnd)
            r, c, v = ac.rank_value_list(rnd, part, rank)
            assert np.array_equal(ac.bits(b.local_values()), ac.bits(ac.assemble_vector_ref(r, v, N, lo, hi))), what + " vector"
            assert np.array_equal(b.partition, part), what
            plan.destroy(); vp.destroy()
        # every triplet stays at home: no halo plan, the launch of one rank
        allt = ac.p1_triplets(nx, ny, coeff)
        keep = (allt[0] >= lo) & (allt[0] < hi)
        home = [tuple(a[(allt[0] >= part[q]) & (allt[0] < part[q + 1])] for a in allt) for q in range(nranks)]
        plan = hp.assembly_plan(allt[0][keep], allt[1][keep], (N, N), backend, row_partition=part)
        assert plan.n_routed == 0 and plan.n_received == 0 and not plan._halo, tag
        check(plan, plan.assemble(allt[2][keep]), home, part, f"{tag} part {pi} at home")
    # an index outside the matrix on one rank: every rank raises
    bad = np.array([0, N if rank == 0 else 1], dtype=np.int64)
    try:
        hp.assembly_plan(bad, bad, (N, N), backend)
        raise AssertionError(f"{tag}: an out-of-range index on rank 0 was accepted")
    except IndexError as exc:
        assert rank == 0 and "1 of the indices" in str(exc), (tag, exc)
    except ValueError as exc:
        assert rank != 0 and "refused on rank(s) [0]" in str(exc), (tag, exc)
    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
