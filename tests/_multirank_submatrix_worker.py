"""Worker for tests/test_gpu_submatrix.py::test_submatrix_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks
share the GPU.  ``A[r, c]``, ``A[:, k]`` and ``v[a:b]`` through the host layer on uneven row partitions, one of them with an
empty rank, with ranges that put a rank wholly inside, wholly outside and partly inside:
  * every rank's slice (rowptr, colval, col_indices, value bits) and both partitions against the numpy restatement
    (tests/_submatrix_cases.py), the empty-range forms included;
  * the gathered ``A[r, c] @ x`` against the one-rank result (a serial backend on the same GPU), bit for bit.
Indexing itself communicates nothing; the product's exchange goes through the ranks' peer windows.
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
    from tests import _submatrix_cases as sc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    serial = hp.backend_rocm_serial(np.float64, np.int32)
    tag = f"[submatrix rank {rank}/{nranks}]"
    n = sc.NR
    parts = [sc.uneven_partition(n, nranks, 1),                                         # rank 1 holds no rows
             np.array([0, 1100, n] if nranks == 2 else [0, 700, 1900, n], dtype=np.int64)]
    ranges = [(0, n, 0, sc.NC), (1200, 2500, 300, 4100), (0, 2000, sc.GAP_LO - 10, sc.GAP_HI + 7), (650, 750, 0, sc.NC),
              (1100, 1900, 17, 4890), (40, 41, 5, 4000), (500, 500, 10, 900), (10, 2900, 500, 500)]
    inside = outside = partly = 0
    for pi, part in enumerate(parts):
        lo, hi = int(part[rank]), int(part[rank + 1])
        for key in ("rand", "rand_finite"):
            C = sc.matrix(key)
            rp, cols, vals = C.rows(lo, hi)
            A = hp.HPCSparseMatrix_local(rp, cols, vals, sc.NC, backend)
            assert np.array_equal(A.row_partition, part), tag
            A1 = hp.HPCSparseMatrix_local(C.indptr, C.indices, C.data, sc.NC, serial) if key == "rand_finite" else None
            for r0, r1, c0, c1 in ranges:
                what = f"{tag} part {pi} {key} [{r0}:{r1}, {c0}:{c1}]"
                e = sc.expected_on_rank(C, part, rank, r0, r1, c0, c1)
                B = A[r0:r1, c0:c1]
                assert np.array_equal(B.row_partition, e["row_partition"]), what
                assert np.array_equal(B.col_partition, e["col_partition"]), what
                assert np.array_equal(B.rowptr, e["rowptr"]) and np.array_equal(B.colval, e["colval"]), what
                assert np.array_equal(B.col_indices, e["col_indices"]), what
                assert np.array_equal(sc.bits(B.nzval.cpu().numpy()), sc.bits(e["vals"])), what
                if r0 < r1 and c0 < c1 and hi > lo:
                    inside += r0 <= lo and hi <= r1
                    outside += hi <= r0 or r1 <= lo
                    partly += (r0 > lo or r1 < hi) and max(lo, r0) < min(hi, r1)
                if A1 is not None and r0 < r1 and c0 < c1:
                    xg = 1.0 + np.cos(np.arange(c1 - c0, dtype=np.float64))
                    y = (B @ hp.HPCVector.from_global(xg, backend)).gather()
                    y1 = (A1[r0:r1, c0:c1] @ hp.HPCVector.from_global(xg, serial)).local_values()
                    assert np.array_equal(sc.bits(y), sc.bits(y1)), what + ": gathered product differs from the one-rank product"
            for k in (sc.NEGZERO_COL, sc.GAP_LO + 3, 0, sc.NC - 1):
                v = A[:, k]
                assert np.array_equal(v.partition, part), tag
                assert np.array_equal(sc.bits(v.local_values()), sc.bits(sc.column_of(C, lo, hi, k))), f"{tag} column {k}"
        vg = np.sin(np.arange(n, dtype=np.float64))
        v = hp.HPCVector.from_global(vg, backend, partition=part)
        for a, b in ((0, n), (1200, 2500), (700, 700), (1099, 1101)):
            w = v[a:b]
            assert np.array_equal(w.partition, hp.subpartition(part, a, b)), tag
            assert np.array_equal(w.local_values(), vg[max(lo, a):max(min(hi, b), max(lo, a))]), tag
            if b > a:
                assert np.array_equal(w.gather(), vg[a:b]), tag
    assert inside and outside and partly, (tag, inside, outside, partly)      # over the partitions, every rank saw all three
    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
