"""Worker for tests/test_gpu_select.py::test_select_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share
the GPU.  ``hp.select``, ``hp.take`` and ``hp.put_`` through the host layer on uneven row partitions, one of them with an
empty rank:
  * every rank's slice (rowptr, colval, col_indices, value bits) and both partitions against the loop restatement
    (tests/_select_cases.py); each rank passes its own rows (permuted, with repeats) and its own piece of the column list;
  * the gathered ``select(...) @ x`` against the one-rank result (a serial backend on the same GPU), bit for bit;
  * ``take`` with off-rank indices, so that the halo plan carries values, against numpy; a case where no rank reads another's
    entries, where no halo plan may exist; ``put_`` against numpy;
  * the collective errors: a row another rank owns, a column listed by two ranks, a ``put_`` index another rank owns --
    raised on every rank.
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
    from tests import _select_cases as sc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    serial = hp.backend_rocm_serial(np.float64, np.int32)
    tag = f"[select rank {rank}/{nranks}]"
    m, n = sc.matrix("edge").shape
    parts = [sc.uneven_partition(m, nranks, 1),                                         # rank 1 holds no rows
             np.array([0, 11, m] if nranks == 2 else [0, 7, 19, m], dtype=np.int64)]
    all_cols = sc.index_list("edge", "cols_unsorted_subset")
    for pi, part in enumerate(parts):
        lo, hi = int(part[rank]), int(part[rank + 1])
        rng = np.random.default_rng(100 + pi)                                           # the same lists on every rank
        rows_by_rank = []
        for r in range(nranks):
            own = np.arange(part[r], part[r + 1], dtype=np.int64)
            rows_by_rank.append(rng.permutation(np.concatenate([own, own[:2]])) if len(own) else own)
        cuts = np.sort(rng.choice(len(all_cols) + 1, nranks - 1))
        if pi == 1:
            cuts[0] = 0                                                                 # rank 0 lists no column
        cols_by_rank = np.split(all_cols, cuts)
        for key in ("edge", "edge_finite"):
            C = sc.matrix(key)
            rp, cols, vals = C.rows(lo, hi)
            A = hp.HPCSparseMatrix_local(rp, cols, vals, n, backend)
            assert np.array_equal(A.row_partition, part), tag
            for what, rows_arg, cols_arg in (("lists", rows_by_rank, cols_by_rank), ("rows only", rows_by_rank, None),
                                             ("cols only", None, cols_by_rank), ("none", None, None)):
                what = f"{tag} part {pi} {key} {what}"
                e = sc.expected_on_rank(C, part, rank, rows_arg, cols_arg, col_partition=A.col_partition)
                B = hp.select(A, None if rows_arg is None else rows_arg[rank], None if cols_arg is None else cols_arg[rank])
                assert np.array_equal(B.row_partition, e["row_partition"]), what
                assert np.array_equal(B.col_partition, e["col_partition"]), what
                assert np.array_equal(B.rowptr, e["rowptr"]) and np.array_equal(B.colval, e["colval"]), what
                assert np.array_equal(B.col_indices, e["col_indices"]), what
                assert np.array_equal(sc.bits(B.nzval.cpu().numpy()), sc.bits(e["vals"])), what
                if key == "edge_finite":
                    A1 = hp.HPCSparseMatrix_local(C.indptr, C.indices, C.data, n, serial)
                    B1 = hp.select(A1, None if rows_arg is None else np.concatenate(rows_arg),
                                   None if cols_arg is None else np.concatenate(cols_arg))
                    assert B1.shape == B.shape, what
                    xg = 1.0 + np.cos(np.arange(B.shape[1], dtype=np.float64))
                    y = (B @ hp.HPCVector.from_global(xg, backend)).gather()
                    y1 = (B1 @ hp.HPCVector.from_global(xg, serial)).local_values()
                    assert np.array_equal(sc.bits(y), sc.bits(y1)), what + ": gathered product differs from the one-rank product"
        # a plan: new values on the same structure, on every rank
        C = sc.matrix("edge_finite")
        rp, cols, vals = C.rows(lo, hi)
        A = hp.HPCSparseMatrix_local(rp, cols, vals, n, backend)
        plan = hp.selection_plan(A, rows_by_rank[rank], cols_by_rank[rank])
        B2 = plan.extract(2 * A)
        e = sc.expected_on_rank(C, part, rank, rows_by_rank, cols_by_rank)
        assert np.array_equal(B2.nzval.cpu().numpy(), 2 * e["vals"]) and B2.structural_hash is plan.matrix.structural_hash, tag

        # -- vectors ---------------------------------------------------------------------------------------------------
        nv = 1000
        vpart = sc.uneven_partition(nv, nranks, 1) if pi == 0 else sc.uniform_partition(nv, nranks)
        vlo, vhi = int(vpart[rank]), int(vpart[rank + 1])
        vg = np.sin(np.arange(nv, dtype=np.float64))
        vg[3], vg[nv - 2] = -0.0, np.inf
        v = hp.HPCVector.from_global(vg, backend, partition=vpart)
        rng = np.random.default_rng(200 + pi)
        idx_by_rank = [rng.integers(0, nv, 300 + 17 * r).astype(np.int64) for r in range(nranks)]      # any index, repeats
        if pi == 1:
            idx_by_rank[nranks - 1] = np.empty(0, dtype=np.int64)                       # a rank that reads nothing
        want_part = np.concatenate([[0], np.cumsum([len(i) for i in idx_by_rank])])
        idx = idx_by_rank[rank]
        w = hp.take(v, idx)
        assert np.array_equal(w.partition, want_part), tag
        assert np.array_equal(sc.bits(w.local_values()), sc.bits(sc.take_of(vg, idx))), f"{tag} take part {pi}"
        ip = hp.index_plan(_dev(torch, idx), vpart, backend)
        foreign = np.unique(idx[(idx < vlo) | (idx >= vhi)])
        assert ip.has_halo and ip.n_ghost == len(foreign), (tag, ip.n_ghost, len(foreign))
        for scale in (1.0, -3.0):                                                       # the plan reuses its exchange
            got = ip.take(hp.HPCVector.from_global(scale * vg, backend, partition=vpart))
            assert np.array_equal(sc.bits(got.local_values()), sc.bits(scale * vg[idx])), f"{tag} plan take part {pi}"
        def repeated(i):
            u, c = np.unique(i, return_counts=True)
            return u[c > 1]

        offenders = [r for r in range(nranks)                                           # a foreign index, or a repeated one
                     if ((idx_by_rank[r] < vpart[r]) | (idx_by_rank[r] >= vpart[r + 1])).any() or len(repeated(idx_by_rank[r]))]
        off = idx[(idx < vlo) | (idx >= vhi)]
        for _ in range(2):                                                              # the collective verdict is kept
            try:
                ip.put_(v, w)
                raise AssertionError(f"{tag}: put_ with indices of other ranks did not raise")
            except ValueError as exc:
                if len(off):
                    assert str(exc) == (f"put_: {len(off)} of the indices are not owned by this rank; the first is "
                                        f"{int(off[0])}"), (tag, str(exc))
                elif len(repeated(idx)):                                                # all owned, but not distinct
                    assert str(exc) == (f"put_: index {int(repeated(idx)[0])} is listed more than once; a scatter with "
                                        "duplicates has no defined winner"), (tag, str(exc))
                else:
                    assert str(exc) == (f"put_: refused on rank(s) {offenders}; this rank's arguments were accepted"), (tag, str(exc))
        assert np.array_equal(sc.bits(v.local_values()), sc.bits(vg[vlo:vhi])), tag     # nothing was written
        ip.destroy()
        # nobody reads another rank's entries: no halo plan is built
        own = np.arange(vlo, vhi, dtype=np.int64)[::-1].copy()
        ip = hp.index_plan(own, vpart, backend)
        assert not ip.has_halo and ip.n_ghost == 0, tag
        assert np.array_equal(ip.take(v).partition, vpart), tag
        assert np.array_equal(sc.bits(ip.take(v).local_values()), sc.bits(vg[own])), tag
        src = hp.HPCVector.from_global(np.arange(nv, dtype=np.float64) + 0.5, backend, partition=vpart)
        u = v.copy()
        assert ip.put_(u, src) is u
        srcs = np.arange(nv, dtype=np.float64) + 0.5
        want = vg.copy()
        for r in range(nranks):                                                         # every rank reversed its own slice
            a, b = int(vpart[r]), int(vpart[r + 1])
            want = sc.put_into(want, np.arange(a, b)[::-1], srcs[a:b])
        assert np.array_equal(sc.bits(u.gather()), sc.bits(want)), f"{tag} put_ part {pi}"
        assert np.array_equal(sc.bits(v.gather()), sc.bits(vg)), tag

        # -- collective errors: raised on every rank -----------------------------------------------------------------------
        C = sc.matrix("edge_finite")
        other = next((r for r in range(nranks) if r != 0 and part[r + 1] > part[r]), None)
        if other is not None:                                                           # a second rank with rows exists
            bad_rows = np.array([int(part[other])], dtype=np.int64) if rank == 0 else rows_by_rank[rank]
            try:
                hp.select(A, bad_rows, None)
                raise AssertionError(f"{tag}: a row of another rank did not raise")
            except ValueError as exc:
                if rank == 0:
                    assert str(exc) == f"select: row {int(part[other])} is owned by rank {other}; repartition first", str(exc)
                else:
                    assert "refused on rank(s) [0]" in str(exc), str(exc)
        dup = [np.array([5, 9], dtype=np.int64) if r in (0, nranks - 1) else np.empty(0, dtype=np.int64) for r in range(nranks)]
        dup[0] = np.array([9, 5, 2], dtype=np.int64)
        try:
            hp.select(A, None, dup[rank])
            raise AssertionError(f"{tag}: a column listed by two ranks did not raise")
        except ValueError as exc:
            assert "select: column 5 is listed more than once" in str(exc), str(exc)
        try:
            hp.select(A, None, np.array([n], dtype=np.int64) if rank == nranks - 1 else dup[rank])
            raise AssertionError(f"{tag}: a column outside the matrix did not raise")
        except IndexError as exc:
            assert rank == nranks - 1 and "lie outside" in str(exc), str(exc)
        except ValueError as exc:
            assert rank != nranks - 1 and f"refused on rank(s) [{nranks - 1}]" in str(exc), str(exc)
    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


if __name__ == "__main__":
    main()
