"""COO assembly on the device with a reusable structure: ``hp.assembly_plan``, ``hp.sparse_from_coo`` -- Julia's
``sparse(I, J, V, m, n)`` (the idiom the reference's users build operators with, followed by
``HPCSparseMatrix(A, backend)``, src/sparse.jl:398-413) for a loop that produces new values on the same ``(I, J)`` at every
step.

::

    plan = hp.assembly_plan(rows, cols, (m, n), backend)      # once per (rows, cols): sort, structure, hash
    A = plan.assemble(vals)                                   # every step: one kernel, no host work, no upload of structure
    plan.assemble_(A, vals2)                                  # or rewrite A.nzval in place
    b = hp.assembly_plan(idx, None, (m,), backend).assemble(f)          # the right-hand side: an HPCVector

``rows`` / ``cols`` are global 0-based indices (int64 device tensors, or numpy integer arrays that the plan uploads once),
``vals`` a float64 device tensor or numpy array of the same length in the caller's order.  Duplicates are summed.

Structure.  It depends on ``(rows, cols)`` only: an entry exists for every distinct ``(i, j)`` present, also when its values
sum to zero -- explicit zeros are kept, as Julia and scipy keep them -- and columns ascend within a row.  Every result of one
plan shares the plan's structure arrays and structural hash (``template._with_values``), so VectorPlans, pattern tables and
the preconditioners' ``update`` paths are paid once.

Sum order (it fixes the bits).  Let the contributions of one output entry sit at positions ``p1 < p2 < ... < pL`` of the
rank's value list and ``CH = hpcla_assemble_chunk()`` (512).  If ``L <= CH``: ``s = v[p1]; s = s + v[p2]; ...`` left to
right, started from the first value and not from 0.0, so a lone ``-0.0`` stays ``-0.0``.  If ``L > CH``: consecutive chunks
of ``CH`` contributions are summed by that rule and the partial sums are added left to right in chunk order.  Only adds
occur, there are no atomics, and two calls give the same bits.  An index of the vector form that nothing contributes to
holds ``+0.0``.

Across ranks.  Each rank passes its own triplets; one whose row belongs to another rank is routed to the owner.  At plan
time the off-rank ``(row, col)`` lists travel through the host and a width-1 single-buffered halo plan is built whose send
list is the positions of those triplets in ``vals``, grouped by owner.  The rank's value list is then
``[vals | received]``: its own contributions in input order, then the received ones in ascending sender rank, each in the
sender's order.  ``assemble`` is halo_begin(vals), halo_end, the kernel.  The bits of a result therefore depend on the
partition and on which rank contributed what, within rounding; when no rank routes anything no halo plan exists and a rank
launches what one rank launches.

Plan time: the keys ``(row - row_lo) * ncols + col`` and the count of refused indices on the device, one stable
``torch.sort`` as plumbing (as matmat.py does), then the library's kernels (csrc/assemble.hip over csrc/scan.h): segment
heads, ``seg_ptr``, ``rowptr``, the global columns; ``HPCSparseMatrix_local_device`` finishes the structure.  A plan's
errors (an index outside the shape, with how many and the first offender; a Float32 backend; lengths, dtypes, shapes) are
raised on every rank together.  ``assemble`` / ``assemble_`` check length, dtype and the target on the host, on the rank
that holds them -- a collective verdict would put a host exchange into every step -- read nothing back, and run on the
caller's stream.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _capi
from .backends import (attach_halo_windows, comm_allgather, comm_alltoall_counts, comm_exchange_arrays, comm_rank, comm_size,
                       create_halo_plan, halo_ghost_ptr, require_device)
from .partition import compute_partition_hash, uniform_partition
from .vectors import HPCVector, current_stream_ptr, dptr

_INT32_MAX = int(np.iinfo(np.int32).max)


def _torch():
    import torch
    return torch


def _is_tensor(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def _index_array(a, name: str):
    """A 1-D list of indices: an int64 torch tensor as it is, anything else as a numpy int64 array."""
    if _is_tensor(a):
        if a.dtype != _torch().int64:
            raise TypeError(f"assembly_plan: {name} must be int64, got {a.dtype}")
        if a.dim() != 1:
            raise ValueError(f"assembly_plan: {name} must be one-dimensional, got {a.dim()} dimensions")
        return a
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError(f"assembly_plan: {name} must hold integers, got {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"assembly_plan: {name} must be one-dimensional, got {a.ndim} dimensions")
    if a.dtype == np.uint64 and len(a) and int(a.max()) > int(np.iinfo(np.int64).max):
        raise IndexError(f"assembly_plan: {name} holds an index beyond int64")
    return np.ascontiguousarray(a, dtype=np.int64)


def _out_of_range(n_bad: int, first: int, r: int, c: Optional[int], shape) -> IndexError:
    where = f"row {r}" if c is None else f"({r}, {c})"
    return IndexError(f"assembly_plan: {n_bad} of the indices lie outside the shape {tuple(shape)}; the first is {where} "
                      f"at position {first}")


def check_arguments(T, rows, cols, shape, row_partition, col_partition, rank: int, nranks: int):
    """The argument rules, on host values only (a device tensor is asked for its dtype and length, never read).  Returns
    ``(rows, cols, m, ncols, row_partition, col_partition)`` with numpy inputs as int64 arrays; ``cols`` None and
    ``ncols`` 1 for the vector form.  Indices given as numpy arrays are range-checked here; device tensors on the device."""
    if np.dtype(T) != np.dtype(np.float64):
        raise TypeError("assembly_plan: offered for Float64 backends only")
    shape = tuple(int(s) for s in shape) if isinstance(shape, (tuple, list)) else None
    vector = cols is None
    if shape is None or len(shape) != (1 if vector else 2) or min(shape) < 0:
        raise ValueError("assembly_plan: shape is (m, n) with rows and cols, or (n,) with cols None (the vector form)")
    m, ncols = shape[0], (1 if vector else shape[1])
    rows = _index_array(rows, "rows")
    n_in = int(rows.shape[0])
    if not vector:
        cols = _index_array(cols, "cols")
        if int(cols.shape[0]) != n_in:
            raise ValueError(f"assembly_plan: rows and cols differ in length: {n_in} and {int(cols.shape[0])}")
    if row_partition is None:
        row_partition = uniform_partition(m, nranks)
    row_partition = np.asarray(row_partition, dtype=np.int64)
    if (len(row_partition) != nranks + 1 or row_partition[0] != 0 or row_partition[-1] != m
            or np.any(np.diff(row_partition) < 0)):
        raise ValueError(f"assembly_plan: row_partition must ascend from 0 to {m} in {nranks + 1} steps")
    if col_partition is None:
        col_partition = uniform_partition(ncols, nranks)
    col_partition = np.asarray(col_partition, dtype=np.int64)
    if not vector and (len(col_partition) != nranks + 1 or col_partition[0] != 0 or col_partition[-1] != ncols):
        raise ValueError(f"assembly_plan: col_partition must run from 0 to {ncols} in {nranks + 1} steps")
    nrows_local = int(row_partition[rank + 1] - row_partition[rank])
    if nrows_local * ncols >= 2 ** 63:
        raise ValueError(f"assembly_plan: {nrows_local} local rows times {ncols} columns do not fit a 63-bit key")
    if ncols == 0:
        raise ValueError("assembly_plan: a matrix needs at least one column")
    if n_in and not (_is_tensor(rows) and (vector or _is_tensor(cols))):
        bad = np.zeros(n_in, dtype=bool)
        if not _is_tensor(rows):
            bad |= (rows < 0) | (rows >= m)
        if not vector and not _is_tensor(cols):
            bad |= (cols < 0) | (cols >= ncols)
        if bad.any():
            p = int(np.flatnonzero(bad)[0])
            r = int(rows[p].item()) if _is_tensor(rows) else int(rows[p])
            c = None if vector else (int(cols[p].item()) if _is_tensor(cols) else int(cols[p]))
            raise _out_of_range(int(bad.sum()), p, r, c, shape)
    return rows, cols, m, ncols, row_partition, col_partition


def check_values(vals, n_in: int):
    """``vals`` of an assemble call: one-dimensional float64 of the plan's length (host values only)."""
    if _is_tensor(vals):
        if vals.dtype != _torch().float64:
            raise TypeError(f"assemble: vals must be float64, got {vals.dtype}")
        shape = tuple(vals.shape)
    else:
        vals = np.asarray(vals)
        if vals.dtype != np.float64:
            raise TypeError(f"assemble: vals must be float64, got {vals.dtype}")
        shape = vals.shape
    if len(shape) != 1 or int(shape[0]) != n_in:
        raise ValueError(f"assemble: vals must hold {n_in} values, one per triplet of the plan, got shape {tuple(shape)}")
    return vals


def _raise_together(comm, err: Optional[Exception], what: str = "assembly_plan") -> None:
    """Every rank learns whether any rank refuses and all raise: a rank raising alone would leave the others waiting in the
    next collective (as spgemm_local does for its row limit)."""
    refused = comm_allgather(comm, np.array([1 if err is not None else 0], dtype=np.int64))
    if err is not None:
        raise err
    if refused.any():
        ranks = np.flatnonzero(refused).tolist()
        raise ValueError(f"{what}: refused on rank(s) {ranks}; this rank's arguments were accepted")


class AssemblyPlan:
    """The inverted index of one ``(rows, cols)`` list.  ``n_in``: this rank's triplets; ``nnz``: this rank's output entries
    (distinct pairs; local length for the vector form); ``template``: the structure (an HPCSparseMatrix whose values are
    zero, or None for the vector form); ``n_routed``: triplets this rank sends to the owners of their rows;
    ``n_received``: triplets it receives; ``max_duplicates``: the longest list of contributions to one entry."""

    def __init__(self, rows, cols, shape, backend, row_partition=None, col_partition=None):
        comm = backend.comm
        rank, nranks = comm_rank(comm), comm_size(comm)
        err = None
        try:
            rows, cols, m, ncols, row_partition, col_partition = check_arguments(backend.T, rows, cols, shape, row_partition,
                                                                                 col_partition, rank, nranks)
        except (TypeError, ValueError, IndexError) as exc:
            err = exc
        _raise_together(comm, err)
        require_device(backend, "assembly_plan")
        torch = _torch()
        lib = _capi.load()
        dev = backend.torch_device
        self.backend = backend
        self.vector = cols is None
        self.shape = (m,) if self.vector else (m, ncols)
        self.row_partition, self.col_partition = row_partition, col_partition
        lo, hi = int(row_partition[rank]), int(row_partition[rank + 1])
        self.n_in = int(rows.shape[0])
        s = current_stream_ptr()

        def on_device(a):
            return a.to(dev).contiguous() if _is_tensor(a) else torch.from_numpy(a).to(dev)

        rows_d = on_device(rows)
        cols_d = None if self.vector else on_device(cols)

        def keys_of(r_d, c_d):
            n = int(r_d.numel())
            key = torch.empty(n, dtype=torch.int64, device=dev)
            counts = torch.empty(4, dtype=torch.int64, device=dev)
            _capi.call("hpcla_assemble_keys", dptr(r_d), dptr(c_d), n, lo, hi, m, ncols, 0, dptr(key), dptr(counts), s)
            return key, [int(c) for c in counts.cpu().tolist()]

        key, (n_bad, first_bad, n_off, _first_off) = keys_of(rows_d, cols_d)
        err = None
        if n_bad:
            err = _out_of_range(n_bad, first_bad, int(rows_d[first_bad].item()),
                                None if self.vector else int(cols_d[first_bad].item()), self.shape)
        _raise_together(comm, err)
        self.n_routed = n_off
        self.n_received = 0
        self._halo = ctypes.c_void_p()
        self._ghost = ctypes.c_void_p()
        routed_anywhere = nranks > 1 and bool(comm_allgather(comm, np.array([n_off], dtype=np.int64)).any())
        if routed_anywhere:
            key = self._route(key, rows_d, cols_d, keys_of)
        del rows_d, cols_d
        n_list = int(key.numel())                                  # the rank's value list: [vals | received]
        self._n_list = n_list
        key, perm = torch.sort(key, stable=True)                   # plumbing, as matmat._build_product_map
        n_keep = n_list - n_off                                    # the routed triplets carry the largest key: they sort last
        key, perm = key[:n_keep], perm[:n_keep]
        self._n_perm = n_keep
        self._i64 = n_list > _INT32_MAX
        sfx = "i64" if self._i64 else "i32"
        pdt = torch.int64 if self._i64 else torch.int32
        self._sfx = sfx
        self._perm = perm.to(pdt).contiguous()
        del perm
        nloc = hi - lo
        if self.vector:
            self.template = None
            self.nnz = nloc
            self.partition_hash = compute_partition_hash(row_partition)
            seg_ptr = torch.empty(nloc + 1, dtype=pdt, device=dev)
            _capi.call(f"hpcla_assemble_row_starts_{sfx}", dptr(key), n_keep, nloc, 1, 0, dptr(seg_ptr), s)
        else:
            seg_ptr = torch.empty(n_keep + 1, dtype=pdt, device=dev)
            ukey = torch.empty(n_keep, dtype=torch.int64, device=dev)
            work = torch.empty(lib.hpcla_assemble_work_bytes(n_keep), dtype=torch.uint8, device=dev)
            nnz = ctypes.c_int64()
            _capi.call(f"hpcla_assemble_segments_{sfx}", dptr(key), n_keep, dptr(seg_ptr), dptr(ukey), ctypes.byref(nnz),
                       dptr(work), s)
            self.nnz = int(nnz.value)
            seg_ptr = seg_ptr[:self.nnz + 1].clone() if self.nnz < n_keep else seg_ptr
            rowptr = torch.empty(nloc + 1, dtype=torch.int64, device=dev)
            colidx = torch.empty(self.nnz, dtype=torch.int64, device=dev)
            _capi.call("hpcla_assemble_row_starts_i64", dptr(ukey), self.nnz, nloc, ncols, 0, dptr(rowptr), s)
            _capi.call("hpcla_assemble_columns", dptr(ukey), self.nnz, ncols, 0, dptr(colidx), s)
            del ukey, work
            from .sparse import HPCSparseMatrix_local_device
            self.template = HPCSparseMatrix_local_device(rowptr, colidx, torch.zeros(self.nnz, dtype=torch.float64, device=dev),
                                                         ncols, backend, col_partition=col_partition)
            if not np.array_equal(self.template.row_partition, row_partition):
                raise ValueError("assembly_plan: row_partition inconsistent across ranks")
            self.template._ensure_hash()                           # shared by every result through _with_values
        del key
        self._seg_ptr = seg_ptr
        self.max_duplicates = int((seg_ptr[1:] - seg_ptr[:-1]).max().item()) if self.nnz else 0
        chunk = int(lib.hpcla_assemble_chunk())
        self._work = (torch.empty(lib.hpcla_assemble_values_work_bytes(n_keep), dtype=torch.uint8, device=dev)
                      if self.max_duplicates > chunk else None)
        self._keep = None

    # -- the second stage: triplets of other ranks' rows ---------------------------------------------------------------
    def _route(self, key, rows_d, cols_d, keys_of):
        """COLLECTIVE (some rank routes).  Sends the off-rank (row, col) pairs to the owners of their rows through the host,
        builds the halo plan that carries their values at every assemble, and returns the keys of [own | received]."""
        torch = _torch()
        backend = self.backend
        comm = backend.comm
        rank, nranks = comm_rank(comm), comm_size(comm)
        dev = backend.torch_device
        off = torch.nonzero(key == np.iinfo(np.int64).max).flatten()
        off_pos = off.cpu().numpy()
        off_rows = rows_d[off].cpu().numpy()
        off_cols = None if self.vector else cols_d[off].cpu().numpy()
        owner = np.searchsorted(self.row_partition, off_rows, side="right") - 1
        order = np.argsort(owner, kind="stable")                   # grouped by owner, each group in input order
        counts = np.bincount(owner, minlength=nranks).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(counts)])
        send_ranks = [r for r in range(nranks) if counts[r]]
        groups = [order[starts[r]:starts[r + 1]] for r in send_ranks]
        incoming = comm_alltoall_counts(comm, counts)
        recv_ranks = [r for r in range(nranks) if incoming[r]]
        recv_counts = [int(incoming[r]) for r in recv_ranks]
        got_rows = comm_exchange_arrays(comm, send_ranks, [off_rows[g] for g in groups], recv_ranks, recv_counts, np.int64)
        got_cols = None
        if not self.vector:
            got_cols = comm_exchange_arrays(comm, send_ranks, [off_cols[g] for g in groups], recv_ranks, recv_counts, np.int64)
        self.n_received = int(sum(recv_counts))
        if self.n_in + self.n_received > np.iinfo(np.int64).max // 2:
            raise OverflowError("assembly_plan: the value list does not fit")
        has = bool(send_ranks or recv_ranks)
        if has:
            self._halo = create_halo_plan(backend, send_ranks, [off_pos[g].astype(np.int64) for g in groups], np.int64,
                                          recv_ranks, recv_counts, 1)
        attach_halo_windows(backend, self._halo if has else None)  # collective: ranks without traffic vote too
        if has:
            self._ghost, n_ghost = halo_ghost_ptr(self._halo)      # a constant of the single-buffered plan
            assert n_ghost == self.n_received, (n_ghost, self.n_received)
        if not self.n_received:
            return key
        r_d = torch.from_numpy(np.concatenate(got_rows)).to(dev)
        c_d = None if self.vector else torch.from_numpy(np.concatenate(got_cols)).to(dev)
        key_recv, (n_bad, _f, n_foreign, _g) = keys_of(r_d, c_d)
        if n_bad or n_foreign:                                     # the senders checked both: a defect, not an input error
            raise RuntimeError(f"assembly_plan: {n_bad + n_foreign} routed triplets do not belong to this rank's rows")
        return torch.cat([key, key_recv])

    # -- assembly ------------------------------------------------------------------------------------------------------
    def _values_into(self, out, vals) -> None:
        vals = check_values(vals, self.n_in)
        torch = _torch()
        if not _is_tensor(vals):
            vals = torch.from_numpy(np.ascontiguousarray(vals)).to(self.backend.torch_device)
        elif vals.device != out.device:
            raise ValueError(f"assemble: vals lives on {vals.device}, the plan on {out.device}")
        vals = vals.contiguous()
        s = current_stream_ptr()
        if self._halo:
            _capi.call("hpcla_halo_begin", self._halo, dptr(vals) if self.n_in else None, s)
            _capi.call("hpcla_halo_end", self._halo, s)
        _capi.call(f"hpcla_assemble_values_f64_{self._sfx}", dptr(self._seg_ptr), dptr(self._perm) if self._n_perm else None,
                   self.nnz, self._n_perm, dptr(vals) if self.n_in else None, self.n_in,
                   self._ghost if self.n_received else None, self.n_received, self.max_duplicates, dptr(out),
                   dptr(self._work), s)
        self._keep = vals                                          # an uploaded copy lives until the next call has been enqueued

    def assemble(self, vals):
        """A new HPCSparseMatrix (HPCVector for the vector form) with the sums of ``vals``; every result of one plan shares
        the structure arrays and the hash."""
        out = _torch().empty(self.nnz, dtype=_torch().float64, device=self.backend.torch_device)
        self._values_into(out, vals)
        if self.vector:
            return HPCVector(self.partition_hash, self.row_partition, out, self.backend)
        return self.template._with_values(out)

    def assemble_(self, A, vals):
        """Rewrite ``A.nzval`` (``b.v``) in place.  ``A`` must be a result of this plan -- or share its structure arrays, as
        ``A.copy()`` and ``2 * A`` do -- else ValueError.  An opt-in packed copy of A snapshots values: disable it first."""
        if self.vector:
            ok = (isinstance(A, HPCVector) and A.backend is self.backend and np.array_equal(A.partition, self.row_partition)
                  and int(A.v.numel()) == self.nnz and A.v.dtype == _torch().float64 and A.v.is_contiguous())
            target = A.v if ok else None
        else:
            t = self.template
            ok = (hasattr(A, "rowptr_target") and A.rowptr_target is t.rowptr_target and A._colval_target is t._colval_target
                  and A.nnz == self.nnz and A.nzval.is_contiguous())
            target = A.nzval if ok else None
        if not ok:
            raise ValueError("assemble_: the target is not a result of this plan (it does not share the plan's structure)")
        self._values_into(target, vals)
        return A

    def destroy(self) -> None:
        if self._halo:
            _capi.call("hpcla_halo_plan_destroy", self._halo)
            self._halo = ctypes.c_void_p()


def assembly_plan(rows, cols, shape, backend, row_partition=None, col_partition=None) -> AssemblyPlan:
    """The plan of ``sparse(rows, cols, ., m, n)`` on ``backend`` (``cols`` None, ``shape`` ``(n,)``: of a vector).
    Collective.  See the module docstring for the structure, the sum order and the routing across ranks."""
    return AssemblyPlan(rows, cols, shape, backend, row_partition, col_partition)


def sparse_from_coo(rows, cols, vals, shape, backend, row_partition=None, col_partition=None):
    """One shot: Julia's ``sparse(I, J, V, m, n)`` -- ``assembly_plan(...).assemble(vals)``."""
    check_values(vals, int(rows.shape[0]) if hasattr(rows, "shape") else len(rows))
    return assembly_plan(rows, cols, shape, backend, row_partition, col_partition).assemble(vals)
