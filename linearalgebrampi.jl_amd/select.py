"""Index-set selection on DeviceROCm: ``hp.select(A, rows, cols)``, ``hp.take(v, idx)``, ``hp.put_(v, idx, src)`` and their
plans (reference: the index-vector half of src/indexing.jl, from line 1318 on: ``v[idx]`` :1339-1460, ``A[row_idx, col_idx]``
:1654-1815, ``v[idx] = src`` :1871-1985).

::

    K_ff = hp.select(K, free, free)                                  # Dirichlet elimination after assembly
    f_f = hp.take(f, free) - hp.select(K, free, fixed) @ hp.take(g, fixed)
    u_f, info = hp.cg(K_ff, f_f);  hp.put_(u, free, u_f)
    B = hp.select(A, p, p)                                           # the symmetric permutation A[p, p]
    plan = hp.selection_plan(K, free, free);  K2_ff = plan.extract(K2)       # new values on the same structure

Index arguments follow ``hp.assembly_plan``: every rank passes its own array of GLOBAL 0-based indices (a numpy integer
array, or an int64 torch tensor on the host or the device).  ``rows=None`` is this rank's own rows in order, ``cols=None``
all columns in order (the result then keeps ``A.col_partition``).  The result's ``row_partition`` is the cumulative sum of
the ranks' ``len(rows)``, its ``col_partition`` that of the ranks' ``len(cols)``; the global column list is the ranks' lists
in rank order, gathered through the host at plan time as the reference gathers ``col_idx`` (:1662, 1821-1844).  Passing the
same list as rows and cols therefore gives equal partitions, which the solvers require.

``select`` returns an **HPCSparseMatrix**, as range indexing does here; the reference returns a dense ``HPCMatrix``
(:1640-1644), which is unusable at these sizes.  ``rows`` may repeat and come in any order, but on more than one rank they
must be rows the rank owns (moving sparse rows between ranks is ``hp.repartition``'s job).  ``cols`` must be distinct over
all ranks: the reference lets the last duplicate win through a Dict (:1675-1678), here it is a ValueError.  Violations are
raised on every rank together.  Values are moved as integers of the element size (Float64 / Float32), every bit survives,
and ``A`` is left untouched and unhashed.

Plan time: one stable ``torch.sort`` of the gathered column list as plumbing (as assemble.py does), then csrc/select.hip:
the column look-up, count and mark, two scans, rank and fill.  ``SelectionPlan.extract`` is one gather of values.

``take`` may read any global index: entries of other ranks travel by a width-1 single-buffered halo plan over the sorted
unique off-rank indices (none is built when no rank needs one).  ``put_`` takes distinct indices the calling rank owns.
Both are Float64 only.  Not offered: dense ``HPCMatrix`` index-set forms, ``setindex!`` on matrices, row selection across ranks.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _capi
from .assemble import _is_tensor, _raise_together
from .backends import (attach_halo_windows, comm_allgather, comm_alltoall_counts, comm_exchange_arrays, comm_rank, comm_size,
                       create_halo_plan, halo_ghost_ptr, require_device)
from .indexing import _col_indices_dev
from .partition import compute_partition_hash
from .vectors import HPCVector, current_stream_ptr, dptr

_INT32_MAX = int(np.iinfo(np.int32).max)


def _torch():
    import torch
    return torch


def _index_tensor(a, name: str, what: str, dev):
    """A 1-D list of indices as an int64 tensor on ``dev`` (host values are uploaded once)."""
    torch = _torch()
    if _is_tensor(a):
        if a.dtype != torch.int64:
            raise TypeError(f"{what}: {name} must be int64, got {a.dtype}")
        if a.dim() != 1:
            raise ValueError(f"{what}: {name} must be one-dimensional, got {a.dim()} dimensions")
        return a.to(dev).contiguous()
    a = np.asarray(a)
    if a.size == 0 and a.ndim == 1:
        a = a.astype(np.int64)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{what}: {name} must hold integers, got {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"{what}: {name} must be one-dimensional, got {a.ndim} dimensions")
    if a.dtype == np.uint64 and len(a) and int(a.max()) > int(np.iinfo(np.int64).max):
        raise IndexError(f"{what}: {name} holds an index beyond int64")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def _check_range(t, n: int, name: str, what: str) -> None:
    if not t.numel():
        return
    bad = (t < 0) | (t >= n)
    n_bad = int(bad.sum().item())
    if n_bad:
        first = int(_torch().nonzero(bad)[0].item())
        raise IndexError(f"{what}: {n_bad} of the {name} lie outside [0, {n}); the first is {int(t[first].item())} "
                         f"at position {first}")


def _gather_lists(comm, local: np.ndarray):
    """(the ranks' int64 lists concatenated in rank order, their lengths): through the host, padded to the longest."""
    counts = comm_allgather(comm, np.array([len(local)], dtype=np.int64))
    longest = int(counts.max()) if len(counts) else 0
    if comm_size(comm) == 1 or longest == 0:
        return local.copy(), counts
    padded = np.zeros(longest, dtype=np.int64)
    padded[:len(local)] = local
    flat = comm_allgather(comm, padded).reshape(len(counts), longest)
    return np.concatenate([flat[r, :int(counts[r])] for r in range(len(counts))]), counts


def _partition_of(counts) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _select(A, rows, cols):
    """The selection proper.  Returns (B, src): the result and the int64 device positions of its entries in A.nzval."""
    from .sparse import HPCSparseMatrix
    if not isinstance(A, HPCSparseMatrix):
        raise TypeError("select: an HPCSparseMatrix is required")
    require_device(A.backend, "select")
    torch = _torch()
    backend = A.backend
    comm = backend.comm
    rank, nranks = comm_rank(comm), comm_size(comm)
    dev = backend.torch_device
    m, n = A.shape
    lo, hi = int(A.row_partition[rank]), int(A.row_partition[rank + 1])
    rows_d = cols_d = None
    err = None
    try:
        if rows is not None:
            rows_d = _index_tensor(rows, "rows", "select", dev)
            _check_range(rows_d, m, "rows", "select")
            foreign = (rows_d < lo) | (rows_d >= hi)
            if bool(foreign.any().item()):
                r = int(rows_d[int(torch.nonzero(foreign)[0].item())].item())
                owner = int(np.searchsorted(A.row_partition, r, side="right")) - 1
                raise ValueError(f"select: row {r} is owned by rank {owner}; repartition first")
            rows_d = rows_d - lo
        if cols is not None:
            cols_d = _index_tensor(cols, "cols", "select", dev)
            _check_range(cols_d, n, "cols", "select")
    except (TypeError, ValueError, IndexError) as exc:
        err = exc
    _raise_together(comm, err, "select")
    nsel = A.nrows_local if rows is None else int(rows_d.numel())
    row_part = _partition_of(comm_allgather(comm, np.array([nsel], dtype=np.int64)))
    sorted_cols = sorted_pos = None
    if cols is None:
        col_part, width, nsorted = A.col_partition, n, -1
    else:
        if nranks > 1:
            all_cols, counts = _gather_lists(comm, cols_d.cpu().numpy())
            col_part = _partition_of(counts)
            cols_d = torch.from_numpy(all_cols).to(dev)
        else:
            col_part = _partition_of([int(cols_d.numel())])
        width = nsorted = int(cols_d.numel())
        sorted_cols, sorted_pos = torch.sort(cols_d, stable=True)              # plumbing, as assemble.py's sort
        if nsorted > 1:
            same = sorted_cols[1:] == sorted_cols[:-1]                          # the duplicates, from the sort the plan needs anyway
            if bool(same.any().item()):
                c = int(sorted_cols[1:][same][0].item())
                raise ValueError(f"select: column {c} is listed more than once; cols must be distinct over all ranks")
    sfx = "i64" if A.Ti == np.dtype(np.int64) else "i32"
    tdt = A.rowptr_target.dtype
    s = current_stream_ptr()
    lib = _capi.load()
    ci_src = _col_indices_dev(A)
    ncomp = int(ci_src.numel())
    colval_src = A.colval_target()
    work = torch.empty(lib.hpcla_select_work_bytes(nsel, ncomp, width), dtype=torch.uint8, device=dev)
    rowptr_out = torch.empty(nsel + 1, dtype=tdt, device=dev)
    col_indices_out = torch.empty(min(width, ncomp), dtype=torch.int64, device=dev)
    nnz_out, ncomp_out, max_row = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    name = f"hpcla_select_structure_{sfx}"
    status = getattr(lib, name)(dptr(A.rowptr_target), dptr(colval_src), A.nrows_local, A.nnz, dptr(ci_src), ncomp, dptr(rows_d),
                                nsel, dptr(sorted_cols), dptr(sorted_pos), nsorted, width, 0, dptr(rowptr_out),
                                dptr(col_indices_out), ctypes.byref(nnz_out), ctypes.byref(ncomp_out), ctypes.byref(max_row),
                                dptr(work), s)
    nnz = int(nnz_out.value)
    err = None
    if nnz > int(np.iinfo(A.Ti.type).max):               # the entry refuses it too and has returned the total: nothing wraps
        err = OverflowError(f"select: the result's {nnz} entries do not fit the backend index type {A.Ti.name}")
    _raise_together(comm, err, "select")                 # before anything is allocated by nnz
    _capi.check(name, status)
    colval_out = torch.empty(nnz, dtype=tdt, device=dev)
    nzval_out = torch.empty(nnz, dtype=A.nzval.dtype, device=dev)
    src = torch.empty(nnz, dtype=torch.int64, device=dev)
    _capi.call(f"hpcla_select_fill_{sfx}", A.nzval.element_size(), dptr(A.rowptr_target), dptr(colval_src), dptr(A.nzval),
               A.nrows_local, A.nnz, ncomp, dptr(rows_d), nsel, dptr(rowptr_out), nnz, int(max_row.value), 0, dptr(work),
               dptr(colval_out), dptr(nzval_out), dptr(src), s)
    nc = int(ncomp_out.value)
    # the new columns that occur; a short list does not keep the capacity-sized buffer alive
    ci_dev = col_indices_out if nc == int(col_indices_out.numel()) else col_indices_out[:nc].clone()
    # every new column occurs (a symmetric selection of a matrix with a full diagonal, a permutation): the list is
    # 0 .. width - 1 and is not read back
    ci_host = np.arange(width, dtype=np.int64) if nc == width else ci_dev.cpu().numpy()
    B = HPCSparseMatrix(row_part, col_part, ci_host, None, None, nzval_out, rowptr_out, backend)
    B._colval_target = colval_out
    B._col_indices_dev = ci_dev
    return B, src


def select(A, rows=None, cols=None):
    """``A[rows, cols]`` for index lists, as an HPCSparseMatrix (the reference returns a dense HPCMatrix,
    src/indexing.jl:1640-1644, unusable at these sizes).  Collective; see the module docstring for the index arguments, the
    partitions of the result and the rules.  Never hashes ``A``."""
    return _select(A, rows, cols)[0]


class SelectionPlan:
    """``selection_plan(A, rows, cols)``: the structure of ``select(A, rows, cols)`` (``.matrix``) and the position of each of
    its entries in ``A.nzval``.  ``extract(A2)``, for any A2 with A's structure, gathers the values alone and returns a
    matrix that SHARES the plan's structure arrays and structural hash, so the VectorPlans, pattern tables and the
    preconditioners' update paths built over one selection serve them all."""

    def __init__(self, A, rows=None, cols=None):
        self.matrix, self._src = _select(A, rows, cols)
        self.source_hash = A._ensure_hash()
        self.source_nnz = A.nnz
        self.T, self.Ti = A.T, A.Ti
        self.matrix._ensure_hash()                       # shared by every extract() through _with_values

    def extract(self, A2):
        if A2.T != self.T or A2.Ti != self.Ti or A2.nnz != self.source_nnz or A2._ensure_hash() != self.source_hash:
            raise ValueError("SelectionPlan.extract: the matrix does not have the structure the plan was built for")
        B = self.matrix
        out = _torch().empty_like(B.nzval)
        if B.nnz:
            vals = A2.nzval.contiguous()
            if vals.element_size() == 8:
                _capi.call("hpcla_gather_f64_i64", dptr(vals), dptr(self._src), None, dptr(out), B.nnz, 0, current_stream_ptr())
            else:
                _capi.call("hpcla_gather_b32_i64", dptr(vals), dptr(self._src), dptr(out), B.nnz, A2.nnz, 0, current_stream_ptr())
        return B._with_values(out)


def selection_plan(A, rows=None, cols=None) -> SelectionPlan:
    return SelectionPlan(A, rows, cols)


class VectorIndexPlan:
    """``index_plan(idx, partition, backend)``: the positions of ``idx`` in ``[own | ghost]`` and, when some rank reads
    another's entries, the halo plan that carries them.  ``take(v, out=None)`` is the exchange and one kernel, ``put_(v, src)``
    one kernel; ``n_ghost`` is the number of distinct off-rank indices this rank reads, ``has_halo`` whether a halo plan exists
    on this rank, ``exchanges`` whether one exists on any rank."""

    def __init__(self, idx, partition, backend, what: str = "index_plan"):
        comm = backend.comm
        rank, nranks = comm_rank(comm), comm_size(comm)
        torch = _torch()
        partition = np.asarray(partition, dtype=np.int64)
        err = None
        idx_d = None
        try:
            if np.dtype(backend.T) != np.dtype(np.float64):
                raise TypeError(f"{what}: offered for Float64 backends only")
            if len(partition) != nranks + 1 or partition[0] != 0 or np.any(np.diff(partition) < 0):
                raise ValueError(f"{what}: partition must ascend from 0 in {nranks + 1} steps")
            require_device(backend, what)
            idx_d = _index_tensor(idx, "idx", what, backend.torch_device)
            _check_range(idx_d, int(partition[-1]), "indices", what)
        except (TypeError, ValueError, IndexError) as exc:
            err = exc
        _raise_together(comm, err, what)
        dev = backend.torch_device
        self.backend = backend
        self.partition = partition
        self.partition_hash = compute_partition_hash(partition)
        self.n = int(idx_d.numel())
        self.result_partition = _partition_of(comm_allgather(comm, np.array([self.n], dtype=np.int64)))
        self.result_hash = compute_partition_hash(self.result_partition)
        lo, hi = int(partition[rank]), int(partition[rank + 1])
        self.n_own = hi - lo
        self._halo = ctypes.c_void_p()
        self._ghost = ctypes.c_void_p()
        self.n_ghost = 0
        self._idx = idx_d
        self._put_error = False                          # unknown until the first put_
        foreign = (idx_d < lo) | (idx_d >= hi)
        n_off = int(foreign.sum().item())
        self.n_foreign = n_off
        uniq = None
        self.exchanges = nranks > 1 and bool(comm_allgather(comm, np.array([n_off], dtype=np.int64)).any())
        if self.exchanges:
            uniq = torch.unique(idx_d[foreign])          # sorted: grouped by owner, ascending within each
            self._exchange(uniq.cpu().numpy())
        pos = idx_d - lo
        if n_off:
            pos = torch.where(foreign, self.n_own + torch.searchsorted(uniq, idx_d), pos)
        self._i64 = self.n_own + self.n_ghost > _INT32_MAX
        self._sfx = "i64" if self._i64 else "i32"
        self._pos = pos.to(torch.int64 if self._i64 else torch.int32).contiguous()

    @property
    def has_halo(self) -> bool:
        return bool(self._halo)

    def _exchange(self, wanted: np.ndarray) -> None:
        """COLLECTIVE (some rank reads another's entries).  Tells the owners which of their entries this rank reads and builds
        the width-1 single-buffered halo plan, as AssemblyPlan._route does: the ghost buffer holds ``wanted`` in order."""
        backend = self.backend
        comm = backend.comm
        rank, nranks = comm_rank(comm), comm_size(comm)
        owner = np.searchsorted(self.partition, wanted, side="right") - 1
        counts = np.bincount(owner, minlength=nranks).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(counts)])
        recv_ranks = [r for r in range(nranks) if counts[r]]
        recv_counts = [int(counts[r]) for r in recv_ranks]
        asked = comm_alltoall_counts(comm, counts)
        send_ranks = [r for r in range(nranks) if asked[r]]
        lists = comm_exchange_arrays(comm, recv_ranks, [wanted[starts[r]:starts[r + 1]] for r in recv_ranks], send_ranks,
                                     [int(asked[r]) for r in send_ranks], np.int64)
        lo = int(self.partition[rank])
        has = bool(send_ranks or recv_ranks)
        if has:
            self._halo = create_halo_plan(backend, send_ranks, [np.asarray(g, dtype=np.int64) - lo for g in lists], np.int64,
                                          recv_ranks, recv_counts, 1)
        attach_halo_windows(backend, self._halo if has else None)  # collective: ranks without traffic vote too
        if has:
            self._ghost, self.n_ghost = halo_ghost_ptr(self._halo)  # a constant of the single-buffered plan
            assert self.n_ghost == len(wanted), (self.n_ghost, len(wanted))

    def _operand(self, v, what: str):
        torch = _torch()
        if not isinstance(v, HPCVector) or v.v.dtype != torch.float64:
            raise TypeError(f"{what}: a Float64 HPCVector is required")
        if v.structural_hash != self.partition_hash:
            raise ValueError(f"{what}: the vector is not on the plan's partition")
        return v

    def take(self, v, out=None):
        """``v[idx]`` on the cumulative sum of the ranks' ``len(idx)``; into ``out`` when given."""
        torch = _torch()
        self._operand(v, "take")
        if out is None:
            out = HPCVector(self.result_hash, self.result_partition,
                            torch.empty(self.n, dtype=torch.float64, device=self.backend.torch_device), self.backend)
        elif (not isinstance(out, HPCVector) or out.structural_hash != self.result_hash or out.v.dtype != torch.float64
              or not out.v.is_contiguous()):
            raise ValueError("take: out must be a contiguous Float64 HPCVector on the partition take returns")
        x = v.v.contiguous()
        s = current_stream_ptr()
        if self._halo:
            _capi.call("hpcla_halo_begin", self._halo, dptr(x) if self.n_own else None, s)
            _capi.call("hpcla_halo_end", self._halo, s)
        _capi.call(f"hpcla_select_take_f64_{self._sfx}", dptr(x) if self.n_own else None, self.n_own,
                   self._ghost if self.n_ghost else None, self.n_ghost, dptr(self._pos), self.n, 0, dptr(out.v), s)
        self._keep = x                                   # a contiguous copy lives until the next call has been enqueued
        return out

    def put_(self, v, src):
        """``v[idx] = src`` in place: ``idx`` must be distinct indices this rank owns, ``src`` an HPCVector on the partition
        ``take`` returns."""
        torch = _torch()
        if self._put_error is False:
            err = None
            if self.n_foreign:
                lo = int(self.partition[comm_rank(self.backend.comm)])
                bad = self._idx[(self._idx < lo) | (self._idx >= lo + self.n_own)]
                err = ValueError(f"put_: {self.n_foreign} of the indices are not owned by this rank; the first is "
                                 f"{int(bad[0].item())}")
            elif self.n > 1:
                srt = torch.sort(self._idx).values
                same = srt[1:] == srt[:-1]
                if bool(same.any().item()):
                    err = ValueError(f"put_: index {int(srt[1:][same][0].item())} is listed more than once; a scatter with "
                                     "duplicates has no defined winner")
            try:
                _raise_together(self.backend.comm, err, "put_")
            except ValueError as exc:                    # the COLLECTIVE verdict is kept: every later put_ raises on every rank
                self._put_error = exc
                raise
            self._put_error = None
        elif self._put_error is not None:
            raise self._put_error
        self._operand(v, "put_")
        if not v.v.is_contiguous():
            raise ValueError("put_: the target's local values must be contiguous")
        if not isinstance(src, HPCVector) or src.v.dtype != torch.float64:
            raise TypeError("put_: src must be a Float64 HPCVector")
        if src.structural_hash != self.result_hash:
            raise ValueError("put_: src must be on the partition take returns (the cumulative sum of the ranks' len(idx))")
        x = src.v.contiguous()
        _capi.call(f"hpcla_select_put_f64_{self._sfx}", dptr(v.v), self.n_own, dptr(self._pos), dptr(x), self.n, 0,
                   current_stream_ptr())
        self._keep = x
        return v

    def destroy(self) -> None:
        """Frees the halo plan.  COLLECTIVE when some rank reads another's entries (``exchanges``): the ranks drain their
        devices and meet first, so that no peer still stores into a ghost window that is about to be unmapped."""
        if self.exchanges:
            from .sparse import _quiesce
            _quiesce([self.backend])
            self.exchanges = False
        if self._halo:
            _capi.call("hpcla_halo_plan_destroy", self._halo)
            self._halo = ctypes.c_void_p()
            self._ghost, self.n_ghost = ctypes.c_void_p(), 0


def index_plan(idx, partition, backend) -> VectorIndexPlan:
    """The plan of ``v[idx]`` / ``v[idx] = src`` for vectors on ``partition``.  Collective."""
    return VectorIndexPlan(idx, partition, backend)


def _vector_of(v, what: str) -> None:
    if not isinstance(v, HPCVector):
        raise TypeError(f"{what}: an HPCVector is required")


def take(v, idx, out: Optional[HPCVector] = None) -> HPCVector:
    """``v[idx]``: ``index_plan(idx, v.partition, v.backend).take(v, out)``.  Collective; ``idx`` may hold any global index."""
    _vector_of(v, "take")
    plan = VectorIndexPlan(idx, v.partition, v.backend, "take")
    try:
        return plan.take(v, out)
    finally:
        plan.destroy()                                               # drains the device first: the kernel reads the ghost buffer


def put_(v, idx, src) -> HPCVector:
    """``v[idx] = src`` in place.  Collective; ``idx``: distinct indices the calling rank owns (ValueError otherwise)."""
    _vector_of(v, "put_")
    plan = VectorIndexPlan(idx, v.partition, v.backend, "put_")
    try:
        return plan.put_(v, src)
    finally:
        plan.destroy()
