"""HPCMatrix (dense, row-partitioned) on DeviceROCm and its products: dense ``A * x`` and ``transpose(A) * x``, the Gram
product ``transpose(X) * Y``, and dense times sparse ``X * A`` / ``transpose(X) * A``.  ``HPCSparseMatrix * HPCMatrix``
(SpMM) is in spmm_plans.py.

Reference: container + ``HPCMatrix_local`` (src/dense.jl:59-69, 125-156), ``HPCMatrix(M, backend)`` (:185-201), the
dense products (src/dense.jl:397-658, 1210-1310) and dense times sparse (src/sparse.jl:3617-3690).

Layout: the reference's local block is a column-major Julia ``Matrix`` (src/dense.jl:63).  On the
device the local block is stored ROW-major (a ``(rows_local, k)`` torch tensor): at k=16 one row is
exactly one 128-byte line, so the gather of a B row per stored entry of A is a single full-line
read, and ghost rows travel as contiguous ``count*k`` RCCL messages.  Column-major callers convert
with ``hpcla_transpose_f64``.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np

from . import _capi
from .backends import (HPCBackend, assert_backends_compatible, comm_allgather, comm_rank, comm_size, create_halo_plan,
                       halo_ghost_ptr)
from .partition import compute_partition_hash, uniform_partition
from .vectors import current_stream_ptr, dptr


def _torch():
    import torch
    return torch


class HPCMatrix:
    """``HPCMatrix{T,B}`` (src/dense.jl:59-69): ``row_partition``, ``col_partition``, local block
    ``A`` (device, row-major ``(rows_local, ncols)``), ``backend``."""

    def __init__(self, row_partition, col_partition, A_dev, backend: HPCBackend):
        self.structural_hash = None
        self.row_partition = np.asarray(row_partition, dtype=np.int64)
        self.col_partition = np.asarray(col_partition, dtype=np.int64)
        self.A = A_dev
        self.backend = backend

    @property
    def shape(self):
        return int(self.row_partition[-1]), int(self.A.shape[1])

    def __matmul__(self, x):
        from .sparse import HPCSparseMatrix
        from .vectors import HPCVector
        if isinstance(x, HPCVector):
            return dense_matvec(self, x)
        if isinstance(x, HPCSparseMatrix):
            return dense_sparse_matmat(self, x)
        return NotImplemented

    def __mul__(self, other):
        """``A * x`` or ``A * a`` (scalar: src/dense.jl:1317-1327, 1818-1838), on the device."""
        if isinstance(other, (int, float, np.floating, np.integer)):
            return self._scaled(float(other), divide=False)
        return self.__matmul__(other)

    def __rmul__(self, a):
        if isinstance(a, (int, float, np.floating, np.integer)):
            return self._scaled(float(a), divide=False)
        return NotImplemented

    def __truediv__(self, a):
        return self._scaled(float(a), divide=True)

    def _scaled(self, a: float, divide: bool) -> "HPCMatrix":
        from .vectors import rd16, sfx_of
        src = rd16(self.A if self.A.is_contiguous() else self.A.contiguous())     # the vector kernels' 16-byte accesses
        out = _torch().empty_like(src)
        if divide:
            _capi.call(f"hpcla_divide_{sfx_of(self.backend)}", dptr(src), a, dptr(out), src.numel(), current_stream_ptr())
        else:
            _capi.call(f"hpcla_scale_{sfx_of(self.backend)}", a, dptr(src), dptr(out), src.numel(), current_stream_ptr())
        return HPCMatrix(self.row_partition, self.col_partition, out, self.backend)

    def norm(self, p: float = 2) -> float:
        """``norm(A, p)`` (src/dense.jl:1399-1420): the entries as one long vector (p = 2: Frobenius)."""
        from .vectors import HPCVector, norm as vnorm
        flat = (self.A if self.A.is_contiguous() else self.A.contiguous()).view(-1)
        sizes = comm_allgather(self.backend.comm, np.array([flat.numel()], dtype=np.int64))
        part = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        return vnorm(HPCVector(compute_partition_hash(part), part, flat, self.backend), p)

    def __getitem__(self, key):
        """``A[:, k]`` (src/indexing.jl:385-393): column k (0-based here) as an HPCVector on A's row
        partition -- the operand of the reference's SpMM column loop.  Stays on the device.  Two ranges,
        ``A[r0:r1, c0:c1]`` and the ``:`` forms (src/indexing.jl:300-369), give the block as an HPCMatrix (indexing.py)."""
        from .vectors import HPCVector
        if not (isinstance(key, tuple) and len(key) == 2 and key[0] == slice(None) and isinstance(key[1], (int, np.integer))):
            if isinstance(key, tuple) and len(key) == 2 and isinstance(key[0], slice) and isinstance(key[1], slice):
                from .indexing import dense_getitem
                return dense_getitem(self, key)
            raise TypeError("HPCMatrix indexing supports A[:, k] and A[rows, cols] with unit-step ranges only")
        k, n = int(key[1]), int(self.A.shape[1])
        if k < 0 or k >= n:
            raise IndexError(f"HPCMatrix column index out of bounds: k={k}, ncols={n}")
        return HPCVector(compute_partition_hash(self.row_partition), self.row_partition,
                         self.A[:, k].contiguous(), self.backend)

    def local_values(self) -> np.ndarray:
        return self.A.detach().cpu().numpy()

    def gather(self) -> np.ndarray:
        """``Matrix(A)`` (src/HPCLinearAlgebra.jl:840-880): parity checks only."""
        from .backends import CommSerial, _dist, _host_device
        loc = self.local_values()
        comm = self.backend.comm
        if isinstance(comm, CommSerial):
            return loc
        torch = _torch()
        dev = _host_device(comm)
        sizes = np.diff(self.row_partition)
        nmax, k = int(sizes.max()), loc.shape[1]
        pad = torch.zeros((nmax, k), dtype=self.A.dtype, device=dev)
        pad[:loc.shape[0]] = torch.from_numpy(loc).to(dev)
        outs = [torch.empty_like(pad) for _ in range(comm_size(comm))]
        _dist().all_gather(outs, pad, group=comm.group)
        return np.concatenate([o[:int(s)].cpu().numpy() for o, s in zip(outs, sizes)], axis=0)

    @classmethod
    def from_global(cls, M, backend: HPCBackend, row_partition=None, col_partition=None):
        """``HPCMatrix(M, backend; row_partition, col_partition)`` (src/dense.jl:185-201)."""
        torch = _torch()
        M = np.asarray(M, dtype=backend.T)
        nranks, rank = comm_size(backend.comm), comm_rank(backend.comm)
        if row_partition is None:
            row_partition = uniform_partition(M.shape[0], nranks)
        if col_partition is None:
            col_partition = uniform_partition(M.shape[1], nranks)
        lo, hi = int(row_partition[rank]), int(row_partition[rank + 1])
        loc = torch.from_numpy(np.ascontiguousarray(M[lo:hi, :])).to(backend.torch_device)
        return cls(row_partition, col_partition, loc, backend)


def HPCMatrix_local(A_local, backend: HPCBackend, col_partition=None) -> HPCMatrix:
    """src/dense.jl:125-156: row partition inferred by Allgather of ``[nrows, ncols]``."""
    torch = _torch()
    if isinstance(A_local, np.ndarray):
        A_local = torch.from_numpy(np.ascontiguousarray(A_local, dtype=backend.T))
    from .vectors import torch_dtype_of
    A_local = A_local.to(device=backend.torch_device, dtype=torch_dtype_of(backend)).contiguous()
    nranks = comm_size(backend.comm)
    info = comm_allgather(backend.comm, np.array(list(A_local.shape), dtype=np.int64)).reshape(nranks, 2)
    if not np.all(info[:, 1] == info[0, 1]):                       # src/dense.jl:139-143
        raise ValueError("HPCMatrix_local: All ranks must have the same number of columns. "
                         f"Got column counts: {info[:, 1].tolist()}")
    row_partition = np.concatenate([[0], np.cumsum(info[:, 0])]).astype(np.int64)
    if col_partition is None:
        col_partition = uniform_partition(int(A_local.shape[1]), nranks)
    return HPCMatrix(row_partition, col_partition, A_local, backend)


# ---- dense A * x (src/dense.jl:397-658) -------------------------------------------
_dense_vector_plan_cache: Dict[tuple, object] = {}


def clear_dense_plan_cache() -> None:
    for halo, _ghost in _dense_vector_plan_cache.values():
        if halo:
            _capi.call("hpcla_halo_plan_destroy", halo)
    _dense_vector_plan_cache.clear()
    _dense_transpose_cache.clear()


def _dense_vector_plan(A: HPCMatrix, x):
    """DenseMatrixVectorPlan (src/dense.jl:424-538): every rank needs the WHOLE of x, so each rank
    sends its slice to all others.  Memoized on (A's partitions, x's partition) like
    _dense_vector_plan_cache (src/dense.jl:596-606).  Returns (halo plan, its ghost buffer): NULL handles on one rank."""
    backend = A.backend
    rank, nranks = comm_rank(backend.comm), comm_size(backend.comm)
    key = (compute_partition_hash(A.row_partition), compute_partition_hash(A.col_partition), x.structural_hash)
    if key in _dense_vector_plan_cache:
        return _dense_vector_plan_cache[key]
    halo, ghost = ctypes.c_void_p(), ctypes.c_void_p()
    if nranks > 1:
        others = [r for r in range(nranks) if r != rank]
        n_own = int(x.partition[rank + 1] - x.partition[rank])
        sizes = np.diff(x.partition)
        send_to = [r for r in others if n_own > 0]
        recv_from = [r for r in others if sizes[r] > 0]
        halo = create_halo_plan(backend, send_to, [np.arange(n_own)] * len(send_to), np.int64, recv_from,
                                [int(sizes[r]) for r in recv_from], 1)
        ghost, _ = halo_ghost_ptr(halo)                 # a constant of the single-buffered plan
    _dense_vector_plan_cache[key] = (halo, ghost)
    return halo, ghost


def dense_matvec(A: HPCMatrix, x, y=None):
    """``A * x`` / ``mul!(y, A, x)`` for a dense row-partitioned A (src/dense.jl:614-658)."""
    from .vectors import HPCVector, f64_only
    f64_only(A.backend, "dense A*x")
    torch = _torch()
    assert_backends_compatible(A.backend, x.backend)
    backend = A.backend
    rank = comm_rank(backend.comm)
    nloc, ncols = int(A.A.shape[0]), int(A.A.shape[1])
    if int(x.partition[-1]) != ncols:
        raise ValueError(f"dimension mismatch: A has {ncols} columns, x has length {int(x.partition[-1])}")
    if y is None:
        y = HPCVector(compute_partition_hash(A.row_partition), A.row_partition,
                      torch.empty(nloc, dtype=torch.float64, device=backend.torch_device), backend)
    elif y.local_length != nloc:
        raise ValueError("mul!: y has the wrong local length")
    halo, ghost = _dense_vector_plan(A, x)
    s = current_stream_ptr()
    n_lo, n_own = int(x.partition[rank]), int(x.partition[rank + 1] - x.partition[rank])
    n_hi = ncols - n_lo - n_own
    if halo:
        _capi.call("hpcla_halo_begin", halo, dptr(x.v), s)
        _capi.call("hpcla_halo_end", halo, s)
    Ac = A.A if A.A.is_contiguous() else A.A.contiguous()
    x_lo = ghost if n_lo else None
    x_hi = ctypes.c_void_p(ghost.value + 8 * n_lo) if (n_hi and ghost.value) else None
    _capi.call("hpcla_gemv_rowmajor_f64", dptr(Ac), ncols, nloc, x_lo, n_lo, dptr(x.v), n_own, x_hi, n_hi,
               dptr(y.v), s)
    return y


class TransposedHPCMatrix:
    """Lazy ``transpose(A)`` of a dense HPCMatrix (``Transpose(A)``, src/dense.jl:952)."""

    def __init__(self, parent: HPCMatrix):
        self.parent = parent

    @property
    def shape(self):
        m, n = self.parent.shape
        return n, m

    def __matmul__(self, x):
        from .sparse import HPCSparseMatrix
        from .vectors import HPCVector
        if isinstance(x, HPCVector):
            return dense_matvec_t(self.parent, x)
        if isinstance(x, HPCMatrix):
            return dense_matmat_t(self.parent, x)
        if isinstance(x, HPCSparseMatrix):
            return dense_sparse_matmat_t(self.parent, x)
        return NotImplemented

    __mul__ = __matmul__

    def materialize(self) -> HPCMatrix:
        """``copy(transpose(X))`` (src/dense.jl:978): the n x m transpose as an HPCMatrix with rows on ``X.col_partition``
        and columns on ``X.row_partition`` (the reference ``DenseTransposePlan``'s partitions), moved device to device."""
        return _materialize_transpose(self.parent, self.parent.col_partition)


def dense_matvec_t(A: HPCMatrix, x):
    """``transpose(A) * x`` without materialising the transpose (src/dense.jl:1210-1261).  The reference
    gathers x onto A's row partition through a DenseTransposeVectorPlan (CPU-staged), multiplies the
    local block transposed, all-reduces the ncols partial sums on the host and keeps the own column
    slice.  Here: x is aligned to ``A.row_partition`` device to device (repartition.py; a no-op when
    it already is), ``hpcla_gemv_t_rowmajor_f64`` forms the partial column sums, RCCL all-reduces them
    in place, and the own slice of ``A.col_partition`` is the result."""
    from .vectors import f64_only
    f64_only(A.backend, "transpose(A)*x for dense A")
    from .repartition import repartition_vector
    from .vectors import HPCVector
    torch = _torch()
    assert_backends_compatible(A.backend, x.backend)
    backend = A.backend
    rank = comm_rank(backend.comm)
    nloc, ncols = int(A.A.shape[0]), int(A.A.shape[1])
    if int(x.partition[-1]) != int(A.row_partition[-1]):
        raise ValueError(f"dimension mismatch: transpose(A) has {int(A.row_partition[-1])} columns, "
                         f"x has length {int(x.partition[-1])}")
    xa = repartition_vector(x, A.row_partition)
    dev = backend.torch_device
    full = torch.empty(ncols, dtype=torch.float64, device=dev)
    work = torch.empty(max(1, _capi.load().hpcla_gemv_t_work_bytes(nloc, ncols) // 8), dtype=torch.float64, device=dev)
    Ac = A.A if A.A.is_contiguous() else A.A.contiguous()
    s = current_stream_ptr()
    _capi.call("hpcla_gemv_t_rowmajor_f64", dptr(Ac), ncols, nloc, ncols, dptr(xa.v), dptr(full), dptr(work), s)
    _capi.call("hpcla_allreduce_f64", backend.rccl, dptr(full), ncols, 0, s)
    lo, hi = int(A.col_partition[rank]), int(A.col_partition[rank + 1])
    return HPCVector(compute_partition_hash(A.col_partition), A.col_partition.copy(), full[lo:hi].clone(), backend)


def _tensor_layout(A):
    """(tensor, leading dimension, layout) of a 2-D device block for the C ABI: a row-major view on its own row stride, a
    column-major view (a transposed tensor) on its column stride, anything else as one contiguous copy.  The leading
    dimension is at least 1 (the entries check a lower bound only)."""
    n, w = int(A.shape[0]), int(A.shape[1])
    if A.stride(1) == 1 and (n <= 1 or A.stride(0) >= w):
        return A, max(int(A.stride(0)), w, 1), _capi.LAYOUT_ROW
    if A.stride(0) == 1 and (w <= 1 or A.stride(1) >= n):
        return A, max(int(A.stride(1)), n, 1), _capi.LAYOUT_COL
    return A.contiguous(), max(w, 1), _capi.LAYOUT_ROW


def dense_matmat_t(X: HPCMatrix, Y: HPCMatrix) -> HPCMatrix:
    """``transpose(X) * Y`` of two dense row-partitioned blocks (src/dense.jl:1286-1310), the m x k inner-product matrix
    of block methods.  The reference runs k column products ``transpose(X) * Y[:, j]`` (X read k times, k host
    all-reduces); here Y is aligned to ``X.row_partition`` device to device (a no-op when it already is),
    ``hpcla_gram_*`` forms the whole local m x k product in one pass over both blocks (X read once when ``X is Y``, the
    result then exactly symmetric) and all-reduces it in double.  The result is an HPCMatrix on ``X.col_partition``
    rows and ``uniform_partition(k)`` columns; its local block is this rank's rows of the reduced matrix, rounded once
    to the backend's element type."""
    from .repartition import repartition_dense
    from .vectors import sfx_of, torch_dtype_of
    torch = _torch()
    assert_backends_compatible(X.backend, Y.backend)
    backend = X.backend
    nranks, rank = comm_size(backend.comm), comm_rank(backend.comm)
    if int(Y.row_partition[-1]) != int(X.row_partition[-1]):
        raise ValueError(f"dimension mismatch: transpose(X) has {int(X.row_partition[-1])} columns, "
                         f"Y has {int(Y.row_partition[-1])} rows")
    same = Y is X
    if not np.array_equal(Y.row_partition, X.row_partition):
        Y = repartition_dense(Y, X.row_partition)             # device to device (Float64 backends)
    nloc, m, k = int(X.A.shape[0]), int(X.A.shape[1]), int(Y.A.shape[1])
    Xa, ldx, xl = _tensor_layout(X.A)
    Ya, ldy, yl = (Xa, ldx, xl) if same else _tensor_layout(Y.A)
    dev = backend.torch_device
    C = torch.empty((m, k), dtype=torch.float64, device=dev)
    work = torch.empty(max(1, _capi.load().hpcla_gram_work_bytes(nloc, m, k) // 8), dtype=torch.float64, device=dev)
    xp, yp = dptr(Xa), dptr(Ya)
    if nloc == 0:                 # no rows to read: one non-NULL pointer for both says X'X (C mirrored like on the other ranks)
        xp = yp = dptr(C) if same else ctypes.c_void_p(0)
    _capi.call(f"hpcla_gram_{sfx_of(backend)}", backend.rccl, xp, ldx, xl, yp, ldy, yl, nloc, m, k,
               dptr(C), dptr(work), current_stream_ptr())
    lo, hi = int(X.col_partition[rank]), int(X.col_partition[rank + 1])
    loc = C[lo:hi].to(dtype=torch_dtype_of(backend), copy=True)
    return HPCMatrix(X.col_partition.copy(), uniform_partition(k, nranks), loc, backend)


# ---- dense x sparse: transpose(X) * A and X * A (src/sparse.jl:3617-3690) -------------------------------------------------
_dense_transpose_cache: Dict[tuple, object] = {}
_spmm_t_cache: Dict[tuple, "SpmmTPlan"] = {}


def _at(t, offset: int) -> ctypes.c_void_p:
    """Device pointer ``offset`` doubles into the tensor t."""
    return ctypes.c_void_p(t.data_ptr() + 8 * int(offset))


def _transpose_blocks(M, P, Q, backend):
    """The transpose of the row-partitioned block matrix whose local rows are ``M`` (n_me x m, any layout; rows on P):
    this rank's rows ``Q[rank]:Q[rank+1]`` of the m x P[-1] transpose, row-major.  One hpcla_transpose_f64 into the send
    layout, one hpcla_exchange_ranges_f64, one strided placement per source rank (hpcla_transpose_f64 on row-major
    blocks); with one rank the first transpose is the result."""
    from .repartition import exchange_ranges
    from .transpose import DenseTransposeLists
    torch = _torch()
    nranks, rank = comm_size(backend.comm), comm_rank(backend.comm)
    dev = backend.torch_device
    n_me, m = int(M.shape[0]), int(M.shape[1])
    s = current_stream_ptr()
    Ma, ld, lay = _tensor_layout(M)
    T = torch.empty((m, n_me), dtype=torch.float64, device=dev)        # this rank's rows, transposed
    _capi.call("hpcla_transpose_f64", dptr(Ma), ld, lay, dptr(T), max(n_me, 1), _capi.LAYOUT_COL, n_me, m, s)
    if nranks == 1:
        return T
    key = (compute_partition_hash(P), compute_partition_hash(Q), rank)
    L = _dense_transpose_cache.get(key)
    if L is None:
        L = _dense_transpose_cache[key] = DenseTransposeLists(P, Q, rank)
    buf = torch.empty(max(L.n_buf, 1), dtype=torch.float64, device=dev)
    exchange_ranges(backend, T, buf, L.send_ranks, L.send_offsets, L.send_counts, L.recv_ranks, L.recv_offsets,
                    L.recv_counts, L.local_src, L.local_dst, L.local_count, 1)
    out = torch.empty((L.q_me, L.ncols), dtype=torch.float64, device=dev)
    for _q, off, n_q, c0 in L.blocks:
        _capi.call("hpcla_transpose_f64", _at(buf, off), n_q, _capi.LAYOUT_ROW, _at(out, c0), max(L.ncols, 1),
                   _capi.LAYOUT_ROW, L.q_me, n_q, s)
    return out


def _materialize_transpose(X: HPCMatrix, Q) -> HPCMatrix:
    """``copy(transpose(X))`` with its rows on the partition Q of X's columns (``X.col_partition`` for the public
    ``materialize()``; ``A.row_partition`` when X * A needs the transpose aligned with A's rows)."""
    from .repartition import check_partition
    from .vectors import f64_only
    f64_only(X.backend, "copy(transpose(X)) for dense X")
    Q = check_partition(Q, int(X.A.shape[1]), comm_size(X.backend.comm))
    local = _transpose_blocks(X.A, X.row_partition, Q, X.backend)
    return HPCMatrix(Q.copy(), X.row_partition.copy(), local, X.backend)


class SpmmTPlan:
    """Memoised plan of ``transpose(X) * A`` for one sparse structure (key: the structural hash, the column partition and
    the index type): the host lists of ``transpose.HostSpmmTPlan`` and the device CSC of this rank's rows over the split
    column space (``hpcla_spmm_t_struct_*``), in Int32 when the plan narrows an Int64 matrix as the SpMV plans do
    (sparse.can_narrow_indices).  The CSC keeps ``perm``, not values: every call reads the calling matrix's nzval."""

    def __init__(self, A):
        from .sparse import can_narrow_indices, narrowed_rowptr, narrowing_enabled, split_colval
        from .transpose import HostSpmmTPlan
        torch = _torch()
        backend = A.backend
        dev = backend.torch_device
        self.host = h = HostSpmmTPlan(A.col_indices, A.col_partition, backend.comm)
        a64 = A.Ti == np.dtype(np.int64)
        narrowed = bool(a64 and narrowing_enabled() and can_narrow_indices(A.nnz, A.nrows_local, h.n_own, h.n_ghost))
        self.is_i64 = a64 and not narrowed
        if max(h.ncols_split, A.nnz) > np.iinfo(np.int64 if self.is_i64 else np.int32).max:
            raise OverflowError("transpose(X)*A: split column space does not fit the index type")
        sfx = "i64" if self.is_i64 else "i32"
        tdt = torch.int64 if self.is_i64 else torch.int32
        colval_split, _ = split_colval(A, h.cmap, to_i32=narrowed)
        rowptr = narrowed_rowptr(A) if narrowed else A.rowptr_target
        self.colptr = torch.empty(h.ncols_split + 1, dtype=tdt, device=dev)
        self.rowidx = torch.empty(max(A.nnz, 1), dtype=tdt, device=dev)
        self.perm = torch.empty(max(A.nnz, 1), dtype=tdt, device=dev)
        wb = int(_capi.load().hpcla_spmm_t_struct_work_bytes(A.nnz, h.ncols_split, int(self.is_i64)))
        if wb < 0:
            raise _capi.HPCLAError("hpcla_spmm_t_struct_work_bytes", wb, "sort workspace query failed")
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        _capi.call(f"hpcla_spmm_t_struct_{sfx}", dptr(rowptr), dptr(colval_split), A.nrows_local, A.nnz, h.ncols_split,
                   dptr(self.colptr), dptr(self.rowidx), dptr(self.perm), dptr(work), wb, current_stream_ptr())
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
        self.acc = (up(h.acc_rows), up(h.acc_ptr), up(h.acc_pos)) if len(h.acc_rows) else None
        del work, colval_split                       # (stream-ordered frees: the build has been queued before them)


def _spmm_t_plan(A) -> SpmmTPlan:
    from .sparse import narrowing_enabled
    key = (A._ensure_hash(), compute_partition_hash(A.col_partition), str(A.Ti), narrowing_enabled())
    plan = _spmm_t_cache.get(key)
    if plan is None:
        plan = _spmm_t_cache[key] = SpmmTPlan(A)
    return plan


def _spmm_t(Xloc, Q, A) -> HPCMatrix:
    """``transpose(X) * A`` for X's local rows ``Xloc`` (A.nrows_local x m, any layout) aligned with A's rows: an m x n
    HPCMatrix with rows on the partition Q of m and columns on ``uniform_partition(n)``.  One rank: the product writes
    the result block itself (column-major W = the row-major m x n block).  N > 1: W row-major over the split column space,
    its ghost rows sent back to their owners, the owners' rows completed in ascending rank order
    (``hpcla_spmm_t_accumulate_f64``), then this rank's rows of the transpose collected (``_transpose_blocks``)."""
    from .repartition import exchange_ranges
    torch = _torch()
    backend = A.backend
    nranks = comm_size(backend.comm)
    dev = backend.torch_device
    nloc, m, n = int(Xloc.shape[0]), int(Xloc.shape[1]), int(A.shape[1])
    if nloc != A.nrows_local:
        raise ValueError("transpose(X)*A: X's local rows do not match A's")
    plan = _spmm_t_plan(A)
    h = plan.host
    s = current_stream_ptr()
    Xa, ldx, xl = _tensor_layout(Xloc)
    if xl == _capi.LAYOUT_COL and nloc > 0 and m > 0:   # the product reads X as rows: one conversion
        rows = torch.empty((nloc, m), dtype=torch.float64, device=dev)
        _capi.call("hpcla_transpose_f64", dptr(Xa), ldx, xl, dptr(rows), m, _capi.LAYOUT_ROW, nloc, m, s)
        Xa, ldx, xl = rows, m, _capi.LAYOUT_ROW
    sfx = "i64" if plan.is_i64 else "i32"

    def product(W, ldw, layout):
        _capi.call(f"hpcla_spmm_t_f64_{sfx}", dptr(plan.colptr), dptr(plan.rowidx), dptr(plan.perm), dptr(A.nzval),
                   h.ncols_split, dptr(Xa) if nloc else None, ldx, xl, m, dptr(W), ldw, layout, s)
    if nranks == 1:
        out = torch.empty((m, n), dtype=torch.float64, device=dev)
        product(out, max(n, 1), _capi.LAYOUT_COL)
        return HPCMatrix(np.asarray(Q, dtype=np.int64).copy(), uniform_partition(n, 1), out, backend)
    W = torch.empty((h.ncols_split, m), dtype=torch.float64, device=dev)
    product(W, max(m, 1), _capi.LAYOUT_ROW)
    if m > 0:
        R = torch.empty((max(h.n_recv, 1), m), dtype=torch.float64, device=dev)
        exchange_ranges(backend, W, R, h.back_ranks, h.back_offsets, h.back_counts, h.from_ranks, h.from_offsets,
                        h.from_counts, 0, 0, 0, m)
        if plan.acc is not None:
            rows_d, ptr_d, pos_d = plan.acc
            _capi.call("hpcla_spmm_t_accumulate_f64", dptr(W), m, dptr(R), m, dptr(rows_d), dptr(ptr_d), dptr(pos_d),
                       int(rows_d.numel()), m, s)
    local = _transpose_blocks(W[:h.n_own], A.col_partition, Q, backend)
    return HPCMatrix(np.asarray(Q, dtype=np.int64).copy(), uniform_partition(n, nranks), local, backend)


def dense_sparse_matmat_t(X: HPCMatrix, A) -> HPCMatrix:
    """``transpose(X) * A`` for a dense X (p x m) and a sparse A (p x n) (src/sparse.jl:3660-3690): the m x n product
    with rows on ``X.col_partition`` (as ``transpose(A) * b`` returns ``A.col_partition``) and columns on
    ``uniform_partition(n)``.  The reference loops over the n columns of A (a sparse column extraction, a mat-vec with
    its own all-reduce and a host copy each); here one transposed SpMM over this rank's rows (``hpcla_spmm_t_f64_*``: A^T X
    from A's own rows, no A^T) plus, with N > 1, the reverse halo.  X on another row partition is aligned with
    ``repartition_dense`` first."""
    from .repartition import repartition_dense
    from .vectors import f64_only
    f64_only(A.backend, "transpose(X)*A for sparse A")
    assert_backends_compatible(X.backend, A.backend)
    if int(X.row_partition[-1]) != int(A.row_partition[-1]):
        raise ValueError(f"dimension mismatch: transpose(X) has {int(X.row_partition[-1])} columns, "
                         f"A has {int(A.row_partition[-1])} rows")
    if not np.array_equal(X.row_partition, A.row_partition):
        X = repartition_dense(X, A.row_partition)                # device to device
    return _spmm_t(X.A, X.col_partition, A)


def dense_sparse_matmat(X: HPCMatrix, A) -> HPCMatrix:
    """``X * A`` for a dense X (m x p) and a sparse A (p x n) (src/sparse.jl:3617-3652): the m x n product with rows on
    ``X.row_partition`` and columns on ``uniform_partition(n)``, computed as ``transpose(transpose(X)) * A`` -- the
    transpose of X materialised straight onto ``A.row_partition`` (no second repartition pass), then the transposed
    SpMM."""
    from .vectors import f64_only
    f64_only(A.backend, "X*A for sparse A")
    assert_backends_compatible(X.backend, A.backend)
    if int(X.A.shape[1]) != int(A.row_partition[-1]):
        raise ValueError(f"dimension mismatch: X has {int(X.A.shape[1])} columns, A has {int(A.row_partition[-1])} rows")
    Xt = _materialize_transpose(X, A.row_partition)
    return _spmm_t(Xt.A, X.row_partition, A)
