"""Range indexing on DeviceROCm: ``v[a:b]``, ``X[r, c]``, ``A[r, c]`` and ``A[:, k]`` (reference: src/indexing.jl:79-121,
300-393, 691-914).

Semantics are the reference's, restated for the 0-based layer: keys are ``slice`` objects with step ``None`` or 1, half-open;
``None`` bounds mean the ends; explicit bounds must satisfy ``0 <= start <= stop <= n`` (IndexError otherwise: the reference
errors on an out-of-bounds range, it does not clamp).  Negative bounds, other steps and other key types are a TypeError.  Every
form is collective -- all ranks pass the same key -- and none communicates: the result's row partition is the intersection
of every rank's rows with the range (``subpartition``), its column partition ``uniform_partition(width, nranks)``.  An empty
range gives the reference's empty object, whose ROW partition is ``uniform_partition(nrows, nranks)`` for the matrices
(src/indexing.jl:318-325, 709-724).

Vectors and dense blocks are tensor slices copied on the device.  The sparse forms run csrc/submatrix.hip: locate and mark,
two scans, one coalesced fill (``A[r, c]``), or one look-up per row (``A[:, k]``); nothing of the matrix visits the host.
``SubmatrixPlan`` keeps an extraction's structure and source map so that cutting the same block out of another matrix of the
same structure is the values pass alone.
"""
from __future__ import annotations

import ctypes
from typing import Tuple

import numpy as np

from . import _capi
from .backends import comm_rank, comm_size, require_device
from .partition import compute_partition_hash, local_window, subpartition, uniform_partition
from .vectors import HPCVector, current_stream_ptr, dptr


def _torch():
    import torch
    return torch


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def parse_range(key, n: int, what: str) -> Tuple[int, int]:
    """``key`` (a slice with step None or 1) as the half-open range ``(start, stop)`` of ``[0, n]``."""
    if not isinstance(key, slice):
        raise TypeError(f"{what}: a range key must be a slice, got {type(key).__name__}")
    if key.step is not None and not (_is_int(key.step) and int(key.step) == 1):
        raise TypeError(f"{what}: only unit-step ranges are supported, got step {key.step!r}")
    for b in (key.start, key.stop):
        if b is not None and not _is_int(b):
            raise TypeError(f"{what}: range bounds must be integers, got {b!r}")
        if b is not None and int(b) < 0:
            raise TypeError(f"{what}: negative bounds are not supported, got {b!r}")
    start = 0 if key.start is None else int(key.start)
    stop = int(n) if key.stop is None else int(key.stop)
    if start > stop or stop > n:
        raise IndexError(f"{what} range out of bounds: {start}:{stop}, length={n}")
    return start, stop


def _two_ranges(key, shape, what: str):
    if not (isinstance(key, tuple) and len(key) == 2):
        raise TypeError(f"{what} indexing takes two keys: [rows, cols]")
    return parse_range(key[0], shape[0], f"{what} row"), parse_range(key[1], shape[1], f"{what} column")


# -- v[a:b] (src/indexing.jl:79-121) ----------------------------------------------------------------------------------
def vector_getitem(v: HPCVector, key) -> HPCVector:
    start, stop = parse_range(key, len(v), "HPCVector")
    part = subpartition(v.partition, start, stop)                 # an empty range: all-empty partition (:90-95)
    lo, hi = local_window(v.partition, comm_rank(v.backend.comm), start, stop)
    return HPCVector(compute_partition_hash(part), part, v.v[lo:hi].clone(), v.backend)


# -- X[r, c] (src/indexing.jl:300-369) --------------------------------------------------------------------------------
def dense_getitem(X, key):
    from .dense import HPCMatrix
    (r0, r1), (c0, c1) = _two_ranges(key, X.shape, "HPCMatrix")
    comm = X.backend.comm
    rank, nranks = comm_rank(comm), comm_size(comm)
    col_part = uniform_partition(c1 - c0, nranks)
    if r0 == r1 or c0 == c1:                                      # :318-325
        row_part = uniform_partition(r1 - r0, nranks)
        block = X.A.new_empty((int(row_part[rank + 1] - row_part[rank]), c1 - c0))
        return HPCMatrix(row_part, col_part, block, X.backend)
    lo, hi = local_window(X.row_partition, rank, r0, r1)
    block = X.A[lo:hi, c0:c1].clone(memory_format=_torch().contiguous_format)       # always a copy, row-major
    return HPCMatrix(subpartition(X.row_partition, r0, r1), col_part, block, X.backend)


# -- A[r, c] (src/indexing.jl:691-855) --------------------------------------------------------------------------------
def _col_indices_dev(A):
    """A's global column ids on the device (structure, uploaded once per matrix; device-built matrices have it already)."""
    ci = getattr(A, "_col_indices_dev", None)
    if ci is None:
        ci = A._col_indices_dev = _torch().from_numpy(np.ascontiguousarray(A.col_indices, dtype=np.int64)).to(A.backend.torch_device)
    return ci


def _empty_sparse(A, nrows_local: int, row_part, col_part):
    from .sparse import HPCSparseMatrix
    torch = _torch()
    dev = A.backend.torch_device
    out = HPCSparseMatrix(row_part, col_part, np.empty(0, dtype=np.int64), None, None,
                          torch.empty(0, dtype=A.nzval.dtype, device=dev),
                          torch.zeros(nrows_local + 1, dtype=A.rowptr_target.dtype, device=dev), A.backend)
    out._colval_target = torch.empty(0, dtype=A.rowptr_target.dtype, device=dev)
    out._col_indices_dev = torch.empty(0, dtype=torch.int64, device=dev)
    return out


def _extract(A, r0: int, r1: int, c0: int, c1: int):
    """The extraction proper.  Returns (B, src_start, lo): the result, the per-row source starts (device int64; None for
    the empty forms) and this rank's first selected local row."""
    from .sparse import HPCSparseMatrix
    require_device(A.backend, "A[rows, cols]")
    torch = _torch()
    comm = A.backend.comm
    rank, nranks = comm_rank(comm), comm_size(comm)
    col_part = uniform_partition(c1 - c0, nranks)
    if r0 == r1 or c0 == c1:                                      # :709-724: the empty matrix has a UNIFORM row partition
        row_part = uniform_partition(r1 - r0, nranks)
        return _empty_sparse(A, int(row_part[rank + 1] - row_part[rank]), row_part, col_part), None, 0
    row_part = subpartition(A.row_partition, r0, r1)
    lo, hi = local_window(A.row_partition, rank, r0, r1)
    nsel = hi - lo
    # col_indices is sorted: the global window [c0, c1) is the window [j0, j1) of compressed local columns
    j0, j1 = (int(j) for j in np.searchsorted(A.col_indices, [c0, c1], side="left"))
    width = j1 - j0
    dev = A.backend.torch_device
    sfx = "i64" if A.Ti == np.dtype(np.int64) else "i32"
    tdt = A.rowptr_target.dtype
    s = current_stream_ptr()
    lib = _capi.load()
    work = torch.empty(lib.hpcla_submatrix_work_bytes(nsel, width), dtype=torch.uint8, device=dev)
    src_start = torch.empty(nsel, dtype=torch.int64, device=dev)
    rowptr_out = torch.empty(nsel + 1, dtype=tdt, device=dev)
    col_indices_out = torch.empty(width, dtype=torch.int64, device=dev)
    colval_src = A.colval_target()
    nnz_out, ncomp = ctypes.c_int64(), ctypes.c_int64()
    _capi.call(f"hpcla_submatrix_structure_{sfx}", dptr(A.rowptr_target), dptr(colval_src), A.nrows_local, A.nnz, lo, hi, j0, j1,
               0, dptr(_col_indices_dev(A)) if width else None, c0, dptr(src_start), dptr(rowptr_out), dptr(col_indices_out),
               ctypes.byref(nnz_out), ctypes.byref(ncomp), dptr(work), s)
    colval_out = torch.empty(nnz_out.value, dtype=tdt, device=dev)
    nzval_out = torch.empty(nnz_out.value, dtype=A.nzval.dtype, device=dev)
    _capi.call(f"hpcla_submatrix_fill_{sfx}", A.nzval.element_size(), dptr(colval_src), dptr(A.nzval), A.nnz, dptr(src_start),
               dptr(rowptr_out), nsel, nnz_out.value, j0, j1, 0, dptr(work), dptr(colval_out), dptr(nzval_out), s)
    # the kept columns that occur; a short list does not keep the window-sized buffer alive
    ci_dev = col_indices_out if ncomp.value == width else col_indices_out[:ncomp.value].clone()
    B = HPCSparseMatrix(row_part, col_part, ci_dev.cpu().numpy(), None, None, nzval_out, rowptr_out, A.backend)
    B._colval_target = colval_out
    B._col_indices_dev = ci_dev
    return B, src_start, lo


def sparse_column(A, k: int) -> HPCVector:
    """``A[:, k]`` (src/indexing.jl:872-914): the stored value of (i, k), +0.0 where nothing is stored, on A's row partition."""
    require_device(A.backend, "A[:, k]")
    torch = _torch()
    n = A.shape[1]
    if k < 0 or k >= n:
        raise IndexError(f"HPCSparseMatrix column index out of bounds: k={k}, ncols={n}")
    jk = int(np.searchsorted(A.col_indices, k, side="left"))
    out = torch.zeros(A.nrows_local, dtype=A.nzval.dtype, device=A.backend.torch_device)
    if jk < len(A.col_indices) and int(A.col_indices[jk]) == k and A.nrows_local > 0:
        sfx = "i64" if A.Ti == np.dtype(np.int64) else "i32"
        _capi.call(f"hpcla_sparse_column_{sfx}", A.nzval.element_size(), dptr(A.rowptr_target), dptr(A.colval_target()),
                   dptr(A.nzval), A.nrows_local, A.nnz, jk, 0, dptr(out), current_stream_ptr())
    return HPCVector(compute_partition_hash(A.row_partition), A.row_partition, out, A.backend)


def diag(A, reciprocal: bool = False) -> HPCVector:
    """``diag(A)``: the main diagonal of a square Float64 HPCSparseMatrix as an HPCVector on ``A.row_partition``, looked up on
    the device (one lane per local row): the stored value bit for bit, +0.0 where nothing is stored.  ``reciprocal=True``
    returns ``1 ./ diag(A)`` from the same pass (``hp.cg``'s Jacobi preconditioner).  Off-diagonals are not offered."""
    from .sparse import HPCSparseMatrix
    if not isinstance(A, HPCSparseMatrix):
        raise ValueError("diag: an HPCSparseMatrix is required")
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"diag: the matrix must be square, got {A.shape[0]} x {A.shape[1]}")
    if A.backend.T != np.dtype(np.float64):
        raise ValueError("diag: offered for Float64 backends only")
    require_device(A.backend, "diag(A)")
    torch = _torch()
    out = torch.zeros(A.nrows_local, dtype=A.nzval.dtype, device=A.backend.torch_device)
    if A.nrows_local > 0:
        sfx = "i64" if A.Ti == np.dtype(np.int64) else "i32"
        ci = _col_indices_dev(A)
        row_start = int(A.row_partition[comm_rank(A.backend.comm)])
        _capi.call(f"hpcla_sparse_diag_f64_{sfx}", dptr(A.rowptr_target), dptr(A.colval_target()), dptr(A.nzval), A.nrows_local,
                   A.nnz, 0, dptr(ci) if A.nnz else None, int(ci.numel()), row_start, int(bool(reciprocal)), dptr(out),
                   current_stream_ptr())
    return HPCVector(compute_partition_hash(A.row_partition), A.row_partition, out, A.backend)


def sparse_getitem(A, key):
    if isinstance(key, tuple) and len(key) == 2 and _is_int(key[1]):
        if not (isinstance(key[0], slice) and key[0] == slice(None)):
            raise TypeError("HPCSparseMatrix: a single column is A[:, k]; a single row or entry is not supported")
        return sparse_column(A, int(key[1]))
    (r0, r1), (c0, c1) = _two_ranges(key, A.shape, "HPCSparseMatrix")
    return _extract(A, r0, r1, c0, c1)[0]


class SubmatrixPlan:
    """``get_submatrix_plan(A, rows, cols)``: the structure of ``A[rows, cols]`` and the map back into A's entries (one source
    start per kept row).  ``extract(A2)``, for any A2 with A's structure, copies the values alone and returns a matrix that
    SHARES the plan's structure arrays and structural hash, so the VectorPlans built over one extraction serve them all.
    An explicit object, not a cache: plain ``A[r, c]`` never hashes A."""

    def __init__(self, A, rows, cols):
        (r0, r1), (c0, c1) = _two_ranges((rows, cols), A.shape, "HPCSparseMatrix")
        self.rows, self.cols = (r0, r1), (c0, c1)
        self.source_hash = A._ensure_hash()
        self.source_nnz = A.nnz
        self.T, self.Ti = A.T, A.Ti
        self.matrix, self._src_start, self._row_lo = _extract(A, r0, r1, c0, c1)
        self.matrix._ensure_hash()                       # shared by every extract() through _with_values

    def extract(self, A2):
        if A2.T != self.T or A2.Ti != self.Ti or A2.nnz != self.source_nnz or A2._ensure_hash() != self.source_hash:
            raise ValueError("SubmatrixPlan.extract: the matrix does not have the structure the plan was built for")
        B = self.matrix
        out = _torch().empty_like(B.nzval)
        if B.nnz:
            sfx = "i64" if self.Ti == np.dtype(np.int64) else "i32"
            _capi.call(f"hpcla_submatrix_values_{sfx}", A2.nzval.element_size(), dptr(A2.nzval), A2.nnz, dptr(self._src_start),
                       dptr(B.rowptr_target), B.nrows_local, B.nnz, 0, dptr(out), current_stream_ptr())
        return B._with_values(out)


def get_submatrix_plan(A, rows=slice(None), cols=slice(None)) -> SubmatrixPlan:
    return SubmatrixPlan(A, rows, cols)
