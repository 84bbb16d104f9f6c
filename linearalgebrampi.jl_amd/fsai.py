"""fsai(): the factorised sparse approximate inverse preconditioner (Kolotilina-Yeremin) of a symmetric positive definite ``A``.

``G`` is sparse lower triangular with ``diag(G A G') = 1`` on a pattern (A's own lower triangle, or the one of a given
``pattern`` matrix), and ``M = G' G`` approximates ``inv(A)``; it is symmetric positive definite by construction.  Applying it
is two SpMVs, ``Gt @ (G @ r)``, on ordinary matrices with ordinary plans; building it is one small dense Cholesky per row,
all rows at once (csrc/fsai.hip).  The pattern is restricted to the columns a rank owns, so neither the setup nor the product
communicates: across ranks this is block-Jacobi FSAI, and the iteration count of ``cg`` depends mildly on the partition.

Limits: Float64, ``cg`` only, at most 32 owned entries per pattern row (the diagonal included), ``A`` symmetric positive
definite -- only the lower triangle of ``A`` is read.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _capi
from .sparse import HPCSparseMatrix, HPCSparseMatrix_local_device, get_vector_plan, mul_
from .vectors import HPCVector, current_stream_ptr, dptr, f64_only

MAX_ROW = 32
_CAP, _NO_DIAG, _NOT_SPD = 1, 2, 3


def _torch():
    import torch
    return torch


def check_arguments(T, shape, row_partition, col_partition, pattern=None) -> None:
    """The argument rules, on host values only: ``T`` the element type, ``shape`` and the partitions A's; ``pattern``, when
    given, the (shape, row_partition, col_partition) of the pattern matrix."""
    if np.dtype(T) != np.dtype(np.float64):
        raise TypeError("fsai: offered for Float64 backends only")
    if int(shape[0]) != int(shape[1]):
        raise ValueError(f"fsai: the matrix must be square, got {shape[0]} x {shape[1]}")
    if not np.array_equal(np.asarray(row_partition), np.asarray(col_partition)):
        raise ValueError("fsai: A's rows and columns must be partitioned alike")
    if pattern is not None:
        pshape, prow, pcol = pattern
        if tuple(int(v) for v in pshape) != tuple(int(v) for v in shape) or not np.array_equal(np.asarray(prow), np.asarray(row_partition)) \
                or not np.array_equal(np.asarray(pcol), np.asarray(col_partition)):
            raise ValueError("fsai: the pattern must have A's shape and partitions")


def error_message(code: int, global_row: int) -> str:
    if code == _CAP:
        return (f"fsai: a pattern row has more than {MAX_ROW} owned entries on or below the diagonal (row {global_row}); "
                "thin the pattern")
    if code == _NO_DIAG:
        return f"fsai: row {global_row} stores no diagonal"
    return f"fsai: A is not positive definite on the pattern of row {global_row}"


class FSAI:
    """``M = Gt G``.  ``G`` and ``Gt`` are HPCSparseMatrix objects on A's partitions, ``max_row`` the largest number of entries
    in a row of ``G`` (over all ranks)."""

    def __init__(self, G: HPCSparseMatrix, Gt: HPCSparseMatrix, max_row: int):
        self.G = G
        self.Gt = Gt
        self.max_row = int(max_row)
        self._u = None

    def apply(self, r: HPCVector, out: Optional[HPCVector] = None) -> HPCVector:
        """``out = Gt @ (G @ r)``; r on A's row partition."""
        if self._u is None or self._u.structural_hash != r.structural_hash or self._u.v.device != r.v.device:
            self._u = r.similar()
        out = r.similar() if out is None else out
        mul_(self._u, self.G, r)
        mul_(out, self.Gt, self._u)
        return out


def fsai(A: HPCSparseMatrix, pattern: Optional[HPCSparseMatrix] = None) -> FSAI:
    """Build the FSAI preconditioner of a symmetric positive definite ``A`` for ``hp.cg(A, b, M=hp.fsai(A))``.

    Row i of ``G`` lives on the columns of pattern row i that this rank owns and that are <= i; the diagonal is always part
    of it.  ``pattern``: an HPCSparseMatrix partitioned like ``A`` whose structure is used instead of A's, for instance
    ``hp.spgemm(A, A)``.  Raises ValueError when a pattern row has more than 32 such entries, when a row of ``A`` stores no
    diagonal, or when ``A`` is not positive definite on a row's pattern (a NaN counts); every rank raises together."""
    from .backends import comm_allgather, comm_rank
    from .transpose import transpose
    f64_only(A.backend, "fsai")
    check_arguments(A.backend.T, A.shape, A.row_partition, A.col_partition,
                    None if pattern is None else (pattern.shape, pattern.row_partition, pattern.col_partition))
    torch = _torch()
    backend = A.backend
    dev = backend.torch_device
    rank = comm_rank(backend.comm)
    row_start = int(A.row_partition[rank])
    n = A.nrows_local
    x = HPCVector.zeros(A.col_partition, backend)                # the partition the plans are keyed by
    plan = get_vector_plan(A, x)
    P, pplan = (A, plan) if pattern is None else (pattern, get_vector_plan(pattern, x))
    if plan.is_i64 != pplan.is_i64:
        raise NotImplementedError("fsai: the plans of A and of the pattern use different index widths")
    sfx = "i64" if plan.is_i64 else "i32"
    s = current_stream_ptr()
    lib = _capi.load()

    g_rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    info = torch.zeros(3, dtype=torch.int64, device=dev)
    work = torch.empty(max(lib.hpcla_fsai_work_bytes(n) // 8, 1), dtype=torch.int64, device=dev)
    structure = (dptr(pplan.rowptr_of(P)), dptr(pplan.colval_split), dptr(plan.rowptr_of(A)), dptr(plan.colval_split))
    _capi.call(f"hpcla_fsai_count_f64_{sfx}", *structure, n, plan.n_own, 0, dptr(g_rowptr), dptr(info), dptr(work), s)
    nnz, max_m = (int(v) for v in info[:2].cpu().tolist())       # the sizes G is allocated by
    g_cols = torch.empty(nnz, dtype=torch.int64, device=dev)
    g_vals = torch.empty(nnz, dtype=torch.float64, device=dev)
    if 1 <= max_m <= MAX_ROW:
        _capi.call(f"hpcla_fsai_factor_f64_{sfx}", *structure, dptr(A.nzval), n, plan.n_own, 0, row_start, max_m,
                   dptr(g_rowptr), dptr(g_cols), dptr(g_vals), dptr(info), s)
    word = int(info[2].item())                                   # the one read-back of the error word
    mine = [0, 0, max_m] if word == -1 else [word & 3, row_start + (word >> 2), max_m]
    every = comm_allgather(backend.comm, np.array(mine, dtype=np.int64)).reshape(-1, 3)
    failed = every[every[:, 0] != 0]
    if len(failed):
        code, row = min((int(r), int(c)) for c, r, _ in failed)[::-1]
        raise ValueError(error_message(code, row))
    window = (row_start, row_start + n - 1) if n > 0 else (0, 0)
    G = HPCSparseMatrix_local_device(g_rowptr, g_cols, g_vals, int(A.shape[1]), backend, col_partition=A.col_partition,
                                     col_window=window)
    Gt = transpose(G).materialize()
    return FSAI(G, Gt, int(every[:, 2].max()))
