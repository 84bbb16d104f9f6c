"""ilu0(): the fine-grained incomplete LU factorisation of a square ``A`` as a preconditioner for ``hp.gmres`` and ``hp.bicgstab``.

The classical ILU(0) is a sequential factorisation and two sparse triangular solves per application; neither fits a device
whose kernels never wait on one another.  The fine-grained form does (csrc/ilu.hip):

* the factors come from Chow-Patel sweeps: every stored entry of ``L`` (unit lower, strict part stored) and ``U`` is updated at
  once from the previous sweep's values, ``s = a_ij - sum_{k < min(i, j)} l_ik u_kj``, ``l_ij = s / u_jj``, ``u_ij = s``, starting
  from ``l_ij = a_ij / a_jj``, ``u_ij = a_ij``;
* the two triangular solves are replaced by truncated Jacobi iterations (Anzt, Chow, Dongarra): ``z = N_U(N_L(r))`` with
  ``N_L(r) = sum_{k <= solve_sweeps} (-L_strict)^k r`` and ``N_U(y) = sum_{k <= solve_sweeps} (-D^-1 U_strict)^k D^-1 y``.  That is
  a fixed linear operator, so plain (non-flexible) GMRES and BiCGStab stay valid.

The pattern is the part of A's rows whose columns this rank owns, so neither the setup nor the application communicates: across
ranks this is block-Jacobi ILU, and the iteration count depends on the partition.

Limits: Float64, ``gmres`` and ``bicgstab`` only, no fill (level 0), fewer than 2^31 owned entries per rank.  The sweeps
converge for the diagonally dominant matrices tested; they are not guaranteed to converge for an arbitrary ``A``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _capi
from .sparse import HPCSparseMatrix, get_vector_plan
from .vectors import HPCVector, current_stream_ptr, dptr, f64_only

MAX_SWEEPS = 64
MAX_SOLVE_SWEEPS = 16
_NO_DIAG, _BAD_DIAG, _BAD_PIVOT = 1, 2, 3


def _torch():
    import torch
    return torch


def check_arguments(T, shape, row_partition, col_partition, sweeps=3, solve_sweeps=3) -> None:
    """The argument rules, on host values only: ``T`` the element type, ``shape`` and the partitions A's."""
    if np.dtype(T) != np.dtype(np.float64):
        raise TypeError("ilu0: offered for Float64 backends only")
    if int(shape[0]) != int(shape[1]):
        raise ValueError(f"ilu0: the matrix must be square, got {shape[0]} x {shape[1]}")
    if not np.array_equal(np.asarray(row_partition), np.asarray(col_partition)):
        raise ValueError("ilu0: A's rows and columns must be partitioned alike")
    if not 1 <= int(sweeps) <= MAX_SWEEPS:
        raise ValueError(f"ilu0: sweeps must be in 1..{MAX_SWEEPS}, got {sweeps}")
    if not 1 <= int(solve_sweeps) <= MAX_SOLVE_SWEEPS:
        raise ValueError(f"ilu0: solve_sweeps must be in 1..{MAX_SOLVE_SWEEPS}, got {solve_sweeps}")


def error_message(code: int, global_row: int, sweeps: int) -> str:
    if code == _NO_DIAG:
        return f"ilu0: row {global_row} stores no diagonal"
    if code == _BAD_DIAG:
        return f"ilu0: the diagonal of row {global_row} is zero or NaN"
    return f"ilu0: the pivot of row {global_row} is zero or not finite after {sweeps} sweeps"


class ILU0:
    """``z = N_U(N_L(r))`` on the factors of this rank's owned block.  ``sweeps``, ``solve_sweeps``: as given to ``ilu0``;
    ``nnz``: the block's stored entries; ``lanes``: lanes per row of the triangular sweep (1, 2, 4 or 8)."""

    def __init__(self, A: HPCSparseMatrix, sweeps: int, solve_sweeps: int):
        self.shape = tuple(int(v) for v in A.shape)
        self.row_partition = np.array(A.row_partition, dtype=np.int64)
        self.backend = A.backend
        self.sweeps, self.solve_sweeps = int(sweeps), int(solve_sweeps)
        self.lanes = 1
        self.n = int(A.nrows_local)
        self.nnz = 0
        self.row_start = 0
        self._t = None

    # -- setup --------------------------------------------------------------------------------------------------------------------
    def _structure(self, A: HPCSparseMatrix) -> None:
        """The owned block's CSR and its column-wise view: two launches, one read-back (the entry count), one stable sort."""
        from .backends import comm_rank
        torch = _torch()
        dev = self.backend.torch_device
        n = self.n
        self.row_start = int(A.row_partition[comm_rank(self.backend.comm)])
        x = HPCVector.zeros(A.col_partition, self.backend)         # the partition the plans are keyed by
        plan = get_vector_plan(A, x)
        sfx = "i64" if plan.is_i64 else "i32"
        s = current_stream_ptr()
        lib = _capi.load()
        i32 = dict(dtype=torch.int32, device=dev)
        self._info = torch.zeros(2, dtype=torch.int64, device=dev)
        self._rowptr = torch.zeros(n + 1, **i32)
        work = torch.empty(max(lib.hpcla_ilu_work_bytes(n) // 8, 1), dtype=torch.int64, device=dev)
        structure = (dptr(plan.rowptr_of(A)), dptr(plan.colval_split))
        _capi.call(f"hpcla_ilu_count_f64_{sfx}", *structure, n, plan.n_own, 0, dptr(self._rowptr), dptr(self._info), dptr(work), s)
        nnz = int(self._info[0].item())
        if nnz >= 2 ** 31:
            raise NotImplementedError("ilu0: the owned block needs fewer than 2^31 stored entries")
        self.nnz = nnz
        self._cols, self._rows = torch.zeros(nnz, **i32), torch.zeros(nnz, **i32)
        self._diag = torch.full((n,), -1, **i32)
        self._map = torch.zeros(nnz, dtype=torch.int64, device=dev)
        _capi.call(f"hpcla_ilu_fill_f64_{sfx}", *structure, dptr(A.nzval), n, plan.n_own, 0, dptr(self._rowptr), dptr(self._cols),
                   dptr(self._rows), dptr(self._diag), dptr(self._map), dptr(self._info), s)
        # the entries of column j in ascending row: positions are row-major, so a stable sort by column keeps the rows ascending
        cols = self._cols.to(torch.int64)
        self._cpos = torch.sort(cols, stable=True).indices.to(torch.int32)
        self._cptr = torch.zeros(n + 1, **i32)
        if n:
            self._cptr[1:] = torch.cumsum(torch.bincount(cols, minlength=n), 0).to(torch.int32)
        f64 = dict(dtype=torch.float64, device=dev)
        self._a = torch.zeros(nnz, **f64)
        self._f, self._g = torch.zeros(nnz, **f64), torch.zeros(nnz, **f64)
        self._dinv = torch.zeros(n, **f64)

    def _check_diagonal(self) -> None:
        """The fill's test of the stored diagonals (zero or NaN: code 2) on the values just gathered, for ``update``: the fill
        saw the first matrix's values only.  Every row stores its diagonal, or the build had raised.  Leaves the error word at
        the smallest failing row's, or at all ones; enqueues only."""
        torch = _torch()
        d = self._a[self._diag.to(torch.int64)]
        rows = torch.arange(self.n, dtype=torch.int64, device=d.device)
        words = torch.where((d == 0) | (d != d), (rows << 2) | _BAD_DIAG, torch.full_like(rows, 2 ** 62))
        word = words.min()
        self._info[1:2] = torch.where(word < 2 ** 62, word, torch.full_like(word, -1))

    def _factor(self, A: HPCSparseMatrix, new_values: bool = False) -> None:
        """Values, the initial guess, the sweeps, the pivots: enqueued in a row; then the one read-back of the error word."""
        from .backends import comm_allgather
        s = current_stream_ptr()
        n, nnz = self.n, self.nnz
        index = (dptr(self._cols), dptr(self._rows), dptr(self._diag))
        _capi.call("hpcla_ilu_gather_f64", dptr(A.nzval), dptr(self._map), nnz, dptr(self._a), s)
        if new_values and n:
            self._check_diagonal()
        _capi.call("hpcla_ilu_init_f64", *index, dptr(self._a), nnz, dptr(self._f), s)
        for _ in range(self.sweeps):
            _capi.call("hpcla_ilu_sweep_f64", dptr(self._rowptr), *index, dptr(self._cptr), dptr(self._cpos), dptr(self._a),
                       dptr(self._f), dptr(self._g), nnz, s)
            self._f, self._g = self._g, self._f
        _capi.call("hpcla_ilu_pivots_f64", dptr(self._diag), dptr(self._f), n, dptr(self._dinv), dptr(self._info), s)
        word = int(self._info[1].item())
        mine = [0, 0] if word == -1 else [word & 3, self.row_start + (word >> 2)]
        every = comm_allgather(self.backend.comm, np.array(mine, dtype=np.int64)).reshape(-1, 2)
        failed = every[every[:, 0] != 0]
        if len(failed):
            row, code = min((int(r), int(c)) for c, r in failed)
            raise ValueError(error_message(code, row, self.sweeps))

    def update(self, A: HPCSparseMatrix) -> "ILU0":
        """New values of ``A`` on the structure this object was built for: one gather and the sweeps, no index work.  Raises as
        ``ilu0`` does, a zero or NaN diagonal among the new values included; the object can be updated again afterwards."""
        if tuple(int(v) for v in A.shape) != self.shape or not np.array_equal(A.row_partition, self.row_partition) \
                or int(A.nrows_local) != self.n or int(A.nnz) < self.nnz:
            raise ValueError("ilu0: update needs a matrix with the structure the factors were built for")
        self._info[1:2].fill_(-1)                                  # the error word, as the count leaves it
        self._factor(A, new_values=True)
        return self

    # -- application ------------------------------------------------------------------------------------------------------------
    def _enqueue(self, r_ptr: int, out_ptr: int) -> None:
        """``out = N_U(N_L(r))`` on raw device pointers of ``n`` doubles (the solvers pass basis columns)."""
        if self._t is None:
            torch = _torch()
            self._t = torch.zeros((2, max(self.n, 1)), dtype=torch.float64, device=self.backend.torch_device)
        _capi.call("hpcla_ilu_apply_f64", dptr(self._rowptr), dptr(self._cols), dptr(self._diag), dptr(self._f), dptr(self._dinv),
                   r_ptr, dptr(self._t[0]), dptr(self._t[1]), out_ptr, self.n, self.solve_sweeps, self.lanes, current_stream_ptr())

    def apply(self, r: HPCVector, out: Optional[HPCVector] = None) -> HPCVector:
        """``out = N_U(N_L(r))``; r on A's row partition.  Enqueues only."""
        if int(r.partition[-1]) != self.shape[0] or r.local_length != self.n:
            raise ValueError("ilu0: r must be partitioned like the rows of A")
        out = r.similar() if out is None else out
        if out.local_length != self.n:
            raise ValueError("ilu0: out must be partitioned like r")
        if self.n:
            self._enqueue(dptr(r.v), dptr(out.v))
        return out

    def factors(self):
        """Host copies ``(rowptr, local columns, L/U values, row_start)`` of this rank's block: CSR with ascending columns; an
        entry below the diagonal is ``l_ij`` (the unit diagonal of L is not stored), the others are ``u_ij``."""
        return (self._rowptr.cpu().numpy().astype(np.int64), self._cols.cpu().numpy().astype(np.int64),
                self._f.cpu().numpy().copy(), self.row_start)


def ilu0(A: HPCSparseMatrix, sweeps: int = 3, solve_sweeps: int = 3) -> ILU0:
    """Build the fine-grained ILU(0) preconditioner of ``A`` for ``hp.gmres(A, b, M=hp.ilu0(A))`` and ``hp.bicgstab``.

    ``sweeps`` (1..64) Chow-Patel sweeps build the factors on the entries of A whose column this rank owns; ``solve_sweeps``
    (1..16) Jacobi sweeps stand for each triangular solve of an application.  The pattern need not be structurally symmetric.
    Raises ValueError when a row stores no diagonal, when a stored diagonal is zero or NaN, or when a pivot ``u_ii`` is zero or
    not finite after the last sweep; the message names the global row and every rank raises together."""
    f64_only(A.backend, "ilu0")
    check_arguments(A.backend.T, A.shape, A.row_partition, A.col_partition, sweeps, solve_sweeps)
    M = ILU0(A, sweeps, solve_sweeps)
    M._structure(A)
    M._factor(A)
    return M
