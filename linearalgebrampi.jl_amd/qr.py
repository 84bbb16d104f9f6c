"""Tall-skinny Householder QR of a dense row-partitioned block (``hp.qr``) and dense least squares on it (``hp.lstsq``).

``X`` is an ``n x k`` HPCMatrix, ``1 <= k <= 32``, ``n >= k``.  The factorisation is a communication-avoiding Householder QR
(TSQR, csrc/qr.hip): panels of ``PANEL_ROWS`` rows are factored independently, their ``k x k`` triangles are stacked ``fan(k)``
at a time and factored again until one triangle is left; with N ranks every rank's triangle goes into one all-reduced
``(N k) x k`` stack that every rank factors redundantly with the same code, so ``R`` has the same bits on every rank.  ``Q`` is
formed by applying the stored reflectors top down to ``[D; 0]``, ``D = sign(diag R)``: it is orthonormal to rounding whatever
the condition number of ``X`` is -- a Gram/Cholesky orthonormalisation loses ``kappa^2 eps``, ``X inv(R)`` loses ``kappa eps``.
The reference has no QR of an HPCMatrix; composed from its operators (src/dense.jl:1286-1310) the job is CholQR.

    launches   one factor launch per level, one all-reduce (N > 1), one sign kernel, one form-Q launch per level
    read-back  R: k^2 doubles, once
    bytes      32 n k with Q (read X, write the reflectors into the Q buffer, read them, write Q); 8 n k with mode="r"

``hp.lstsq`` factors the augmented block ``[X b]`` with ``mode="r"``: with ``R_aug = [[R, z], [0, rho]]`` the minimiser of
``||X c - b||`` is ``c = R \\ z`` and the residual norm is ``|rho|``.  No ``Q`` is formed and ``X`` is passed over once.

Everything above :func:`qr` is plain Python and numpy, importable without a device: the argument rules and the shape of the
tree (levels and nodes per level).  The constants mirror the library's (``hpcla_qr_panel_rows``, ``hpcla_qr_fan``).
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

MAX_K = 32                      # the widest block: a lane keeps a row of k doubles in registers
PANEL_ROWS = 256                # rows of a level-0 panel (hpcla_qr_panel_rows)
MODES = ("reduced", "r")


# ---- the host's part: no device ------------------------------------------------------------------------------------------------
def fan(k: int) -> int:
    """Triangles a node of an upper level stacks (``hpcla_qr_fan``): ``PANEL_ROWS / KT``, ``KT`` the register tile 4, 8, 16 or 32."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"qr: k must be in 1..{MAX_K}, got {k}")
    return PANEL_ROWS // (4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else 32)


def tree_levels(rows: int, k: int) -> List[int]:
    """Nodes per level, bottom up, of the tree over a matrix of ``rows`` rows: ``ceil(rows / PANEL_ROWS)`` panels, then
    ``fan(k)`` triangles per node until one node is left.  No rows: no levels."""
    f = fan(k)
    if rows <= 0:
        return []
    nodes = [-(-int(rows) // PANEL_ROWS)]
    while nodes[-1] > 1:
        nodes.append(-(-nodes[-1] // f))
    return nodes


def tree_shape(n_loc: int, k: int, nranks: int = 1) -> Tuple[List[int], int, List[int]]:
    """The shape of a factorisation: (nodes per level of this rank's tree, rows of the rank stack, nodes per level of the stack's
    tree).  One rank has no stack: ``(levels, 0, [])``."""
    nranks = int(nranks)
    if nranks < 1:
        raise ValueError("qr: nranks must be positive")
    stack_rows = nranks * int(k) if nranks > 1 else 0
    return tree_levels(n_loc, k), stack_rows, tree_levels(stack_rows, k)


def check_arguments(n: int, k, mode: str = "reduced", m: int = 0, what: str = "qr") -> int:
    """The argument rules that need no device: ``mode``, ``1 <= k``, ``k + m <= 32`` (``m`` right-hand sides), ``n >= k``.
    Returns ``k``."""
    if mode not in MODES:
        raise ValueError(f"{what}: mode must be 'reduced' or 'r', got {mode!r}")
    k, m = int(k), int(m)
    if k < 1 or k + m > MAX_K:
        if m:
            raise ValueError(f"{what}: needs 1 <= k and k + m <= {MAX_K} (columns of X plus right-hand sides), got k = {k}, m = {m}")
        raise ValueError(f"{what}: k must be in 1..{MAX_K}, got {k}")
    if int(n) < k:
        raise ValueError(f"{what}: needs n >= k rows, got n = {int(n)}, k = {k}")
    return k


def solve_augmented(R_aug: np.ndarray, k: int):
    """``(C, rnorms)`` from the ``(k + m) x (k + m)`` triangle of ``[X B]``: ``C = R \\ Z`` by back-substitution, ``rnorms[j]``
    the 2-norm of column ``j`` of the trailing ``m x m`` triangle.  Raises ``ValueError("lstsq: X is rank deficient")`` when
    ``min |r_ii| <= k eps max |r_ii|`` over the X part (zero counts as deficient)."""
    R_aug = np.asarray(R_aug, dtype=np.float64)
    R, Z, T = R_aug[:k, :k], R_aug[:k, k:], R_aug[k:, k:]
    d = np.abs(np.diag(R))
    if d.min() <= k * np.finfo(np.float64).eps * d.max():
        raise ValueError("lstsq: X is rank deficient")
    C = np.zeros_like(Z)
    for i in range(k - 1, -1, -1):
        C[i] = (Z[i] - R[i, i + 1:] @ C[i + 1:]) / R[i, i]
    return C, np.sqrt(np.sum(T * T, axis=0))


# ---- the device's part ---------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _factor(backend, Xa, ld: int, n_loc: int, k: int, want_q: bool):
    """One ``hpcla_qr_f64`` on the rows ``Xa`` (row-major on the pitch ``ld``).  Returns (Q's local block or None, R on the host)."""
    from . import _capi
    from .backends import comm_size
    from .vectors import current_stream_ptr, dptr
    torch = _torch()
    lib = _capi.load()
    f64 = dict(dtype=torch.float64, device=backend.torch_device)
    nranks = comm_size(backend.comm)
    # a rank without rows still passes a Q pointer: NULL means "R only" to the library
    Q = torch.empty((max(n_loc, 1), k), **f64) if want_q else None
    R = torch.empty((k, k), **f64)
    work = torch.empty(max(1, lib.hpcla_qr_work_bytes(n_loc, k, nranks, int(want_q)) // 8), **f64)
    _capi.call("hpcla_qr_f64", backend.rccl, dptr(Xa) if n_loc else None, ld, n_loc, k, dptr(Q), k, dptr(R), dptr(work),
               current_stream_ptr())
    return (Q[:n_loc] if want_q else None), R.cpu().numpy()          # the call's only read-back


def _row_major(A, k: int):
    """(tensor, pitch): a row-major block on any pitch >= k is read in place (a column range of a wider buffer included);
    anything else goes through one contiguous copy."""
    from . import _capi
    from .dense import _tensor_layout
    Xa, ld, layout = _tensor_layout(A)
    if layout != _capi.LAYOUT_ROW:
        Xa, ld = A.contiguous(), max(k, 1)
    return Xa, ld


def qr(X, mode: str = "reduced"):
    """``Q, R = hp.qr(X)``; ``R = hp.qr(X, mode="r")``.  ``X`` is an ``n x k`` Float64 HPCMatrix, ``1 <= k <= 32``, ``n >= k``
    over all ranks (a rank may hold fewer than ``k`` rows, or none).

    ``Q`` is a new HPCMatrix on X's partitions (row-major local block on pitch ``k``; ``X`` is not modified) with ``Q'Q = I`` to
    rounding whatever the condition number, a rank-deficient or zero ``X`` included: the leading ``k`` columns of the
    accumulated Householder reflectors.  ``R`` is a host ``(k, k)`` float64 array, upper triangular with exact zeros below the
    diagonal and a non-negative diagonal (the signs are folded into ``Q``), the same bits on every rank.  ``mode="r"`` stores no
    reflectors and makes no second pass.

    Limits.  Float64 only; ``k <= 32``; no pivoting.  Column norms are plain sums of squares: entries beyond about ``1e154`` in
    magnitude overflow.  Non-finite input raises nothing: the NaNs propagate into ``R`` and ``Q``.  The bits depend on the rows
    per rank and ``k``: two partitions of the same ``X`` agree to rounding, not to the bit."""
    from .dense import HPCMatrix
    from .vectors import f64_only
    if not isinstance(X, HPCMatrix):
        raise TypeError("qr: X must be an HPCMatrix")
    f64_only(X.backend, "qr")
    n, k = X.shape
    k = check_arguments(n, k, mode)
    n_loc = int(X.A.shape[0])
    Xa, ld = _row_major(X.A, k)
    Q, R = _factor(X.backend, Xa, ld, n_loc, k, mode == "reduced")
    if mode == "r":
        return R
    return HPCMatrix(X.row_partition.copy(), X.col_partition.copy(), Q, X.backend), R


def lstsq(X, b):
    """``c, rnorm = hp.lstsq(X, b)``: the minimiser of ``||X c - b||_2`` for a tall dense ``X`` (``n x k``) and an HPCVector
    ``b``, and the residual norm.  ``C, rnorms = hp.lstsq(X, B)`` for an HPCMatrix ``B`` of ``m`` columns, ``k + m <= 32``.
    ``b`` on another partition than X's rows is repartitioned.  ``c`` is an HPCVector on ``X.col_partition`` (as
    ``hp.transpose(X) @ b`` returns), ``C`` an HPCMatrix with its rows on ``X.col_partition``; ``rnorm`` a float, ``rnorms`` a
    numpy array.

    One QR of the augmented block ``[X b]`` with ``mode="r"`` (one device copy builds it; ``X`` is passed over once, no ``Q``),
    then a host back-substitution.  Raises ``ValueError("lstsq: X is rank deficient")`` when ``min |r_ii| <= k eps max |r_ii|``
    on the diagonal of the unpivoted ``R`` of ``X``.  Limits as for :func:`qr`."""
    from .backends import assert_backends_compatible, comm_rank, comm_size
    from .dense import HPCMatrix
    from .partition import compute_partition_hash, uniform_partition
    from .repartition import repartition_dense, repartition_vector
    from .vectors import HPCVector, f64_only
    torch = _torch()
    if not isinstance(X, HPCMatrix):
        raise TypeError("lstsq: X must be an HPCMatrix")
    f64_only(X.backend, "lstsq")
    single = isinstance(b, HPCVector)
    if not single and not isinstance(b, HPCMatrix):
        raise TypeError("lstsq: b must be an HPCVector or an HPCMatrix")
    assert_backends_compatible(X.backend, b.backend)
    f64_only(b.backend, "lstsq")
    n, k = X.shape
    m = 1 if single else int(b.A.shape[1])
    if m < 1:
        raise ValueError("lstsq: B needs at least one column")
    k = check_arguments(n, k, "r", m, what="lstsq")
    nb = int(b.partition[-1]) if single else int(b.row_partition[-1])
    if nb != n:
        raise ValueError(f"dimension mismatch: X has {n} rows, b has {nb}")
    if single:
        rhs = repartition_vector(b, X.row_partition).v.view(-1, 1)
    else:
        rhs = repartition_dense(b, X.row_partition).A
    backend = X.backend
    n_loc = int(X.A.shape[0])
    aug = torch.cat((X.A, rhs), dim=1)                           # the one device copy: (n_loc, k + m), row-major
    _, R_aug = _factor(backend, aug, k + m, n_loc, k + m, False)
    C, rnorms = solve_augmented(R_aug, k)
    rank, nranks = comm_rank(backend.comm), comm_size(backend.comm)
    lo, hi = int(X.col_partition[rank]), int(X.col_partition[rank + 1])
    loc = torch.from_numpy(np.ascontiguousarray(C[lo:hi])).to(backend.torch_device)
    if single:
        c = HPCVector(compute_partition_hash(X.col_partition), X.col_partition.copy(), loc[:, 0].contiguous(), backend)
        return c, float(rnorms[0])
    return HPCMatrix(X.col_partition.copy(), uniform_partition(m, nranks), loc, backend), rnorms
