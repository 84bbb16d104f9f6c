"""Extreme eigenpairs of a symmetric ``A`` (``hp.eigsh``): thick-restart Lanczos with full reorthogonalisation.

The other question next to ``A x = b``: the largest or smallest eigenvalues of a symmetric ``A`` and their vectors -- a condition
number, a spectral bound for a smoother, a Fiedler vector, vibration modes, the ``sigma`` of ``A - sigma I`` that ``hp.minres`` is
documented for.  The reference has no eigensolver; a caller of its operators composes Lanczos from ``A*p``
(src/sparse.jl:2096-2128), ``dot`` (src/vectors.jl:798-812) and broadcast updates (src/vectors.jl:1203-1226): with twice-applied
classical Gram-Schmidt the step that orthogonalises against ``c`` basis columns is ``2c`` dots, ``2c`` axpys and ``2c + 1`` host
read-backs, and the restart is a dense product plus a copy back.  Here a step is one SpMV and the fused GMRES kernels of
csrc/vecops.hip (``gmres_dots``, ``gmres_update``, ``gmres_next``) with a Lanczos small step that keeps the projected matrix
(``hpcla_eigsh_update_f64``); the host enqueues a whole cycle in one library call (``hpcla_eigsh_steps_f64_*``, csrc/solvers.hip) and reads back
once per cycle; the restart compresses the basis in place in one pass (``hpcla_eigsh_rotate_f64``, csrc/eigsh.hip).

Thick-restart Lanczos (Wu and Simon; for symmetric ``A`` it is Krylov-Schur).  ``m = ncv``, ``j`` counts columns inside a cycle,
``p`` is the number of columns the last restart kept (0 in the first cycle).  Gate order and rounding order
(tests/_eigsh_cases.py restates them):

    start          V_0 = v0 / sqrt(v0.v0)
    step j = p..m-1
                   w = A V_j
                   h1 = V_{0..j}^T w;  w = w - V h1
                   h2 = V_{0..j}^T w;  w = w - V h2;  nn = w.w
                   gate N  nn != nn: "breakdown", nothing of column j is stored
                   T[i, j] = h1[i] + h2[i] for i <= j;  beta[j] = hn = sqrt(nn)
                   gate I  nn == 0: "invariant", column j is stored
                   V_{j+1} = w / hn
    cycle end      the host reads T, beta and the state (the cycle's one read-back) and builds the symmetric T: the upper
                   triangle from the device's columns p..m-1, diag(theta_kept) in the top-left p x p, the lower triangle the
                   mirror (after a restart the device's own dots recompute the arrow column p: nothing is uploaded for it)
                   theta, S = numpy.linalg.eigh(T);  the k wanted Ritz values by ``which``
                   rho_i = |beta[m-1] S[m-1, i]|;  anorm = max |theta|;  converged when every wanted rho_i <= tol anorm
                   "maxiter" at the first cycle end with iterations >= maxiter
                   restart: keep p = k + (m - k) // 2 Ritz pairs (the wanted ones and the next in the same ordering),
                   V[:, 0:p] <- V[:, 0:m] S_p in place, V_p <- V_m (one launch)
    end            X = V[:, 0:c] S[:, wanted], written straight into the row-major block of the HPCMatrix
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from . import _capi
from .backends import comm_bcast_bytes, comm_rank, comm_size
from .partition import compute_partition_hash, uniform_partition
from .sparse import get_vector_plan
from .vectors import HPCVector, current_stream_ptr, dptr, f64_only, norm, rd16_vector

_BREAKDOWN, _INVARIANT = 2, 4                               # the device's statuses next to 0 = running: include/hpcla_rocm.h
_SMALL = ("T", "beta", "h1", "h2", "nn", "hn")
MAX_NCV = 64
WHICH = ("LA", "SA", "LM")


def _torch():
    import torch
    return torch


@dataclass
class EigshInfo:
    """What ``eigsh`` reports.  ``iterations`` counts Lanczos steps (one SpMV each), ``residual_norms`` holds the estimates
    ``|beta_m S[m-1, i]|`` of ``||A x_i - vals_i x_i||`` aligned with ``vals``, ``history`` the largest wanted estimate at
    every cycle end, ``anorm`` the largest ``|theta|`` of the last cycle (the norm the stop rule is relative to)."""
    converged: bool
    status: str
    iterations: int
    restarts: int
    residual_norms: np.ndarray
    history: List[float] = field(default_factory=list)
    anorm: float = 0.0


# ---- the host's part: pure numpy ---------------------------------------------------------------------------------------------
def check_arguments(n: int, k, which, ncv, maxiter) -> Tuple[int, int, int]:
    """The argument rules that need no device.  Returns (k, ncv, maxiter)."""
    if which in ("SM", "BE") or which not in WHICH:
        if which == "SM":
            raise ValueError("eigsh: which='SM' is not offered: interior and smallest-magnitude pairs need shift-invert, and this "
                             "package has no factorisation for it (which: 'LA', 'SA' or 'LM')")
        raise ValueError(f"eigsh: which must be 'LA', 'SA' or 'LM', got {which!r}")
    k = int(k)
    if k < 1:
        raise ValueError(f"eigsh: k must be at least 1, got {k}")
    if ncv is None:
        ncv = min(n, MAX_NCV, max(2 * k + 1, 20))
    ncv = int(ncv)
    if not k + 1 <= ncv <= min(MAX_NCV, n):
        raise ValueError(f"eigsh: ncv must satisfy k + 1 <= ncv <= min({MAX_NCV}, n) = {min(MAX_NCV, n)}, got k = {k}, ncv = {ncv}")
    maxiter = 10 * n if maxiter is None else int(maxiter)
    if maxiter < 0:
        raise ValueError("eigsh: maxiter must be non-negative")
    return k, ncv, maxiter


def wanted_order(theta: np.ndarray, which: str) -> np.ndarray:
    """Indices of the Ritz values, the most wanted first.  Ties (``"LM"``: ``|theta|`` equal) go to the larger algebraic value,
    then to the lower index, so the order is a function of the values alone."""
    theta = np.asarray(theta, dtype=np.float64)
    idx = np.arange(len(theta))
    if which == "LA":
        return np.lexsort((idx, -theta))
    if which == "SA":
        return np.lexsort((idx, theta))
    if which == "LM":
        return np.lexsort((idx, -theta, -np.abs(theta)))
    raise ValueError(f"eigsh: which must be 'LA', 'SA' or 'LM', got {which!r}")


def kept_count(k: int, m: int) -> int:
    """Ritz pairs a restart keeps: the k wanted and half of the rest, k <= p < m."""
    return k + (m - k) // 2


def assemble_T(T_dev: np.ndarray, theta_kept: np.ndarray, p: int, c: int) -> np.ndarray:
    """The symmetric c x c projected matrix.  ``T_dev[j]`` is the device's column j (entries 0..j); columns p..c-1 give the upper
    triangle, diag(theta_kept) the top-left p x p, the lower triangle mirrors the upper."""
    T = np.zeros((c, c))
    q = min(p, c)
    T[np.arange(q), np.arange(q)] = theta_kept[:q]
    for j in range(p, c):
        T[:j + 1, j] = T_dev[j, :j + 1]
    return np.triu(T) + np.triu(T, 1).T


def estimates(beta_last: float, S: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """rho_i = |beta[c-1] S[c-1, i]| for the Ritz pairs idx."""
    return np.abs(beta_last * S[-1, idx])


def select(theta: np.ndarray, S: np.ndarray, beta_last: float, k: int, which: str):
    """The (at most) k wanted pairs in ascending order of the value: (indices, vals, rho, anorm)."""
    order = wanted_order(theta, which)[:k]
    order = order[np.lexsort((order, theta[order]))]
    anorm = float(np.max(np.abs(theta))) if len(theta) else 0.0
    return order, theta[order].copy(), estimates(beta_last, S, order), anorm


# ---- the workspace -------------------------------------------------------------------------------------------------------------
class EigshWorkspace:
    """What an ``eigsh`` solve allocates: ``ncv + 1`` basis columns at a pitch rounded up to an even number of doubles (every
    column is then 16-byte aligned even when the local length is odd), w, the small arrays (T, beta, h1, h2, nn, hn in one
    buffer), the scratch of the gated kernels whose last 32 bytes are the solve's device state (done_iter, status), and the device
    copy of S (at most 64 x 64).  Reusable: every solve resets all of it."""

    def __init__(self, b_like: HPCVector, ncv: int = 20):
        torch = _torch()
        lib = _capi.load()
        f64_only(b_like.backend, "eigsh")
        ncv = int(ncv)
        if not 1 <= ncv <= MAX_NCV:
            raise ValueError(f"eigsh: ncv must be in 1..{MAX_NCV}, got {ncv}")
        f64 = dict(dtype=torch.float64, device=b_like.v.device)
        self.ncv = ncv
        self.w = b_like.similar()
        self.ldv = b_like.local_length + (b_like.local_length & 1)
        self.V = torch.zeros((ncv + 1) * self.ldv, **f64)
        self.small = torch.zeros(lib.hpcla_eigsh_small_offset(ncv, len(_SMALL)), **f64)
        self.work = torch.zeros(lib.hpcla_gmres_work_bytes(ncv) // 8, **f64)
        self.state = self.work[-4:].view(torch.int64)                  # done_iter, status, not used, reserved
        self.S = torch.zeros(ncv * ncv, **f64)

    def fits(self, b: HPCVector, ncv: int) -> bool:
        return self.ncv == ncv and self.w.structural_hash == b.structural_hash and self.w.v.device == b.v.device

    def small_array(self, name: str):
        """A view of one of the small arrays (T, beta, h1, h2, nn, hn)."""
        lib = _capi.load()
        i = _SMALL.index(name)
        return self.small[lib.hpcla_eigsh_small_offset(self.ncv, i):lib.hpcla_eigsh_small_offset(self.ncv, i + 1)]


def _rotate(ws: EigshWorkspace, n_loc: int, S_cols: np.ndarray, move_last: bool, out=None) -> None:
    """Upload S (c x q, column j contiguous on the device) and make the one rotate launch: in place, or into ``out`` (row-major)."""
    torch = _torch()
    c, q = S_cols.shape
    ws.S[:c * q].copy_(torch.from_numpy(np.ascontiguousarray(S_cols.T).reshape(-1)))
    if out is None:
        _capi.call("hpcla_eigsh_rotate_f64", dptr(ws.V), ws.ldv, c, q, dptr(ws.S), int(move_last), None, 0, 0, n_loc,
                   current_stream_ptr())
    else:
        _capi.call("hpcla_eigsh_rotate_f64", dptr(ws.V), ws.ldv, c, q, dptr(ws.S), 0, dptr(out), q, 1, n_loc, current_stream_ptr())


def _block(A, local):
    """The local rows of X as an HPCMatrix on A's row partition."""
    from .dense import HPCMatrix
    return HPCMatrix(A.row_partition, uniform_partition(int(local.shape[1]), comm_size(A.backend.comm)), local, A.backend)


def eigsh(A, k: int = 6, which: str = "LA", ncv: Optional[int] = None, tol: float = 1e-10, maxiter: Optional[int] = None,
          v0: Optional[HPCVector] = None, seed: int = 0, return_eigenvectors: bool = True,
          workspace: Optional[EigshWorkspace] = None):
    """The ``k`` largest (``which="LA"``), smallest (``"SA"``) or largest-magnitude (``"LM"``) eigenvalues of a symmetric ``A``
    and their vectors, by thick-restart Lanczos with full reorthogonalisation.  The caller asserts the symmetry; it is not
    checked.  Returns ``(vals, X, info)``: ``vals`` is a numpy array of the wanted eigenvalues in ascending order, ``X`` an
    ``n x k`` HPCMatrix on A's row partition whose column i belongs to ``vals[i]`` (``None`` with
    ``return_eigenvectors=False``), ``info`` an :class:`EigshInfo`.

    ``ncv`` is the number of basis columns per cycle, ``k + 1 <= ncv <= min(64, n)`` (default ``min(n, 64, max(2k + 1, 20))``);
    a cycle keeps ``ncv + 1`` columns of the local length.  ``v0`` is an HPCVector on A's row partition; the default is
    ``numpy.random.default_rng(seed).uniform(-1, 1, n)`` over the global length, each rank taking its slice, so the start does
    not depend on the number of ranks.  ``"SM"`` and ``"BE"`` raise ``ValueError``: interior and smallest-magnitude pairs need
    shift-invert, and this package has no factorisation for it.

    Stops at the first cycle end where every wanted estimate ``|beta_m S[m-1, i]| <= tol * anorm`` with ``anorm`` the largest
    ``|theta|`` of the cycle (relative to the matrix norm, so an eigenvalue at or near 0 can converge); as ``"maxiter"`` at the
    first cycle end with ``iterations >= maxiter`` (default ``10 n``; cycles are never cut short); as ``"invariant"`` when the
    new Lanczos vector is exactly zero -- the Ritz pairs of the ``c`` finished columns are then exact, the solve is converged
    when ``c >= k`` and otherwise returns the ``c`` pairs found with ``converged=False``; as ``"breakdown"`` on a NaN (``vals``
    is then NaN and ``X`` zero).

    Limits.  The gates are exact-zero and NaN tests, as everywhere in this package.  Single-vector Lanczos finds ONE vector per
    distinct eigenvalue: a multiple eigenvalue is returned once, and the copies it misses are replaced by the next distinct
    values.  The square 16 x 16 Poisson grid has ``lambda_ij = lambda_ji``; a ``k = 4`` run returns a wrong set there while
    every residual is within ``tol``.  A block method is the remedy: ``hp.lobpcg`` (lobpcg.py) finds a multiple eigenvalue with
    its multiplicity.

    The host reads back once per cycle and never inside one.  With N ranks every rank computes the same T from all-reduced
    values; still only rank 0's decision and rank 0's S are used (broadcast), so no rank leaves the loop alone and no two ranks
    rotate with an S that differs in a bit."""
    torch = _torch()
    f64_only(A.backend, "eigsh")
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"eigsh: the matrix must be square, got {A.shape[0]} x {A.shape[1]}")
    n = int(A.shape[0])
    k, m, maxiter = check_arguments(n, k, which, ncv, maxiter)
    if not tol >= 0:
        raise ValueError("eigsh: tol must be non-negative")
    if v0 is None:
        v0 = HPCVector.from_global(np.random.default_rng(seed).uniform(-1.0, 1.0, n), A.backend, partition=A.row_partition)
    elif not isinstance(v0, HPCVector) or v0.structural_hash != compute_partition_hash(A.row_partition):
        raise ValueError("eigsh: v0 must be an HPCVector partitioned like the rows of A")
    v0 = rd16_vector(v0)                                         # the start kernel reads it 16 bytes at a time
    ws = workspace if workspace is not None and workspace.fits(v0, m) else EigshWorkspace(v0, m)
    plan = get_vector_plan(A, ws.w)
    if plan.result_partition_hash != ws.w.structural_hash:
        raise ValueError("eigsh: the columns of A must be partitioned like its rows")
    comm, rank0 = A.backend.rccl, comm_rank(A.backend.comm) == 0
    n_loc = ws.w.local_length
    sfx = "i64" if plan.is_i64 else "i32"
    blk = plan.matrix_block(A)
    spmv = (blk[0], comm, *blk[1:])

    # -- start: V_0 = v0 / sqrt(v0.v0) ---------------------------------------------------------------------------------------------
    ws.small.zero_()
    ws.work.zero_()                                              # done_iter = 0, status = running
    ws.V.zero_()
    ws.w.v.zero_()
    hn = ws.small_array("hn")
    norm(v0, 2, out=hn)                                          # the all-reduced sum of squares; the square root is the caller's
    hn.sqrt_()
    _capi.call("hpcla_gmres_next_f64", dptr(v0.v), dptr(hn), None, dptr(ws.V), None, n_loc, dptr(ws.state), current_stream_ptr())

    iterations = restarts = p = 0
    theta_kept = np.zeros(0)
    history: List[float] = []
    nbytes = 8 * (3 + m + m * m)
    while True:
        _capi.call(f"hpcla_eigsh_steps_f64_{sfx}", *spmv, dptr(ws.V), ws.ldv, dptr(ws.w.v), dptr(ws.small), dptr(ws.work), m, p,
                   m - p, iterations + 1, current_stream_ptr())
        payload = None
        if rank0:                                                # the cycle's one read-back, the projected problem, the decision
            host = torch.cat([ws.small, ws.work[-4:]]).cpu().numpy()
            done, status = (int(v) for v in host[-4:-2].view(np.int64))
            c = m if status == 0 else p + (done - iterations)
            packed = np.zeros(3 + m + m * m)
            if status != _BREAKDOWN and c >= 1:
                T = assemble_T(host[:m * m].reshape(m, m), theta_kept, p, c)
                if np.all(np.isfinite(T)):
                    theta, S = np.linalg.eigh(T)
                    packed[2] = host[m * m + c - 1]              # beta[c-1]
                    packed[3:3 + c] = theta
                    packed[3 + m:3 + m + c * c] = S.reshape(-1)
                else:
                    status = _BREAKDOWN
            packed[0], packed[1] = status, c
            payload = packed.tobytes()
        packed = np.frombuffer(comm_bcast_bytes(A.backend.comm, payload, nbytes), dtype=np.float64)
        status, c, beta_last = int(packed[0]), int(packed[1]), float(packed[2])
        if status == _BREAKDOWN:                                 # gate N: maybe the poison of an expired exchange wait -- ask
            from .sparse import check_exchange_health
            check_exchange_health(A.backend)
            X = _block(A, torch.zeros((n_loc, k), dtype=torch.float64, device=ws.V.device)) if return_eigenvectors else None
            return np.full(k, np.nan), X, EigshInfo(False, "breakdown", iterations + max(c - p, 0), restarts, np.full(k, np.nan),
                                                    history, float("nan"))
        iterations += c - p
        theta, S = packed[3:3 + c].copy(), packed[3 + m:3 + m + c * c].reshape(c, c).copy()
        idx, vals, rho, anorm = select(theta, S, beta_last, k, which)
        history.append(float(rho.max()))
        if status == _INVARIANT:
            converged, name = c >= k, "invariant"
        elif bool(np.all(rho <= tol * anorm)):
            converged, name = True, "converged"
        elif iterations >= maxiter:
            converged, name = False, "maxiter"
        else:                                                    # restart: the wanted pairs and the next in the same ordering
            p = kept_count(k, m)
            keep = wanted_order(theta, which)[:p]
            theta_kept = theta[keep].copy()
            _rotate(ws, n_loc, S[:, keep], move_last=True)
            restarts += 1
            continue
        X = None
        if return_eigenvectors:
            out = torch.zeros((n_loc, len(idx)), dtype=torch.float64, device=ws.V.device)
            _rotate(ws, n_loc, S[:, idx], move_last=False, out=out)
            X = _block(A, out)
        return vals, X, EigshInfo(converged, name, iterations, restarts, rho, history, anorm)
