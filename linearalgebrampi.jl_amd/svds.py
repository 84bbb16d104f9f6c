"""The largest singular triplets of a rectangular ``A`` (``hp.svds``): thick-restart Golub-Kahan-Lanczos bidiagonalisation.

The truncated SVD next to ``hp.eigsh``: a low-rank approximation of a rectangular ``A``, ``||A||_2`` (the reference's ``opnorm``
offers 1 and Inf only), the numerical rank or condition of a least-squares operator before ``hp.lsqr``, principal components of
a sparse data matrix.  ``hp.eigsh`` on an explicitly formed ``transpose(A) * A`` squares the condition number, costs an SpGEMM
and a denser matrix, and returns no left vectors.  The reference has no SVD (its ``svd`` would be a dense LAPACK call); a caller
of its operators composes the method from ``A*v`` (src/sparse.jl:2096-2128), ``transpose(A)*u`` (src/sparse.jl:2136-2142),
``dot`` (src/vectors.jl:798-812) and broadcast updates (src/vectors.jl:1203-1226): with twice-applied classical Gram-Schmidt on
both sides the step that orthogonalises against ``c`` columns on each side is ``4c`` dots, ``4c`` axpys and ``4c + 2`` host
read-backs, and the restart is two dense products plus their copies back.  Here a step is two SpMVs -- on ``A``'s plan and on
the plan of the materialised, cached ``transpose(A)``, as in ``hp.lsqr`` -- and, per side, the fused GMRES kernels of
csrc/vecops.hip (``gmres_dots``, ``gmres_update``, ``gmres_next``) with a Golub-Kahan small step that keeps the projected
matrix (``hpcla_svds_update_f64``); the host enqueues a whole cycle in one library call (``hpcla_svds_steps_f64_*``, csrc/solvers.hip) and reads
back once per cycle; the restart compresses each basis in place in one pass (``hpcla_eigsh_rotate_f64``, csrc/eigsh.hip).

Thick-restart bidiagonalisation with full two-sided reorthogonalisation (Baglama and Reichel; SLEPc's TRLBD).  ``m = ncv``, ``j``
counts columns inside a cycle, ``p`` is the number of columns the last restart kept (0 in the first cycle).  Gate order and
rounding order (tests/_svds_cases.py restates them):

    start          V_0 = v0 / sqrt(v0.v0)
    step j = p..m-1
      left half    u = A V_j
                   g1 = U_{0..j-1}^T u;  u = u - U g1
                   g2 = U_{0..j-1}^T u;  u = u - U g2;  aa = u.u        (j = 0: the norm alone)
                   gate N  aa != aa: "breakdown", nothing of column j is stored
                   B[i, j] = g1[i] + g2[i] for i < j;  B[j, j] = alpha_j = sqrt(aa)
                   gate Z  aa == 0: "invariant" with c = j finished triplets; column j of B is stored:
                           A V_{0..j} = U_{0..j-1} B[0:j, 0:j+1] and A^T U_{0..j-1} = V_{0..j} B[0:j, 0:j+1]^T hold exactly
                   U_j = u / alpha_j
      right half   v = A^T U_j
                   h1 = V_{0..j}^T v;  v = v - V h1
                   h2 = V_{0..j}^T v;  v = v - V h2;  bb = v.v
                   gate N' bb != bb: "breakdown", beta_j is not stored
                   beta_j = sqrt(bb)
                   gate Z' bb == 0: "invariant" with c = j + 1 finished triplets
                   V_{j+1} = v / beta_j
    cycle end      the host reads B, beta and the state (the cycle's one read-back) and builds the upper-triangular B: the
                   device's columns p..c-1, diag(s_kept) in the top-left p x p (after a restart the device's own dots recompute
                   the arrow column p: nothing is uploaded for it); behind gate Z the c x (c + 1) block with column c
                   P, s, Q = numpy.linalg.svd(B);  the k wanted triplets are the first k (s is descending)
                   rho_i = |beta_{c-1} P[c-1, i]| (0 behind gate Z);  anorm = s[0];  converged when every wanted
                   rho_i <= tol anorm;  "maxiter" at the first cycle end with iterations >= maxiter
                   restart: keep p = k + (m - k) // 2 triplets, V[:, 0:p] <- V[:, 0:m] Q_p in place with V_p <- V_m,
                   U[:, 0:p] <- U[:, 0:m] P_p in place (two launches)
    end            U = U[:, 0:c] P[:, wanted] and V = V[:, 0:c (+1 behind gate Z)] Q[:, wanted], written straight into the
                   row-major blocks of the two HPCMatrix results
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from . import _capi
from .backends import comm_bcast_bytes, comm_rank, comm_size
from .eigsh import kept_count
from .partition import compute_partition_hash, uniform_partition
from .sparse import get_vector_plan
from .transpose import TransposedHPCSparseMatrix
from .vectors import HPCVector, current_stream_ptr, dptr, f64_only, norm, rd16_vector

_BREAKDOWN, _INVARIANT = 2, 4                               # the device's statuses next to 0 = running: include/hpcla_rocm.h
_SMALL = ("B", "beta", "g1", "g2", "h1", "h2", "aa", "bb", "dv")
MAX_NCV = 64


def _torch():
    import torch
    return torch


@dataclass
class SvdsInfo:
    """What ``svds`` reports.  ``iterations`` counts bidiagonalisation steps (one product with ``A`` and one with its transpose
    each), ``residual_norms`` holds the estimates ``|beta_m P[m-1, i]|`` of ``||A' u_i - s_i v_i||`` aligned with ``s`` (the
    other residual ``A v_i - s_i u_i`` is zero up to rounding by construction), ``history`` the largest wanted estimate at every
    cycle end, ``anorm`` the largest singular value of the last cycle's projected matrix (the norm the stop rule is relative
    to)."""
    converged: bool
    status: str
    iterations: int
    restarts: int
    residual_norms: np.ndarray
    history: List[float] = field(default_factory=list)
    anorm: float = 0.0


# ---- the host's part: pure numpy ---------------------------------------------------------------------------------------------
def check_arguments(M: int, N: int, k, which, ncv, maxiter) -> Tuple[int, int, int]:
    """The argument rules that need no device.  Returns (k, ncv, maxiter)."""
    if which != "LM":
        if which == "SM":
            raise ValueError("svds: which='SM' is not offered: the smallest singular values need harmonic Ritz restarts or "
                             "shift-invert, and neither is here (which: 'LM')")
        raise ValueError(f"svds: which must be 'LM', got {which!r}")
    n = min(M, N)
    k = int(k)
    if k < 1:
        raise ValueError(f"svds: k must be at least 1, got {k}")
    if ncv is None:
        ncv = min(n, MAX_NCV, max(2 * k + 1, 20))
    ncv = int(ncv)
    if not k + 1 <= ncv <= min(MAX_NCV, n):
        raise ValueError(f"svds: ncv must satisfy k + 1 <= ncv <= min({MAX_NCV}, M, N) = {min(MAX_NCV, n)}, got k = {k}, "
                         f"ncv = {ncv}")
    maxiter = 10 * n if maxiter is None else int(maxiter)
    if maxiter < 0:
        raise ValueError("svds: maxiter must be non-negative")
    return k, ncv, maxiter


def finished_columns(status: int, done: int, iterations: int, p: int, m: int, beta: np.ndarray) -> Tuple[int, bool]:
    """(c, gate_z) from the device's state: the finished triplets of the cycle, and whether the left half's gate Z stopped it
    (then column c of B is stored too).  Gate Z' leaves beta[c - 1] == 0 behind and c > p; see include/hpcla_rocm.h."""
    if status == 0:
        return m, False
    c = p + (done - iterations)
    if status != _INVARIANT:
        return c, False
    return c, not (c > p and beta[c - 1] == 0.0)


def assemble_B(B_dev: np.ndarray, s_kept: np.ndarray, p: int, c: int, cols: int) -> np.ndarray:
    """The c x cols upper-triangular projected matrix (cols = c, or c + 1 behind gate Z).  ``B_dev[j]`` is the device's column j
    (entries 0..j); columns p..cols-1 come from it, diag(s_kept) is the top-left p x p."""
    B = np.zeros((c, cols))
    q = min(p, c)
    B[np.arange(q), np.arange(q)] = s_kept[:q]
    for j in range(p, cols):
        r = min(j + 1, c)
        B[:r, j] = B_dev[j, :r]
    return B


# ---- the workspace -------------------------------------------------------------------------------------------------------------
class SvdsWorkspace:
    """What an ``svds`` solve allocates: ``ncv`` left basis columns on A's rows and ``ncv + 1`` right basis columns on A's
    columns, each at a pitch rounded up to an even number of doubles (every column is then 16-byte aligned even when the local
    length is odd), u and v, the small arrays (B, beta, g1, g2, h1, h2, aa, bb, dv in one buffer), the scratch of the gated
    kernels whose last 32 bytes are the solve's device state (done_iter, status), and the device copies of P and Q.  Reusable:
    every solve resets all of it."""

    def __init__(self, A, ncv: int = 20):
        torch = _torch()
        lib = _capi.load()
        if isinstance(A, TransposedHPCSparseMatrix):
            A = A.materialize()
        f64_only(A.backend, "svds")
        ncv = int(ncv)
        if not 1 <= ncv <= MAX_NCV:
            raise ValueError(f"svds: ncv must be in 1..{MAX_NCV}, got {ncv}")
        self.ncv = ncv
        self.u = HPCVector.zeros(A.row_partition, A.backend)
        self.v = HPCVector.zeros(A.col_partition, A.backend)
        f64 = dict(dtype=torch.float64, device=self.u.v.device)
        self.ldu = self.u.local_length + (self.u.local_length & 1)
        self.ldv = self.v.local_length + (self.v.local_length & 1)
        self.U = torch.zeros(ncv * self.ldu, **f64)
        self.V = torch.zeros((ncv + 1) * self.ldv, **f64)
        self.small = torch.zeros(lib.hpcla_svds_small_offset(ncv, len(_SMALL)), **f64)
        self.work = torch.zeros(lib.hpcla_gmres_work_bytes(ncv) // 8, **f64)
        self.state = self.work[-4:].view(torch.int64)                  # done_iter, status, not used, reserved
        self.P = torch.zeros(ncv * ncv, **f64)
        self.Q = torch.zeros((ncv + 1) * ncv, **f64)

    def fits(self, A, ncv: int) -> bool:
        if isinstance(A, TransposedHPCSparseMatrix):
            rows, cols, backend = A.parent.col_partition, A.parent.row_partition, A.parent.backend
        else:
            rows, cols, backend = A.row_partition, A.col_partition, A.backend
        return (self.ncv == ncv and self.u.structural_hash == compute_partition_hash(rows)
                and self.v.structural_hash == compute_partition_hash(cols) and self.u.backend is backend)

    def small_array(self, name: str):
        """A view of one of the small arrays (B, beta, g1, g2, h1, h2, aa, bb, dv)."""
        lib = _capi.load()
        i = _SMALL.index(name)
        return self.small[lib.hpcla_svds_small_offset(self.ncv, i):lib.hpcla_svds_small_offset(self.ncv, i + 1)]


def _rotate(basis, ld: int, S_dev, n_loc: int, S_cols: np.ndarray, move_last: bool, out=None) -> None:
    """Upload S (c x q, column j contiguous on the device) and make the one rotate launch: in place, or into ``out`` (row-major)."""
    torch = _torch()
    c, q = S_cols.shape
    S_dev[:c * q].copy_(torch.from_numpy(np.ascontiguousarray(S_cols.T).reshape(-1)))
    if out is None:
        _capi.call("hpcla_eigsh_rotate_f64", dptr(basis), ld, c, q, dptr(S_dev), int(move_last), None, 0, 0, n_loc,
                   current_stream_ptr())
    else:
        _capi.call("hpcla_eigsh_rotate_f64", dptr(basis), ld, c, q, dptr(S_dev), 0, dptr(out), q, 1, n_loc, current_stream_ptr())


def _block(A, row_partition, local):
    """The local rows of a result as an HPCMatrix on the given row partition."""
    from .dense import HPCMatrix
    return HPCMatrix(row_partition, uniform_partition(int(local.shape[1]), comm_size(A.backend.comm)), local, A.backend)


def svds(A, k: int = 6, which: str = "LM", ncv: Optional[int] = None, tol: float = 1e-10, maxiter: Optional[int] = None,
         v0: Optional[HPCVector] = None, seed: int = 0, return_singular_vectors: bool = True,
         workspace: Optional[SvdsWorkspace] = None):
    """The ``k`` largest singular values of an ``A`` of any shape ``M x N`` (an HPCSparseMatrix, or a lazy ``transpose(B)``,
    which is materialised as ``hp.lsqr`` does and then has ``B`` as its transpose) with their left and right vectors, by
    thick-restart Golub-Kahan-Lanczos bidiagonalisation with full two-sided reorthogonalisation.  Returns ``(U, s, V, info)``:
    ``s`` is a numpy array of the singular values in DESCENDING order -- Julia's ``svd(A).S`` order; ``hp.eigsh`` stays
    ascending -- ``U`` an ``M x k`` HPCMatrix on A's row partition and ``V`` an ``N x k`` HPCMatrix on A's column partition
    whose columns i belong to ``s[i]`` (both ``None`` with ``return_singular_vectors=False``), ``info`` an :class:`SvdsInfo`.

    ``ncv`` is the number of basis columns per cycle, ``k + 1 <= ncv <= min(64, M, N)`` (default
    ``min(M, N, 64, max(2k + 1, 20))``); a cycle keeps ``ncv + 1`` right and ``ncv`` left basis columns on the device.  ``v0`` is
    an HPCVector on A's COLUMN partition; the default is ``numpy.random.default_rng(seed).uniform(-1, 1, N)`` over the global
    length, each rank taking its slice, so the start does not depend on the number of ranks.  ``which`` is ``"LM"`` only:
    ``"SM"`` raises ``ValueError``, because the smallest singular values need harmonic Ritz restarts or shift-invert and neither
    is here.

    Stops at the first cycle end where every wanted estimate ``|beta_m P[m-1, i]| <= tol * anorm`` with ``anorm`` the largest
    singular value of the cycle's projected matrix; as ``"maxiter"`` at the first cycle end with ``iterations >= maxiter``
    (default ``10 min(M, N)``; cycles are never cut short); as ``"invariant"`` when a new left or right vector is exactly zero --
    the triplets of the ``c`` finished columns are then exact, the solve is converged when ``c >= k`` and otherwise returns the
    ``c`` triplets found with ``converged=False``; as ``"breakdown"`` on a NaN (``s`` is then NaN and the blocks zero).
    ``residual_norms[i]`` estimates ``||A' u_i - s_i v_i||``; the other residual ``A v_i - s_i u_i`` is zero up to rounding by
    construction.

    Limits.  The gates are exact-zero and NaN tests, as everywhere in this package.  A single-vector method finds ONE triplet per
    distinct singular value: a multiple singular value is returned once.  ``"LM"`` only, Float64 only, ``ncv <= 64``.

    The host reads back once per cycle and never inside one.  With N ranks every rank computes the same B from all-reduced
    values; still only rank 0's decision and rank 0's P and Q are used (broadcast), so no rank leaves the loop alone and no two
    ranks rotate with a matrix that differs in a bit."""
    torch = _torch()
    backend = A.parent.backend if isinstance(A, TransposedHPCSparseMatrix) else A.backend
    f64_only(backend, "svds")
    if isinstance(A, TransposedHPCSparseMatrix):
        A = A.materialize()
    M, N = int(A.shape[0]), int(A.shape[1])
    k, m, maxiter = check_arguments(M, N, k, which, ncv, maxiter)
    if not tol >= 0:
        raise ValueError("svds: tol must be non-negative")
    if v0 is None:
        v0 = HPCVector.from_global(np.random.default_rng(seed).uniform(-1.0, 1.0, N), backend, partition=A.col_partition)
    elif not isinstance(v0, HPCVector) or v0.structural_hash != compute_partition_hash(A.col_partition):
        raise ValueError("svds: v0 must be an HPCVector partitioned like the columns of A")
    v0 = rd16_vector(v0)                                         # the start kernel reads it 16 bytes at a time
    At = TransposedHPCSparseMatrix(A).materialize()
    ws = workspace if workspace is not None and workspace.fits(A, m) else SvdsWorkspace(A, m)
    plan, plan_t = get_vector_plan(A, ws.v), get_vector_plan(At, ws.u)
    if plan.is_i64 != plan_t.is_i64:
        raise NotImplementedError("svds: the plans of A and of its transpose use different index widths (one of them was "
                                  "narrowed to Int32, the other could not be: a dimension or the nonzero count is near 2^31)")
    comm, rank0 = backend.rccl, comm_rank(backend.comm) == 0
    m_loc, n_loc = ws.u.local_length, ws.v.local_length
    sfx = "i64" if plan.is_i64 else "i32"
    blocks = plan.matrix_block(A) + plan_t.matrix_block(At)

    # -- start: V_0 = v0 / sqrt(v0.v0) ---------------------------------------------------------------------------------------------
    ws.small.zero_()
    ws.work.zero_()                                              # done_iter = 0, status = running
    ws.U.zero_()
    ws.V.zero_()
    ws.u.v.zero_()
    ws.v.v.zero_()
    dv = ws.small_array("dv")
    norm(v0, 2, out=dv)                                          # the all-reduced sum of squares; the square root is the caller's
    dv.sqrt_()
    _capi.call("hpcla_gmres_next_f64", dptr(v0.v), dptr(dv), None, dptr(ws.V), None, n_loc, dptr(ws.state), current_stream_ptr())

    def blocks_of(cols):
        if not return_singular_vectors:
            return None, None
        z = lambda rows: torch.zeros((rows, cols), dtype=torch.float64, device=ws.V.device)
        return z(m_loc), z(n_loc)

    iterations = restarts = p = 0
    s_kept = np.zeros(0)
    history: List[float] = []
    nbytes = 8 * (4 + m + m * m + (m + 1) * m)
    while True:
        _capi.call(f"hpcla_svds_steps_f64_{sfx}", comm, *blocks, dptr(ws.U), ws.ldu, dptr(ws.V), ws.ldv, dptr(ws.u.v),
                   dptr(ws.v.v), dptr(ws.small), dptr(ws.work), m, p, m - p, iterations + 1, current_stream_ptr())
        payload = None
        if rank0:                                                # the cycle's one read-back, the projected problem, the decision
            host = torch.cat([ws.small, ws.work[-4:]]).cpu().numpy()
            done, status = (int(x) for x in host[-4:-2].view(np.int64))
            beta = host[m * m:m * m + m]
            c, gate_z = finished_columns(status, done, iterations, p, m, beta)
            packed = np.zeros(4 + m + m * m + (m + 1) * m)
            if status != _BREAKDOWN and c >= 1:
                B = assemble_B(host[:m * m].reshape(m, m), s_kept, p, c, c + int(gate_z))
                if np.all(np.isfinite(B)):
                    P, s, Qh = np.linalg.svd(B, full_matrices=False)
                    packed[2] = 0.0 if gate_z else beta[c - 1]
                    packed[4:4 + c] = s
                    packed[4 + m:4 + m + c * c] = P.reshape(-1)
                    packed[4 + m + m * m:4 + m + m * m + (c + int(gate_z)) * c] = Qh.T.reshape(-1)
                else:
                    status = _BREAKDOWN
            packed[0], packed[1], packed[3] = status, c, int(gate_z)
            payload = packed.tobytes()
        packed = np.frombuffer(comm_bcast_bytes(backend.comm, payload, nbytes), dtype=np.float64)
        status, c, beta_last, cq = int(packed[0]), int(packed[1]), float(packed[2]), int(packed[1]) + int(packed[3])
        if status == _BREAKDOWN:                                 # gates N, N': maybe the poison of an expired exchange wait -- ask
            from .sparse import check_exchange_health
            check_exchange_health(backend)
            Ub, Vb = blocks_of(k)
            nan = np.full(k, np.nan)
            return (_block(A, A.row_partition, Ub) if Ub is not None else None, nan,
                    _block(A, A.col_partition, Vb) if Vb is not None else None,
                    SvdsInfo(False, "breakdown", iterations + max(c - p, 0), restarts, nan.copy(), history, float("nan")))
        iterations += c - p
        s = packed[4:4 + c].copy()
        P = packed[4 + m:4 + m + c * c].reshape(c, c).copy()
        Q = packed[4 + m + m * m:4 + m + m * m + cq * c].reshape(cq, c).copy()
        kk = min(k, c)
        rho = np.abs(beta_last * P[c - 1, :kk]) if c else np.zeros(0)
        anorm = float(s[0]) if c else 0.0
        history.append(float(rho.max()) if kk else 0.0)
        if status == _INVARIANT:
            converged, name = c >= k, "invariant"
        elif bool(np.all(rho <= tol * anorm)):
            converged, name = True, "converged"
        elif iterations >= maxiter:
            converged, name = False, "maxiter"
        else:                                                    # restart: the p largest triplets
            p = kept_count(k, m)
            s_kept = s[:p].copy()
            _rotate(ws.V, ws.ldv, ws.Q, n_loc, Q[:, :p], move_last=True)
            _rotate(ws.U, ws.ldu, ws.P, m_loc, P[:, :p], move_last=False)
            restarts += 1
            continue
        Ub, Vb = blocks_of(kk)
        if Ub is not None and kk:
            _rotate(ws.U, ws.ldu, ws.P, m_loc, P[:, :kk], move_last=False, out=Ub)
            _rotate(ws.V, ws.ldv, ws.Q, n_loc, Q[:, :kk], move_last=False, out=Vb)
        return (_block(A, A.row_partition, Ub) if Ub is not None else None, s[:kk].copy(),
                _block(A, A.col_partition, Vb) if Vb is not None else None,
                SvdsInfo(converged, name, iterations, restarts, rho, history, anorm))
