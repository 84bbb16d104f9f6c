"""Extreme eigenpairs of a symmetric ``A``, or of a symmetric-definite pencil ``(A, B)``, with their multiplicities
(``hp.lobpcg``): the locally optimal block preconditioned conjugate gradient method (Knyazev), no soft locking, no constraints.

``hp.eigsh`` iterates one vector and so finds one vector per distinct eigenvalue; a block of ``k`` vectors finds a ``k``-fold
eigenvalue ``k`` times.  The reference has no eigensolver.  Composed from its operators an iteration is ``A * W``
(src/sparse.jl:2391-2413), three ``transpose(.) * .`` per Gram matrix (src/dense.jl:1286-1310: a pass over the block and a host
all-reduce per COLUMN), and broadcast updates for the residual and for ``S C``.  Here an iteration is the few launches
below and one read-back:

    start   X = X0;  AX = A X;  (theta, C, all) = RR(X'AX, X'X);  X = X C;  AX = AX C;  anorm = max|all|
            fewer than k kept directions in this first RR: ValueError("lobpcg: X0 is rank deficient")
    it = 1, 2, ...
      1     R = AX - X diag(theta);  rn_j = ||R_j||_2 (all-reduced);  W = M .* R          hpcla_lobpcg_residual_f64
      2     AW = A W                                                                      the SpMM of hp.spmm, its exchange included
      3     S = [X W P], AS = [AX AW AP] (iteration 1: S = [X W]);  G_B = S'S, G_A = S'AS one hpcla_gram_f64, one all-reduce
      4     ONE read-back on rank 0 (rn^2, G_A, G_B) and the decision, in this order:
              any non-finite value      -> "breakdown" (vals NaN, X zero)
              all rn_j <= tol * anorm   -> "converged": the CURRENT theta, X are returned (the combine below is not applied)
              it > maxiter              -> "maxiter", same return
            else (theta, C, all) = RR(G_A, G_B);  anorm = max(anorm, max|all|);  rank 0's (decision, theta, C) is broadcast
      5     [X | P] <- S C,  [AX | AP] <- AS C in place, one pass                          hpcla_lobpcg_combine_f64
              pp_j = sum_{i >= k} S[r,i] C[i,j] (i ascending)      P'[r,j] = pp_j
              px_j = sum_{i <  k} S[r,i] C[i,j] (i ascending)      X'[r,j] = px_j + pp_j

``RR`` is the whitened Rayleigh-Ritz step (:func:`rayleigh_ritz`): pure numpy, importable without a device, like everything
above the workspace class in this file.  It replaces a tall CholQR: a dependent or zero column of ``W`` or ``P`` is dropped on
the host and never factorised.

With a ``B`` (``A x = lambda B x``, ``B`` symmetric positive definite: a sparse matrix, or the positive weights of a diagonal
one) a third block ``BS = [BX BW BP]`` is carried along, the Gram matrix of the basis is ``S'BS``, and the returned ``X`` is
B-orthonormal.  Only products with ``B`` are needed, no solve:

    start   X = X0;  AX = A X;  BX = B X;  (theta, C, all) = RR(X'AX, X'BX);  X, AX, BX <- . C;  anorm = max|all|
    it = 1, 2, ...
      1     R = AX - BX diag(theta);  W = M .* R;  the sums of R_j^2, AX_j^2, BX_j^2 (all-reduced, ONE reduction of 48 doubles);
            a diagonal B: BW = b .* W in the same pass                                    hpcla_lobpcg_residual_gen_f64
      2     AW = A W;  a sparse B: BW = B W                                               one SpMM, or two
      3     G_A = S'AS, G_B = S'BS                                                        one hpcla_gram_f64 of S against [AS | BS]
      4     ONE read-back on rank 0 and the decision (:func:`decide_gen`), in this order:
              any non-finite value, or a negative diagonal entry of S'BS (B is not positive definite there) -> "breakdown"
              all ||R_j|| <= tol (||A x_j|| + |theta_j| ||B x_j||)  -> "converged"
              it > maxiter                                          -> "maxiter"
            else the same RR and broadcast
      5     the combine of 5 above, and a second call of the same kernel for [BX | BP] <- BS C

Layout.  One row-major ``(n_loc, 6k)`` buffer ``[X W P | AX AW AP]`` holds every tall block, so ONE Gram call with ``S`` as the
left and the whole buffer as the right operand yields ``[G_B | G_A]``.  The residual kernel writes ``W`` twice: into the buffer
and into a block on ``spmm_pitch(A, k)`` (``k``, or ``k + 1`` for an odd ``k >= 3``), which is the operand the SpMM machinery
(``_spmm_plan``, the exchange, the kernel choice) takes as it is; ``AW`` returns into the buffer with one strided device copy.
Bytes per local row and iteration, next to the SpMM's own traffic: residual ``8 (2k [+1]) + 16k``, the copy of ``AW`` ``16k``,
the Gram pass ``8 * 6k`` (every column is read once per 64-column panel: ``8 * 9k`` at ``k = 16``), the combine
``16 * 3k + 32k``: about ``200 k`` bytes.  The workspace is ``8 n_loc (6k + spmm_pitch)`` bytes plus the Gram partials
(``hpcla_gram_work_bytes(n_loc, 3k, 6k)``, at most 32 MiB) and a few KiB of small arrays; the SpMM allocates its result
(``8 n_loc spmm_pitch``) per product, as ``A @ B`` does.

With a ``B`` the buffer is ``(n_loc, 9k)``, ``[X W P | AX AW AP | BX BW BP]``; the Gram call takes ``S`` on the left and the
``6k`` columns ``[AS | BS]`` on the right, so its product keeps the ``3k x 6k`` shape: ``[G_A | G_B]``.  Bytes per local row
and iteration: residual ``8 (2k [+1 minv] [+1 b]) + 16k`` and ``+ 8k`` for ``BW`` of a diagonal ``B``, the copy of ``AW``
``16k`` (and of ``BW`` ``16k`` with a sparse ``B``, next to its SpMM), the Gram pass ``8 * 9k`` (``8 * 12k`` at ``k = 16``),
the two combines ``16 * 3k + 32k`` and ``8 * 3k + 16k``: about ``270 k`` bytes with a diagonal ``B``.  The workspace grows by
``24 k n_loc`` bytes.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

MAX_K = 16                      # the block width the kernels take: 3k <= 48 columns of a row are the register / LDS tile
C_PITCH = 16                    # row pitch of the uploaded C (include/hpcla_rocm.h)
RR_DROP = 1e-12                 # directions of the scaled S'S below RR_DROP * lam_max are dropped
WHICH = ("SA", "LA")
_GO, _CONVERGED, _BREAKDOWN, _MAXITER, _DEFICIENT = 0, 1, 2, 3, 5


@dataclass
class LobpcgInfo:
    """What ``lobpcg`` reports.  ``iterations`` counts the SpMMs after the start, the last one included (an iteration decides
    after its SpMM, so a solve that stops in iteration ``it`` has made ``it`` of them); ``residual_norms`` holds
    ``||A x_i - vals_i x_i||`` of the returned pairs as the residual kernel computed them from the implicitly updated ``AX``,
    aligned with ``vals``; ``history`` the largest of them at every iteration; ``anorm`` the largest ``|Ritz value|`` any
    projection of the solve produced (the norm the stop rule is relative to).

    With a ``B``: ``residual_norms`` holds ``||A x_i - vals_i B x_i||``, the left-hand sides of the stop rule, and
    ``residual_scales`` its right-hand sides without the factor ``tol``, ``||A x_i|| + |vals_i| ||B x_i||`` (an empty array
    with ``B=None``); ``anorm`` is then a bound on the spectrum of the pencil from inside, not on ``||A||``, and the stop rule
    does not use it."""
    converged: bool
    status: str
    iterations: int
    residual_norms: np.ndarray
    history: List[float] = field(default_factory=list)
    anorm: float = 0.0
    residual_scales: np.ndarray = field(default_factory=lambda: np.zeros(0))


# ---- the host's part: pure numpy ---------------------------------------------------------------------------------------------
def check_arguments(n: int, k, which, tol, maxiter) -> Tuple[int, int]:
    """The argument rules that need no device.  Returns (k, maxiter)."""
    if which not in WHICH:
        if which == "SM":
            raise ValueError("lobpcg: which='SM' is not offered: interior and smallest-magnitude pairs need shift-invert, and this "
                             "package has no factorisation for it (which: 'SA' or 'LA')")
        raise ValueError(f"lobpcg: which must be 'SA' or 'LA', got {which!r}")
    k = int(k)
    if not 1 <= k <= min(MAX_K, n):
        raise ValueError(f"lobpcg: k must satisfy 1 <= k <= min({MAX_K}, n) = {min(MAX_K, n)}, got {k}")
    if not tol >= 0:
        raise ValueError("lobpcg: tol must be non-negative")
    maxiter = 10 * n if maxiter is None else int(maxiter)
    if maxiter < 0:
        raise ValueError("lobpcg: maxiter must be non-negative")
    return k, maxiter


def rayleigh_ritz(G_A: np.ndarray, G_B: np.ndarray, k: int, which: str):
    """The whitened Rayleigh-Ritz step on the Gram matrices ``G_A = S'AS`` and ``G_B = S'S`` of a basis ``S`` of m columns.
    Returns ``(theta, C, all)``: the (at most) ``k`` wanted Ritz values in ascending order, the ``m x len(theta)`` coefficients
    with ``(S C)'(S C) = I`` and ``(S C)' A (S C) = diag(theta)``, and every Ritz value of the kept space.

    Both matrices are symmetrised and scaled to a unit diagonal of ``G_B`` (a zero column keeps the divisor 1 and drops out
    next); the directions of the scaled ``G_B`` with ``lam_i <= RR_DROP * lam_max`` are dropped, the rest whitened.  The Gram
    matrix squares the basis's condition number: ``RR_DROP = 1e-12`` sits four decades above double epsilon."""
    if which not in WHICH:
        raise ValueError(f"lobpcg: which must be 'SA' or 'LA', got {which!r}")
    G_A = np.asarray(G_A, dtype=np.float64)
    G_B = np.asarray(G_B, dtype=np.float64)
    G_A, G_B = (G_A + G_A.T) / 2, (G_B + G_B.T) / 2
    d = np.sqrt(np.diag(G_B))
    d = np.where(d == 0, 1.0, d)
    dinv = 1.0 / d
    G_A, G_B = dinv[:, None] * G_A * dinv[None, :], dinv[:, None] * G_B * dinv[None, :]
    lam, U = np.linalg.eigh(G_B)
    kept = lam > RR_DROP * lam.max()
    Wh = U[:, kept] / np.sqrt(lam[kept])
    H = Wh.T @ G_A @ Wh
    H = (H + H.T) / 2
    th, Z = np.linalg.eigh(H)
    q = min(int(k), len(th))
    picked = np.arange(q) if which == "SA" else np.arange(len(th) - q, len(th))
    C = dinv[:, None] * (Wh @ Z[:, picked])
    return th[picked].copy(), C, th


def decide(rn2: np.ndarray, G_A: np.ndarray, G_B: np.ndarray, theta: np.ndarray, anorm: float, it: int, k: int, which: str,
           tol: float, maxiter: int):
    """Step 4 of iteration ``it``: (decision, rn, theta, C, anorm).  ``theta`` and ``C`` are new only with decision ``_GO``."""
    if not (np.all(np.isfinite(rn2)) and np.all(np.isfinite(G_A)) and np.all(np.isfinite(G_B))):
        return _BREAKDOWN, np.full(k, np.nan), theta, None, anorm
    rn = np.sqrt(rn2)
    if bool(np.all(rn <= tol * anorm)):
        return _CONVERGED, rn, theta, None, anorm
    if it > maxiter:
        return _MAXITER, rn, theta, None, anorm
    theta, C, every = rayleigh_ritz(G_A, G_B, k, which)
    return _GO, rn, theta, C, max(anorm, float(np.max(np.abs(every))))


def grams(G: np.ndarray, k: int, m: int):
    """(G_A, G_B) of the first ``m`` columns of S out of the device's ``3k x 6k`` product ``S' [S | AS]``."""
    return G[:m, 3 * k:3 * k + m], G[:m, :m]


def grams_gen(G: np.ndarray, k: int, m: int):
    """(G_A, G_B) of the first ``m`` columns of S out of the device's ``3k x 6k`` product ``S' [AS | BS]``."""
    return G[:m, :m], G[:m, 3 * k:3 * k + m]


def scales_gen(sums: np.ndarray, theta: np.ndarray, k: int):
    """(rn, scale) of the pencil's stop rule from the residual kernel's three groups of sums (16 apart): ``rn_j = ||R_j||`` and
    ``scale_j = ||A x_j|| + |theta_j| ||B x_j||``."""
    rn, na, nb = (np.sqrt(sums[MAX_K * q:MAX_K * q + k]) for q in range(3))
    return rn, na + np.abs(theta[:k]) * nb


def positive_on_basis(G_B: np.ndarray) -> bool:
    """False where ``S'BS`` has a negative diagonal entry: ``B`` is not positive definite on that basis column."""
    return not bool(np.any(np.diag(G_B) < 0))


def decide_gen(sums: np.ndarray, G_A: np.ndarray, G_B: np.ndarray, theta: np.ndarray, anorm: float, it: int, k: int, which: str,
               tol: float, maxiter: int):
    """Step 4 of iteration ``it`` with a ``B``: (decision, rn, scale, theta, C, anorm).  ``sums`` are the 48 doubles of the
    residual kernel, ``G_B = S'BS``.  ``theta`` and ``C`` are new only with decision ``_GO``."""
    used = np.concatenate([sums[MAX_K * q:MAX_K * q + k] for q in range(3)])
    if not (np.all(np.isfinite(used)) and np.all(np.isfinite(G_A)) and np.all(np.isfinite(G_B))) or not positive_on_basis(G_B):
        return _BREAKDOWN, np.full(k, np.nan), np.full(k, np.nan), theta, None, anorm
    rn, scale = scales_gen(sums, theta, k)
    if bool(np.all(rn <= tol * scale)):
        return _CONVERGED, rn, scale, theta, None, anorm
    if it > maxiter:
        return _MAXITER, rn, scale, theta, None, anorm
    theta, C, every = rayleigh_ritz(G_A, G_B, k, which)
    return _GO, rn, scale, theta, C, max(anorm, float(np.max(np.abs(every))))


def check_b(kind: Optional[str], n: int, a_hash, shape=None, row_hash=None, col_hash=None, same_backend: bool = True) -> Optional[str]:
    """The rules for ``B`` that need no device, on a description of it: ``kind`` is None, ``"sparse"`` (an HPCSparseMatrix:
    ``shape``, the hashes of its row and column partitions) or ``"vector"`` (an HPCVector: ``shape = (length,)`` and the hash
    of its partition as ``row_hash``), anything else for any other object; ``a_hash`` is the hash of A's row partition.
    Returns None, ``"sparse"`` or ``"diagonal"``."""
    if kind is None:
        return None
    if kind == "sparse":
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError(f"lobpcg: B must be square, got {shape[0]} x {shape[1]}")
        if not same_backend:
            raise ValueError("lobpcg: B must be on A's backend")
        if shape[0] != n or row_hash != a_hash or col_hash != a_hash:
            raise ValueError("lobpcg: B must be partitioned like the rows of A, rows and columns")
        return "sparse"
    if kind == "vector":
        if not same_backend:
            raise ValueError("lobpcg: B must be on A's backend")
        if tuple(shape) != (n,) or row_hash != a_hash:
            raise ValueError("lobpcg: B must be an HPCVector on A's row partition (the diagonal of a lumped B)")
        return "diagonal"
    raise ValueError("lobpcg: B must be None, an HPCSparseMatrix or an HPCVector of positive weights on A's row partition")


_STATUS = {_CONVERGED: "converged", _BREAKDOWN: "breakdown", _MAXITER: "maxiter"}


# ---- the workspace -------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


class LobpcgWorkspace:
    """What a ``lobpcg`` solve allocates for ``A`` and ``k``: the ``(n_loc, 6k)`` buffer ``[X W P | AX AW AP]``, the SpMM's
    operand ``(n_loc, spmm_pitch(A, k))``, the partials of the residual sums and of the Gram pass, the read-back buffer
    (16 sums and the ``3k x 6k`` Gram product) and the upload buffer (16 ``theta`` and ``C`` at 48 x 16).  Reusable: every
    solve resets all of it.

    With a ``B`` (anything but None: only whether there is one counts) the buffer is ``(n_loc, 9k)``,
    ``[X W P | AX AW AP | BX BW BP]``, the read-back buffer holds 48 sums, and the partials are those of
    ``hpcla_lobpcg_gen_work_bytes``.  A workspace of one shape does not fit a solve of the other (:meth:`fits`)."""

    def __init__(self, A, k: int, B=None):
        from . import _capi
        from .spmm_plans import spmm_pitch
        from .vectors import f64_only
        torch = _torch()
        lib = _capi.load()
        f64_only(A.backend, "lobpcg")
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"lobpcg: k must be in 1..{MAX_K}, got {k}")
        f64 = dict(dtype=torch.float64, device=A.backend.torch_device)
        self.k, self.n_loc, self.pitch = k, int(A.nrows_local), spmm_pitch(A, k)
        self.row_hash = A._ensure_hash()
        self.gen = B is not None
        self.Q = torch.zeros((self.n_loc, (9 if self.gen else 6) * k), **f64)
        self.Wp = torch.zeros((self.n_loc, self.pitch), **f64)
        self.small = torch.zeros((3 if self.gen else 1) * MAX_K + 18 * k * k, **f64)
        self.up = torch.zeros(MAX_K + 3 * MAX_K * C_PITCH, **f64)
        work_bytes = lib.hpcla_lobpcg_gen_work_bytes if self.gen else lib.hpcla_lobpcg_work_bytes
        self.rwork = torch.zeros(max(1, work_bytes(self.n_loc, k) // 8), **f64)
        self.gwork = torch.zeros(max(1, lib.hpcla_gram_work_bytes(self.n_loc, 3 * k, 6 * k) // 8), **f64)

    def fits(self, A, k: int, B=None) -> bool:
        from .spmm_plans import spmm_pitch
        return (self.k == k and self.n_loc == int(A.nrows_local) and self.row_hash == A._ensure_hash()
                and self.pitch == spmm_pitch(A, k) and self.Q.device == A.backend.torch_device and self.gen == (B is not None))

    def reset(self) -> None:
        for t in (self.Q, self.Wp, self.small, self.up):
            t.zero_()


def _block(A, local):
    from .dense import HPCMatrix
    from .backends import comm_size
    from .partition import uniform_partition
    return HPCMatrix(A.row_partition, uniform_partition(int(local.shape[1]), comm_size(A.backend.comm)), local, A.backend)


def _minv(A, M):
    """The inverse-diagonal weights as an HPCVector on A's row partition, or None."""
    import math
    from .partition import compute_partition_hash
    from .vectors import HPCVector, maximum, minimum, rd16_vector
    if M is None:
        return None
    if isinstance(M, str):
        if M != "jacobi":
            raise ValueError(f"lobpcg: unknown preconditioner {M!r} (None, 'jacobi' or an HPCVector of positive weights)")
        from .indexing import diag
        d = diag(A)
        mag = HPCVector(d.structural_hash, d.partition, d.v.abs(), d.backend)
        if not (minimum(mag) > 0 and math.isfinite(maximum(mag))):
            raise ValueError("lobpcg: M='jacobi' needs a diagonal without zero or non-finite entries (it applies 1 ./ abs(diag(A)))")
        mag.v = 1.0 / mag.v
        return mag
    if not isinstance(M, HPCVector) or M.structural_hash != compute_partition_hash(A.row_partition):
        raise ValueError("lobpcg: M must be None, 'jacobi' or an HPCVector on A's row partition")
    M = rd16_vector(M)                                           # one clone of misaligned weights for the check and the solve
    if not (minimum(M) > 0):
        raise ValueError("lobpcg: M must be positive definite (minimum(M) > 0)")
    return M


def _b_operand(A, B):
    """(form, operand) of ``B``: (None, None), ("sparse", the matrix) or ("diagonal", the weights as an HPCVector on aligned
    storage).  The rules are :func:`check_b`'s; the weights must be positive."""
    from .backends import backends_compatible
    from .partition import compute_partition_hash
    from .sparse import HPCSparseMatrix
    from .vectors import HPCVector, f64_only, minimum, rd16_vector
    if B is None:
        return None, None
    n, a_hash = int(A.shape[0]), compute_partition_hash(A.row_partition)
    if isinstance(B, HPCSparseMatrix):
        f64_only(B.backend, "lobpcg")
        return check_b("sparse", n, a_hash, tuple(B.shape), compute_partition_hash(B.row_partition),
                       compute_partition_hash(B.col_partition), backends_compatible(A.backend, B.backend)), B
    if isinstance(B, HPCVector):
        f64_only(B.backend, "lobpcg")
        form = check_b("vector", n, a_hash, (len(B),), B.structural_hash, None, backends_compatible(A.backend, B.backend))
        B = rd16_vector(B)                                       # one clone of misaligned weights for the check and the solve
        if not (minimum(B) > 0):
            raise ValueError("lobpcg: B must be positive definite (minimum(B) > 0)")
        return form, B
    return check_b("other", n, a_hash), None                     # raises: neither of the two


def lobpcg(A, k: int = 6, which: str = "SA", X0=None, M=None, tol: float = 1e-8, maxiter: Optional[int] = None, seed: int = 0,
           workspace: Optional[LobpcgWorkspace] = None, B=None):
    """The ``k`` smallest (``which="SA"``) or largest (``"LA"``) eigenvalues of a symmetric ``A`` and their vectors by LOBPCG,
    multiple eigenvalues with their multiplicity.  The caller asserts the symmetry; it is not checked.  Returns
    ``(vals, X, info)``: ``vals`` a numpy array in ascending order, ``X`` an ``n x k`` HPCMatrix on A's row partition whose
    column i belongs to ``vals[i]``, ``info`` a :class:`LobpcgInfo`.

    ``k`` is the block width, ``1 <= k <= min(16, n)``.  ``X0`` is an HPCMatrix of ``k`` columns on A's row partition; the
    default is ``numpy.random.default_rng(seed).uniform(-1, 1, (n, k))`` over the global shape, each rank taking its rows, so
    the start does not depend on the number of ranks.  A rank-deficient ``X0`` raises ``ValueError``.  ``"SM"`` and ``"BE"``
    raise ``ValueError``.

    ``M`` preconditions the residual block: ``None``, ``"jacobi"`` (``1 ./ abs(diag(A))``, as ``hp.minres``) or an HPCVector
    of positive weights on A's row partition.  It is meant for ``which="SA"`` of a positive definite ``A``; on a diagonally
    dominant matrix Jacobi with ``"LA"`` did not converge in the prototype of this scheme.

    ``B`` makes it the generalised problem ``A x = lambda B x`` (a stiffness and a mass matrix): ``vals`` are then the ``k``
    smallest or largest eigenvalues of the pencil and ``X`` is B-orthonormal, ``X' B X = I``.  ``B`` is an HPCSparseMatrix --
    square, on A's backend, rows and columns partitioned like the rows of A; the caller asserts that it is symmetric positive
    definite, it is not checked -- or an HPCVector of positive weights on A's row partition, the diagonal of a lumped mass
    matrix (``minimum(B) > 0`` is checked; ``B W`` then costs no product).  Only products with ``B`` are made, no solve.
    ``B=None`` is the standard problem, with the launches and the bits it had before ``B`` existed.

    Stops at the first iteration where every ``||A x_j - theta_j x_j|| <= tol * anorm``, ``anorm`` being the largest
    ``|Ritz value|`` any projection has produced so far -- a lower bound of ``||A||_2`` that only grows, so an eigenvalue at 0
    can converge (default ``tol = 1e-8``); as ``"maxiter"`` in iteration ``maxiter + 1`` (default ``10 n``); as ``"breakdown"``
    on a non-finite value (``vals`` is then NaN and ``X`` zero).  With a ``B`` the rule is the normwise backward error of every
    pair, which needs no norm of either matrix: ``||A x_j - theta_j B x_j|| <= tol (||A x_j|| + |theta_j| ||B x_j||)``
    (``info.residual_norms`` and ``info.residual_scales``); and a negative diagonal entry of ``S'BS`` -- ``B`` is not positive
    definite on a basis column -- is a ``"breakdown"`` too.

    Limits.  The projected matrices are Gram matrices, which square the basis's condition number: residuals below about
    ``1e-9 ||A||`` may stagnate, and the solve then ends as ``"maxiter"`` (two of eighteen ``tol = 1e-10`` runs of the
    prototype did; with a ``B``, the lumped 2-D finite-element pencil on a 16 x 16 grid at ``k = 5``, ``"SA"``, whose block
    cuts through a double eigenvalue, stagnated at 2.3 ``tol`` for ``tol = 1e-8``).  ``k <= 16``.  No soft locking, no
    constraints, Float64 only.

    The host reads back once per iteration (rank 0) and uploads ``theta`` and ``C`` once.  With N ranks only rank 0 decides
    and only its ``theta`` and ``C`` are used (broadcast), so no rank leaves the loop alone and no two ranks combine with a
    ``C`` that differs in a bit."""
    from . import _capi
    from .backends import comm_bcast_bytes, comm_rank
    from .dense import HPCMatrix
    from .partition import compute_partition_hash
    from .spmm_plans import _spmm_plan, spmm
    from .vectors import current_stream_ptr, dptr, f64_only
    torch = _torch()
    f64_only(A.backend, "lobpcg")
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"lobpcg: the matrix must be square, got {A.shape[0]} x {A.shape[1]}")
    n = int(A.shape[0])
    k, maxiter = check_arguments(n, k, which, tol, maxiter)
    if X0 is None:
        X0 = HPCMatrix.from_global(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, k)), A.backend,
                                   row_partition=A.row_partition)
    elif (not isinstance(X0, HPCMatrix) or int(X0.A.shape[1]) != k
          or compute_partition_hash(X0.row_partition) != compute_partition_hash(A.row_partition)):
        raise ValueError(f"lobpcg: X0 must be an HPCMatrix of k = {k} columns partitioned like the rows of A")
    minv = _minv(A, M)
    b_form, b_op = _b_operand(A, B)
    if b_form is not None:
        return _lobpcg_gen(A, b_form, b_op, k, which, X0, minv, tol, maxiter, workspace)
    ws = workspace if workspace is not None and workspace.fits(A, k) else LobpcgWorkspace(A, k)
    comm, rank0 = A.backend.rccl, comm_rank(A.backend.comm) == 0
    n_loc, ld = ws.n_loc, 6 * k
    Q, rn2_dev, G_dev = ws.Q, ws.small[:MAX_K], ws.small[MAX_K:]
    Wp = _block(A, ws.Wp[:, :k])                                 # the SpMM's operand: rows on spmm_pitch, taken as it is
    if compute_partition_hash(_spmm_plan(A, Wp)[0].result_partition) != compute_partition_hash(A.row_partition):
        raise ValueError("lobpcg: the columns of A must be partitioned like its rows")
    at = lambda col: dptr(Q[:, col:]) if n_loc else dptr(None)   # noqa: E731  (the block that starts at column col)
    nbytes = 8 * (2 + 2 * MAX_K + 3 * MAX_K * C_PITCH)

    def product(dst_col):                                        # A * (the block in Wp) into columns dst_col .. + k of Q
        Q[:, dst_col:dst_col + k].copy_(spmm(A, Wp).A)

    def gram():
        _capi.call("hpcla_gram_f64", comm, at(0), ld, _capi.LAYOUT_ROW, at(0), ld, _capi.LAYOUT_ROW, n_loc, 3 * k, 6 * k,
                   dptr(G_dev), dptr(ws.gwork), current_stream_ptr())

    def exchange_decision(make):
        """Rank 0 reads back (the iteration's one read-back) and decides; every rank gets (decision, anorm, rn, theta, C)."""
        payload = None
        if rank0:
            host = ws.small.cpu().numpy()
            decision, rn, th, C, an = make(host[:k].copy(), host[MAX_K:].reshape(3 * k, 6 * k))
            packed = np.zeros(nbytes // 8)
            packed[0], packed[1] = decision, an
            packed[2:2 + k], packed[2 + MAX_K:2 + MAX_K + len(th)] = rn, th
            if C is not None:
                Cp = np.zeros((3 * MAX_K, C_PITCH))
                Cp[:C.shape[0], :C.shape[1]] = C
                packed[2 + 2 * MAX_K:] = Cp.reshape(-1)
            payload = packed.tobytes()
        packed = np.frombuffer(comm_bcast_bytes(A.backend.comm, payload, nbytes), dtype=np.float64)
        return int(packed[0]), float(packed[1]), packed[2:2 + k].copy(), packed[2 + MAX_K:2 + MAX_K + k].copy(), packed[2 + MAX_K:]

    def combine(upload, c_rest):
        ws.up.copy_(torch.from_numpy(upload.copy()))             # theta (16) and C (48 x 16) in one upload
        _capi.call("hpcla_lobpcg_combine_f64", at(0), ld, at(3 * k), ld, dptr(ws.up[MAX_K:]), k, c_rest, n_loc,
                   current_stream_ptr())

    def broken(iterations, history):
        from .sparse import check_exchange_health
        check_exchange_health(A.backend)                         # maybe the poison of an expired exchange wait -- ask
        X = _block(A, torch.zeros((n_loc, k), dtype=torch.float64, device=Q.device))
        return np.full(k, np.nan), X, LobpcgInfo(False, "breakdown", iterations, np.full(k, np.nan), history, float("nan"))

    # -- start: X = X0, AX = A X, the first Rayleigh-Ritz ------------------------------------------------------------------------
    ws.reset()
    ws.Wp[:, :k].copy_(X0.A)
    Q[:, :k].copy_(X0.A)
    product(3 * k)
    gram()

    def first(rn2, G):
        G_A, G_B = grams(G, k, k)
        if not (np.all(np.isfinite(G_A)) and np.all(np.isfinite(G_B))):
            return _BREAKDOWN, np.zeros(k), np.zeros(0), None, float("nan")
        th, C, every = rayleigh_ritz(G_A, G_B, k, which)
        if len(th) < k:
            return _DEFICIENT, np.zeros(k), np.zeros(0), None, 0.0
        return _GO, np.zeros(k), th, C, float(np.max(np.abs(every)))

    decision, anorm, rn, theta, upload = exchange_decision(first)
    history: List[float] = []
    if decision == _DEFICIENT:
        raise ValueError("lobpcg: X0 is rank deficient")
    if decision == _BREAKDOWN:
        return broken(0, history)
    combine(upload, 0)

    it = 0
    while True:
        it += 1
        _capi.call("hpcla_lobpcg_residual_f64", comm, at(0), ld, at(3 * k), ld, dptr(ws.up), dptr(minv.v) if minv is not None else None,
                   at(k), ld, dptr(ws.Wp) if n_loc else None, ws.pitch, n_loc, k, dptr(rn2_dev), dptr(ws.rwork),
                   current_stream_ptr())
        product(4 * k)
        gram()
        m = 2 * k if it == 1 else 3 * k
        prev_theta, prev_anorm = theta, anorm
        decision, anorm, rn, theta, upload = exchange_decision(
            lambda rn2, G: decide(rn2, *grams(G, k, m), prev_theta, prev_anorm, it, k, which, tol, maxiter))
        if decision == _BREAKDOWN:
            return broken(it, history)
        history.append(float(rn.max()))
        if decision != _GO:
            X = _block(A, Q[:, :k].clone())
            return theta, X, LobpcgInfo(decision == _CONVERGED, _STATUS[decision], it, rn, history, anorm)
        combine(upload, m - k)


def _lobpcg_gen(A, b_form: str, B, k: int, which: str, X0, minv, tol: float, maxiter: int, workspace):
    """``lobpcg`` with a ``B``, after the argument checks: ``b_form`` is "sparse" (``B`` an HPCSparseMatrix) or "diagonal"
    (``B`` an HPCVector of positive weights).  The steps are the module docstring's second list."""
    from . import _capi
    from .backends import comm_bcast_bytes, comm_rank
    from .partition import compute_partition_hash
    from .spmm_plans import _spmm_plan, spmm
    from .vectors import current_stream_ptr, dptr
    torch = _torch()
    sparse_b = b_form == "sparse"
    ws = workspace if workspace is not None and workspace.fits(A, k, B) else LobpcgWorkspace(A, k, B)
    comm, rank0 = A.backend.rccl, comm_rank(A.backend.comm) == 0
    n_loc, ld = ws.n_loc, 9 * k
    Q, sums_dev, G_dev = ws.Q, ws.small[:3 * MAX_K], ws.small[3 * MAX_K:]
    Wp = _block(A, ws.Wp[:, :k])                                 # the operand of both SpMMs: rows on spmm_pitch
    a_hash = compute_partition_hash(A.row_partition)
    if compute_partition_hash(_spmm_plan(A, Wp)[0].result_partition) != a_hash:
        raise ValueError("lobpcg: the columns of A must be partitioned like its rows")
    at = lambda col: dptr(Q[:, col:]) if n_loc else dptr(None)   # noqa: E731  (the block that starts at column col)
    nbytes = 8 * (2 + 3 * MAX_K + 3 * MAX_K * C_PITCH)

    def product(Mat, dst_col):                                   # Mat * (the block in Wp) into columns dst_col .. + k of Q
        Q[:, dst_col:dst_col + k].copy_(spmm(Mat, Wp).A)

    def gram():                                                  # S' [AS | BS]: the 3k x 6k product [G_A | G_B]
        _capi.call("hpcla_gram_f64", comm, at(0), ld, _capi.LAYOUT_ROW, at(3 * k), ld, _capi.LAYOUT_ROW, n_loc, 3 * k, 6 * k,
                   dptr(G_dev), dptr(ws.gwork), current_stream_ptr())

    def exchange_decision(make):
        """Rank 0 reads back (the iteration's one read-back) and decides; every rank gets (decision, anorm, rn, scale, theta, C)."""
        payload = None
        if rank0:
            host = ws.small.cpu().numpy()
            decision, rn, scale, th, C, an = make(host[:3 * MAX_K].copy(), host[3 * MAX_K:].reshape(3 * k, 6 * k))
            packed = np.zeros(nbytes // 8)
            packed[0], packed[1] = decision, an
            packed[2:2 + k], packed[2 + MAX_K:2 + MAX_K + k], packed[2 + 2 * MAX_K:2 + 2 * MAX_K + len(th)] = rn, scale, th
            if C is not None:
                Cp = np.zeros((3 * MAX_K, C_PITCH))
                Cp[:C.shape[0], :C.shape[1]] = C
                packed[2 + 3 * MAX_K:] = Cp.reshape(-1)
            payload = packed.tobytes()
        packed = np.frombuffer(comm_bcast_bytes(A.backend.comm, payload, nbytes), dtype=np.float64)
        return (int(packed[0]), float(packed[1]), packed[2:2 + k].copy(), packed[2 + MAX_K:2 + MAX_K + k].copy(),
                packed[2 + 2 * MAX_K:2 + 2 * MAX_K + k].copy(), packed[2 + 2 * MAX_K:])

    def combine(upload, c_rest):
        ws.up.copy_(torch.from_numpy(upload.copy()))             # theta (16) and C (48 x 16) in one upload
        _capi.call("hpcla_lobpcg_combine_f64", at(0), ld, at(3 * k), ld, dptr(ws.up[MAX_K:]), k, c_rest, n_loc,
                   current_stream_ptr())
        _capi.call("hpcla_lobpcg_combine_f64", at(6 * k), ld, None, 0, dptr(ws.up[MAX_K:]), k, c_rest, n_loc,
                   current_stream_ptr())                         # [BX | BP] <- BS C: the same kernel on the third block

    def broken(iterations, history):
        from .sparse import check_exchange_health
        check_exchange_health(A.backend)                         # maybe the poison of an expired exchange wait -- ask
        X = _block(A, torch.zeros((n_loc, k), dtype=torch.float64, device=Q.device))
        nan = np.full(k, np.nan)
        return nan, X, LobpcgInfo(False, "breakdown", iterations, nan.copy(), history, float("nan"), nan.copy())

    # -- start: X = X0, AX = A X, BX = B X, the first Rayleigh-Ritz -----------------------------------------------------------
    ws.reset()
    ws.Wp[:, :k].copy_(X0.A)
    Q[:, :k].copy_(X0.A)
    product(A, 3 * k)
    if sparse_b:
        if compute_partition_hash(_spmm_plan(B, Wp)[0].result_partition) != a_hash:
            raise ValueError("lobpcg: B must be partitioned like the rows of A, rows and columns")
        product(B, 6 * k)
    else:
        torch.mul(Q[:, :k], B.v[:, None], out=Q[:, 6 * k:7 * k])
    gram()

    def first(sums, G):
        G_A, G_B = grams_gen(G, k, k)
        if not (np.all(np.isfinite(G_A)) and np.all(np.isfinite(G_B))) or not positive_on_basis(G_B):
            return _BREAKDOWN, np.zeros(k), np.zeros(k), np.zeros(0), None, float("nan")
        th, C, every = rayleigh_ritz(G_A, G_B, k, which)
        if len(th) < k:
            return _DEFICIENT, np.zeros(k), np.zeros(k), np.zeros(0), None, 0.0
        return _GO, np.zeros(k), np.zeros(k), th, C, float(np.max(np.abs(every)))

    decision, anorm, rn, scale, theta, upload = exchange_decision(first)
    history: List[float] = []
    if decision == _DEFICIENT:
        raise ValueError("lobpcg: X0 is rank deficient")
    if decision == _BREAKDOWN:
        return broken(0, history)
    combine(upload, 0)

    it = 0
    while True:
        it += 1
        _capi.call("hpcla_lobpcg_residual_gen_f64", comm, at(3 * k), ld, at(6 * k), ld, dptr(ws.up),
                   dptr(minv.v) if minv is not None else None, None if sparse_b else dptr(B.v), at(k), ld,
                   dptr(ws.Wp) if n_loc else None, ws.pitch, None if sparse_b else at(7 * k), 0 if sparse_b else ld, n_loc, k,
                   dptr(sums_dev), dptr(ws.rwork), current_stream_ptr())
        product(A, 4 * k)
        if sparse_b:
            product(B, 7 * k)
        gram()
        m = 2 * k if it == 1 else 3 * k
        prev_theta, prev_anorm = theta, anorm
        decision, anorm, rn, scale, theta, upload = exchange_decision(
            lambda sums, G: decide_gen(sums, *grams_gen(G, k, m), prev_theta, prev_anorm, it, k, which, tol, maxiter))
        if decision == _BREAKDOWN:
            return broken(it, history)
        history.append(float(rn.max()))
        if decision != _GO:
            X = _block(A, Q[:, :k].clone())
            return theta, X, LobpcgInfo(decision == _CONVERGED, _STATUS[decision], it, rn, history, anorm, scale)
        combine(upload, m - k)
