"""Shared cases of the truncated SVD (``hp.svds``) and a numpy restatement of its loop.

The restatement is plain arrays; it follows the device loop's gate order and rounding order literally (csrc/solvers.hip,
``svds_steps_impl``; the kernels in csrc/vecops.hip and csrc/eigsh.hip): the start is a division by ``sqrt(v0.v0)``, the running
subtractions of the two Gram-Schmidt passes of either half run over the basis columns in ascending order,
``B[i, j] = g1[i] + g2[i]``, ``B[j, j] = sqrt(aa)``, ``beta[j] = sqrt(bb)``, gates N, Z, N' and Z' are tested where the device
tests them, the host's cycle end (the assembly of B, ``numpy.linalg.svd``, the estimates, the stop rules, the choice of p) is
stated again here and not imported from the package, and the restart forms each new column as ``acc = V_0 S[0, j];
acc = acc + V_i S[i, j]`` with i ascending (``_eigsh_cases.rotate``).  It is an independent statement of the algorithm, not of
the device's summation order: ``dot`` can be swapped (``_bicgstab_cases.DOTS``: four summation orders) to measure how far the
order alone moves B, the singular values and the step counts, which is where the margins of tests/test_gpu_svds.py come from
(tests/test_svds_cases.py re-measures and prints them).

Cases (v0 = numpy.random.default_rng(seed).uniform(-1, 1, N), seed 0)
  tall(nx, ny)     ``_lsqr_cases.tall``: 2n x n, the 5-point matrix stacked on a diagonal; 24 x 20 (960 x 480) and, for the first
                   cycle alone, 65 x 63 (8190 x 4095: an odd local length on the right side, two reduction workgroups).
  wide(nx, ny)     its transpose, n x 2n.
  plain            ``_eigsh_cases.plain_poisson`` at 24 x 20: square, symmetric; its singular values are its eigenvalues.
  exact            diag(1..12) with v0 = e_3 (gate Z' after one step) and with the default start at ncv = 12 (one cycle); a
                   rank-deficient diagonal stacked on a zero block (gate Z).

Figures of this restatement, tol = 1e-10, are printed by tests/test_svds_cases.py and quoted in tests/test_gpu_svds.py.
"""
import math

import numpy as np

from tests import _bicgstab_cases as bc
from tests import _eigsh_cases as ec
from tests import _lsqr_cases as lc
from tests import _pcg_cases as pc

DOTS = bc.DOTS
TOL = 1e-10
T_RTOL = ec.T_RTOL         # first-cycle B and beta against the restatement, relative to max|B|: the project's margin, 1e-12
VAL_RTOL = 1e-12           # singular values against numpy.linalg.svd of the dense matrix, relative to anorm
SPREAD = 1e-13             # bound on the CPU spread of B and of the singular values over the four summation orders
SIZE = (24, 20)
RANK_CASE = ("tall", 4, 20)
LARGE_SIZE = pc.LARGE_SIZE  # 65 x 63, tall: 8190 x 4095
# (matrix, k, ncv) of the convergence tests
CONVERGENCE = [(name, k, ncv) for name in ("tall", "wide", "plain") for k, ncv in ((4, 20), (1, 8), (16, 64))]


def matrix(orc, name, size=SIZE):
    """(rowptr, colidx, vals, ncols), global 0-based CSR (int64 indices)."""
    if name == "plain":
        rowptr, colidx, vals = ec.plain_poisson(orc, *size)
        return rowptr, colidx, vals, len(rowptr) - 1
    return lc.CASES[name](orc, *size)[:4]


def matrices(orc):
    return {name: matrix(orc, name) for name in ("tall", "wide", "plain")}


def dense_singular_values(rowptr, colidx, vals, ncols):
    return np.linalg.svd(lc.dense_of(rowptr, colidx, vals, ncols), compute_uv=False)


def rank_deficient():
    """diag(4, 0, 0, 0) stacked on a 2 x 4 zero block (6 x 4, rank 1), as (rowptr, colidx, vals, ncols)."""
    rowptr, colidx, vals = pc.diag_matrix(np.array([4.0, 0.0, 0.0, 0.0]))
    rowptr = np.concatenate([rowptr, np.full(2, rowptr[-1])])
    return (*lc.csr(rowptr, colidx, vals), 4)


# Three null directions next to e_0.  Every value up to gate Z is exact in any summation order: V_0 = (1, 1, 1, 1) / 2,
# u = (2, 0, ...), alpha_0 = 2, U_0 = e_0, v = 4 e_0, h1 = 2, v = (3, -1, -1, -1), h2 = 0, beta_0 = sqrt(12); then u = A V_1 =
# t e_0, g1 = t, u - t U_0 = 0: gate Z at column 1 with one finished triplet, sqrt(2^2 + t^2) = 4.
RANK_DEFICIENT_V0 = np.array([1.0, 1.0, 1.0, 1.0])


def start_vector(n, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def subtract(w, W, h):
    """The running subtraction over the columns in ascending order (W: columns as rows)."""
    for i in range(len(h)):
        w = w - h[i] * W[i]
    return w


def small_step(side, j, c1, c2, nn, B, beta):
    """The small step of one half of column j on B (B[i, j]) and beta, updated in place; c1, c2 are that half's two passes'
    coefficients (used on the left side only).  Returns (status, divisor): "breakdown" (gates N, N': nothing stored),
    "invariant" (gates Z, Z': stored) or "running"."""
    if nn != nn:
        return "breakdown", None
    r = math.sqrt(nn)
    if side == 0:
        for i in range(j):
            B[i, j] = c1[i] + c2[i]
        B[j, j] = r
    else:
        beta[j] = r
    return ("invariant" if nn == 0.0 else "running"), r


def cycle(A, At, U, V, B, beta, p, m, dot):
    """Columns p .. m-1 on U (m x M rows), V ((m + 1) x N rows), B and beta in place.  Returns (status, finished triplets c,
    gate_z: the left half stopped, so B holds column c too)."""
    for j in range(p, m):
        u = A(V[j])
        g1 = np.array([dot(U[i], u) for i in range(j)])
        u = subtract(u, U, g1)
        g2 = np.array([dot(U[i], u) for i in range(j)])
        u = subtract(u, U, g2)
        status, alpha = small_step(0, j, g1, g2, dot(u, u), B, beta)
        if status != "running":
            return status, j, status == "invariant"
        U[j] = u / alpha
        v = At(U[j])
        h1 = np.array([dot(V[i], v) for i in range(j + 1)])
        v = subtract(v, V, h1)
        h2 = np.array([dot(V[i], v) for i in range(j + 1)])
        v = subtract(v, V, h2)
        status, bj = small_step(1, j, h1, h2, dot(v, v), B, beta)
        if status == "breakdown":
            return status, j, False
        if status == "invariant":
            return status, j + 1, False
        V[j + 1] = v / bj
    return "running", m, False


def projected(B, s_kept, p, c, cols):
    """The c x cols upper-triangular projected matrix: diag(s_kept) top-left, the cycle's columns p .. cols-1."""
    out = np.zeros((c, cols))
    for i in range(min(p, c)):
        out[i, i] = s_kept[i]
    for j in range(p, cols):
        r = min(j + 1, c)
        out[:r, j] = B[:r, j]
    return out


def svds(rowptr, colidx, vals, ncols, k=6, ncv=None, tol=TOL, maxiter=None, v0=None, seed=0, dot=bc._dot_np, first_B=None):
    """The solver's loop on the host.  Returns (U (M x k), s (descending), V (N x k), dict(status, converged, iterations,
    restarts, residual_norms, history, anorm)).  ``first_B``: a dict that receives the first cycle's B (m x m) and beta."""
    rowptr, colidx, vals = lc.csr(rowptr, colidx, vals)
    M, N = len(rowptr) - 1, int(ncols)
    n = min(M, N)
    m = min(n, 64, max(2 * k + 1, 20)) if ncv is None else ncv
    maxiter = 10 * n if maxiter is None else maxiter
    rt, ct, vt = lc.transpose_csr(rowptr, colidx, vals, N)
    A = lambda x: pc.matvec(rowptr, colidx, vals, x)
    At = lambda y: pc.matvec(rt, ct, vt, y)
    v0 = start_vector(N, seed) if v0 is None else np.asarray(v0, dtype=np.float64)
    U, V = np.zeros((m, M)), np.zeros((m + 1, N))
    V[0] = v0 / math.sqrt(dot(v0, v0))
    B, beta = np.zeros((m, m)), np.zeros(m)
    p, iterations, restarts, s_kept, history = 0, 0, 0, np.zeros(0), []
    while True:
        B[:], beta[:] = 0.0, 0.0
        with np.errstate(all="ignore"):
            status, c, gate_z = cycle(A, At, U, V, B, beta, p, m, dot)
        if first_B is not None and not first_B:
            first_B.update(B=B.copy(), beta=beta.copy())
        if status == "breakdown":
            return np.zeros((M, k)), np.full(k, np.nan), np.zeros((N, k)), dict(
                status="breakdown", converged=False, iterations=iterations + max(c - p, 0), restarts=restarts,
                residual_norms=np.full(k, np.nan), history=history, anorm=math.nan)
        iterations += c - p
        if c == 0:
            return np.zeros((M, 0)), np.zeros(0), np.zeros((N, 0)), dict(
                status="invariant", converged=False, iterations=iterations, restarts=restarts, residual_norms=np.zeros(0),
                history=[0.0], anorm=0.0)
        cq = c + int(gate_z)
        P, s, Qh = np.linalg.svd(projected(B, s_kept, p, c, cq), full_matrices=False)
        Q = Qh.T
        kk = min(k, c)
        rho = np.zeros(kk) if gate_z else np.abs(beta[c - 1] * P[c - 1, :kk])
        anorm = float(s[0])
        history.append(float(rho.max()))
        if status == "invariant":
            done = ("invariant", c >= k)
        elif np.all(rho <= tol * anorm):
            done = ("converged", True)
        elif iterations >= maxiter:
            done = ("maxiter", False)
        else:
            p = k + (m - k) // 2
            s_kept = s[:p].copy()
            last = V[m].copy()
            V[:p] = ec.rotate(V[:m], Q[:, :p])
            V[p] = last
            U[:p] = ec.rotate(U[:m], P[:, :p])
            restarts += 1
            continue
        return ec.rotate(U[:c], P[:, :kk]).T, s[:kk].copy(), ec.rotate(V[:cq], Q[:, :kk]).T, dict(
            status=done[0], converged=done[1], iterations=iterations, restarts=restarts, residual_norms=rho, history=history,
            anorm=anorm)


def figures(rowptr, colidx, vals, ncols, U, s, V, info, sv, tol=TOL):
    """The accuracy figures of one solve against the dense singular values ``sv``: value error, the two true residuals, the
    estimate against the true residual (all relative to anorm; the first residual also in units of tol anorm), the absolute
    orthogonality of U and V, and the smallest u_i' A v_i."""
    rowptr, colidx, vals = lc.csr(rowptr, colidx, vals)
    rt, ct, vt = lc.transpose_csr(rowptr, colidx, vals, ncols)
    k, anorm = len(s), info["anorm"] if isinstance(info, dict) else info.anorm
    rho = info["residual_norms"] if isinstance(info, dict) else info.residual_norms
    AV = np.stack([pc.matvec(rowptr, colidx, vals, V[:, i]) for i in range(k)], axis=1)
    AtU = np.stack([pc.matvec(rt, ct, vt, U[:, i]) for i in range(k)], axis=1)
    true = np.linalg.norm(AtU - V * s, axis=0)
    return dict(err=np.abs(s - sv[:k]).max() / anorm, res=true.max() / (tol * anorm),
                left=np.linalg.norm(AV - U * s, axis=0).max() / anorm, est=np.abs(true - rho).max() / anorm,
                orth=max(np.abs(U.T @ U - np.eye(k)).max(), np.abs(V.T @ V - np.eye(k)).max()),
                sign=float(np.einsum("ij,ij->j", U, AV).min()))
