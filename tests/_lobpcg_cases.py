"""Shared cases of the block eigensolver (``hp.lobpcg``) and a numpy restatement of its whole solve.

The restatement is plain arrays.  It imports ONE thing from the package, the host's whitened Rayleigh-Ritz step
(``rayleigh_ritz``, pure numpy), and states everything else again: the start, the decision order of step 4, the growth of
``anorm``, the choice of the Gram blocks in iteration 1, and the rounding orders of the two kernels --

  residual   t = theta_j * X[r, j];  d = AX[r, j] - t;  W[r, j] = minv[r] * d        (three separately rounded operations)
  combine    px = 0;  px = px + S[r, i] * C[i, j], i < k ascending;  pp the same over i >= k;  X' = px + pp;  P' = pp

so the kernels alone are compared bit for bit.  The Gram matrices are NOT a statement of the device's summation order:
``gram`` can be swapped (``GRAMS``: four summation orders) and ``noise`` adds a relative perturbation to every Gram entry, to
measure how far rounding alone moves the iteration counts, the values and the residuals.  That is where the margins of
tests/test_gpu_lobpcg.py come from; tests/test_lobpcg_cases.py re-measures and prints them.

Matrices (dense on the host, CSR for the device)
  poisson16   the oracle's 5-point matrix on the SQUARE 16 x 16 grid: lambda_ij = lambda_ji, every off-diagonal pair is double
  triple      diag(1, 1, 1, 2, linspace(3, 50, 196)): a triple eigenvalue
  rand300     300 x 300 random symmetric, density 0.03, entries uniform(-1, 1);  rand300s the same shifted by -0.5 I
  ddom257 / ddom513   diag(linspace(1, 1000, n)) + a sparse symmetric perturbation (4 entries of uniform(-0.1, 0.1) per row):
              positive definite and diagonally dominant, the Jacobi case

Figures of this restatement at tol = 1e-8, seed 0 (tests/test_lobpcg_cases.py::test_restatement_converges_on_every_case prints
them): iterations are in ITERATIONS below; values within 4.3e-15 ||A||, true residuals <= 0.98 tol anorm, X'X - I <= 8.3e-15.
"""
import math
import sys

import numpy as np

from tests import _bicgstab_cases as bc
from tests import _eigsh_cases as ec

TOL = 1e-8
VAL_RTOL = 1e-12            # theta and anorm of the first iterations against the restatement, relative to anorm
RED_RTOL = 1e-12            # the project's margin for its reductions, relative to the sum of |terms|
ORTH_TOL = 1e-12
# |info.residual_norms - true residual| / anorm: the drift of the implicitly updated AX.  Every combine adds a rounding error of
# a few epsilon anorm to AX, so about iterations x epsilon = 120 x 1.1e-16 ~ 1.3e-14 at most; the restatement's largest over
# the cases is 4.2e-16.  The CPU test re-measures it against this bound; the GPU test adds it to 1e-12 anorm.
DRIFT = 2e-14
# iterations of the restatement (seed 0, tol 1e-8, numpy's matmul as the Gram order), in the order of CONVERGENCE
ITERATIONS = [107, 93, 87, 75, 52, 71, 110, 75, 102, 107, 7, 18, 16, 28, 9, 17, 16, 26]


def host():
    """The package's host part (linearalgebrampi.jl_amd/lobpcg.py): importable without a device."""
    import hpcla_amd as hp
    return sys.modules[hp.lobpcg.__module__]


# ---- matrices ----------------------------------------------------------------------------------------------------------------
def csr_of(dense):
    n = dense.shape[0]
    mask = dense != 0
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    colidx = np.nonzero(mask)[1].astype(np.int64)
    return rowptr, colidx, dense[mask].astype(np.float64), n


def _symmetric_sparse(n, per_row, scale, seed):
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    count = n * per_row // 2
    i, j = rng.integers(0, n, count), rng.integers(0, n, count)
    v = rng.uniform(-scale, scale, count)
    keep = i != j
    M[i[keep], j[keep]] = v[keep]
    M = np.triu(M, 1) + np.triu(M.T, 1)          # one value per unordered pair
    return M + M.T


def rand300(shift=0.0):
    n = 300
    rng = np.random.default_rng(300)
    U = np.triu(np.where(rng.uniform(0, 1, (n, n)) < 0.03, rng.uniform(-1, 1, (n, n)), 0.0))
    return U + np.triu(U, 1).T + shift * np.eye(n)


def ddom(n):
    return np.diag(np.linspace(1.0, 1000.0, n)) + _symmetric_sparse(n, 4, 0.1, n)


def dense_matrices(orc):
    return {"poisson16": bc.dense_of(*ec.plain_poisson(orc, 16, 16)),
            "triple": np.diag(np.concatenate([[1.0, 1.0, 1.0, 2.0], np.linspace(3.0, 50.0, 196)])),
            "rand300": rand300(), "rand300s": rand300(-0.5), "ddom257": ddom(257), "ddom513": ddom(513)}


# (matrix, k, which, M)
CONVERGENCE = ([("poisson16", 4, "SA", None), ("poisson16", 4, "LA", None), ("poisson16", 2, "SA", None), ("poisson16", 3, "SA", None),
                ("triple", 4, "SA", None),
                ("rand300", 5, "LA", None), ("rand300", 5, "SA", None), ("rand300", 3, "SA", None),
                ("rand300s", 5, "SA", None), ("rand300s", 3, "LA", None)]
               + [(f"ddom{n}", k, "SA", "jacobi") for n in (257, 513) for k in (1, 7, 8, 16)])
SPREAD_CASES = [("poisson16", 4, "SA", None), ("rand300", 5, "LA", None), ("ddom257", 8, "SA", "jacobi")]
FIRST_CASES = SPREAD_CASES[:2]          # the first iterations are compared with the restatement on these (well conditioned) two
RANK_CASE = ("poisson16", 4)


def poisson16_exact(k, which):
    """The k wanted eigenvalues of the 16 x 16 grid from the closed form 4 - 2cos(i pi/17) - 2cos(j pi/17), ascending."""
    c = 2.0 * np.cos(np.arange(1, 17) * math.pi / 17)
    ev = np.sort((4.0 - c[:, None] - c[None, :]).reshape(-1))
    return ev[:k] if which == "SA" else ev[-k:]


def reference_values(ev, k, which):
    return ev[:k] if which == "SA" else ev[-k:]


# ---- the kernels' rounding orders --------------------------------------------------------------------------------------------
def residual(X, AX, theta, minv=None):
    """(W, d): the block the kernel stores and the residual before ``minv`` whose column sums of squares it returns."""
    t = theta[None, :] * X
    d = AX - t
    return (minv[:, None] * d if minv is not None else d), d


def combine(S, C, k, c_rest):
    """(X', P') of one block: S is n x (>= k + c_rest), C is (k + c_rest) x k.  P' is zero-sized with c_rest = 0."""
    n = S.shape[0]
    px, pp = np.zeros((n, k)), np.zeros((n, k))
    for i in range(k):
        px = px + S[:, i:i + 1] * C[i:i + 1, :]
    for i in range(k, k + c_rest):
        pp = pp + S[:, i:i + 1] * C[i:i + 1, :]
    return px + pp, (pp if c_rest else np.zeros((n, 0)))


# ---- Gram matrices under four summation orders ---------------------------------------------------------------------------------
def _gram_matmul(S, Y):
    return S.T @ Y


def _gram_reversed(S, Y):
    return S[::-1].copy().T @ Y[::-1].copy()


def _gram_chunked(S, Y):
    out = np.zeros((S.shape[1], Y.shape[1]))
    for r in range(0, S.shape[0], 64):
        out = out + S[r:r + 64].T @ Y[r:r + 64]
    return out


def _gram_sequential(S, Y):
    out = np.zeros((S.shape[1], Y.shape[1]))
    for r in range(S.shape[0]):
        out = out + S[r][:, None] * Y[r][None, :]
    return out


GRAMS = {"matmul": _gram_matmul, "reversed": _gram_reversed, "chunked": _gram_chunked, "sequential": _gram_sequential}


# ---- the solve -----------------------------------------------------------------------------------------------------------------
def start_block(n, k, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, k))


def lobpcg(A, k, which="SA", X0=None, minv=None, tol=TOL, maxiter=None, seed=0, gram=_gram_matmul, noise=0.0, noise_seed=0,
           trace=None):
    """The solver's loop on a dense symmetric ``A``.  Returns (vals, X, dict(status, converged, iterations, residual_norms,
    history, anorm)).  ``noise``: every Gram entry G_ij gets ``noise * sqrt(G_ii G_jj) * standard normal`` added (G_ii of S'S).
    ``trace``: a list that receives (theta, anorm) after every Rayleigh-Ritz step, the start's first."""
    RR = host().rayleigh_ritz
    n = A.shape[0]
    maxiter = 10 * n if maxiter is None else maxiter
    nrng = np.random.default_rng(noise_seed)

    def grams(S, AS):
        G_B, G_A = gram(S, S), gram(S, AS)
        if noise:
            d = np.sqrt(np.abs(np.diag(G_B)))
            G_B = G_B + noise * d[:, None] * d[None, :] * nrng.standard_normal(G_B.shape)
            G_A = G_A + noise * d[:, None] * d[None, :] * nrng.standard_normal(G_A.shape)
        return G_A, G_B

    def info(status, it, rn, history, anorm):
        return dict(status=status, converged=status == "converged", iterations=it, residual_norms=rn, history=history, anorm=anorm)

    X = start_block(n, k, seed) if X0 is None else np.array(X0, dtype=np.float64)
    AX = A @ X
    G_A, G_B = grams(X, AX)
    history = []
    if not (np.all(np.isfinite(G_A)) and np.all(np.isfinite(G_B))):
        return np.full(k, np.nan), np.zeros((n, k)), info("breakdown", 0, np.full(k, np.nan), history, float("nan"))
    theta, C, every = RR(G_A, G_B, k, which)
    if len(theta) < k:
        raise ValueError("lobpcg: X0 is rank deficient")
    X, _ = combine(X, C, k, 0)
    AX, _ = combine(AX, C, k, 0)
    anorm = float(np.max(np.abs(every)))
    if trace is not None:
        trace.append((theta.copy(), anorm))
    P = AP = np.zeros((n, k))
    it = 0
    while True:
        it += 1
        W, R = residual(X, AX, theta, minv)
        rn2 = (R * R).sum(axis=0)
        AW = A @ W
        m = 2 * k if it == 1 else 3 * k
        S, AS = np.hstack([X, W, P])[:, :m], np.hstack([AX, AW, AP])[:, :m]
        G_A, G_B = grams(S, AS)
        if not (np.all(np.isfinite(rn2)) and np.all(np.isfinite(G_A)) and np.all(np.isfinite(G_B))):
            return np.full(k, np.nan), np.zeros((n, k)), info("breakdown", it, np.full(k, np.nan), history, float("nan"))
        rn = np.sqrt(rn2)
        history.append(float(rn.max()))
        if np.all(rn <= tol * anorm):
            return theta, X, info("converged", it, rn, history, anorm)
        if it > maxiter:
            return theta, X, info("maxiter", it, rn, history, anorm)
        theta, C, every = RR(G_A, G_B, k, which)
        anorm = max(anorm, float(np.max(np.abs(every))))
        if trace is not None:
            trace.append((theta.copy(), anorm))
        X, P = combine(S, C, k, m - k)
        AX, AP = combine(AS, C, k, m - k)


def jacobi_weights(A):
    return 1.0 / np.abs(np.diag(A))


def figures(A, ev, vals, X, info, k, which):
    """(eigenvalue error / ||A||_2, true residual / (tol anorm), ||X'X - I||_max, |residual_norms - true| / anorm)."""
    norm2 = float(np.max(np.abs(ev)))
    true = np.linalg.norm(A @ X - X * vals[None, :], axis=0)
    return (float(np.abs(vals - reference_values(ev, k, which)).max() / norm2), float(true.max() / (TOL * info["anorm"])),
            float(np.abs(X.T @ X - np.eye(k)).max()), float(np.abs(true - info["residual_norms"]).max() / info["anorm"]))
