"""Shared cases of the block eigensolver on a pencil (``hp.lobpcg`` with ``B``: ``A x = lambda B x``) and a numpy restatement
of its whole solve.

Like tests/_lobpcg_cases.py, which it builds on and does not change, the restatement is plain arrays.  It imports ONE thing from
the package, the host's whitened Rayleigh-Ritz step (``rayleigh_ritz``, pure numpy), and states everything else again: the start
with its third block ``BX``, the decision order of step 4 with the scale-free stop rule and the test of the diagonal of
``S'BS``, the growth of ``anorm``, the choice of the Gram blocks in iteration 1, and the rounding order of the residual kernel --

  residual   t = theta_j * BX[r, j];  d = AX[r, j] - t;  w = minv[r] * d;  W[r, j] = w;  BW[r, j] = bdiag[r] * w
             (every operation separately rounded);  three sums per column: d^2, AX^2, BX^2

-- so the kernel alone is compared bit for bit.  The combine is ``_lobpcg_cases.combine``, applied to three blocks.

Matrices (dense on the host, CSR for the device): linear finite elements on a uniform grid with Dirichlet ends
  fem1d(n)   K = tridiag(-1, 2, -1) / h,  M = tridiag(1, 4, 1) h / 6,  h = 1 / (n + 1)
  fem2d(N)   K = K1 (x) M1 + M1 (x) K1,  M = M1 (x) M1 on the N x N grid: both 9-point matrices; the spectrum of the pencil is
             symmetric in the two grid directions, so lambda_ij = lambda_ji is double for i != j
  lumped     diag(rowsum(M)): the mass matrix as an HPCVector of positive weights, or as a sparse diagonal matrix

Figures of this restatement at tol = 1e-8, seed 0 (tests/test_lobpcg_gen_cases.py::test_restatement_converges_on_every_case
prints them): iterations are in ITERATIONS below; eigenvalues within 2.7e-6 of the bound of the GPU test, true residuals
<= 0.97 tol x the true scale, X'BX - I <= 3.7e-15.
"""
import numpy as np

from tests import _lobpcg_cases as lc

TOL = lc.TOL
MAX_K = 16

# (matrices, B form, k, which); the lumped k = 5 "SA" case is left out on purpose: the restatement stagnates at 2.3 tol there
# (the Gram-matrix limit that the solver's docstring names)
CONVERGENCE = [("fem2d16", "consistent", 4, "SA"), ("fem2d16", "consistent", 4, "LA"),
               ("fem2d16", "lumped", 4, "SA"), ("fem2d16", "lumped", 4, "LA"),
               ("fem2d16", "consistent", 5, "SA"), ("fem1d200", "consistent", 3, "LA")]
# iterations of the restatement (seed 0, tol 1e-8, numpy's matmul as the Gram order), in the order of CONVERGENCE.  A record, not
# a yardstick: the counts of the long runs move by a few with the summation order of the Gram matrices (the prototype this scheme
# was tried with gave 166 and 84 where this file gives 169 and 85), so the tests hold them to the suite's cap, 1.5 x + 5
ITERATIONS = [78, 169, 85, 78, 53, 282]
FIRST_CASE = ("fem2d16", 4, "SA")       # the first iterations are compared with the restatement here, both forms of B
RANK_CASE = ("fem2d16", 4, "SA")


def host():
    return lc.host()


# ---- matrices ----------------------------------------------------------------------------------------------------------------
def fem1d(n):
    """(K, M) of linear elements on n interior points of (0, 1)."""
    h = 1.0 / (n + 1)
    off = np.eye(n, k=1) + np.eye(n, k=-1)
    return (2.0 * np.eye(n) - off) / h, (4.0 * np.eye(n) + off) * h / 6.0


def fem2d(N):
    K1, M1 = fem1d(N)
    return np.kron(K1, M1) + np.kron(M1, K1), np.kron(M1, M1)


def lumped(M):
    """The row sums of M: the diagonal of the lumped mass matrix."""
    return M.sum(axis=1)


def pencils():
    """name -> (K, M), dense."""
    return {"fem2d16": fem2d(16), "fem1d200": fem1d(200)}


def b_of(M, form):
    """The dense B of a case: M itself, or its lumped diagonal as a matrix."""
    return M if form == "consistent" else np.diag(lumped(M))


# ---- the kernel's rounding order ---------------------------------------------------------------------------------------------
def residual_gen(AX, BX, theta, minv=None, bdiag=None):
    """(W, BW, d): the block the kernel stores, ``bdiag .* W`` (None without ``bdiag``) and the residual before ``minv``."""
    t = theta[None, :] * BX
    d = AX - t
    W = minv[:, None] * d if minv is not None else d
    return W, (bdiag[:, None] * W if bdiag is not None else None), d


def sums_gen(d, AX, BX):
    """The 48 doubles of the residual kernel from numpy's column sums: group q at 16 q, entries j >= k zero."""
    k = d.shape[1]
    out = np.zeros(3 * MAX_K)
    for q, block in enumerate((d, AX, BX)):
        out[MAX_K * q:MAX_K * q + k] = (block * block).sum(axis=0)
    return out


def decide_gen(sums, G_A, G_B, theta, anorm, it, k, which, tol, maxiter):
    """The decision order of step 4 with a B, restated: (status or None, rn, scale, theta, C, anorm)."""
    used = np.concatenate([sums[MAX_K * q:MAX_K * q + k] for q in range(3)])
    nan = np.full(k, np.nan)
    if not (np.all(np.isfinite(used)) and np.all(np.isfinite(G_A)) and np.all(np.isfinite(G_B))):
        return "breakdown", nan, nan, theta, None, anorm
    if np.any(np.diag(G_B) < 0):                                 # B is not positive definite on a basis column
        return "breakdown", nan, nan, theta, None, anorm
    rn = np.sqrt(sums[:k])
    scale = np.sqrt(sums[MAX_K:MAX_K + k]) + np.abs(theta) * np.sqrt(sums[2 * MAX_K:2 * MAX_K + k])
    if np.all(rn <= tol * scale):
        return "converged", rn, scale, theta, None, anorm
    if it > maxiter:
        return "maxiter", rn, scale, theta, None, anorm
    theta, C, every = host().rayleigh_ritz(G_A, G_B, k, which)
    return None, rn, scale, theta, C, max(anorm, float(np.max(np.abs(every))))


# ---- the solve -----------------------------------------------------------------------------------------------------------------
def lobpcg_gen(A, B, k, which="SA", minv=None, tol=TOL, maxiter=None, X0=None, seed=0, gram=lc.GRAMS["matmul"], trace=None):
    """The solver's loop on a dense symmetric ``A`` and ``B``: a dense symmetric positive definite matrix, or a 1-D array of
    positive weights (the diagonal form: ``BW`` then comes from the residual step, as on the device).  Returns (vals, X,
    dict(status, converged, iterations, residual_norms, residual_scales, history, anorm)).  ``trace``: a list that receives
    (theta, anorm) after every Rayleigh-Ritz step, the start's first."""
    RR = host().rayleigh_ritz
    n = A.shape[0]
    maxiter = 10 * n if maxiter is None else maxiter
    bdiag = B if B.ndim == 1 else None

    def info(status, it, rn, scale, history, anorm):
        return dict(status=status, converged=status == "converged", iterations=it, residual_norms=rn, residual_scales=scale,
                    history=history, anorm=anorm)

    def broken(it, history):
        nan = np.full(k, np.nan)
        return nan, np.zeros((n, k)), info("breakdown", it, nan.copy(), nan.copy(), history, float("nan"))

    X = lc.start_block(n, k, seed) if X0 is None else np.array(X0, dtype=np.float64)
    AX = A @ X
    BX = bdiag[:, None] * X if bdiag is not None else B @ X
    G_A, G_B = gram(X, AX), gram(X, BX)
    history = []
    if not (np.all(np.isfinite(G_A)) and np.all(np.isfinite(G_B))) or np.any(np.diag(G_B) < 0):
        return broken(0, history)
    theta, C, every = RR(G_A, G_B, k, which)
    if len(theta) < k:
        raise ValueError("lobpcg: X0 is rank deficient")
    X, AX, BX = (lc.combine(blk, C, k, 0)[0] for blk in (X, AX, BX))
    anorm = float(np.max(np.abs(every)))
    if trace is not None:
        trace.append((theta.copy(), anorm))
    P = AP = BP = np.zeros((n, k))
    it = 0
    while True:
        it += 1
        W, BW, d = residual_gen(AX, BX, theta, minv, bdiag)
        sums = sums_gen(d, AX, BX)
        AW = A @ W
        if bdiag is None:
            BW = B @ W
        m = 2 * k if it == 1 else 3 * k
        S, AS, BS = (np.hstack(blocks)[:, :m] for blocks in ((X, W, P), (AX, AW, AP), (BX, BW, BP)))
        status, rn, scale, theta, C, anorm = decide_gen(sums, gram(S, AS), gram(S, BS), theta, anorm, it, k, which, tol, maxiter)
        if status == "breakdown":
            return broken(it, history)
        history.append(float(rn.max()))
        if status is not None:
            return theta, X, info(status, it, rn, scale, history, anorm)
        if trace is not None:
            trace.append((theta.copy(), anorm))
        (X, P), (AX, AP), (BX, BP) = (lc.combine(blk, C, k, m - k) for blk in (S, AS, BS))


# ---- the figures the tests check -------------------------------------------------------------------------------------------------
def reference(K, Bd, k, which):
    """(the k wanted eigenvalues of the pencil in ascending order, lambda_min(B)) from scipy.linalg.eigh on the dense pair."""
    import scipy.linalg
    ev = scipy.linalg.eigh(K, Bd, eigvals_only=True)
    return lc.reference_values(ev, k, which), float(np.linalg.eigvalsh(Bd)[0])


def figures(K, Bd, want, bmin, vals, X, tol=TOL):
    """(eigenvalue error / its bound, true residual / (tol x true scale), ||X'BX - I||_max), everything from dense numpy.
    The bound: for a B-normalised x, |theta - lambda| <= ||B^{-1/2} r|| <= ||r|| / sqrt(lambda_min(B)); a converged pair has
    ||r|| <= tol (||A x|| + |theta| ||B x||); the factor 2 as elsewhere in the suite."""
    AX, BX = K @ X, Bd @ X
    true = np.linalg.norm(AX - BX * vals[None, :], axis=0)
    scale = np.linalg.norm(AX, axis=0) + np.abs(vals) * np.linalg.norm(BX, axis=0)
    bound = 2 * tol * scale / np.sqrt(bmin)
    return (float((np.abs(vals - want) / bound).max()), float((true / (tol * scale)).max()),
            float(np.abs(X.T @ BX - np.eye(X.shape[1])).max()))
