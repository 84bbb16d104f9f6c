"""Shared cases of the least-squares solver (``hp.lsqr``) and a numpy restatement of its loop.

The restatement is plain arrays; it follows the device loop's gate order and rounding order literally (csrc/solvers.hip,
``lsqr_iterations_impl``; the kernels in csrc/vecops.hip): uhat and vhat are kept unnormalised next to their norms beta and
alpha, every update is a separately rounded divide / multiply / subtract in the order the kernels use, the scalars of the
step are formed by the same expressions, and gate U and the three stop gates are tested where the device tests them.  It is
an independent statement of the algorithm, not of the device's summation order: ``dot`` can be swapped
(``_bicgstab_cases.DOTS``: four summation orders) to measure how far the order alone moves histories and iteration counts,
which is where the margins of tests/test_gpu_lsqr.py come from (tests/test_lsqr_cases.py re-measures and prints them).

Cases
  tall(nx, ny)    2n x n, n = nx ny: rows 0 .. n-1 the oracle's unscaled 5-point ``poisson2d_rows(nx, ny)``, rows n .. 2n-1 the
                  diagonal 0.5 (1 + u_i), u = fill_uniform(0, n, 0xD1A6); b = fill_uniform(0, 2n, 0xBEEF): inconsistent.
                  Condition number 10.8 .. 11.2.  33x31: n = 1023, m = 2046 (an odd and an even length: the scalar tail).
  wide(nx, ny)    the transpose of tall (n x 2n), columns ascending within a row; b = fill_uniform(0, n, 0xBEEF): consistent,
                  LSQR from x0 = 0 returns the minimum-norm solution.
  exact           diag(2, 0), diag(1, 0), [[1, 0], [0, 1], [1, 1]], the identity, diag(1, NaN), b = 0 (values in
                  tests/test_lsqr_cases.py).
"""
import math

import numpy as np

from tests import _bicgstab_cases as bc
from tests import _pcg_cases as pc

SIZES = pc.SIZES
DOTS = bc.DOTS
HEAD = 13                  # history entries compared with the restatement
LARGE_SIZE = pc.LARGE_SIZE  # 65 x 63, tall: 8190 x 4095; the same head, HIST_RTOL is 80 times the CPU spread there (1.2e-14)
HIST_RTOL = 1e-12          # ... to this margin: 20 x the CPU spread of four summation orders (measured <= 7.1e-15)
DAMPS = (0.0, 0.3)
RANK_SIZE = (24, 20)       # the case of the history-head and rank tests


def csr(rowptr, colidx, vals):
    return np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64), np.asarray(vals, dtype=np.float64)


def transpose_csr(rowptr, colidx, vals, ncols):
    """CSR of the transpose, columns ascending within a row (the order transpose(A).materialize() stores)."""
    rowptr, colidx, vals = csr(rowptr, colidx, vals)
    row_of = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    order = np.lexsort((row_of, colidx))
    counts = np.bincount(colidx, minlength=ncols)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), row_of[order], vals[order]


def dense_of(rowptr, colidx, vals, ncols):
    m = len(rowptr) - 1
    dense = np.zeros((m, ncols))
    dense[np.repeat(np.arange(m), np.diff(rowptr)), colidx] = vals
    return dense


def tall(orc, nx, ny):
    """(rowptr, colidx, vals, ncols, b) of the 2n x n case, global 0-based CSR (int64 indices)."""
    n = nx * ny
    rows = orc.poisson2d_rows(nx, ny, 0, n)
    d = 0.5 * (1.0 + orc.fill_uniform(0, n, pc.SEED_SCALE))
    rowptr = np.concatenate([rows.rowptr, rows.rowptr[-1] + np.arange(1, n + 1)]).astype(np.int64)
    colidx = np.concatenate([rows.colidx, np.arange(n)]).astype(np.int64)
    vals = np.concatenate([rows.vals, d])
    return rowptr, colidx, vals, n, orc.fill_uniform(0, 2 * n, pc.SEED_RHS)


def wide(orc, nx, ny):
    """(rowptr, colidx, vals, ncols, b) of the n x 2n case: the transpose of tall."""
    rowptr, colidx, vals, n, _ = tall(orc, nx, ny)
    rt, ct, vt = transpose_csr(rowptr, colidx, vals, n)
    return rt, ct, vt, 2 * n, orc.fill_uniform(0, n, pc.SEED_RHS)


CASES = {"tall": tall, "wide": wide}

# the exact and degenerate cases: (rowptr, colidx, vals, ncols)
DIAG20 = (*csr([0, 1, 2], [0, 1], [2.0, 0.0]), 2)
DIAG10 = (*csr([0, 1, 2], [0, 1], [1.0, 0.0]), 2)
DIAG1NAN = (*csr([0, 1, 2], [0, 1], [1.0, math.nan]), 2)
THREE_BY_TWO = (*csr([0, 1, 2, 4], [0, 1, 0, 1], [1.0, 1.0, 1.0, 1.0]), 2)       # [[1, 0], [0, 1], [1, 1]]


def identity(n):
    return (*pc.diag_matrix(np.ones(n)), n)


def augmented(dense, b, damp):
    """The dense system [A; damp I], [b; 0]."""
    m, n = dense.shape
    if damp == 0.0:
        return dense, b
    return np.vstack([dense, damp * np.eye(n)]), np.concatenate([b, np.zeros(n)])


def lsqr(rowptr, colidx, vals, ncols, b, damp=0.0, rtol=1e-8, atol=0.0, ntol=1e-8, maxiter=None, x0=None, dot=bc._dot_np):
    """The solver's loop on the host.  Returns (x, iterations, status, residual_norms, normal_residual_norms, anorm)."""
    rowptr, colidx, vals = csr(rowptr, colidx, vals)
    n = int(ncols)
    maxiter = 10 * n if maxiter is None else maxiter
    rt, ct, vt = transpose_csr(rowptr, colidx, vals, n)
    A = lambda v: pc.matvec(rowptr, colidx, vals, v)
    At = lambda u: pc.matvec(rt, ct, vt, u)
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    uh = b.copy() if x0 is None else b - A(x)
    uu = dot(uh, uh)
    beta = math.sqrt(uu) if uu >= 0 else math.nan
    bb = uu if x0 is None else dot(b, b)
    if bb == 0.0:
        return np.zeros(n), 0, "converged", [0.0], [0.0], 0.0
    thr2 = max(rtol * math.sqrt(bb), atol) ** 2
    ntol2 = ntol * ntol
    hist_r = [beta]
    with np.errstate(all="ignore"):
        tv = At(uh)
        if uu == 0.0:                                               # gate U of the setup: vhat stays 0
            vh, vv = np.zeros(n), 0.0
        else:
            vh = tv / beta
            vv = dot(vh, vh)
        alpha = _sqrt(vv)
        hist_n = [_sqrt(vv * uu)]                                    # (alpha beta)^2: the pair holds squares
        if uu <= thr2:
            return x, 0, "converged", hist_r, hist_n, 0.0
        if not math.isfinite(vv):
            return x, 0, "breakdown", hist_r, hist_n, 0.0
        if vv == 0.0:
            return x, 0, "least_squares", hist_r, hist_n, 0.0
        if maxiter == 0:
            return x, 0, "maxiter", hist_r, hist_n, 0.0
        w = vh / alpha
        phibar, rhobar, res2, anorm2 = beta, alpha, 0.0, 0.0
        for j in range(1, maxiter + 1):
            tu = A(vh)
            uh = tu / alpha - (alpha / beta) * uh
            uu = dot(uh, uh)
            beta1 = _sqrt(uu)
            tv = At(uh)
            if uu == 0.0:                                           # gate U: exact termination, the step below ends the solve
                vv = 0.0
            else:
                vh = tv / beta1 - (beta1 / alpha) * vh
                vv = dot(vh, vh)
            st = step(alpha, uu, vv, damp, phibar, rhobar, res2, anorm2)
            alpha1, phibar, rhobar, res2, anorm2 = st["alpha"], st["phibar"], st["rhobar"], st["res2"], st["anorm2"]
            t1, t2, rn2, arn, arn2 = st["t1"], st["t2"], st["rn2"], st["arn"], st["arn2"]
            if not (math.isfinite(rn2) and math.isfinite(arn)):
                return x, j - 1, "breakdown", hist_r, hist_n, _sqrt(anorm2)
            hist_r.append(_sqrt(rn2))
            hist_n.append(_sqrt(arn2))
            stop = "converged" if rn2 <= thr2 else ("least_squares" if arn2 <= (ntol2 * anorm2) * rn2 else None)
            alpha, beta = alpha1, st["beta"]
            x = x + t1 * w
            if stop:
                return x, j, stop, hist_r, hist_n, _sqrt(anorm2)
            w = vh / alpha - t2 * w
    return x, maxiter, "maxiter", hist_r, hist_n, math.sqrt(anorm2)


def step(alpha, uu, vv, damp, phibar, rhobar, res2, anorm2):
    """The scalar step of an iteration in Python floats, every operation separately rounded in the device's order.  alpha is
    the old alpha; uu and vv are the new sums.  Returns the new value of every scalar slot and the history pair."""
    with np.errstate(all="ignore"):
        beta1, alpha1 = _sqrt(uu), _sqrt(vv)
        anorm2 = anorm2 + ((alpha * alpha + beta1 * beta1) + damp * damp)
        rhobar1 = _sqrt(rhobar * rhobar + damp * damp)
        psi = _div(damp, rhobar1) * phibar
        phibar = _div(rhobar, rhobar1) * phibar
        res2 = res2 + psi * psi
        rho = _sqrt(rhobar1 * rhobar1 + beta1 * beta1)
        c = _div(rhobar1, rho)
        s = _div(beta1, rho)
        theta = s * alpha1
        rhobar = -c * alpha1
        phi = c * phibar
        phibar = s * phibar
        t1 = _div(phi, rho)
        t2 = _div(theta, rho)
        rn2 = phibar * phibar + res2
        arn = alpha1 * abs(s * phi)
    return dict(alpha=alpha1, beta=beta1, anorm2=anorm2, res2=res2, rho=rho, c=c, s=s, theta=theta, rhobar=rhobar, phi=phi,
                phibar=phibar, t1=t1, t2=t2, rn2=rn2, arn=arn, arn2=arn * arn)


def _div(a, b):
    return float(np.float64(a) / np.float64(b))                    # IEEE division: x / 0 is +-inf or NaN, never an exception


def _sqrt(v):
    return math.sqrt(v) if v >= 0 else math.nan
