"""Shared cases of the converging CG solver (``hp.cg``) and a numpy restatement of its loop.

The restatement is plain arrays with ``np.dot``; it follows the device loop's gate order (csrc/solvers.hip,
``pcg_iterations_impl``): Ap and pAp, gate A (breakdown), the residual update with both sums, gate B (the stop rule), then the
deferred x update together with the direction update.  It is an independent statement of the algorithm, not of the device's
summation order: histories are compared to ``CG_RTOL``, iteration counts to +-2 (tests/test_gpu_pcg.py has the basis).

Cases
  scaled Poisson   A = S P S with P the oracle's 5-point ``poisson2d_rows(nx, ny)`` and s_i = 10**u_i,
                   u = fill_uniform(0, n, 0xD1A6); each entry is P_ij * (s_i * s_j), so A is exactly symmetric and its
                   diagonal spans four orders of magnitude; b = fill_uniform(0, n, 0xBEEF).  16x16, 24x20 and 33x31
                   (n = 1023: an odd length, the update kernels' scalar tail).
  diagonal         A = diag(1 + u), n = 37: Jacobi solves it in one iteration, after which the recurrence would run on
                   rounding noise.
  breakdown        A = -I, and A = diag(1, -1, 2, 3) with b = (1, 2, 1, 1) whose first p.Ap is positive and second is not.
"""
import math

import numpy as np

CG_RTOL = 1e-12            # the project's CG history margin (tests/test_gpu_parity.py)
# The stop rules test the RECURRENCE's residual; the convergence tests hold the TRUE residual (||b - A x||, an eigen or singular
# residual), computed from the returned x, to this many times the rule's limit -- at their rtol = 1e-8: 2e-8 ||b||
TRUE_RES_RTOL = 2e-8       # cg, bicgstab, gmres, lsqr: ||b - A x|| / ||b|| of a solve that converged at rtol = 1e-8
TRUE_RES_FACTOR = 2.0      # minres, eigsh, svds, lobpcg: the true residual in units of their own limit (rtol ||b||_M, tol anorm); a
#                            bound of its own: changing one of the two does not move the other
SEED_SCALE = 0xD1A6
SEED_RHS = 0xBEEF
SIZES = [(16, 16), (24, 20), (33, 31)]
HEAD = 13                  # history entries compared with the restatement
# One case per solver above one reduction workgroup: 65 x 63 = 4095 rows is odd and gives two stage-1 partials (8190 rows of the
# stacked cases: four).  Only the head of the history is compared there, and no dense matrix is built at this size.
LARGE_SIZE = (65, 63)
LARGE_MARGIN_FACTOR = 10   # a margin used at LARGE_SIZE is at least this many times the CPU spread of four summation orders


def scaled_poisson(orc, nx, ny):
    """(rowptr, colidx, vals, b) of the scaled Poisson case, global 0-based CSR (int64 indices)."""
    n = nx * ny
    rows = orc.poisson2d_rows(nx, ny, 0, n)
    s = 10.0 ** orc.fill_uniform(0, n, SEED_SCALE)
    row_of = np.repeat(np.arange(n), np.diff(rows.rowptr))
    vals = rows.vals * (s[row_of] * s[rows.colidx])
    return rows.rowptr.copy(), rows.colidx.copy(), vals, orc.fill_uniform(0, n, SEED_RHS)


def diagonal_case(orc, n=37):
    d = 1.0 + orc.fill_uniform(0, n, SEED_SCALE)
    return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64), d, orc.fill_uniform(0, n, SEED_RHS)


def diag_matrix(d):
    d = np.asarray(d, dtype=np.float64)
    n = len(d)
    return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64), d


def host_diag(rowptr, colidx, vals, row_start=0):
    """Main diagonal of CSR rows [row_start, row_start + nloc) with global columns: the stored value, +0.0 where none."""
    nloc = len(rowptr) - 1
    out = np.zeros(nloc)
    for i in range(nloc):
        a, b = int(rowptr[i]), int(rowptr[i + 1])
        hit = np.flatnonzero(colidx[a:b] == row_start + i)
        if len(hit):
            out[i] = vals[a + hit[0]]
    return out


def matvec(rowptr, colidx, vals, x):
    prod = vals * x[colidx]
    y = np.zeros(len(rowptr) - 1)
    nz = np.flatnonzero(np.diff(rowptr) > 0)
    if len(nz):
        y[nz] = np.add.reduceat(prod, rowptr[nz])
    return y


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pcg(rowptr, colidx, vals, b, dinv=None, rtol=1e-8, atol=0.0, maxiter=None, x0=None, dot=np.dot):
    """The solver's loop on the host.  Returns (x, iterations, status, residual_norms).  ``dot`` can be swapped for another
    summation order (``_bicgstab_cases.DOTS``) to measure what the order alone does to the history."""
    n = len(b)
    maxiter = 10 * n if maxiter is None else maxiter
    A = lambda v: matvec(rowptr, colidx, vals, v)
    prec = (lambda v: v.copy()) if dinv is None else (lambda v: dinv * v)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    r = b.copy() if x0 is None else b - A(x)
    z = prec(r)
    p = z.copy()
    rr, rz = float(dot(r, r)), float(dot(r, z))
    bb = float(dot(b, b))
    if bb == 0.0:
        return np.zeros(n), 0, "converged", [0.0]
    thr = max(rtol * math.sqrt(bb), atol) ** 2
    hist = [math.sqrt(rr)]
    if rr <= thr:
        return x, 0, "converged", hist
    for j in range(1, maxiter + 1):
        Ap = A(p)
        pAp = float(dot(p, Ap))
        if not (pAp > 0):                                   # gate A
            return x, j - 1, "breakdown", hist
        a = rz / pAp
        r = r - a * Ap
        z = prec(r)
        rr, rz_new = float(dot(r, r)), float(dot(r, z))
        hist.append(math.sqrt(rr))
        converged = rr <= thr                               # gate B
        beta = rz_new / rz
        x = x + a * p                                       # the deferred x update rides on the direction update
        p = z + beta * p
        rz = rz_new
        if converged:
            return x, j, "converged", hist
    return x, maxiter, "maxiter", hist
