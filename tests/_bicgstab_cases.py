"""Shared cases of the BiCGStab solver (``hp.bicgstab``) and a numpy restatement of its loop.

The restatement is plain arrays; it follows the device loop's gate order and rounding order literally (csrc/solvers.hip,
``bicgstab_iterations_impl``; the kernels in csrc/vecops.hip): every update is a separately rounded multiply and add in the
order the kernels use, alpha / omega / beta are formed by the same expressions, and gates A, S, T, B, O are tested where the
device tests them.  It is an independent statement of the algorithm, not of the device's summation order: ``dot`` can be
swapped (``DOTS``: four summation orders) to measure how far the order alone moves histories and iteration counts, which is
where the margins of tests/test_gpu_bicgstab.py come from.

Cases
  convection-diffusion   the oracle's 5-point ``poisson2d_rows(nx, ny)`` with its west / east / south / north entries (column
                         offsets -1, +1, -nx, +nx) set to -1.5, -0.5, -1.3, -0.7, then the two-sided scaling of
                         ``_pcg_cases.scaled_poisson`` (same seeds): A_ij * (s_i * s_j).  Not symmetric.  b as there.
                         16x16, 24x20 and 33x31 (n = 1023: an odd length, the kernels' scalar tail).
  freeze                 ``_pcg_cases.diagonal_case`` and ``diag_matrix``: Jacobi (and the identity) solve at the half step.
  breakdown              [[0, 1], [-1, 0]] with b = (1, 0): rhat.v = 0 in iteration 1;  diag(1, 0) with b = (1, 1): rhat.v = 0 in
                         iteration 2, after one full step to x = (1, 3).
  half step              16x16 with Jacobi and rtol = 0.7 stops at gate S of iteration 8 with ||s_8|| = 0.655 |b| > 0: a history whose
                         last entry is a sum of squares of s that N ranks must not sum again (sqrt(2) * 0.655 > 0.7).
  -I                     converges at iteration 1 (the half step); CG reports a breakdown on it.
"""
import math

import numpy as np

from tests import _pcg_cases as pc

SIZES = pc.SIZES
HEAD = 5                   # history entries compared with the restatement
LARGE_SIZE = pc.LARGE_SIZE  # 65 x 63: the same head, HIST_RTOL is 30 times the CPU spread there (3.3e-14, with Jacobi)
HIST_RTOL = 1e-12          # ... to this margin (basis: tests/test_gpu_bicgstab.py)
HALF_SIZE, HALF_RTOL, HALF_ITERATIONS = (16, 16), 0.7, 8      # the half-step case
HALF_HIST_RTOL = 1e-11     # its whole history: 45 times the CPU spread of four summation orders (2.2e-13, entry 7)
WEST, EAST, SOUTH, NORTH = -1.5, -0.5, -1.3, -0.7

ROT = (np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int64), np.array([1.0, -1.0]))    # [[0, 1], [-1, 0]]
ROT_B = np.array([1.0, 0.0])
SINGULAR = (np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int64), np.array([1.0, 0.0]))  # diag(1, 0), both stored
SINGULAR_B = np.array([1.0, 1.0])


def convection_diffusion(orc, nx, ny):
    """(rowptr, colidx, vals, b) of the scaled convection-diffusion case, global 0-based CSR (int64 indices)."""
    n = nx * ny
    rows = orc.poisson2d_rows(nx, ny, 0, n)
    row_of = np.repeat(np.arange(n), np.diff(rows.rowptr))
    off = rows.colidx - row_of
    vals = rows.vals.copy()
    for o, val in ((-1, WEST), (1, EAST), (-nx, SOUTH), (nx, NORTH)):
        vals[off == o] = val
    s = 10.0 ** orc.fill_uniform(0, n, pc.SEED_SCALE)
    vals = vals * (s[row_of] * s[rows.colidx])
    return rows.rowptr.copy(), rows.colidx.copy(), vals, orc.fill_uniform(0, n, pc.SEED_RHS)


def dense_of(rowptr, colidx, vals):
    n = len(rowptr) - 1
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(rowptr)), colidx] = vals
    return dense


def _dot_np(a, c):
    return float(np.dot(a, c))


def _dot_fsum(a, c):
    return math.fsum((a * c).tolist())


def _dot_reversed(a, c):
    return float(np.dot(a[::-1].copy(), c[::-1].copy()))


def _dot_sequential(a, c):
    return float(np.cumsum(a * c)[-1]) if len(a) else 0.0


DOTS = {"np.dot": _dot_np, "fsum": _dot_fsum, "reversed": _dot_reversed, "sequential": _dot_sequential}


def bicgstab(rowptr, colidx, vals, b, dinv=None, rtol=1e-8, atol=0.0, maxiter=None, x0=None, dot=_dot_np):
    """The solver's loop on the host.  Returns (x, iterations, status, residual_norms)."""
    n = len(b)
    maxiter = 10 * n if maxiter is None else maxiter
    A = lambda u: pc.matvec(rowptr, colidx, vals, u)
    K = (lambda u: u) if dinv is None else (lambda u: dinv * u)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    r = b.copy() if x0 is None else b - A(x)
    rhat, p = r.copy(), r.copy()
    rr = dot(r, r)
    rho = rr                                                    # rhat.r with rhat = r
    bb = rr if x0 is None else dot(b, b)
    if bb == 0.0:
        return np.zeros(n), 0, "converged", [0.0]
    thr = max(rtol * math.sqrt(bb), atol) ** 2
    hist = [math.sqrt(rr)]
    if rr <= thr:
        return x, 0, "converged", hist
    for j in range(1, maxiter + 1):
        ph = K(p)
        v = A(ph)
        rv = dot(rhat, v)
        if not (abs(rho) > 0 and abs(rv) > 0):                  # gate A (false for NaN too)
            return x, j - 1, "breakdown", hist
        alpha = rho / rv
        s = r - alpha * v
        sh = K(s)
        t = A(sh)
        ts, tt, ss = dot(t, s), dot(t, t), dot(s, s)
        if ss <= thr:                                           # gate S: the half step
            x = x + alpha * ph
            hist.append(math.sqrt(ss))
            return x, j, "converged", hist
        if not (tt > 0):                                        # gate T
            return x, j - 1, "breakdown", hist
        omega = ts / tt
        x = (x + alpha * ph) + omega * sh
        r = s - omega * t
        rho_new, rr = dot(rhat, r), dot(r, r)
        hist.append(math.sqrt(rr))
        if rr <= thr:                                           # gate B
            return x, j, "converged", hist
        if ts == 0:                                             # gate O
            return x, j, "breakdown", hist
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        rho = rho_new
    return x, maxiter, "maxiter", hist
