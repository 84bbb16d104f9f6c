"""Shared cases of the restarted GMRES solver (``hp.gmres``) and a numpy restatement of its loop.

The restatement is plain arrays; it follows the device loop's gate order and rounding order literally (csrc/solvers.hip,
``gmres_iterations_impl``; the kernels in csrc/vecops.hip): every multiply, add, subtract, divide and sqrt is rounded separately
in the order the kernels use, the running subtractions run over the basis columns in ascending order, the Givens rotations and
the back substitution are the small step's own expressions, and gates R, D, C are tested where the device tests them.  It is an
independent statement of the algorithm, not of the device's summation order: ``dot`` can be swapped (``_bicgstab_cases.DOTS``:
four summation orders) to measure how far the order alone moves histories and iteration counts, which is where the margins of
tests/test_gpu_gmres.py come from.

Cases
  convection-diffusion   ``_bicgstab_cases.convection_diffusion`` at 16x16, 24x20 and 33x31 (n = 1023: an odd length, so the basis
                         pitch is n + 1 and the kernels' scalar tail runs).
  ROT                    [[0, 1], [-1, 0]] with b = (1, 0): ``hp.bicgstab`` reports a breakdown, GMRES converges at step 2 to
                         x = (0, 1).
  -I, diagonal           -I converges at step 1 with a residual of exactly 0; ``_pcg_cases.diagonal_case`` under Jacobi at step 1.
  ZERO                   a 2x2 matrix of stored zeros with b = (1, 1): gate D in step 1, 0 iterations, x = 0.
  NILP                   [[0, 1], [0, 0]] with b = (0, 1): gate D in step 2, iterations 1, history [1, 1], x = 0.
  stagnation             16x16 under Jacobi with restart = 1 or 2 makes no progress and ends as "maxiter".

Figures of this restatement (tests/test_gmres_cases.py re-measures and prints them), rtol = 1e-8, at restart 30 / 8:

    case     jacobi       none
    16x16    56 / 102     228 / 321
    24x20    169 / 135    297 / 370
    33x31    262 / 194    344 / 573

identical under all four summation orders; true residual 0.51 - 0.996 rtol; the first HEAD = 9 history entries spread by at
most 9.3e-16 over the four orders (restart = 5, so the head crosses a restart), the whole history by up to 6.2e-3 (33x31, none,
restart = 8), which is why only a head is compared; the history falls at every step (its largest relative step is -7.2e-6).
tests/test_gmres_cases.py asserts the bounds the GPU tests rest on and prints the current figures.
"""
import math

import numpy as np

from tests import _bicgstab_cases as bc
from tests import _pcg_cases as pc

SIZES = bc.SIZES
RESTARTS = (30, 8)
HEAD = 9                   # history entries compared with the restatement (restart = 5: the head crosses a restart)
HEAD_RESTART = 5
LARGE_SIZE = pc.LARGE_SIZE  # 65 x 63: the same head and restart, HIST_RTOL is 430 times the CPU spread there (2.3e-15)
HIST_RTOL = 1e-12          # ... to this margin, the project's history margin; the CPU spread must stay below 1e-13
RISE_RTOL = 1e-12          # the history never rises by more than this, relative

ROT, ROT_B = bc.ROT, bc.ROT_B
ZERO = (np.array([0, 2, 4], dtype=np.int64), np.array([0, 1, 0, 1], dtype=np.int64), np.zeros(4))       # stored zeros
ZERO_B = np.array([1.0, 1.0])
NILP = (np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int64), np.array([1.0, 0.0]))    # [[0, 1], [0, 0]]
NILP_B = np.array([0.0, 1.0])


def small_step(j, h1, h2, nn, cs, sn, R, g, thr):
    """The small step of column j on the arrays cs, sn (m), R (m x m, R[i, j]), g (m + 1), updated in place.
    Returns (status, hist_k): "breakdown" (gate D, nothing stored, hist_k None), "converged" (gate C) or "running"."""
    c = j + 1
    col = np.empty(c + 1)
    for i in range(c):
        col[i] = h1[i] + h2[i]
    col[c] = math.sqrt(nn) if nn >= 0 else math.nan
    for i in range(j):
        t = cs[i] * col[i] + sn[i] * col[i + 1]
        col[i + 1] = (-sn[i]) * col[i] + cs[i] * col[i + 1]
        col[i] = t
    dd = col[j] * col[j] + col[j + 1] * col[j + 1]
    d = math.sqrt(dd) if dd >= 0 else math.nan
    if not (d > 0):                                             # gate D (false for NaN too)
        return "breakdown", None
    cs[j] = col[j] / d
    sn[j] = col[j + 1] / d
    R[:j, j] = col[:j]
    R[j, j] = d
    gn = (-sn[j]) * g[j]
    g[j + 1] = gn
    g[j] = cs[j] * g[j]
    e = gn * gn
    return ("converged" if e <= thr else "running"), e


def back_substitution(c, R, g):
    y = np.zeros(c)
    for i in range(c - 1, -1, -1):
        t = g[i]
        for l in range(i + 1, c):
            t = t - R[i, l] * y[l]
        y[i] = t / R[i, i]
    return y


def basis_combination(V, y):
    """u = y[0] V_0;  u = u + y[i] V_i ascending (V: columns as rows of a 2-D array)."""
    u = y[0] * V[0]
    for i in range(1, len(y)):
        u = u + y[i] * V[i]
    return u


def subtract_columns(w, V, h):
    """w = ((w - h[0] V_0) - h[1] V_1) - ..."""
    for i in range(len(h)):
        w = w - h[i] * V[i]
    return w


def gmres(rowptr, colidx, vals, b, dinv=None, rtol=1e-8, atol=0.0, restart=30, maxiter=None, x0=None, dot=bc._dot_np):
    """The solver's loop on the host.  Returns (x, iterations, status, residual_norms)."""
    n, m = len(b), restart
    maxiter = 10 * n if maxiter is None else maxiter
    A = lambda u: pc.matvec(rowptr, colidx, vals, u)
    K = (lambda u: u) if dinv is None else (lambda u: dinv * u)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    w = b - np.zeros(n) if x0 is None else b - A(x)
    rr = dot(w, w)
    bb = rr if x0 is None else dot(b, b)
    if bb == 0.0:
        return np.zeros(n), 0, "converged", [0.0]
    thr = max(rtol * math.sqrt(bb), atol) ** 2
    hist = [rr]
    sq = lambda h: [math.sqrt(v) for v in h]
    if rr <= thr or maxiter == 0:
        return x, 0, "converged" if rr <= thr else "maxiter", sq(hist)
    V = np.zeros((m + 1, n))
    cs, sn, R, g = np.zeros(m), np.zeros(m), np.zeros((m, m)), np.zeros(m + 1)

    def start(w, rr):
        beta = math.sqrt(rr)
        g[:] = 0.0
        g[0] = beta
        V[0] = w / beta
        return K(V[0])

    def finish(x, c):
        if c == 0:
            return x
        return x + K(basis_combination(V, back_substitution(c, R, g)))

    z = start(w, rr)
    for k in range(1, maxiter + 1):
        j = (k - 1) % m
        c = j + 1
        w = A(z)
        h1 = np.array([dot(V[i], w) for i in range(c)])
        w = subtract_columns(w, V, h1)
        h2 = np.array([dot(V[i], w) for i in range(c)])
        w = subtract_columns(w, V, h2)
        nn = dot(w, w)
        status, e = small_step(j, h1, h2, nn, cs, sn, R, g, thr)
        if status == "breakdown":                               # gate D: column j is not stored, the open cycle has j columns
            return finish(x, j), k - 1, "breakdown", sq(hist)
        hist.append(e)
        if status == "converged":                               # gate C
            return finish(x, c), k, "converged", sq(hist)
        hn = math.sqrt(nn)
        if c < m:
            V[c] = w / hn
            z = K(V[c])
            continue
        x = finish(x, c)                                        # cycle end, then the restart
        w = b - A(x)
        rr = dot(w, w)
        if rr <= thr:                                           # gate R
            hist[k] = rr
            return x, k, "converged", sq(hist)
        z = start(w, rr)
    return finish(x, maxiter % m), maxiter, "maxiter", sq(hist)
