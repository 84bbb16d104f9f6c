"""Shared cases of the MINRES solver (``hp.minres``) and a numpy restatement of its loop.

The restatement is plain arrays; it follows the device loop's gate order and rounding order literally (csrc/solvers.hip,
``minres_iterations_impl``; the kernels in csrc/vecops.hip): the Lanczos vectors r1 and r2 are kept unnormalised next to their
M-norms oldb and beta, every update is a separately rounded divide / multiply / subtract in the order the kernels use
(``residual_update``, ``direction_update``), the scalars of the step are formed by the same expressions (``step``), and gates
N, G and C are tested where the device tests them.  It is an independent statement of the algorithm, not of the device's
summation order: ``dot`` can be swapped (``_bicgstab_cases.DOTS``: four summation orders) to measure how far the order alone
moves histories and iteration counts, which is where the margins of tests/test_gpu_minres.py come from
(tests/test_minres_cases.py re-measures and prints them).

Cases (b = fill_uniform(0, len, 0xBEEF) throughout)
  saddle(nx, ny)         2n x 2n, n = nx ny: [[K, 0.5 I], [0.5 I, -K]] with K the oracle's unscaled 5-point
                         ``poisson2d_rows(nx, ny)`` plus 1 on the diagonal; columns ascending within a row.  Half the eigenvalues
                         are negative; condition number 7.6 .. 7.9.
  scaled_saddle(nx, ny)  entry ij of saddle times s_i s_j, s = 10 ** fill_uniform(0, 2n, 0xD1A6): exactly symmetric, the
                         diagonal spans two orders of magnitude and has both signs; used with the Jacobi weights 1 / |diag|.
  shifted(nx, ny)        the 5-point matrix with 0.3 subtracted from the diagonal; 33 x 31: n = 1023 (an odd length: the
                         kernels' scalar tail), 21 negative eigenvalues.
  exact                  I, -I, diag(1, -1, 2, 3), diag(1, 0), diag(1, NaN), b = 0, maxiter = 0 (values in
                         tests/test_minres_cases.py).
"""
import math

import numpy as np

from tests import _bicgstab_cases as bc
from tests import _pcg_cases as pc

SIZES = pc.SIZES
DOTS = bc.DOTS
HEAD = 13                  # history entries compared with the restatement
LARGE_SIZE = pc.LARGE_SIZE  # 65 x 63: 8190 rows stacked, 4095 shifted; the same head, HIST_RTOL is 90 times the spread (1.1e-14)
HIST_RTOL = pc.CG_RTOL     # ... to the project's history margin, 1e-12 (the CPU spread of four summation orders: <= 1e-14)
RANK_SIZE = (24, 20)       # the case of the history-head and rank tests: 960 rows
SHIFT_SIZE = (33, 31)
SHIFT = 0.3
# np.dot's iteration count at rtol = 1e-8 and (fewest, most) over the four summation orders, measured with the committed
# restatement: (name, size, preconditioned)
EXPECTED = {("saddle", (16, 16), False): (120, 120, 120), ("saddle", (24, 20), False): (136, 136, 136),
            ("saddle", (33, 31), False): (142, 142, 142), ("scaled_saddle", (16, 16), True): (120, 120, 120),
            ("scaled_saddle", (24, 20), True): (138, 138, 138), ("scaled_saddle", (33, 31), True): (142, 142, 142),
            ("shifted", (33, 31), False): (351, 346, 352), ("shifted", (33, 31), True): (348, 346, 351)}


def saddle(orc, nx, ny):
    """(rowptr, colidx, vals, b) of the 2n x 2n saddle-point case, global 0-based CSR (int64 indices)."""
    n = nx * ny
    rows = orc.poisson2d_rows(nx, ny, 0, n)
    rp, ci = rows.rowptr.astype(np.int64), rows.colidx.astype(np.int64)
    row_of = np.repeat(np.arange(n), np.diff(rp))
    kv = rows.vals + (ci == row_of)                                # K = P + I
    counts = np.diff(rp) + 1
    rowptr = np.concatenate([[0], np.cumsum(np.concatenate([counts, counts]))]).astype(np.int64)
    colidx = np.empty(rowptr[-1], dtype=np.int64)
    vals = np.empty(rowptr[-1])
    for i in range(n):
        a, b_ = int(rp[i]), int(rp[i + 1])
        k = b_ - a
        top, bot = int(rowptr[i]), int(rowptr[n + i])
        colidx[top:top + k], vals[top:top + k] = ci[a:b_], kv[a:b_]          # [K, 0.5 I]
        colidx[top + k], vals[top + k] = n + i, 0.5
        colidx[bot], vals[bot] = i, 0.5                                        # [0.5 I, -K]
        colidx[bot + 1:bot + 1 + k], vals[bot + 1:bot + 1 + k] = n + ci[a:b_], -kv[a:b_]
    return rowptr, colidx, vals, orc.fill_uniform(0, 2 * n, pc.SEED_RHS)


def scaled_saddle(orc, nx, ny):
    rowptr, colidx, vals, b = saddle(orc, nx, ny)
    s = 10.0 ** orc.fill_uniform(0, len(b), pc.SEED_SCALE)
    row_of = np.repeat(np.arange(len(b)), np.diff(rowptr))
    return rowptr, colidx, vals * (s[row_of] * s[colidx]), b


def shifted(orc, nx, ny):
    n = nx * ny
    rows = orc.poisson2d_rows(nx, ny, 0, n)
    rp, ci = rows.rowptr.astype(np.int64), rows.colidx.astype(np.int64)
    row_of = np.repeat(np.arange(n), np.diff(rp))
    return rp, ci, rows.vals - SHIFT * (ci == row_of), orc.fill_uniform(0, n, pc.SEED_RHS)


def jacobi(rowptr, colidx, vals):
    """The weights of ``M="jacobi"``: 1 ./ abs(diag(A))."""
    return 1.0 / np.abs(pc.host_diag(rowptr, colidx, vals))


def all_cases(orc):
    """{(name, size, preconditioned): (rowptr, colidx, vals, b, dinv)}: every case the tests solve."""
    out = {}
    for size in SIZES:
        case = saddle(orc, *size)
        out["saddle", size, False] = (*case, None)
        case = scaled_saddle(orc, *size)
        out["scaled_saddle", size, True] = (*case, jacobi(*case[:3]))
    case = shifted(orc, *SHIFT_SIZE)
    out["shifted", SHIFT_SIZE, False] = (*case, None)
    out["shifted", SHIFT_SIZE, True] = (*case, jacobi(*case[:3]))
    return out


def large_cases(orc):
    """[(name, (rowptr, colidx, vals, b), dinv)] at LARGE_SIZE: the three cases of the history-head test, no dense matrices."""
    out = [("saddle", saddle(orc, *LARGE_SIZE), None)]
    case = scaled_saddle(orc, *LARGE_SIZE)
    out.append(("scaled_saddle", case, jacobi(*case[:3])))
    out.append(("shifted", shifted(orc, *LARGE_SIZE), None))
    return out


dense_of = bc.dense_of


def m_norm(r, dinv):
    """sqrt(r . M r) on the host: the norm of the stop rule."""
    return math.sqrt(float(np.dot(r, r if dinv is None else dinv * r)))


# ---- the kernels, element for element ----------------------------------------------------------------------------------
def residual_update(t, r2, r1, dinv, beta, oldb, yt, first):
    """minres_r: (rn, yn) with yn = rn without a preconditioner."""
    with np.errstate(all="ignore"):
        alfa = _div(yt, beta * beta)
        rn = t / beta - _div(alfa, beta) * r2
        if not first:
            rn = rn - _div(beta, oldb) * r1
        return rn, (rn if dinv is None else dinv * rn)


def step(s, yt, bb):
    """The scalar step of an iteration in Python floats, every operation separately rounded in the device's order.  ``s``: the
    scalars before the step (beta, oldb, cs, sn, dbar, epsln, phibar).  Returns (gate, scalars after): gate "N" or "G" leaves
    the scalars as they were."""
    with np.errstate(all="ignore"):
        beta = s["beta"]
        alfa = _div(yt, beta * beta)
        if not (bb >= 0.0 and math.isfinite(bb) and math.isfinite(alfa)):
            return "N", s
        betan = math.sqrt(bb)
        oldeps = s["epsln"]
        delta = s["cs"] * s["dbar"] + s["sn"] * alfa
        gbar = s["sn"] * s["dbar"] - s["cs"] * alfa
        epsln = s["sn"] * betan
        dbar = (-s["cs"]) * betan
        gamma = _sqrt(gbar * gbar + betan * betan)
        if not (gamma > 0.0):
            return "G", s
        cs = _div(gbar, gamma)
        sn = _div(betan, gamma)
        phi = cs * s["phibar"]
        phibar = sn * s["phibar"]
    return None, dict(beta=betan, oldb=beta, alfa=alfa, cs=cs, sn=sn, dbar=dbar, epsln=epsln, oldeps=oldeps, delta=delta,
                      gbar=gbar, gamma=gamma, phi=phi, phibar=phibar)


def direction_update(y, w1, w2, x, s):
    """minres_xw with the scalars after the step: (w, x)."""
    with np.errstate(all="ignore"):
        w = ((y / s["oldb"] - s["oldeps"] * w1) - s["delta"] * w2) / s["gamma"]
        return w, x + s["phi"] * w


# ---- the loop ------------------------------------------------------------------------------------------------------------
def minres(rowptr, colidx, vals, b, dinv=None, rtol=1e-8, atol=0.0, maxiter=None, x0=None, dot=bc._dot_np):
    """The solver's loop on the host.  Returns (x, iterations, status, residual_norms)."""
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    maxiter = 10 * n if maxiter is None else maxiter
    A = lambda v: pc.matvec(rowptr, colidx, vals, v)
    prec = (lambda v: v) if dinv is None else (lambda v: dinv * v)
    with np.errstate(all="ignore"):
        x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
        r2 = b.copy() if x0 is None else b - A(x)
        y = prec(r2)
        rr0 = dot(r2, y)
        bb = rr0 if x0 is None else dot(b, prec(b))
        if bb == 0.0:
            return np.zeros(n), 0, "converged", [0.0]
        thr = max(rtol * _sqrt(bb), atol) ** 2
        hist = [_sqrt(rr0)]
        if rr0 <= thr:
            return x, 0, "converged", hist
        if maxiter == 0:
            return x, 0, "maxiter", hist
        beta1 = _sqrt(rr0)
        s = dict(beta=beta1, oldb=0.0, cs=-1.0, sn=0.0, dbar=0.0, epsln=0.0, phibar=beta1)
        r1, w1, w2 = np.zeros(n), np.zeros(n), np.zeros(n)
        for j in range(1, maxiter + 1):
            t = A(y)
            yt = dot(y, t)
            rn, yn = residual_update(t, r2, r1, dinv, s["beta"], s["oldb"], yt, j == 1)
            gate, s = step(s, yt, dot(rn, yn))
            if gate:
                return x, j - 1, "breakdown", hist
            res2 = s["phibar"] * s["phibar"]
            hist.append(math.sqrt(res2))
            w, x = direction_update(y, w1, w2, x, s)
            if res2 <= thr:
                return x, j, "converged", hist
            r1, r2, y, w1, w2 = r2, rn, yn, w2, w
    return x, maxiter, "maxiter", hist


def _div(a, b):
    return float(np.float64(a) / np.float64(b))                    # IEEE division: x / 0 is +-inf or NaN, never an exception


def _sqrt(v):
    return math.sqrt(v) if v >= 0 else math.nan
