"""Shared cases of the fine-grained ILU(0) preconditioner (``hp.ilu0``), numpy restatements of its setup and application, and
``hp.gmres`` / ``hp.bicgstab`` taking a callable ``K``.

The restatements are the kernels' algorithms (csrc/ilu.hip) on plain arrays:

  ``block_csr``     a rank's owned block: the entries of its rows whose column lies in [row_start, row_start + nloc), local
                    columns, ascending within a row.
  ``sweep_factors`` the initial guess l_ij = a_ij / a_jj, u_ij = a_ij, then Chow-Patel sweeps from the previous sweep's values:
                    s = a_ij - sum_{k < min(i, j)} l_ik u_kj with separately rounded multiplies and subtractions in ascending k
                    (``descending=True``: the same sum from the largest k down -- a second order, for the margin), l_ij = s / u_jj
                    with the previous u_jj, u_ij = s.
  ``exact_ilu0``    the classical row-wise (IKJ) ILU(0) on the same pattern: the sweeps' fixed point.
  ``apply``         z = N_U(N_L(r)): y_0 = r, y_{m+1} = r - L y_m;  z_0 = D^-1 y, z_{m+1} = D^-1 (y - U_strict z_m).
  ``ilu_blocks``    the block-Jacobi form over a row partition, ``apply_blocks`` its application.
  ``gmres_op`` / ``bicgstab_op``   ``_gmres_cases.gmres`` and ``_bicgstab_cases.bicgstab`` (same gate and rounding order, same small
                    step) with a callable K in place of ``dinv .*``.

Cases
  convection-diffusion   ``_bicgstab_cases.convection_diffusion`` at ``_pcg_cases.SIZES`` and ``LARGE_SIZE``.
  nonsymmetric banded    n = 300, half-bandwidth w: a_ij = -1 / (1 + |i - j|) below the diagonal, -0.4 / (1 + |i - j|) above,
                         a_ii = 1 + the row's absolute sum.  Rows of 1 .. 2 w off-diagonals (w = 16: up to 32; the first row of
                         w = 1 has one, an inner row of w = 15 has 30, and ``BANDED_W`` walks the merge lengths in between).
  asymmetric pattern     n = 120, strictly diagonally dominant: (i, i - 1) on every row but the multiples of 5 (whose lower part
                         is empty), (i, i - 7) on even rows, (i, i + 2) on rows that are not multiples of 3 (an empty upper part
                         on the multiples of 3 and the last two rows), (i, i + 11) on odd rows: entries (i, j) without (j, i)
                         throughout, rows 0, 15, 30, ... with the diagonal alone on one side or both.
  diagonal, 1 x 1        ``_pcg_cases.diagonal_case``; [[2.5]].
  three faults           ``three_faults``: 600 banded rows whose row 40 has a NaN diagonal, row 300 stores no diagonal and row 520
                         has a zero diagonal, healed one at a time in row order (the order of the error word).

Margins (tests/test_ilu_cases.py re-measures each and asserts the relation stated here):
  EXACT_RTOL   40 sweeps against ``exact_ilu0``, largest relative deviation of an entry over the cases: measured 5.06e-14
               (banded16; 3.3e-14 at banded15, 5.0e-16 at banded8, 0 on the stencil, asymmetric and diagonal cases); 100 times it.
  ILU_RTOL     the device's factors against ``sweep_factors``: ten times the largest relative difference between the ascending
               and the descending sum at 3 sweeps over the cases, measured 7.52e-16 (banded15; 4.1e-16 on the 33 x 31 stencil,
               whose diagonal entries sum two products).
  HEAD         history entries of the preconditioned solves compared with the restatement: the CPU spread over
               ``_bicgstab_cases.DOTS`` of the first HEAD entries stays below HIST_RTOL / 10 = 1e-13.  Measured over the four
               sizes, one block: GMRES 4.8e-15 with ``_gmres_cases.HEAD`` = 9 at restart 5; BiCGStab 9.4e-14 over the first four
               entries (33 x 31), while the fifth spreads by 8.9e-12 (24 x 20), so HEAD_BICGSTAB = 4 is one shorter than
               ``_bicgstab_cases.HEAD``, the way ``_gmres_cases.HEAD`` was chosen.
  Iterations   ``gmres_op`` at restart 30, rtol = 1e-8, against Jacobi's 56 / 169 / 262 / 360 at 16x16, 24x20, 33x31, 65x63:
               1 block 17 / 21 / 27 / 89, 2 blocks 20 / 25 / 31 / 91, 3 blocks 22 / 27 / 32 / 95, 8 blocks 25 / 30 / 40 / 121;
               the largest ratio is 0.446 (16x16 in 8 blocks).  ``bicgstab_op``: 10 .. 16, 13 .. 17, 19 .. 22, 35 .. 39.
"""
import math

import numpy as np

from tests import _bicgstab_cases as bc
from tests import _gmres_cases as gc
from tests import _pcg_cases as pc

BANDED_N = 300
BANDED_W = [1, 3, 8, 15, 16]
ASYM_N = 120
BLOCKS = [1, 2, 3, 8]
JACOBI_FACTOR = 0.5         # gmres_op's count against Jacobi's on every size and block count (the issue's condition)
EXACT_SWEEPS = 40
EXACT_RTOL = 5.1e-12
ILU_RTOL = 7.6e-15
HEAD_GMRES = gc.HEAD
HEAD_BICGSTAB = 4
HEAD_RESTART = gc.HEAD_RESTART
HIST_RTOL = gc.HIST_RTOL
FAULT_ROWS = (40, 300, 520)                                     # NaN diagonal, no stored diagonal, zero diagonal


class NoDiagonal(ValueError):
    def __init__(self, row):
        super().__init__(f"row {row}")
        self.row = row


class BadDiagonal(ValueError):
    def __init__(self, row):
        super().__init__(f"row {row}")
        self.row = row


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def banded(w, n=BANDED_N, lower=1.0, upper=0.4):
    rowptr, cols, vals = [0], [], []
    for i in range(n):
        js = list(range(max(0, i - w), min(n, i + w + 1)))
        off = {j: -(lower if j < i else upper) / (1.0 + abs(i - j)) for j in js if j != i}
        for j in js:
            cols.append(j)
            vals.append(1.0 + sum(abs(v) for v in off.values()) if j == i else off[j])
        rowptr.append(len(cols))
    return np.array(rowptr, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals, dtype=np.float64)


def asymmetric_pattern(n=ASYM_N):
    rowptr, cols, vals = [0], [], []
    for i in range(n):
        row = {}
        if i % 5 and i - 1 >= 0:
            row[i - 1] = -0.9
        if i % 2 == 0 and i - 7 >= 0:
            row[i - 7] = 0.3
        if i % 3 and i + 2 < n:
            row[i + 2] = -0.6
        if i % 2 and i + 11 < n:
            row[i + 11] = 0.25
        row[i] = 1.0 + sum(abs(v) for v in row.values())
        for j in sorted(row):
            cols.append(j)
            vals.append(row[j])
        rowptr.append(len(cols))
    return np.array(rowptr, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals, dtype=np.float64)


def one_by_one():
    return np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int64), np.array([2.5])


def three_faults(heal=0, n=600, w=3):
    """``banded(w, n)`` with three faults, the first ``heal`` of them (in row order) taken out again."""
    rowptr, colidx, vals = banded(w, n)
    at = lambda r: int(rowptr[r] + np.flatnonzero(colidx[rowptr[r]:rowptr[r + 1]] == r)[0])
    vals = vals.copy()
    if heal < 3:
        vals[at(FAULT_ROWS[2])] = 0.0
    if heal < 1:
        vals[at(FAULT_ROWS[0])] = np.nan
    if heal < 2:
        keep = np.ones(len(colidx), dtype=bool)
        keep[at(FAULT_ROWS[1])] = False
        rowptr = rowptr.copy()
        rowptr[FAULT_ROWS[1] + 1:] -= 1
        colidx, vals = colidx[keep], vals[keep]
    return rowptr, colidx, vals


def factor_cases(orc, large=False):
    """name -> (rowptr, colidx, vals, b) of every case the factors are checked on."""
    out = {}
    sizes = list(pc.SIZES) + ([pc.LARGE_SIZE] if large else [])
    for nx, ny in sizes:
        out[f"convdiff{nx}x{ny}"] = bc.convection_diffusion(orc, nx, ny)
    for w in BANDED_W:
        out[f"banded{w}"] = (*banded(w), orc.fill_uniform(0, BANDED_N, pc.SEED_RHS))
    out["asymmetric"] = (*asymmetric_pattern(), orc.fill_uniform(0, ASYM_N, pc.SEED_RHS))
    out["diagonal"] = pc.diagonal_case(orc)
    out["one"] = (*one_by_one(), np.array([3.0]))
    return out


# ---- the block ----------------------------------------------------------------------------------------------------------------------
def block_csr(rowptr, colidx, vals, row_start=0):
    """(rowptr, local columns ascending, values) of the owned block of the rows given (global columns)."""
    nloc = len(rowptr) - 1
    bp, bcols, bvals = [0], [], []
    for i in range(nloc):
        c = colidx[rowptr[i]:rowptr[i + 1]] - row_start
        v = vals[rowptr[i]:rowptr[i + 1]]
        own = np.flatnonzero((c >= 0) & (c < nloc))
        order = own[np.argsort(c[own], kind="stable")]
        bcols.append(c[order])
        bvals.append(v[order])
        bp.append(bp[-1] + len(order))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return np.array(bp, dtype=np.int64), cat(bcols, np.int64), cat(bvals, np.float64)


def _diagonal_positions(bp, bc, bv, row_start):
    n = len(bp) - 1
    row_of = np.repeat(np.arange(n), np.diff(bp))
    dpos = np.full(n, -1, dtype=np.int64)
    on = np.flatnonzero(bc == row_of)
    dpos[row_of[on]] = on
    for i in range(n):                                          # the smallest failing row first, as the error word has it
        if dpos[i] < 0:
            raise NoDiagonal(row_start + i)
        d = bv[dpos[i]]
        if d == 0.0 or d != d:
            raise BadDiagonal(row_start + i)
    return row_of, dpos


def _products(bp, bc, row_of):
    """For every entry (i, j): the positions of l_ik and u_kj over the k < min(i, j) that both store, ascending k."""
    n = len(bp) - 1
    by_col = [[] for _ in range(n)]
    for p in range(len(bc)):
        by_col[bc[p]].append(p)                                 # ascending row: positions are row-major
    ent, lpos, upos = [], [], []
    for p in range(len(bc)):
        i, j = int(row_of[p]), int(bc[p])
        m = min(i, j)
        row = {int(bc[q]): q for q in range(bp[i], bp[i + 1]) if bc[q] < m}
        for q in by_col[j]:
            k = int(row_of[q])
            if k >= m:
                break
            if k in row:
                ent.append(p)
                lpos.append(row[k])
                upos.append(q)
    return np.array(ent, dtype=np.int64), np.array(lpos, dtype=np.int64), np.array(upos, dtype=np.int64)


def sweep_factors(bp, bc, bv, sweeps, row_start=0, descending=False):
    """The factor values after ``sweeps`` sweeps, aligned with the block."""
    row_of, dpos = _diagonal_positions(bp, bc, bv, row_start)
    nnz = len(bc)
    lower = row_of > bc
    f = np.where(lower, bv / bv[dpos[bc]], bv) if nnz else bv.copy()
    ent, lpos, upos = _products(bp, bc, row_of)
    count = np.bincount(ent, minlength=nnz) if nnz else np.zeros(0, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(count)])[:-1] if nnz else count
    depth = int(count.max()) if nnz else 0
    for _ in range(sweeps):
        s = bv.copy()
        for t in range(depth):                                  # the t-th product of every entry that has one: the order of one lane
            has = np.flatnonzero(count > t)
            at = first[has] + (count[has] - 1 - t if descending else t)
            s[has] = s[has] - f[lpos[at]] * f[upos[at]]
        f = np.where(lower, s / f[dpos[bc]], s)
    return f


def exact_ilu0(bp, bc, bv):
    """The row-wise ILU(0) on the block's pattern, aligned with the block."""
    n = len(bp) - 1
    f = bv.copy()
    dpos = np.zeros(n, dtype=np.int64)
    for i in range(n):
        lo, hi = int(bp[i]), int(bp[i + 1])
        at = {int(bc[p]): p for p in range(lo, hi)}
        dpos[i] = at[i]
        for p in range(lo, hi):
            k = int(bc[p])
            if k >= i:
                break
            f[p] = f[p] / f[dpos[k]]
            for q in range(dpos[k] + 1, int(bp[k + 1])):
                j = int(bc[q])
                if j in at:
                    f[at[j]] = f[at[j]] - f[p] * f[q]
    return f


def split_factors(bp, bc, f):
    """(L_strict, U_strict, diagonal of U) of a block's factor values: two CSR triples and a vector."""
    n = len(bp) - 1
    row_of = np.repeat(np.arange(n), np.diff(bp))
    lo, up = row_of > bc, row_of < bc
    ptr = lambda mask: np.concatenate([[0], np.cumsum(np.bincount(row_of[mask], minlength=n))]).astype(np.int64)
    d = np.zeros(n)
    d[row_of[row_of == bc]] = f[row_of == bc]
    return (ptr(lo), bc[lo], f[lo]), (ptr(up), bc[up], f[up]), d


def apply(bp, bc, f, r, solve_sweeps):
    L, U, d = split_factors(bp, bc, f)
    y = r.copy()
    for _ in range(solve_sweeps):
        y = r - pc.matvec(*L, y)
    z = y / d
    for _ in range(solve_sweeps):
        z = (y - pc.matvec(*U, z)) / d
    return z


def ilu_blocks(rowptr, colidx, vals, partition, sweeps=3, factors=None):
    """The block-Jacobi factors of a row partition (a list of boundaries): [(bp, bc, f, row_start), ...]."""
    out = []
    for lo, hi in zip(partition[:-1], partition[1:]):
        lo, hi = int(lo), int(hi)
        a, b = int(rowptr[lo]), int(rowptr[hi])
        bp, bcols, bv = block_csr(rowptr[lo:hi + 1] - a, colidx[a:b], vals[a:b], lo)
        f = sweep_factors(bp, bcols, bv, sweeps, lo) if factors is None else factors(bp, bcols, bv)
        out.append((bp, bcols, f, lo))
    return out


def apply_blocks(blocks, r, solve_sweeps=3):
    z = np.zeros(len(r))
    for bp, bcols, f, lo in blocks:
        hi = lo + len(bp) - 1
        z[lo:hi] = apply(bp, bcols, f, r[lo:hi], solve_sweeps)
    return z


def operator(blocks, solve_sweeps=3):
    return lambda r: apply_blocks(blocks, r, solve_sweeps)


def equal_blocks(n, k):
    return [(n * j) // k for j in range(k + 1)]


# ---- the two solvers with a callable K ------------------------------------------------------------------------------------------
def gmres_op(rowptr, colidx, vals, b, K, rtol=1e-8, atol=0.0, restart=30, maxiter=None, x0=None, dot=bc._dot_np):
    """``_gmres_cases.gmres`` with ``K`` a callable: (x, iterations, status, residual_norms)."""
    n, m = len(b), restart
    maxiter = 10 * n if maxiter is None else maxiter
    A = lambda u: pc.matvec(rowptr, colidx, vals, u)
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
        g[:] = 0.0
        g[0] = math.sqrt(rr)
        V[0] = w / g[0]
        return K(V[0])

    def finish(x, c):
        if c == 0:
            return x
        return x + K(gc.basis_combination(V, gc.back_substitution(c, R, g)))

    z = start(w, rr)
    for k in range(1, maxiter + 1):
        j = (k - 1) % m
        c = j + 1
        w = A(z)
        h1 = np.array([dot(V[i], w) for i in range(c)])
        w = gc.subtract_columns(w, V, h1)
        h2 = np.array([dot(V[i], w) for i in range(c)])
        w = gc.subtract_columns(w, V, h2)
        nn = dot(w, w)
        status, e = gc.small_step(j, h1, h2, nn, cs, sn, R, g, thr)
        if status == "breakdown":
            return finish(x, j), k - 1, "breakdown", sq(hist)
        hist.append(e)
        if status == "converged":
            return finish(x, c), k, "converged", sq(hist)
        if c < m:
            V[c] = w / math.sqrt(nn)
            z = K(V[c])
            continue
        x = finish(x, c)
        w = b - A(x)
        rr = dot(w, w)
        if rr <= thr:
            hist[k] = rr
            return x, k, "converged", sq(hist)
        z = start(w, rr)
    return finish(x, maxiter % m), maxiter, "maxiter", sq(hist)


def bicgstab_op(rowptr, colidx, vals, b, K, rtol=1e-8, atol=0.0, maxiter=None, x0=None, dot=bc._dot_np):
    """``_bicgstab_cases.bicgstab`` with ``K`` a callable: (x, iterations, status, residual_norms)."""
    n = len(b)
    maxiter = 10 * n if maxiter is None else maxiter
    A = lambda u: pc.matvec(rowptr, colidx, vals, u)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    r = b.copy() if x0 is None else b - A(x)
    rhat, p = r.copy(), r.copy()
    rr = dot(r, r)
    rho = rr
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
        if not (abs(rho) > 0 and abs(rv) > 0):                  # gate A
            return x, j - 1, "breakdown", hist
        alpha = rho / rv
        s = r - alpha * v
        sh = K(s)
        t = A(sh)
        ts, tt, ss = dot(t, s), dot(t, t), dot(s, s)
        if ss <= thr:                                           # gate S
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
