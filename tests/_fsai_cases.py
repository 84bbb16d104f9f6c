"""Shared cases of the factorised sparse approximate inverse preconditioner (``hp.fsai``), a numpy restatement of its setup and
of ``hp.cg`` with ``M = Gt G``.

The restatement of the setup is the kernel's algorithm (csrc/fsai.hip) on plain arrays, one row at a time: J_i = the pattern
columns of row i inside the owned window and below i, ascending, then i; S = A[J_i, J_i] (an unstored entry is 0);
``fsai_cholesky`` factors S = L L' right-looking, column by column, with the kernel's operation order (divide the column by the
root of the pivot, subtract the outer product entry by entry, separately rounded) and back-substitutes L' y = e_m from the last
row up; ``fsai_solve`` is the independent form S^-1 e_m / sqrt((S^-1)_mm) through ``np.linalg.solve``.  ``row_start`` and the
local row count give the rank-local form: the rows are a rank's, the columns are global, and columns outside
[row_start, row_start + nloc) are ignored.

``pcg_op`` is ``_pcg_cases.pcg`` with z = Gt (G r) and r.z formed as u.u, u = G r, in the same gate order.

Cases
  scaled Poisson   ``_pcg_cases.scaled_poisson`` at 16x16, 24x20, 33x31 (1023 rows: an odd tail for the row groups).
  banded           n = 300, half-bandwidth w: a_ij = -1 / (1 + |i - j|) for 0 < |i - j| <= w, a_ii = 1 + the row's absolute sum
                   (strictly diagonally dominant, SPD).  Row i has m = min(i, w) + 1, so one matrix walks m from 1 up, across
                   the edges of the lane classes (4|5, 8|9, 16|17, 32).  w = 32 gives m = 33: over the cap.
  diagonal         ``_pcg_cases.diagonal_case``: G = diag(d^-1/2), CG converges in one iteration.
  not SPD          diag(1, -1, 2, 3); [[1, 2], [2, 1]] in rows 1..2 of the identity of size 5 (positive diagonal, second pivot
                   1 - 4 < 0 at row 2).
  no diagonal      tridiagonal n = 9 whose row 4 does not store its diagonal.
  pattern          the structure of A^2 for the 16x16 grid (up to 7 entries per row of G).
  three faults     ``three_faults``: 600 banded rows with a NaN diagonal, a diagonal that is not stored and a pivot that is not
                   positive, healed one at a time (the order of the error word).
  pattern is not A ``pattern_is_not_a``: a 40-row block whose pattern rows hold columns above the diagonal, ghosts in front of
                   the owned columns and entries A does not store, while A stores entries outside the pattern.
"""
import math

import numpy as np

from tests import _pcg_cases as pc

BANDED_N = 300
BANDED_W = [1, 3, 4, 7, 8, 15, 16, 31]
CAP_W = 32
BLOCKS = [1, 2, 3, 8]
JACOBI_FACTOR = 0.7        # pcg_op's iteration count against Jacobi's on the scaled Poisson cases (the issue's condition)
# Value margin of G against fsai_cholesky: LARGE_MARGIN_FACTOR = 10 times the largest relative difference, entry by entry,
# between fsai_cholesky and fsai_solve (two orders of the same sums) over every SPD case of this file.  Measured 4.53e-15
# (scaled Poisson 16x16, whose S carries the scaling's four decades; the banded cases stay below 1.3e-15);
# tests/test_fsai_cases.py re-measures it and holds ten times it below this constant.
FSAI_RTOL = 4.6e-14
# max |diag(G A G') - 1|: the row's g.(A g) is a sum of at most 32 + 32 separately rounded products after a solve with the
# same S; 2 m eps = 7.1e-15 at m = 32 bounds the products' and sums' share.  Measured 8.9e-16 over the cases.
DIAG_ONE_TOL = 1e-14
# The issue's condition holds pcg_op to JACOBI_FACTOR times Jacobi's count for 1, 2, 3 and 8 equal row blocks; 16x16 in 8 blocks
# (32 rows, two grid lines, per block) gives 38 against 53: 0.717.  The issue names this one combination as the one to leave out
# rather than loosen the factor, should the generator land there; it did.
JACOBI_SKIPPED = {((16, 16), 8)}


class NotPositiveDefinite(ValueError):
    def __init__(self, row):
        super().__init__(f"row {row}")
        self.row = row


class NoDiagonal(ValueError):
    def __init__(self, row):
        super().__init__(f"row {row}")
        self.row = row


def banded(w, n=BANDED_N):
    rowptr, cols, vals = [0], [], []
    for i in range(n):
        js = [j for j in range(max(0, i - w), min(n, i + w + 1))]
        off = {j: -1.0 / (1.0 + abs(i - j)) for j in js if j != i}
        for j in js:
            cols.append(j)
            vals.append(1.0 + sum(abs(v) for v in off.values()) if j == i else off[j])
        rowptr.append(len(cols))
    return np.array(rowptr, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals, dtype=np.float64)


def dense_to_csr(D, keep=None):
    """CSR of the nonzeros of a dense matrix (``keep``: a boolean mask of entries to store instead)."""
    D = np.asarray(D, dtype=np.float64)
    mask = (D != 0) if keep is None else keep
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    r, c = np.nonzero(mask)
    return rowptr, c.astype(np.int64), D[r, c]


def not_spd_diag():
    return pc.diag_matrix([1.0, -1.0, 2.0, 3.0]), 1                      # (matrix, the failing global row)


def not_spd_block():
    D = np.eye(5)
    D[1, 2] = D[2, 1] = 2.0
    return dense_to_csr(D), 2


def no_diagonal(n=9, row=4):
    D = 4.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    keep = D != 0
    keep[row, row] = False
    return dense_to_csr(D, keep), row


def square_pattern(rowptr, colidx):
    """(rowptr, colidx) of the structure of A^2: row i is the union of the rows its columns name."""
    n = len(rowptr) - 1
    rows = [colidx[rowptr[i]:rowptr[i + 1]] for i in range(n)]
    out_ptr, out = [0], []
    for i in range(n):
        u = np.unique(np.concatenate([rows[j] for j in rows[i]]))
        out.append(u)
        out_ptr.append(out_ptr[-1] + len(u))
    return np.array(out_ptr, dtype=np.int64), np.concatenate(out).astype(np.int64)


def _factor_cholesky(S, row):
    m = len(S)
    L = S.copy()
    for k in range(m):
        d = L[k, k]
        if not (d > 0.0):
            raise NotPositiveDefinite(row)
        lkk = math.sqrt(d)
        L[k + 1:, k] = L[k + 1:, k] / lkk
        L[k, k] = lkk
        for j in range(k + 1, m):
            L[j:, j] = L[j:, j] - L[j:, k] * L[j, k]
    acc = np.zeros(m)
    acc[m - 1] = 1.0
    y = np.zeros(m)
    for j in range(m - 1, -1, -1):
        y[j] = acc[j] / L[j, j]
        acc[:j] = acc[:j] - L[j, :j] * y[j]
    return y


def _factor_solve(S, row):
    m = len(S)
    e = np.zeros(m)
    e[m - 1] = 1.0
    x = np.linalg.solve(S, e)
    if not (x[m - 1] > 0.0):
        raise NotPositiveDefinite(row)
    return x / math.sqrt(x[m - 1])


def _fsai(rowptr, colidx, vals, row_start, pattern, factor):
    nloc = len(rowptr) - 1
    lo, hi = row_start, row_start + nloc
    prow, pcol = (rowptr, colidx) if pattern is None else pattern
    rows = [dict(zip(colidx[rowptr[i]:rowptr[i + 1]].tolist(), vals[rowptr[i]:rowptr[i + 1]].tolist())) for i in range(nloc)]
    g_rowptr, g_cols, g_vals = [0], [], []
    for i in range(nloc):
        gi = row_start + i
        if gi not in rows[i]:
            raise NoDiagonal(gi)
        pc_ = pcol[prow[i]:prow[i + 1]]
        J = sorted(int(c) for c in pc_ if lo <= c < gi) + [gi]
        assert all(c < hi for c in J)
        S = np.array([[rows[a - row_start].get(b, 0.0) for b in J] for a in J], dtype=np.float64)
        S = np.tril(S) + np.tril(S, -1).T                                # only the lower triangle is read
        g_cols += J
        g_vals += list(factor(S, gi))
        g_rowptr.append(len(g_cols))
    return np.array(g_rowptr, dtype=np.int64), np.array(g_cols, dtype=np.int64), np.array(g_vals, dtype=np.float64)


def fsai_cholesky(rowptr, colidx, vals, row_start=0, pattern=None):
    """G of the rows [row_start, row_start + nloc) in the kernel's operation order: (rowptr, global columns, values)."""
    return _fsai(rowptr, colidx, vals, row_start, pattern, _factor_cholesky)


def fsai_solve(rowptr, colidx, vals, row_start=0, pattern=None):
    return _fsai(rowptr, colidx, vals, row_start, pattern, _factor_solve)


def fsai_blocks(rowptr, colidx, vals, partition, pattern=None, fsai=fsai_cholesky):
    """The block-Jacobi G of a row partition (a list of boundaries): every block by the rank-local form, stacked."""
    ptr, cols, out, total = [np.zeros(1, dtype=np.int64)], [], [], 0
    for lo, hi in zip(partition[:-1], partition[1:]):
        lo, hi = int(lo), int(hi)
        a, b = int(rowptr[lo]), int(rowptr[hi])
        pat = None
        if pattern is not None:
            pa, pb = int(pattern[0][lo]), int(pattern[0][hi])
            pat = (pattern[0][lo:hi + 1] - pa, pattern[1][pa:pb])
        gp, gc, gv = fsai(rowptr[lo:hi + 1] - a, colidx[a:b], vals[a:b], lo, pat)
        ptr.append(gp[1:] + total)
        total += int(gp[-1])
        cols.append(gc)
        out.append(gv)
    return np.concatenate(ptr), np.concatenate(cols), np.concatenate(out)


def equal_blocks(n, k):
    return [(n * j) // k for j in range(k + 1)]


def transpose_csr(rowptr, colidx, vals, ncols):
    row_of = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.argsort(colidx, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=ncols))]).astype(np.int64)
    return tptr, row_of[order].astype(np.int64), vals[order]


def diag_gagt(rowptr, colidx, vals, G):
    """diag(G A G') for a G with global columns over all rows."""
    n = len(rowptr) - 1
    gp, gc, gv = G
    out = np.zeros(n)
    for i in range(n):
        g = np.zeros(n)
        g[gc[gp[i]:gp[i + 1]]] = gv[gp[i]:gp[i + 1]]
        out[i] = float(np.dot(g, pc.matvec(rowptr, colidx, vals, g)))
    return out


def pcg_op(rowptr, colidx, vals, b, G, rtol=1e-8, atol=0.0, maxiter=None, x0=None, dot=np.dot):
    """``_pcg_cases.pcg`` with prec = Gt (G .) and rz = u.u: (x, iterations, status, residual_norms)."""
    n = len(b)
    maxiter = 10 * n if maxiter is None else maxiter
    Gt = transpose_csr(*G, n)
    A = lambda v: pc.matvec(rowptr, colidx, vals, v)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    r = b.copy() if x0 is None else b - A(x)
    u = pc.matvec(*G, r)
    z = pc.matvec(*Gt, u)
    p = z.copy()
    rr, rz = float(dot(r, r)), float(dot(u, u))
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
        rr = float(dot(r, r))
        hist.append(math.sqrt(rr))
        converged = rr <= thr                               # gate B
        u = pc.matvec(*G, r)
        z = pc.matvec(*Gt, u)
        rz_new = float(dot(u, u))
        beta = rz_new / rz
        x = x + a * p                                       # the deferred x update rides on the direction update
        p = z + beta * p
        rz = rz_new
        if converged:
            return x, j, "converged", hist
    return x, maxiter, "maxiter", hist


# ---- inputs of the kernels' C entries, one block at a time ------------------------------------------------------------------
def to_scipy(rowptr, colidx, vals=None, ncols=None):
    """scipy CSR with exactly the stored entries given (ones where ``vals`` is None: a pattern)."""
    import scipy.sparse as sp
    n = len(rowptr) - 1
    vals = np.ones(len(colidx)) if vals is None else vals
    return sp.csr_matrix((np.array(vals, dtype=np.float64), np.array(colidx), np.array(rowptr)), shape=(n, n if ncols is None else ncols))


FAULT_ROWS = (40, 300, 520)                                     # NaN diagonal, no stored diagonal, a pivot that is not positive


def three_faults(heal=0, n=600, w=3):
    """``banded(w, n)`` with three faults, the first ``heal`` of them (in row order) taken out again: the diagonal of row 40 is
    NaN, row 300 does not store its diagonal, and the diagonal of row 520 is 0.01, positive but below the sum of squares of its
    row of L, so its pivot is negative.  (rowptr, colidx, vals); the pattern is the matrix's own."""
    rowptr, colidx, vals = banded(w, n)
    at = lambda r: int(rowptr[r] + np.flatnonzero(colidx[rowptr[r]:rowptr[r + 1]] == r)[0])
    vals = vals.copy()
    if heal < 3:
        vals[at(520)] = 0.01
    if heal < 1:
        vals[at(40)] = np.nan
    if heal < 2:
        keep = np.ones(len(colidx), dtype=bool)
        keep[at(300)] = False
        rowptr = rowptr.copy()
        rowptr[301:] -= 1
        colidx, vals = colidx[keep], vals[keep]
    return rowptr, colidx, vals


def pattern_is_not_a(n=60, lo=10, hi=50):
    """(A, pattern, thinned pattern, partition, block): scipy matrices of n rows whose block [lo, hi) is a 40-row rank-local
    case.  A is banded, half-bandwidth 3, strictly diagonally dominant.  A pattern row i holds i - 1 and i - 2 (stored by A),
    i - 5 (A does not store it), i + 1 and i + 4 (above the diagonal), on every third row columns 2 and 7 (ghosts, in front of
    the owned columns) and on every fourth row column n - 3 (a ghost behind them); the diagonal on odd rows only; never i - 3,
    which A stores.  The thinned pattern drops what the method ignores: the columns above the diagonal and the ghosts."""
    rowptr, colidx, vals = banded(3, n)
    full_ptr, full, thin_ptr, thin = [0], [], [0], []
    for i in range(n):
        cols = {i - 1, i - 2, i - 5, i + 1, i + 4}
        if i % 3 == 0:
            cols |= {2, 7}
        if i % 4 == 0:
            cols.add(n - 3)
        if i % 2:
            cols.add(i)
        cols = sorted(c for c in cols if 0 <= c < n)
        block_lo = lo if lo <= i < hi else 0
        block_hi = hi if lo <= i < hi else n
        kept = [c for c in cols if block_lo <= c < block_hi and c <= i]
        full += cols
        thin += kept
        full_ptr.append(len(full))
        thin_ptr.append(len(thin))
    A = to_scipy(rowptr, colidx, vals)
    P = to_scipy(np.array(full_ptr), np.array(full, dtype=np.int64))
    Pthin = to_scipy(np.array(thin_ptr), np.array(thin, dtype=np.int64))
    return A, P, Pthin, [0, lo, hi, n], 1


def spd_cases(orc):
    """name -> (rowptr, colidx, vals, b, pattern or None) of every SPD case."""
    out = {}
    for nx, ny in pc.SIZES:
        out[f"poisson{nx}x{ny}"] = (*pc.scaled_poisson(orc, nx, ny), None)
    for w in BANDED_W:
        m = banded(w)
        out[f"banded{w}"] = (*m, orc.fill_uniform(0, BANDED_N, pc.SEED_RHS), None)
    out["diagonal"] = (*pc.diagonal_case(orc), None)
    rowptr, colidx, vals, b = pc.scaled_poisson(orc, 16, 16)
    out["pattern16x16"] = (rowptr, colidx, vals, b, square_pattern(rowptr, colidx))
    return out
