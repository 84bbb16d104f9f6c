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

The second half of the module states the kernels one at a time for tests/test_gpu_ilu_kernels.py, which compares bits
(``block_of_split``, ``column_view``, ``merge_products``, ``init_values``, ``sweep_once``, ``pivots``, ``trisweep``, ``apply_chain``;
none of them raises: a bad diagonal gives NaN as on the device), with the cases those tests add: ``arrow``, ``comb``, ``ragged``,
``generated_rows``, ``nnz_edge``, ``duplicated_block``, ``fault_case``, ``pivot_case``, ``shuffled_rows``.

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


# ---- the kernels one at a time (tests/test_gpu_ilu_kernels.py) ------------------------------------------------------------------
# Each function below states one kernel of csrc/ilu.hip on plain arrays, one rounded operation at a time in the kernel's order, so
# that its bits are the kernel's.  None of them raises on a missing or bad diagonal: they put NaN where the kernel does and carry
# Inf / NaN through, as the kernels do when the caller ignores the error word.
NO_DIAG, BAD_DIAG, BAD_PIVOT = 1, 2, 3                           # the codes of the error word
NO_FAILURE = -1                                                  # the word with all bits set, read as int64
KERNEL_FORMS_ON = ("convdiff33x31", "banded16", "asymmetric", "convdiff%dx%d" % pc.LARGE_SIZE)
KERNEL_FORMS_BLOCKS = (3, 8)
SHUFFLED_ON = ("asymmetric", "banded16")
ROW_EDGES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 256 * 1024 + 1]      # the last: SCAN_T * SCAN_B + 1, phase 2's carry
NNZ_EDGES = [1, 255, 256, 257]                                   # around one workgroup of the per-entry kernels
ARROW_N = 300
COMB_N = 96
FAULT_ROW = 150
FAULT_KINDS = ("nan_diagonal", "no_diagonal", "zero_diagonal", "inf_diagonal", "nan_off", "inf_off", "negative_zero_off")
RAGGED_SIZES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023]
LANES = [1, 2, 4, 8]
PIVOT_SIZES = [1, 256, 257, 600]
PIVOT_SPECIALS = [5e-324, float("inf"), 1e-310, 0.0, 1e308, float("nan"), -0.0, float("-inf")]
_ALL_ONES = (1 << 64) - 1


def _lower(word, rows, codes):
    """The error word after an unsigned atomic min with (row << 2) | code of every failing row."""
    w = _ALL_ONES if int(word) == NO_FAILURE else int(word)
    for r, c in zip(np.asarray(rows).tolist(), np.broadcast_to(codes, np.shape(rows)).tolist()):
        w = min(w, (int(r) << 2) | int(c))
    return NO_FAILURE if w == _ALL_ONES else w


def block_of_split(rowptr, colval_split, vals, n_own, base=0):
    """``hpcla_ilu_count`` + ``hpcla_ilu_fill`` + ``hpcla_ilu_gather`` on rows in split form, in any stored order: (bp, bc, brows,
    bdiag, bmap, a_vals, word).  Owned entries (c - base < n_own) are placed per row by a stable sort on the column; ``bmap`` holds
    positions in A's arrays; ``bdiag`` is -1 where no diagonal is stored and, where a row stores its diagonal twice, the position
    of the last stored one; ``word`` is the error word the fill alone leaves."""
    rp = np.asarray(rowptr, dtype=np.int64) - base
    c = np.asarray(colval_split, dtype=np.int64) - base
    vals = np.asarray(vals, dtype=np.float64)
    n = len(rp) - 1
    assert rp[0] == 0 and n == n_own
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    own = np.flatnonzero(c[:rp[n]] < n_own)
    bmap = own[np.lexsort((own, c[own], row_of[own]))]          # by row, then column, then stored position
    bc, brows = c[bmap], row_of[bmap]
    bp = np.concatenate([[0], np.cumsum(np.bincount(brows, minlength=n))]).astype(np.int64)
    bdiag = np.full(n, -1, dtype=np.int64)
    on = np.flatnonzero(bc == brows)
    np.maximum.at(bdiag, brows[on], on)
    a_vals = vals[bmap]
    d = a_vals[np.maximum(bdiag, 0)] if len(a_vals) else np.ones(n)
    code = np.where(bdiag < 0, NO_DIAG, np.where((d == 0.0) | (d != d), BAD_DIAG, 0))
    bad = np.flatnonzero(code)
    return bp, bc, brows, bdiag, bmap, a_vals, _lower(NO_FAILURE, bad[:1], code[bad[:1]])


def column_view(bp, bc):
    """(c_ptr, c_pos): the entries of column j in ascending row as positions into the block, the stable sort of hp/ilu.py."""
    n = len(bp) - 1
    c_pos = np.argsort(bc, kind="stable").astype(np.int64)
    c_ptr = np.concatenate([[0], np.cumsum(np.bincount(bc, minlength=n))]).astype(np.int64)
    return c_ptr, c_pos


def merge_products(bp, bc, brows, c_ptr, c_pos):
    """The two-pointer merge of ``ilu_sweep_kernel`` walked for every entry: (ent, lpos, upos, stats).  The first three list the
    products l_ik * u_kj in the order the lane meets them (entry, position of l_ik, position of u_kj); ``stats[p]`` counts the
    matches, the steps that advance the row pointer alone, those that advance the column pointer alone, and is 1 in its last
    column when the walk ended at the break ``kr >= m || kc >= m`` (entries left on both sides), 0 when a side ran out."""
    bpl, bcl, brl, cpl, cql = (np.asarray(a).tolist() for a in (bp, bc, brows, c_ptr, c_pos))
    ent, lpos, upos = [], [], []
    stats = np.zeros((len(bcl), 4), dtype=np.int64)
    for p in range(len(bcl)):
        i, j = brl[p], bcl[p]
        m = i if i < j else j
        rp, re, cq, ce = bpl[i], bpl[i + 1], cpl[j], cpl[j + 1]
        nm = nr = nc = broke = 0
        while rp < re and cq < ce:
            q = cql[cq]
            kr, kc = bcl[rp], brl[q]
            if kr >= m or kc >= m:
                broke = 1
                break
            if kr == kc:
                ent.append(p)
                lpos.append(rp)
                upos.append(q)
                rp += 1
                cq += 1
                nm += 1
            elif kr < kc:
                rp += 1
                nr += 1
            else:
                cq += 1
                nc += 1
        stats[p] = (nm, nr, nc, broke)
    as_array = lambda v: np.array(v, dtype=np.int64)
    return as_array(ent), as_array(lpos), as_array(upos), stats


def init_values(bc, brows, bdiag, a_vals):
    """``ilu_init_kernel``: l_ij = a_ij / a_jj (NaN where column j stores no diagonal), u_ij = a_ij."""
    if not len(bc):
        return a_vals.copy()
    dj = bdiag[bc]
    with np.errstate(all="ignore"):
        return np.where(brows > bc, a_vals / np.where(dj >= 0, a_vals[np.maximum(dj, 0)], np.nan), a_vals)


def sweep_once(bc, brows, bdiag, a_vals, products, f_old):
    """``ilu_sweep_kernel``: s = a_ij minus the products of ``merge_products`` one at a time in their order, multiply and
    subtraction separately rounded, from ``f_old``; l_ij = s / f_old's u_jj (NaN where column j stores no diagonal), u_ij = s."""
    nnz = len(bc)
    if not nnz:
        return a_vals.copy()
    ent, lpos, upos = products[:3]
    count = np.bincount(ent, minlength=nnz)
    first = np.concatenate([[0], np.cumsum(count)])[:-1]
    s = a_vals.copy()
    dj = bdiag[bc]
    with np.errstate(all="ignore"):
        for t in range(int(count.max())):                       # the t-th product of every entry that has one
            has = np.flatnonzero(count > t)
            at = first[has] + t
            s[has] = s[has] - f_old[lpos[at]] * f_old[upos[at]]
        return np.where(brows > bc, s / np.where(dj >= 0, f_old[np.maximum(dj, 0)], np.nan), s)


def factor_chain(bc, brows, bdiag, a_vals, products, sweeps):
    """[init, after sweep 1, ..., after sweep ``sweeps``]."""
    out = [init_values(bc, brows, bdiag, a_vals)]
    for _ in range(sweeps):
        out.append(sweep_once(bc, brows, bdiag, a_vals, products, out[-1]))
    return out


def pivots(bdiag, f, word_in=NO_FAILURE):
    """``ilu_pivots_kernel``: (dinv, word).  dinv = 1 / u_ii bit for bit (inf for a denormal u, NaN without a diagonal, which
    raises no code here); a u that is zero of either sign, NaN or infinite lowers the word with code 3."""
    has = bdiag >= 0
    u = np.where(has, np.asarray(f, dtype=np.float64)[np.maximum(bdiag, 0)], np.nan)
    with np.errstate(all="ignore"):
        dinv = 1.0 / u
    bad = np.flatnonzero(has & ((u == 0.0) | (u != u) | np.isinf(u)))
    return dinv, _lower(word_in, bad[:1], BAD_PIVOT)


def trisweep(bp, bc, bdiag, f, rhs, inp, dinv, upper, lanes):
    """``ilu_trisweep_kernel<lanes>``: out_i = (rhs_i - sum over the lower (upper) part of row i of f_p * inp[col_p]) [* dinv_i].
    lanes = 1: the running subtraction in stored order.  lanes = 2, 4, 8: lane ``sub`` adds the products at lo + sub, lo + sub +
    lanes, ... to 0.0 in turn, the partial sums meet by the xor butterfly from lanes / 2 down to 1 (every lane adds its
    partner's value to its own), and lane 0's sum is subtracted from rhs_i once.  ``inp is None``: an empty sum."""
    n = len(bp) - 1
    rhs = np.asarray(rhs, dtype=np.float64)
    if inp is None:
        lo = hi = np.zeros(n, dtype=np.int64)
    else:
        lo = bdiag + 1 if upper else bp[:-1]
        hi = bp[1:] if upper else bdiag
    length = np.maximum(hi - lo, 0)
    with np.errstate(all="ignore"):
        if lanes == 1:
            acc = rhs.copy()
            for t in range(int(length.max()) if n else 0):
                rows = np.flatnonzero(length > t)
                p = lo[rows] + t
                acc[rows] = acc[rows] - f[p] * inp[bc[p]]
        else:
            part = np.zeros((n, lanes))
            for sub in range(lanes):
                trips = np.maximum(length - sub + lanes - 1, 0) // lanes
                for t in range(int(trips.max()) if n else 0):
                    rows = np.flatnonzero(trips > t)
                    p = lo[rows] + sub + t * lanes
                    part[rows, sub] = part[rows, sub] + f[p] * inp[bc[p]]
            off = lanes // 2
            while off >= 1:
                part = part + part[:, np.arange(lanes) ^ off]
                off //= 2
            acc = rhs - part[:, 0]
        return acc * dinv if dinv is not None else acc


def apply_chain(bp, bc, bdiag, f, dinv, r, solve_sweeps, lanes):
    """The launches of ``hpcla_ilu_apply_f64``: y_0 = r, y_{m+1} = r - L y_m; z_0 = dinv .* y, z_{m+1} = dinv .* (y - U z_m)."""
    y = np.asarray(r, dtype=np.float64)
    for _ in range(solve_sweeps):
        y = trisweep(bp, bc, bdiag, f, r, y, None, 0, lanes)
    z = None
    for _ in range(solve_sweeps + 1):
        z = trisweep(bp, bc, bdiag, f, y, z, dinv, 1, lanes)
    return z


# ---- their cases ------------------------------------------------------------------------------------------------------------------
def _csr(rows):
    """(rowptr, cols, vals) of a list of rows, each a list of (column, value) in the order to store."""
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.array([c for r in rows for c, _ in r], dtype=np.int64), np.array([v for r in rows for _, v in r], dtype=np.float64)


def _dominant(rows_off):
    """Sorted rows from {column: value} of the off-diagonals of every row, with a_ii = 1 + the row's absolute sum."""
    rows = []
    for i, off in enumerate(rows_off):
        off = dict(off)
        off[i] = 1.0 + sum(abs(v) for v in off.values())
        rows.append(sorted(off.items()))
    return _csr(rows)


def arrow(n=ARROW_N):
    """Diagonal plus a dense last row and last column, nonsymmetric, strictly diagonally dominant: entry (n - 1, n - 1) merges
    n - 1 entries against n - 1 with every k matching.  Its sum starts above 32 and ends below, so its bits depend on the order
    of the terms (a sum whose partial sums stay within one binade rounds every term to the same grid, in any order)."""
    rows = [{n - 1: -0.4 / (1.0 + i % 7) - 0.01 * math.sqrt(i + 1.0)} for i in range(n - 1)]
    rows.append({j: -0.15 / (1.0 + j % 5) - 0.004 * math.sqrt(j + 2.0) for j in range(n - 1)})
    return _dominant(rows)


def comb(n=COMB_N):
    """Row i stores (i, k) for the even k < i, column j stores (k, j) for the k < j that are multiples of 3: the merge of an entry
    matches at the multiples of 6 and advances the row alone at the other even k, the column alone at the odd multiples of 3."""
    rows = [dict() for _ in range(n)]
    for i in range(n):
        for k in range(0, i, 2):
            rows[i][k] = -1.0 / (1.0 + (i - k)) - 0.01 * (k % 7)
        if i % 3 == 0:
            for j in range(i + 1, n):
                rows[i][j] = -0.4 / (1.0 + (j - i)) - 0.01 * (j % 5)
    return _dominant(rows)


def ragged(n, seed=4242):
    """Row i has a lower part of min(i, (7 i) % 20) entries and an upper part of min(n - 1 - i, (5 i) % 19), at seeded columns
    with seeded values in (-0.1, 0.1), and the diagonal 1 + the row's absolute sum."""
    rng = np.random.default_rng(seed + n)
    rows = []
    for i in range(n):
        lower = rng.choice(i, size=min(i, (7 * i) % 20), replace=False) if i else []
        upper = i + 1 + rng.choice(n - 1 - i, size=min(n - 1 - i, (5 * i) % 19), replace=False) if n - 1 - i else []
        rows.append({int(c): float(rng.uniform(-0.1, 0.1)) for c in list(lower) + list(upper)})
    return _dominant(rows)


def generated_rows(nrows, seed=977):
    """(rowptr, colval_split, vals) in split form, base 0, n_own = nrows: every row stores its diagonal and 0 to 2 off-diagonals
    at seeded columns of [0, nrows + max(3, nrows // 4)), the columns from nrows on being ghosts, in the stored order first
    off-diagonal, diagonal, second off-diagonal (not ascending)."""
    rng = np.random.default_rng(seed + nrows)
    n = int(nrows)
    span = n + max(3, n // 4)
    i = np.arange(n, dtype=np.int64)
    k = rng.integers(0, 3, n)
    c1 = (i + 1 + rng.integers(0, span - 1, n)) % span          # never the diagonal
    c2 = (i + 1 + rng.integers(0, span - 1, n)) % span
    c2 = np.where(c2 == c1, span, c2)                           # one more ghost in place of a duplicate
    cols = np.stack([c1, i, c2], axis=1)
    keep = np.stack([k >= 1, np.ones(n, dtype=bool), k == 2], axis=1)
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    colval = cols[keep]
    return rowptr, colval, rng.uniform(0.5, 1.5, len(colval))


def nnz_edge(nnz):
    """A block of exactly ``nnz`` entries: 1 x 1, or the tridiagonal ``banded(1, 86)`` (256 entries) without (85, 84) or with
    (0, 2) = -0.1."""
    if nnz == 1:
        return one_by_one()
    rowptr, cols, vals = banded(1, 86)
    rows = [list(zip(cols[rowptr[i]:rowptr[i + 1]].tolist(), vals[rowptr[i]:rowptr[i + 1]].tolist())) for i in range(86)]
    if nnz == 255:
        rows[85] = [(c, v) for c, v in rows[85] if c != 84]
    elif nnz == 257:
        rows[0].append((2, -0.1))
    else:
        assert nnz == 256
    return _csr(rows)


def duplicated_block():
    """(rowptr, colval_split, vals, n_own) of four owned rows, some of which store a column twice, the diagonal among them; ghosts
    are the columns 4 and 5."""
    rows = [
        [(1, -1.0), (0, 4.0), (0, 5.0), (5, -9.0)],             # the diagonal twice, side by side
        [(1, 6.0), (4, -9.0), (0, -2.0), (1, 0.0), (3, 1.5)],   # the diagonal twice, apart; the last stored one is zero
        [(3, -1.0), (3, -2.0), (2, 7.0), (5, 1.0), (5, 2.0)],   # an off-diagonal twice, a ghost twice
        [(3, 8.0)],
    ]
    return (*_csr(rows), 4)


def fault_case(kind, w=8, r=FAULT_ROW):
    """``banded(w)`` with one fault in row r: a diagonal that is NaN, removed, zero or +Inf, or the off-diagonal (r, r - 2)
    NaN, the off-diagonal (r, r + 2) +Inf, or (r, r - 2) -0.0.  ``kind`` None: the clean matrix."""
    rowptr, cols, vals = banded(w)
    vals = vals.copy()
    at = lambda c: int(rowptr[r] + np.flatnonzero(cols[rowptr[r]:rowptr[r + 1]] == c)[0])
    if kind == "no_diagonal":
        keep = np.ones(len(cols), dtype=bool)
        keep[at(r)] = False
        rowptr = rowptr.copy()
        rowptr[r + 1:] -= 1
        return rowptr, cols[keep], vals[keep]
    where, value = {None: (r, vals[at(r)]), "nan_diagonal": (r, np.nan), "zero_diagonal": (r, 0.0), "inf_diagonal": (r, np.inf),
                    "nan_off": (r - 2, np.nan), "inf_off": (r + 2, np.inf), "negative_zero_off": (r - 2, -0.0)}[kind]
    vals[at(where)] = value
    return rowptr, cols, vals


def pivot_case(nrows, seed=31):
    """(bdiag, f): ``bdiag`` a seeded permutation of the positions with -1 in rows 1 and nrows - 2 (nrows > 3), ``f`` ordinary
    values in (1, 2) with ``PIVOT_SPECIALS`` on the diagonals of eight rows spread over the block (nrows >= 16)."""
    rng = np.random.default_rng(seed + nrows)
    bdiag = rng.permutation(nrows).astype(np.int64)
    f = rng.uniform(1.0, 2.0, nrows)
    if nrows >= 16:
        rows = np.linspace(3, nrows - 1, len(PIVOT_SPECIALS)).astype(np.int64)
        f[bdiag[rows]] = PIVOT_SPECIALS
    if nrows > 3:
        bdiag[[1, nrows - 2]] = -1
    return bdiag, f


def shuffled_rows(rowptr, colval, vals, rng):
    """The same rows with every row's entries in a seeded order: (colval, vals, perm) with new[e] = old[perm[e]]."""
    perm = np.concatenate([rowptr[i] + rng.permutation(int(rowptr[i + 1] - rowptr[i])) for i in range(len(rowptr) - 1)]
                          + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return np.asarray(colval)[perm], np.asarray(vals)[perm], perm


def kernel_cases(orc):
    """name -> (rowptr, colidx, vals): every ``factor_cases`` matrix, the 65 x 63 case included, then ``arrow`` and ``comb``."""
    out = {name: c[:3] for name, c in factor_cases(orc, large=True).items()}
    out["arrow"] = arrow()
    out["comb"] = comb()
    return out


def to_scipy(rowptr, colidx, vals):
    import scipy.sparse as sp
    n = len(rowptr) - 1
    return sp.csr_matrix((np.asarray(vals, dtype=np.float64), np.asarray(colidx), np.asarray(rowptr)), shape=(n, n))


def block_inputs(name, matrix):
    """Every (k, j, partition) a kernel test cuts ``matrix`` into: 1, 2, 3 and 8 equal blocks, the empty ones left out; ``arrow``
    and ``comb`` stay whole (their long merges need the whole row and column)."""
    n = len(matrix[0]) - 1
    for k in (BLOCKS if name not in ("arrow", "comb") else [1]):
        part = equal_blocks(n, k)
        for j in range(k):
            if part[j + 1] > part[j]:
                yield k, j, part


def block_reference(matrix, part, j, sweeps=3):
    """What the restatements say of block j: the split form (Int32, base 0), the block, its column view, its merges and the factor
    values after init and each of ``sweeps`` sweeps."""
    from tests import _amg_cases as ac
    rowptr, split, vals, n_own, ghosts = ac.split_block(to_scipy(*matrix), part, j)
    bp, bcols, brows, bdiag, bmap, a_vals, word = block_of_split(rowptr, split, vals, n_own)
    c_ptr, c_pos = column_view(bp, bcols)
    products = merge_products(bp, bcols, brows, c_ptr, c_pos)
    return dict(split=(rowptr, split, vals), n=n_own, ghosts=len(ghosts), bp=bp, bc=bcols, brows=brows, bdiag=bdiag, bmap=bmap,
                a_vals=a_vals, word=word, c_ptr=c_ptr, c_pos=c_pos, products=products,
                f=factor_chain(bcols, brows, bdiag, a_vals, products, sweeps))
