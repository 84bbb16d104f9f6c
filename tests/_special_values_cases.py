"""Inputs of tests/test_gpu_special_values.py: matrices and operands that hold Inf, NaN, signed zeros, denormals and
finfo.max, built with numpy alone (checked on the CPU against the oracle in tests/test_special_values_cases.py).

Two structures:

* ``general()``: 1 500 x 6 000, most rows 0-11 entries, ten consecutive empty rows, rows of 465, 1 000, 1 100, 1 500, 2 049 and
  3 000 entries (past the 464-entry wave pass of the row-gather kernels, past CHUNK_MM = 1984 and the vector SpMM's pass)
  whose sums are finite, +Inf, -Inf, NaN and an exact zero by construction (LONG_CLASS), one
  column present in every non-empty row (a column of > 1 024 entries: several CHUNK_T passes of the transposed product),
  column 0 and the last column each present in a few dozen rows; ascending duplicate-free columns.
* ``banded()``: the 5-point matrix on a 256 x 130 grid (run tiles, 16-bit columns, packed copy).

Two rules (see the GPU module): ``rule="E"`` operands hold finfo.max as well (overflow in a product or a running sum is
part of the reference's bits); ``rule="C"`` operands do not, and keep finite magnitudes far below 1e150, so that no partial
sum can overflow in any order and the CLASS of every output (NaN / +Inf / -Inf / finite) is a function of the list of
products alone: ``classes_of``.
"""
import functools

import numpy as np

NROWS, NCOLS = 1500, 6000
DENSE_COL = 2999                      # present in every non-empty row
# Rows of at least 465 entries and the class every one of their sums must have, for every operand column and both rules: they
# are what reaches the kernels' multi-pass code, so their expected values must not all be NaN.  Their columns come from BAND
# only, where the operands hold ordinary numbers; their special VALUES are placed by hand (values()), never scattered.
FINITE, PINF, NINF, NAN = 0, 1, 2, 3
LONG = {5: 465, 63: 1500, 64: 2049, 700: 3000, 900: 1100, 901: 1000}
LONG_CLASS = {5: FINITE, 63: FINITE, 64: PINF, 700: NINF, 900: NAN, 901: FINITE}      # 901: all -0.0, an exact zero
BAND = (1000, 4500)
EMPTY = range(300, 310)
ZERO_ROWS = ((10, 0.0), (11, -0.0), (701, -0.0), (901, -0.0))     # whole rows of one signed zero: exact zero sums
NX, NY = 256, 130                     # banded variant
ZERO_ROWS_BANDED = tuple((r, 0.0) for r in range(1000, 1004)) + tuple((r, -0.0) for r in range(20000, 20004))
# (row, offset in the row, value): offsets before and behind the first 464-entry pass and the 1984-entry chunk, and near the end
PLACED = ((64, 100, np.inf), (64, 1000, np.inf), (64, 2040, np.inf),
          (700, 50, -np.inf), (700, 1990, -np.inf), (700, 2990, -np.inf),
          (900, 600, np.nan),
          (5, 3, -0.0), (5, 7, 0.0), (5, 100, "denormal"), (5, 200, "max"), (5, 460, "denormal"),
          (63, 1, -0.0), (63, 470, "denormal"), (63, 900, 0.0), (63, 1495, -0.0))


@functools.lru_cache(maxsize=None)
def _general(seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, NROWS)
    for r, l in LONG.items():
        lens[r] = l
    for r, _ in ZERO_ROWS:
        lens[r] = max(lens[r], 4)
    lens[list(EMPTY)] = 0
    others = np.delete(np.arange(NCOLS), DENSE_COL)
    band = np.setdiff1d(np.arange(*BAND), [DENSE_COL])
    cols = []
    for r, l in enumerate(lens):
        if l == 0:
            continue
        forced = [DENSE_COL]
        if r not in LONG and l >= 3 and r % 37 == 0:
            forced.append(0)
        if r not in LONG and l >= 3 and r % 41 == 0:
            forced.append(NCOLS - 1)
        pool = band if r in LONG else np.setdiff1d(others, forced)
        rest = rng.choice(pool, int(l) - len(forced), replace=False)
        cols.append(np.sort(np.concatenate([forced, rest])))
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rowptr, np.concatenate(cols).astype(np.int64)


def general(seed=1):
    """(rowptr, col) int64 of the general structure."""
    rowptr, col = _general(seed)
    return rowptr.copy(), col.copy()


def positive_operand_rows(n):
    """Operand rows that must hold ordinary POSITIVE numbers in the structure with n columns: the columns that the all -0.0
    rows read (every product of such a row is then -0.0: the reference's sum is 0.0 + -0.0 + ... = +0.0, while a kernel that
    starts from its first product instead of from zero returns -0.0), and the columns of the +-Inf values placed in the long
    rows (their products then keep the sign of the value: a row of +Inf products only, a row of -Inf products only)."""
    if n == NCOLS:
        rowptr, col = _general(1)
        rows = [r for r, z in ZERO_ROWS if np.signbit(z)]
        placed = [col[rowptr[r] + o] for r, o, v in PLACED if isinstance(v, float) and np.isinf(v)]
    elif n == NX * NY:
        rowptr, col, _ = banded()
        rows = [r for r, z in ZERO_ROWS_BANDED if np.signbit(z)]
        placed = []
    else:
        return np.zeros(0, dtype=np.int64)
    return np.unique(np.concatenate([col[rowptr[r]:rowptr[r + 1]] for r in rows] + [np.array(placed, dtype=np.int64)]))


def banded():
    """(rowptr, col, vals) of the 5-point matrix on the NX x NY grid, row i = y * NX + x, columns ascending (the oracle's
    poisson2d_rows, restated)."""
    n = NX * NY
    i = np.arange(n)
    x, y = i % NX, i // NX
    cand = np.stack([i - NX, i - 1, i, i + 1, i + NX], axis=1)
    ok = np.stack([y > 0, x > 0, np.ones(n, bool), x < NX - 1, y < NY - 1], axis=1)
    v = np.tile(np.array([-1.0, -1.0, 4.0, -1.0, -1.0]), (n, 1))
    rowptr = np.concatenate([[0], np.cumsum(ok.sum(1))]).astype(np.int64)
    return rowptr, cand[ok].astype(np.int64), v[ok]


def _scatter(rng, a, value, count, avoid=None):
    idx = rng.choice(len(a), count, replace=False)
    if avoid is not None:
        idx = idx[~avoid[idx]]
    a[idx] = value
    return idx


def values(rowptr, col, T, seed=2, nan=True, base=None, special=True):
    """Stored values: random normal (or `base`), then scattered +0.0, -0.0, +Inf, -Inf, a denormal and a few NaN; whole
    rows of signed zeros (ZERO_ROWS / ZERO_ROWS_BANDED).  General structure: the scattered specials stay out of the long rows,
    whose specials are PLACED so that each long row has the class LONG_CLASS names; the entries of DENSE_COL are ordinary
    positive numbers (a special there would reach every row; positive, so that the transposed product's sum over that
    column has one class per operand column).  special=False: the plain random values."""
    rng = np.random.default_rng(seed)
    vals = (rng.standard_normal(len(col)) if base is None else base.copy()).astype(T)
    is_general = len(rowptr) - 1 == NROWS
    if is_general:
        vals[col == DENSE_COL] = np.abs(vals[col == DENSE_COL]) + T(0.125)
    if not special:
        return vals
    keep = np.zeros(len(col), bool)
    if is_general:
        keep |= col == DENSE_COL
        for r in LONG:
            keep[rowptr[r]:rowptr[r + 1]] = True
    scale = max(1, len(vals) // 16000)
    _scatter(rng, vals, 0.0, 60 * scale, keep)
    _scatter(rng, vals, -0.0, 60 * scale, keep)
    _scatter(rng, vals, np.inf, 25 * scale, keep)
    _scatter(rng, vals, -np.inf, 25 * scale, keep)
    _scatter(rng, vals, np.finfo(T).tiny / 8, 10 * scale, keep)
    if nan:
        _scatter(rng, vals, np.nan, 8 * scale, keep)
    if is_general:
        named = {"denormal": np.finfo(T).tiny / 8, "max": np.finfo(T).max}
        for r, o, v in PLACED:
            assert o < rowptr[r + 1] - rowptr[r] and col[rowptr[r] + o] != DENSE_COL
            vals[rowptr[r] + o] = named.get(v, v)
    for r, z in (ZERO_ROWS if is_general else ZERO_ROWS_BANDED):
        vals[rowptr[r]:rowptr[r + 1]] = z
    return vals


def operand(n, k, T, rule="E", seed=3, pin_ends=True, per=40, ordinary=()):
    """Dense operand (n x k): column c holds ONE kind of special -- +Inf, -Inf, NaN, -0.0 for c % 4 = 0 .. 3 -- at ~`per` rows;
    rule E: finfo.max at ~`per` rows of every column c % 4 == 0.  Row 0 and row n - 1 (what padded / clamped lanes re-read)
    hold the column's special.  n == NCOLS: the specials lie outside BAND (the long rows read ordinary numbers and get their
    classes from the placed values).  positive_operand_rows(n) hold ordinary positive numbers, the rows `ordinary` ordinary ones."""
    rng = np.random.default_rng(seed + 17 * k)
    B = (rng.random((n, k)) - 0.5).astype(T)
    B[B == 0] = T(0.125)
    kinds = (np.inf, -np.inf, np.nan, -0.0)
    per = min(per, max(1, n // 8))
    where = np.setdiff1d(np.arange(n), np.arange(*BAND)) if n == NCOLS else np.arange(n)
    for c in range(k):
        B[rng.choice(where, per, replace=False), c] = kinds[c % 4]
        if rule == "E" and c % 4 == 0:
            B[rng.choice(where, per, replace=False), c] = np.finfo(T).max
        if pin_ends:
            B[0, c] = kinds[c % 4]
            B[n - 1, c] = kinds[c % 4]
    pos = positive_operand_rows(n)
    B[pos] = (rng.random((len(pos), k)) + 0.25).astype(T)
    ordinary = np.asarray(ordinary, dtype=np.int64)
    B[ordinary] = (rng.random((len(ordinary), k)) - 0.75).astype(T)
    return B


def vector(n, T, case, where, seed=4):
    """Reduction operand: uniform in (-0.5, 0.5) with no zero, then one NaN / one +Inf / +Inf and -Inf placed at `where`
    (and, for the pair, at another index)."""
    rng = np.random.default_rng(seed + n)
    x = (rng.random(n) - 0.5).astype(T)
    x[x == 0] = T(0.25)
    if case == "nan":
        x[where] = np.nan
    elif case == "pinf":
        x[where] = np.inf
    elif case == "pinf_ninf":
        x[where] = np.inf
        if n > 1:
            other = (where + n // 2) % n
            x[other if other != where else (where + 1) % n] = -np.inf
    else:
        raise ValueError(case)
    return x


def classes_of(products, axis=0):
    """Order-independent class of a sum from its list of products: any NaN product, or +Inf and -Inf products -> NAN; only
    +Inf -> PINF; only -Inf -> NINF; else FINITE (valid while no finite partial sum can overflow: rule C operands)."""
    p = np.asarray(products)
    nan = np.isnan(p).any(axis=axis)
    pinf = np.isposinf(p).any(axis=axis)
    ninf = np.isneginf(p).any(axis=axis)
    out = np.full(nan.shape, FINITE, dtype=np.int64)
    out[pinf] = PINF
    out[ninf] = NINF
    out[nan | (pinf & ninf)] = NAN
    return out


def csr_classes(rowptr, col, vals, x):
    """(classes, finite reference, bound sum |a||x|) per row of A * x, products formed in double."""
    n = len(rowptr) - 1
    rowid = np.repeat(np.arange(n), np.diff(rowptr))
    with np.errstate(all="ignore"):
        p = vals.astype(np.float64) * x.astype(np.float64)[col]
    cnt = lambda m: np.bincount(rowid, weights=m.astype(np.float64), minlength=n) > 0
    nan, pinf, ninf = cnt(np.isnan(p)), cnt(np.isposinf(p)), cnt(np.isneginf(p))
    cls = np.full(n, FINITE, dtype=np.int64)
    cls[pinf] = PINF
    cls[ninf] = NINF
    cls[nan | (pinf & ninf)] = NAN
    fin = np.where(np.isfinite(p), p, 0.0)
    ref = np.bincount(rowid, weights=fin, minlength=n)
    bound = np.bincount(rowid, weights=np.abs(fin), minlength=n)
    return cls, ref, bound


def class_of_values(got):
    got = np.asarray(got)
    out = np.full(got.shape, FINITE, dtype=np.int64)
    out[np.isposinf(got)] = PINF
    out[np.isneginf(got)] = NINF
    out[np.isnan(got)] = NAN
    return out


def transpose_csr(rowptr, col, vals, ncols):
    """CSR of the transpose with equal columns in stored (= row) order: the order hpcla_spmm_t_struct_* pins."""
    n = len(rowptr) - 1
    rowid = np.repeat(np.arange(n), np.diff(rowptr))
    perm = np.argsort(col, kind="stable")
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=ncols))]).astype(np.int64)
    return t_rowptr, rowid[perm].astype(np.int64), vals[perm]
