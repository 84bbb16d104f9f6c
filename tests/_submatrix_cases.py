"""Cases and the numpy restatement of range indexing (``A[r0:r1, c0:c1]``, ``A[:, k]``; src/indexing.jl:691-914), shared by
tests/test_submatrix_cases.py (CPU: the restatement against scipy, the partitions against a transcription of the reference),
tests/test_gpu_submatrix.py (one rank) and tests/_multirank_submatrix_worker.py (several).

The restatement: mask the stored entries by row window and GLOBAL column window, ``bincount`` -> rowptr, unique kept columns
-> col_indices, colval = rank in that list.  Entries are only selected, never touched, so every comparison is of bits.

Matrices (global CSR, columns ascending within a row, built once per process):
  rand   3 000 x 5 000, row lengths 0 .. ~700: empty rows, rows of exactly 63 / 64 / 65 and 255 / 256 / 257 entries (a lane's
         run, a wave and a 256-thread workgroup boundary are crossed inside a row), one row of 650 (> 512).  Columns
         GAP_LO .. GAP_HI - 1 are stored nowhere.  Row WHOLE_ROW lies wholly inside columns BLOCK_A, row OTHER_ROW wholly inside
         BLOCK_B.  Values carry planted 0.0, -0.0, NaN, +-Inf and denormals; (NEGZERO_ROW, NEGZERO_COL) stores -0.0.
  p5     the 5-point matrix of a 96 x 96 grid (9 216 rows).
  band   70 001 rows, 3 entries per row: SCAN_CHUNK = 1 024 elements per workgroup of the scan (csrc/scan.h), so the row
         scan of the full range runs over 69 chunks and the column scan over as many.
  band263537  the same band with BAND_LONG_ROWS = 263 537 rows (``band<n>`` is the band of n rows).  One workgroup scans the
         chunks' sums 256 at a time and carries the running total from trip to trip, so the carry first matters beyond
         256 * 1 024 = 262 144 scanned elements.  band_long_rows selects 262 157 rows (the row scan has one element more: 257
         chunks, a second trip with one live lane) and cuts them to columns 150 000 .. 262 999, so the chunks of the first
         trip hold none, some or 3 072 entries and those of the second some: a carry from the wrong trip shows in rowptr.
         band_long_cols selects columns 7 .. 263 499 (263 493 wide: 258 chunks) of rows 259 000 .. 263 536, so the columns
         that occur lie on both sides of the first carry and most chunks are empty.
"""
import functools

import numpy as np

SCAN_CHUNK = 1024
BAND_ROWS = 68 * SCAN_CHUNK + 369            # 70 001: several chunks, and not a multiple of one
assert BAND_ROWS == 70001
SCAN_TRIP = 256 * SCAN_CHUNK                 # elements whose chunk sums one trip of the scan's second phase covers
BAND_LONG_ROWS = SCAN_TRIP + SCAN_CHUNK + 369
BAND_LONG = f"band{BAND_LONG_ROWS}"
assert BAND_LONG_ROWS == 263537

NR, NC = 3000, 5000
GAP_LO, GAP_HI = 2000, 2010
BLOCK_A, BLOCK_B = (1000, 1100), (3000, 3100)
WHOLE_ROW, OTHER_ROW = 130, 131
NEGZERO_ROW, NEGZERO_COL = 140, 777
PLANTED_LENGTHS = {100: 0, 101: 63, 102: 64, 103: 65, 104: 255, 105: 256, 106: 257, 107: 650, 108: 0, 0: 0, NR - 1: 0}
SPECIALS = (0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -1.5e-310, 2.2e-308)


class CSR:
    def __init__(self, indptr, indices, data, shape):
        self.indptr = np.asarray(indptr, dtype=np.int64)
        self.indices = np.asarray(indices, dtype=np.int64)
        self.data = data
        self.shape = shape

    def rows(self, lo, hi):
        """rows [lo, hi) as (rowptr from 0, global columns, values)"""
        a, b = self.indptr[lo], self.indptr[hi]
        return self.indptr[lo:hi + 1] - a, self.indices[a:b], self.data[a:b]

    def with_values(self, data):
        return CSR(self.indptr, self.indices, data, self.shape)


@functools.lru_cache(maxsize=None)
def matrix(key: str) -> CSR:
    if key == "rand":
        return _rand()
    if key == "rand_finite":                 # the same structure without the planted non-finite values
        A = _rand()
        rng = np.random.default_rng(11)
        return A.with_values(rng.uniform(-1.0, 1.0, len(A.data)))
    if key == "p5":
        return _five_point(96, 96)
    if key.startswith("band"):
        return _band(BAND_ROWS if key == "band" else int(key[4:]))
    raise KeyError(key)


def _rand() -> CSR:
    rng = np.random.default_rng(20240917)
    lens = rng.integers(0, 701, NR)
    lens[rng.random(NR) < 0.03] = 0
    for r, n in PLANTED_LENGTHS.items():
        lens[r] = n
    pool = np.concatenate([np.arange(0, GAP_LO), np.arange(GAP_HI, NC)])
    cols = []
    for r in range(NR):
        if r == WHOLE_ROW:
            c = np.arange(BLOCK_A[0] + 3, BLOCK_A[1] - 2, 2)
        elif r == OTHER_ROW:
            c = np.arange(BLOCK_B[0], BLOCK_B[1], 3)
        else:
            c = np.sort(rng.choice(pool, int(lens[r]), replace=False))
        if r == NEGZERO_ROW and NEGZERO_COL not in c:
            c = np.sort(np.append(c, NEGZERO_COL))
        cols.append(c)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    indices = np.concatenate(cols)
    data = rng.uniform(-1.0, 1.0, len(indices))
    where = rng.choice(len(indices), 40 * len(SPECIALS), replace=False)
    for k, p in enumerate(where):
        data[p] = SPECIALS[k % len(SPECIALS)]
    a = indptr[NEGZERO_ROW]
    data[a + int(np.searchsorted(indices[a:indptr[NEGZERO_ROW + 1]], NEGZERO_COL))] = -0.0
    return CSR(indptr, indices, data, (NR, NC))


def _five_point(nx, ny) -> CSR:
    n = nx * ny
    idx = np.arange(n)
    i, j = idx % nx, idx // nx
    cand = np.stack([idx - nx, idx - 1, idx, idx + 1, idx + nx], axis=1)
    ok = np.stack([j > 0, i > 0, np.ones(n, bool), i < nx - 1, j < ny - 1], axis=1)
    vals = np.broadcast_to(np.array([-1.0, -1.0, 4.0, -1.0, -1.0]), (n, 5))
    indptr = np.concatenate([[0], np.cumsum(ok.sum(axis=1))])
    return CSR(indptr, cand[ok], np.ascontiguousarray(vals[ok]) + 0.001 * np.arange(ok.sum()), (n, n))


def _band(n) -> CSR:
    idx = np.arange(n)
    cand = np.stack([idx - 1, idx, idx + 1], axis=1)
    ok = (cand >= 0) & (cand < n)
    indptr = np.concatenate([[0], np.cumsum(ok.sum(axis=1))])
    return CSR(indptr, cand[ok], np.sin(np.arange(ok.sum()) + 1.0), (n, n))


# (name, matrix, r0, r1, c0, c1): half-open, 0-based
_ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)
CASES = (
    [(f"rand_rows{n}_fullcols", "rand", 95, 95 + n, 0, NC) for n in _ROW_COUNTS]
    + [
        ("rand_all", "rand", 0, NR, 0, NC),
        ("rand_gap_only", "rand", 90, 400, GAP_LO + 2, GAP_HI - 2),          # a window without a stored column: j0 == j1
        ("rand_block_a", "rand", 90, 400, BLOCK_A[0], BLOCK_A[1]),            # WHOLE_ROW whole, OTHER_ROW (and more) empty
        ("rand_width1", "rand", 0, NR, NEGZERO_COL, NEGZERO_COL + 1),
        ("rand_edge_on_and_between", "rand", 50, 1700, GAP_LO - 10, GAP_LO + 5),    # c0 on a stored column, c1 inside the gap
        ("rand_edge_between_and_on", "rand", 50, 1700, GAP_LO + 5, GAP_HI + 7),
        ("rand_long_rows", "rand", 100, 109, 17, 4890),
        ("rand_rows_empty_form", "rand", 500, 500, 10, 900),                  # both empty-range forms (uniform row partition)
        ("rand_cols_empty_form", "rand", 10, 900, 500, 500),
        ("p5_interior", "p5", 2304, 6912, 2304, 6912),
        ("p5_slab", "p5", 2304, 6912, 0, 9216),
        ("p5_odd", "p5", 97, 4100, 191, 4007),
        ("band_all", "band", 0, BAND_ROWS, 0, BAND_ROWS),                     # 70 001 selected rows: 69 scan chunks
        ("band_mid", "band", 1023, 66000, 1024, 65999),
        ("band_long_rows", BAND_LONG, 5, 5 + SCAN_TRIP + 13, 150_000, 263_000),     # 262 157 selected rows: 257 scan chunks
        ("band_long_cols", BAND_LONG, 259_000, BAND_LONG_ROWS, 7, 263_500),         # 263 493 columns: 258 scan chunks
    ]
)
COLUMN_CASES = (            # (name, matrix, k)
    ("rand_negzero", "rand", NEGZERO_COL), ("rand_gap_absent", "rand", GAP_LO + 3), ("rand_first", "rand", 0),
    ("rand_last", "rand", NC - 1), ("rand_stored", "rand", 1234), ("p5_first", "p5", 0), ("p5_last", "p5", 9215),
    ("band_mid", "band", 40000),
)


def uniform_partition(n, nranks):
    q, r = divmod(int(n), int(nranks))
    return np.concatenate([[0], np.cumsum([q + (1 if k < r else 0) for k in range(nranks)])]).astype(np.int64)


def reference_subpartition_1based(partition, first, last):
    """`_compute_subpartition(partition, first:last)` (src/indexing.jl:38-62), transcribed literally: 1-based boundaries,
    inclusive range."""
    nranks = len(partition) - 1
    new = [0] * (nranks + 1)
    new[0] = 1
    for r in range(1, nranks + 1):
        rank_start = partition[r - 1]
        rank_end = partition[r] - 1
        intersect_start = max(rank_start, first)
        intersect_end = min(rank_end, last)
        count = intersect_end - intersect_start + 1 if intersect_start <= intersect_end else 0
        new[r] = new[r - 1] + count
    return new


def reference_partitions(row_partition, r0, r1, c0, c1):
    """(row partition, column partition) of the reference's result, 0-based, the empty-range quirk included
    (src/indexing.jl:709-730)."""
    nranks = len(row_partition) - 1
    colp = uniform_partition(c1 - c0, nranks)
    if r0 == r1 or c0 == c1:
        return uniform_partition(r1 - r0, nranks), colp
    one_based = [int(p) + 1 for p in row_partition]
    return np.asarray(reference_subpartition_1based(one_based, r0 + 1, r1), dtype=np.int64) - 1, colp


def restate(A: CSR, lo, hi, c0, c1):
    """Rows [lo, hi) of A cut to the global column window [c0, c1): rowptr (int64, from 0), the kept entries' columns
    relative to c0 (``cols``), the compressed form (``col_indices`` ascending, ``colval``) and the values."""
    rp, cols, vals = A.rows(lo, hi)
    row_of = np.repeat(np.arange(hi - lo), np.diff(rp))
    keep = (cols >= c0) & (cols < c1)
    counts = np.bincount(row_of[keep], minlength=hi - lo)
    kept = cols[keep] - c0
    col_indices = np.unique(kept)
    return {"rowptr": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), "cols": kept,
            "col_indices": col_indices.astype(np.int64), "colval": np.searchsorted(col_indices, kept).astype(np.int64),
            "vals": vals[keep]}


def expected_on_rank(A: CSR, row_partition, rank, r0, r1, c0, c1):
    """What rank ``rank`` holds of ``A[r0:r1, c0:c1]`` when A's rows are split by ``row_partition``: the restatement of its
    rows of the range, plus the result's partitions."""
    rowp, colp = reference_partitions(row_partition, r0, r1, c0, c1)
    if r0 == r1 or c0 == c1:
        nloc = int(rowp[rank + 1] - rowp[rank])
        out = {"rowptr": np.zeros(nloc + 1, dtype=np.int64), "cols": np.empty(0, np.int64), "col_indices": np.empty(0, np.int64),
               "colval": np.empty(0, np.int64), "vals": A.data[:0]}
    else:
        lo, hi = max(int(row_partition[rank]), r0), min(int(row_partition[rank + 1]), r1)
        if lo >= hi:
            lo = hi = 0
        out = restate(A, lo, hi, c0, c1)
    out["row_partition"], out["col_partition"] = rowp, colp
    return out


def column_of(A: CSR, lo, hi, k):
    """Rows [lo, hi) of column k: the stored value, +0.0 where none is stored."""
    rp, cols, vals = A.rows(lo, hi)
    out = np.zeros(hi - lo, dtype=A.data.dtype)
    row_of = np.repeat(np.arange(hi - lo), np.diff(rp))
    hit = cols == k
    out[row_of[hit]] = vals[hit]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def uneven_partition(n, nranks, empty_rank):
    """rows split unevenly over the ranks, ``empty_rank`` holding none"""
    live = [r for r in range(nranks) if r != empty_rank]
    w = np.array([3 + 2 * k for k in range(len(live))], dtype=np.float64)
    cuts = np.floor(np.cumsum(w) / w.sum() * n).astype(np.int64)
    cuts[-1] = n
    sizes = np.zeros(nranks, dtype=np.int64)
    sizes[live] = np.diff(np.concatenate([[0], cuts]))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
