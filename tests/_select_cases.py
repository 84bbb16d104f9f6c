"""Cases and the numpy restatement of index-set selection (``hp.select``, ``hp.take``, ``hp.put_``; the index-vector half of
src/indexing.jl, from line 1318 on), shared by tests/test_select_cases.py (CPU: the restatement against scipy),
tests/test_gpu_select.py (one rank) and tests/_multirank_select_worker.py (several).

The restatement is loops: a table from old to new column, then for every selected row the kept entries as (new column,
source position) pairs, sorted; the distinct new columns ascending are col_indices, colval the place of each in that list.
Entries are only moved, so every comparison is of bits.

Matrices (global CSR, columns ascending within a row, built once per process):
  edge    26 rows x 2 600 columns.  SUBSET is a fixed set of 2 300 columns.  For every length L of EDGE_LENGTHS -- 0, 1 and
          cap - 1, cap, cap + 1 for the two caps of the fill (SHORT_CAP = 32 kept entries: lane groups; TILE = 1 024: the row
          in LDS), and 2 * TILE + 3 (the tiled form with a partial last tile) -- one row stores L columns of SUBSET and 7
          outside it (kept length L under a subset map, L + 7 under a full one), and one row stores L columns in all, 3 of
          them (fewer when L < 3) outside SUBSET (kept length L under a full map).  L = 0 gives a row all of whose entries a
          subset map drops, and a row without entries.  Eight more rows have random lengths.  Values carry +0.0, -0.0, +-Inf
          and NaNs with distinct payloads, planted in the first rows' kept entries.
  band    2 * SCAN_CHUNK + 7 rows, 3 entries per row: selecting 2 * SCAN_CHUNK + 1 rows and 2 * SCAN_CHUNK + 1 columns makes
          both scans (csrc/scan.h, SCAN_CHUNK = 1 024 elements per workgroup) cross two chunk boundaries.
  grid33x31, grid24x24   5-point matrices with integer entries (4 and -1): every sum of a product with an integer vector is
          exact, so a permuted product must reproduce the unpermuted one bit for bit.
"""
import functools

import numpy as np

from tests._submatrix_cases import CSR, bits, uneven_partition, uniform_partition  # noqa: F401  (shared helpers)

SHORT_CAP = 32
TILE = 1024
SCAN_CHUNK = 1024
EDGE_LENGTHS = (0, 1, SHORT_CAP - 1, SHORT_CAP, SHORT_CAP + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
EDGE_NC = 2600
EDGE_OUTSIDE = 7
BAND_ROWS = 2 * SCAN_CHUNK + 7
BAND_SELECTED = 2 * SCAN_CHUNK + 1

SPECIAL_BITS = (0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001,
                0x7FF8000000000ABC, 0xFFF8000000000123, 0x7FF80000DEADBEEF, 0x0000000000000001, 0x800000000000F00D)


@functools.lru_cache(maxsize=None)
def subset() -> np.ndarray:
    """SUBSET, ascending"""
    rng = np.random.default_rng(77)
    return np.sort(rng.choice(EDGE_NC, 2300, replace=False)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def matrix(key: str) -> CSR:
    if key == "edge":
        return _edge()
    if key == "edge_finite":                 # the same structure, finite values
        A = _edge()
        return A.with_values(np.random.default_rng(3).uniform(-1.0, 1.0, len(A.data)))
    if key == "band":
        return _band(BAND_ROWS)
    if key.startswith("grid"):
        nx, ny = (int(t) for t in key[4:].split("x"))
        return _grid(nx, ny)
    raise KeyError(key)


def _edge() -> CSR:
    rng = np.random.default_rng(20241021)
    inside = subset()
    outside = np.setdiff1d(np.arange(EDGE_NC), inside)
    cols = []
    for L in EDGE_LENGTHS:                                       # row 2k: L inside + 7 outside; row 2k + 1: L in all
        cols.append(np.sort(np.concatenate([rng.choice(inside, L, replace=False), rng.choice(outside, EDGE_OUTSIDE, replace=False)])))
        d = min(L, 3)
        cols.append(np.sort(np.concatenate([rng.choice(inside, L - d, replace=False), rng.choice(outside, d, replace=False)])))
    for _ in range(8):
        cols.append(np.sort(rng.choice(EDGE_NC, int(rng.integers(0, 90)), replace=False)))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    indices = np.concatenate(cols).astype(np.int64)
    data = rng.uniform(-1.0, 1.0, len(indices))
    raw = data.view(np.uint64)
    k = 0
    for r in (2, 4, 6, 8, 10, 12, 18, 19, 20):                  # specials in kept entries of rows of every form
        a, b = indptr[r], indptr[r + 1]
        kept = a + np.flatnonzero(np.isin(indices[a:b], inside))
        for p in kept[:: max(1, len(kept) // 5)][:5]:
            raw[p] = SPECIAL_BITS[k % len(SPECIAL_BITS)]
            k += 1
    return CSR(indptr, indices, data, (len(cols), EDGE_NC))


def _band(n) -> CSR:
    idx = np.arange(n)
    cand = np.stack([idx - 1, idx, idx + 1], axis=1)
    ok = (cand >= 0) & (cand < n)
    indptr = np.concatenate([[0], np.cumsum(ok.sum(axis=1))])
    return CSR(indptr, cand[ok], np.cos(np.arange(ok.sum()) + 2.0), (n, n))


def _grid(nx, ny) -> CSR:
    n = nx * ny
    idx = np.arange(n)
    i, j = idx % nx, idx // nx
    cand = np.stack([idx - nx, idx - 1, idx, idx + 1, idx + nx], axis=1)
    ok = np.stack([j > 0, i > 0, np.ones(n, bool), i < nx - 1, j < ny - 1], axis=1)
    vals = np.broadcast_to(np.array([-1.0, -1.0, 4.0, -1.0, -1.0]), (n, 5))
    indptr = np.concatenate([[0], np.cumsum(ok.sum(axis=1))])
    return CSR(indptr, cand[ok], np.ascontiguousarray(vals[ok]), (n, n))


def _perm(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def index_list(key: str, spec: str):
    """The index lists of the cases by name (None: the ``None`` argument)."""
    A = matrix(key)
    m, n = A.shape
    if spec == "none":
        return None
    if spec == "rows_perm":
        return _perm(m, 1)
    if spec == "rows_subset":
        return np.sort(_perm(m, 2)[: (2 * m) // 3])
    if spec == "rows_repeats":
        p = _perm(m, 4)
        return np.concatenate([p[:9], p[:9][::-1], [p[0], p[0]], p[9:15]]).astype(np.int64)
    if spec == "rows_empty" or spec == "cols_empty":
        return np.empty(0, dtype=np.int64)
    if spec == "rows_chunks":
        return _perm(m, 5)[:BAND_SELECTED]
    if spec == "cols_identity":
        return np.arange(n, dtype=np.int64)
    if spec == "cols_reversal":
        return np.arange(n, dtype=np.int64)[::-1].copy()
    if spec == "cols_perm":
        return _perm(n, 6)
    if spec == "cols_sorted_subset":
        return subset() if key.startswith("edge") else np.sort(_perm(n, 7)[: (3 * n) // 4])
    if spec == "cols_unsorted_subset":
        s = index_list(key, "cols_sorted_subset")
        return s[_perm(len(s), 8)]
    if spec == "cols_chunks":
        return _perm(n, 9)[:BAND_SELECTED]
    raise KeyError(spec)


# (name, matrix, rows spec, cols spec)
CASES = (
    [(f"edge_rows_perm_{c}", "edge", "rows_perm", c) for c in
     ("cols_identity", "cols_reversal", "cols_perm", "cols_sorted_subset", "cols_unsorted_subset", "none", "cols_empty")]
    + [(f"edge_{r}_cols_unsorted_subset", "edge", r, "cols_unsorted_subset") for r in
       ("rows_subset", "rows_repeats", "none", "rows_empty")]
    + [
        ("edge_none_none", "edge", "none", "none"),
        ("edge_repeats_perm", "edge", "rows_repeats", "cols_perm"),
        ("band_chunks", "band", "rows_chunks", "cols_chunks"),
        ("band_rows_chunks_all_cols", "band", "rows_chunks", "none"),
        ("band_all_rows_reversal", "band", "none", "cols_reversal"),
    ]
)
IDS = [c[0] for c in CASES]


def case_lists(case):
    _, key, rspec, cspec = case
    return index_list(key, rspec), index_list(key, cspec)


def restate(A: CSR, lo, hi, rows, cols):
    """``select`` on the rank that holds rows [lo, hi) of A.  ``rows``: its list of global rows (None: lo .. hi - 1);
    ``cols``: the GLOBAL column list, all ranks' lists concatenated (None: all columns in order).  Returns rowptr (int64,
    from 0), the new global column of every output entry (``cols``), the compressed form (``col_indices`` ascending,
    ``colval``), the values and ``src``, the position of every output entry in the rank's value array."""
    n = A.shape[1]
    if cols is None:
        newcol = np.arange(n, dtype=np.int64)
    else:
        newcol = np.full(n, -1, dtype=np.int64)
        for k, c in enumerate(cols):
            assert newcol[c] == -1, "a duplicated column"
            newcol[c] = k
    rows = range(lo, hi) if rows is None else rows
    first = int(A.indptr[lo]) if lo < A.shape[0] else int(A.indptr[-1])
    rowptr, out_cols, src = [0], [], []
    for r in rows:
        assert lo <= r < hi
        kept = []
        for p in range(int(A.indptr[r]), int(A.indptr[r + 1])):
            c = int(newcol[A.indices[p]])
            if c >= 0:
                kept.append((c, p))
        kept.sort()
        out_cols.extend(c for c, _ in kept)
        src.extend(p for _, p in kept)
        rowptr.append(len(out_cols))
    out_cols = np.asarray(out_cols, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    col_indices = np.asarray(sorted(set(out_cols.tolist())), dtype=np.int64)
    place = {int(c): k for k, c in enumerate(col_indices)}
    colval = np.asarray([place[int(c)] for c in out_cols], dtype=np.int64)
    return {"rowptr": np.asarray(rowptr, dtype=np.int64), "cols": out_cols, "col_indices": col_indices, "colval": colval,
            "vals": A.data[src], "src": src - first}


def expected_on_rank(A: CSR, row_partition, rank, rows_by_rank, cols_by_rank, col_partition=None):
    """What rank ``rank`` holds of ``select(A, rows, cols)`` when A's rows are split by ``row_partition`` and rank r passes
    ``rows_by_rank[r]`` and ``cols_by_rank[r]`` (either list of lists may be None: the ``None`` argument), plus the result's
    partitions: the cumulative sums of the ranks' counts; ``A``'s column partition for ``cols=None``."""
    nranks = len(row_partition) - 1
    lo, hi = int(row_partition[rank]), int(row_partition[rank + 1])
    cols = None if cols_by_rank is None else np.concatenate([np.asarray(c, dtype=np.int64) for c in cols_by_rank])
    out = restate(A, lo, hi, None if rows_by_rank is None else rows_by_rank[rank], cols)
    nrows = [int(row_partition[r + 1] - row_partition[r]) if rows_by_rank is None else len(rows_by_rank[r]) for r in range(nranks)]
    out["row_partition"] = np.concatenate([[0], np.cumsum(nrows)]).astype(np.int64)
    if cols_by_rank is None:
        out["col_partition"] = uniform_partition(A.shape[1], nranks) if col_partition is None else np.asarray(col_partition)
    else:
        out["col_partition"] = np.concatenate([[0], np.cumsum([len(c) for c in cols_by_rank])]).astype(np.int64)
    return out


def take_of(vg, idx):
    """``v[idx]`` for the global values ``vg``"""
    out = np.empty(len(idx), dtype=vg.dtype)
    for k, i in enumerate(idx):
        out[k] = vg[i]
    return out


def put_into(vg, idx, src):
    """``v[idx] = src`` on a copy of the global values ``vg``; ``idx`` distinct"""
    out = vg.copy()
    assert len(set(int(i) for i in idx)) == len(idx)
    for k, i in enumerate(idx):
        out[i] = src[k]
    return out
