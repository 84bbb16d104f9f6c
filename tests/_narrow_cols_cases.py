"""Matrices for tests/test_gpu_narrow_cols.py, in plain numpy (0-based CSR: rowptr int64, ascending columns, values), and the
eligibility rule of the 16-bit column copy written independently of the device encoder.  Checked on the CPU by
tests/test_narrow_cols_cases.py, so that a failure on the GPU is the kernel's and not the test's."""
import numpy as np

RPB = 256                      # rows per block of the SpMV kernels (hpcla_spmv_rows_per_block)
LO, HI = -32768, 32767         # the int16 window around a block's first row
PASS = 464                     # entries a wave stages per pass (csrc/spmv.hip RG_CHW)


def eligible_np(rowptr, col, n_own, blocks=None) -> bool:
    """True when every listed row block (default: all) has only owned columns within [r0 + LO, r0 + HI] of its first row."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    if blocks is None:
        blocks = range((n + RPB - 1) // RPB)
    for b in blocks:
        r0 = RPB * int(b)
        seg = col[rowptr[r0]:rowptr[min(r0 + RPB, n)]]
        if len(seg) and (seg.max() >= n_own or seg.min() < 0 or (seg - r0).min() < LO or (seg - r0).max() > HI):
            return False
    return True


def _csr(n, row_cols, seed):
    """CSR from {row: iterable of columns}; rows not named are empty.  Values: seeded, in [-1, 1) \\ {0}."""
    rng = np.random.default_rng(seed)
    counts = np.zeros(n, dtype=np.int64)
    for r, cs in row_cols.items():
        counts[r] = len(cs)
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    col = np.empty(int(rowptr[-1]), dtype=np.int64)
    for r, cs in row_cols.items():
        cs = np.sort(np.asarray(cs, dtype=np.int64))
        assert len(np.unique(cs)) == len(cs) and cs.min() >= 0 and cs.max() < n
        col[rowptr[r]:rowptr[r + 1]] = cs
    vals = rng.uniform(-1.0, 1.0, size=len(col))
    vals[vals == 0.0] = 0.5
    return rowptr, col, vals


def banded_edges(which: str):
    """Tridiagonal band of 70 000 rows; block 128 (r0 = 32768) also holds column r0 - 32768 = 0 and column r0 + 32767 = 65535,
    exactly on the window's edges.  'past_low' adds r0' - 32769 to a row of block 129, 'past_high' r0' + 32768."""
    n = 70_000
    rc = {i: [c for c in (i - 1, i, i + 1) if 0 <= c < n] for i in range(n)}
    r0 = 128 * RPB
    assert r0 + LO == 0
    rc[r0 + 3] = rc[r0 + 3] + [r0 + LO]
    rc[r0 + 200] = rc[r0 + 200] + [r0 + HI]
    rc[r0 + 77] = rc[r0 + 77] + [r0 + LO, r0 + HI]           # both edges in one row
    r1 = 129 * RPB
    if which == "past_low":
        rc[r1 + 5] = rc[r1 + 5] + [r1 + LO - 1]
    elif which == "past_high":
        rc[r1 + 5] = rc[r1 + 5] + [r1 + HI + 1]
    else:
        assert which == "edges"
    return _csr(n, rc, 11)


def long_and_empty_rows():
    """3000 rows: most empty (whole waves and blocks of empty rows among them), rows of 465, 928, 1500 and 3000 entries (more
    than one pass, a whole number of passes, several passes), a row of exactly one pass, and short rows next to the long
    ones so that a pass holds the tail of a long row together with other rows."""
    n = 3000
    rc = {}

    def band(r, k, start=None):
        s = max(0, min(n - k, (r - k // 2) if start is None else start))
        rc[r] = list(range(s, s + k))
    band(5, 465)
    band(6, 3)
    band(70, 2 * PASS)
    band(71, PASS)
    band(300, 1500)
    band(301, 1)
    band(511, 7)
    band(1024, 3000, 0)            # first row of a block, first lane of a wave
    band(1087, 700)                # last lane of that wave
    band(1088, 2)
    band(2999, 900)                # the last row of the matrix
    for r in range(1500, 1600):
        band(r, 5)
    return _csr(n, rc, 12)


def tail_case(short: int):
    """Pentadiagonal band of 1000 rows whose nnz is `short` entries short of a multiple of 8 (entries of the last rows are dropped
    to get there), so the launch's last pass ends exactly at nnz, `short` short of a vector boundary."""
    n = 1000
    rc = {i: [c for c in (i - 40, i - 1, i, i + 1, i + 40) if 0 <= c < n] for i in range(n)}
    nnz = sum(len(v) for v in rc.values())
    drop = (nnz + short) % 8
    r = n - 1
    while drop:
        if len(rc[r]) > 1:
            rc[r] = rc[r][1:]
            drop -= 1
        else:
            r -= 1
    out = _csr(n, rc, 13 + short)
    assert (8 - len(out[1]) % 8) % 8 == short
    return out
