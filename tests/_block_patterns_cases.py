"""Matrices for tests/test_gpu_block_patterns.py in plain numpy (0-based CSR: rowptr int64, ascending columns, values) and a
numpy MODEL of the pattern rule of csrc/patterns.hip, written independently of the device code: a 256-row block's pattern
is (first entry mod 8, number of rows, row bounds relative to the first entry, columns relative to the first row); the most
frequent patterns are kept up to 256 KiB of table (ties: first occurrence; a pattern that no longer fits is passed over);
the pattern form is used when at least half of the candidate blocks are in the table.  Checked on the CPU by
tests/test_block_patterns_cases.py, so that a failure on the GPU is the kernel's and not the test's."""
import numpy as np

from _narrow_cols_cases import RPB, _csr

HEAD = 272                     # 16-bit entries in front of a pattern's columns (csrc/patterns.h PAT_HEAD)
CAP_BYTES = 256 * 1024
MAX_LEN = 65535


def pattern_keys_np(rowptr, col, blocks=None):
    """{block: key} with key = (phase, nr, relative bounds, relative columns) as a hashable tuple; a block of more than
    65535 entries has key None (no candidate for the table)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    if blocks is None:
        blocks = range((n + RPB - 1) // RPB)
    keys = {}
    for b in blocks:
        r0 = RPB * int(b)
        r1 = min(r0 + RPB, n)
        p0, p1 = int(rowptr[r0]), int(rowptr[r1])
        if p1 - p0 > MAX_LEN:
            keys[int(b)] = None
            continue
        keys[int(b)] = (p0 % 8, r1 - r0, (rowptr[r0:r1 + 1] - p0).tobytes(), (col[p0:p1] - r0).tobytes())
    return keys


def pattern_entries(key) -> int:
    """16-bit entries of one pattern in the table: head + its columns behind `phase` leading slots, a whole number of 8."""
    phase, _nr, _bounds, cols = key
    return HEAD + ((phase + len(cols) // 8 + 7) // 8) * 8          # (cols: int64 bytes, 8 per entry)


def model_table(rowptr, col, blocks=None):
    """What hpcla_block_patterns_info must report: dict(patterns, table_bytes, candidates, patterned), or None when fewer than
    half of the candidates end up in the table (no handle)."""
    keys = pattern_keys_np(rowptr, col, blocks)
    count, first = {}, {}
    for b in sorted(keys):
        k = keys[b]
        if k is None:
            continue
        count[k] = count.get(k, 0) + 1
        first.setdefault(k, b)
    used, kept = 0, {}
    for k in sorted(count, key=lambda k: (-count[k], first[k])):
        need = pattern_entries(k)
        if (used + need) * 2 > CAP_BYTES:
            continue
        kept[k] = used
        used += need
    patterned = sum(count[k] for k in kept)
    if not kept or 2 * patterned < len(keys):
        return None
    return {"patterns": len(kept), "table_bytes": 2 * used, "candidates": len(keys), "patterned": patterned}


def band_with_random_half(seed=21):
    """32 768 rows = 128 blocks: the first half is a 5-point stencil of width 512 cut off at the half (a structured part whose
    blocks repeat), the second half a random band (1 ... 9 columns within +-300 of the row: no two blocks alike)."""
    n, nx = 32768, 512
    half = n // 2
    rng = np.random.default_rng(seed)
    rc = {}
    for i in range(half):
        x = i % nx
        rc[i] = [c for c, ok in ((i - nx, i >= nx), (i - 1, x > 0), (i, True), (i + 1, x < nx - 1), (i + nx, i + nx < half)) if ok]
    for i in range(half, n):
        k = int(rng.integers(1, 10))
        lo, hi = max(half, i - 300), min(n, i + 301)
        rc[i] = rng.choice(np.arange(lo, hi), size=k, replace=False).tolist()
    return _csr(n, rc, seed)


def _tridiag(n):
    return {i: [c for c in (i - 1, i, i + 1) if 0 <= c < n] for i in range(n)}


def one_column_off():
    """40 blocks of a tridiagonal band: blocks 1 ... 38 share one pattern.  In block 20 ONE column is moved by 1 (row r holds
    r - 1, r, r + 2 instead of r - 1, r, r + 1): the same row lengths, the same phase, another pattern.  Returns (csr, block)."""
    n = 40 * RPB
    rc = _tridiag(n)
    r = 20 * RPB + 100
    rc[r] = [r - 1, r, r + 2]
    return _csr(n, rc, 22), 20


def more_patterns_than_the_cap():
    """420 blocks of a pentadiagonal band (5 entries per row, about 3.1 KB per pattern: 84 patterns fill the table): 240 share
    one pattern, every third block from block 30 on gets a column moved by an amount of its own -- 130 patterns that occur once."""
    n = 420 * RPB
    rc = {i: [c for c in (i - 40, i - 1, i, i + 1, i + 40) if 0 <= c < n] for i in range(n)}
    odd = list(range(30, 420, 3))
    for k, b in enumerate(odd):
        r = b * RPB + 50 + (k % 100)
        rc[r] = [r - 40, r - 1, r, r + 1, r + 41 + k]
    return _csr(n, rc, 23), odd


def unstructured(seed=24):
    """300 blocks of random rows (0 ... 10 columns within +-2000): every block is a pattern of its own and the table holds
    only a fraction of them, so the library must create nothing."""
    n = 300 * RPB
    rng = np.random.default_rng(seed)
    rc = {}
    for i in range(n):
        k = int(rng.integers(0, 11))
        if k:
            lo, hi = max(0, i - 2000), min(n, i + 2001)
            rc[i] = rng.choice(np.arange(lo, hi), size=k, replace=False).tolist()
    return _csr(n, rc, seed)
