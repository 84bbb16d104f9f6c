"""Matrices for tests/test_gpu_packed_edges.py and tests/_multirank_packed_worker.py, in plain numpy (0-based CSR: rowptr int64,
ascending columns, values from a small palette), and ``packed_walk``: a numpy restatement of what csrc/packed.hip does with
them -- encode 16-bit block-relative columns and 8-bit value codes, then walk every 256-row block in passes of 2048 entries
counted from the octet-aligned start, carrying each row's running sum across the passes.  Checked on the CPU by
tests/test_packed_cases.py: the generators have the properties their names claim and the walk gives the oracle's bits, so a
failure on the GPU is the kernel's and not the test's.

``packed_walk(..., slip=NAME)`` makes one plausible mistake of the kernel on purpose (``SLIPS`` names the line each mirrors);
the CPU test shows that every one of them changes the bits of at least one case here."""
import numpy as np

from _narrow_cols_cases import banded_edges, eligible_np  # noqa: F401  (eligible_np: the window rule, used by both test files)

RPB = 256                      # rows per block                         (csrc/packed.hip: constexpr int P_RPB = 256)
OCTET = 8                      # entries a lane loads per pass          (P_CHUNK = P_RPB * 8; pa = p0 & ~7)
CHUNK = RPB * OCTET            # entries of a block per pass: 2048      (constexpr int P_CHUNK)
LO, HI = -32768, 32767         # the int16 window around a block's first row (const short *dcol)
SEED_SAMPLE = 1 << 16          # leading values that seed the dictionary (ns = std::min<int64_t>(nnz, 1 << 16))
MISS_CAP = 4096                # bounded list of values the encoder missed (const int CAP = 4096)
MAX_DICT = 256                 # dictionary entries an 8-bit code can name (dict.size() > 256 is refused)

# slip -> the kernel line it mirrors (csrc/packed.hip, spmv_packed_kernel)
SLIPS = {
    "no_carry": "double acc = 0.0;  declared inside the pass loop instead of in front of it",
    "p0_origin": "const int64_t g = pa + c + e0;  with p0 in place of pa (lo / hi stay relative to pa)",
    "lane0_from_pa": "lo = rowptr[r0 + tid] - base - pa;  taken as 0 for the block's first row (the shared octet is summed)",
    "grid_index": "blk = block_list ? block_list[blockIdx.x] : blockIdx.x;  without the list",
    "code7": "s_dict[(cd >> (8 * k)) & 0xff]  with a mask of 0x7f",
    "unsigned_delta": "int64_t idx = r0 + (int)dc[k];  with dc read as unsigned short",
}


def n_blocks(n):
    return (n + RPB - 1) // RPB


def block_span(rowptr, b):
    """(p0, p1, pa, total) of row block b as the kernel computes them."""
    n = len(rowptr) - 1
    r0 = RPB * b
    p0, p1 = int(rowptr[r0]), int(rowptr[min(r0 + RPB, n)])
    pa = p0 & ~(OCTET - 1)
    return p0, p1, pa, p1 - pa


def n_passes(rowptr, b):
    return -(-block_span(rowptr, b)[3] // CHUNK)


def bit_patterns(vals):
    return np.unique(np.ascontiguousarray(vals, dtype=np.float64).view(np.int64))


# ---- the walk ----------------------------------------------------------------------------------------------------------------
def encode(rowptr, col, vals, blocks=None):
    """(dcol int16, code uint8, dict float64) as hpcla_packed_create_i32 leaves them: both arrays zero-padded to the next
    multiple of 8 plus one octet; dcol written for the listed blocks only (the rest stays 0), code for every entry; the
    dictionary sorted ascending.  Asserts what create checks: the window of the listed blocks and at most 256 values."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n, nnz = len(rowptr) - 1, len(col)
    padded = (nnz + 7) // 8 * 8 + 8
    dcol = np.zeros(padded, dtype=np.int16)
    for b in (range(n_blocks(n)) if blocks is None else blocks):
        p0, p1, _, _ = block_span(rowptr, int(b))
        d = col[p0:p1] - RPB * int(b)
        assert len(d) == 0 or (d.min() >= LO and d.max() <= HI), "outside the 16-bit window"
        dcol[p0:p1] = d
    dic = np.unique(vals)                                   # sorted; the palettes hold no NaN and one kind of zero
    assert len(dic) == len(bit_patterns(vals)) <= MAX_DICT
    code = np.zeros(padded, dtype=np.uint8)
    code[:nnz] = np.searchsorted(dic, vals)
    assert np.array_equal(dic[code[:nnz]].view(np.int64), np.asarray(vals).view(np.int64))
    return dcol, code, dic


def packed_walk(rowptr, col, vals, x, n_own=None, blocks=None, sentinel=np.nan, slip=None):
    """y of the packed kernel over the listed blocks (default: all); rows of other blocks hold ``sentinel``."""
    assert slip is None or slip in SLIPS
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    n_own = len(x) if n_own is None else n_own
    dcol, code, dic = encode(rowptr, col, vals, blocks)
    delta = dcol.astype(np.uint16).astype(np.int64) if slip == "unsigned_delta" else dcol.astype(np.int64)
    mask = 0x7f if slip == "code7" else 0xff
    y = np.full(n, sentinel, dtype=np.float64)
    launch = list(range(n_blocks(n))) if blocks is None else [int(b) for b in blocks]
    for pos, blk in enumerate(launch):
        if slip == "grid_index":
            blk = pos
        r0 = RPB * blk
        nr = min(RPB, n - r0)
        p0, p1, pa, total = block_span(rowptr, blk)
        lo = (rowptr[r0:r0 + nr] - pa).tolist()
        hi = (rowptr[r0 + 1:r0 + nr + 1] - pa).tolist()
        if slip == "lane0_from_pa":
            lo[0] = 0
        acc = [0.0] * nr
        origin = p0 if slip == "p0_origin" else pa
        for c in range(0, total, CHUNK):
            m = min(total - c, CHUNK)
            g0 = origin + c
            g1 = min(g0 + (m + OCTET - 1) // OCTET * OCTET, len(dcol))     # whole octets: lanes with e0 < m
            idx = np.clip(r0 + delta[g0:g1], 0, n_own - 1)                 # idx < 0 ? 0 : (idx >= n_own ? n_own - 1 : idx)
            prod = (dic[np.minimum(code[g0:g1] & mask, len(dic) - 1)] * x[idx]).tolist()
            if slip == "no_carry":
                acc = [0.0] * nr
            for t in range(nr):
                a, e = max(lo[t], c), min(hi[t], c + m)
                s = acc[t]
                for j in range(a, e):
                    s += prod[j - c] if j - c < len(prod) else 0.0
                acc[t] = s
        y[r0:r0 + nr] = acc
    return y


# ---- builders ----------------------------------------------------------------------------------------------------------------
def _pick(palette, count, rng):
    return np.asarray(palette, dtype=np.float64)[rng.integers(len(palette), size=count)]


def _from_rows(row_cols, n):
    """CSR from a list of per-row column arrays (sorted here)."""
    counts = np.array([len(c) for c in row_cols], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    col = np.concatenate([np.sort(np.asarray(c, dtype=np.int64)) for c in row_cols]) if len(row_cols) else np.empty(0, np.int64)
    assert len(rowptr) == n + 1
    return rowptr, col


PAL9 = (10.0 / 3.0, -2.0 / 3.0, -1.0 / 6.0)                       # centre, edge, corner
PAL27 = (88.0 / 26.0, -6.0 / 26.0, -3.0 / 26.0, -2.0 / 26.0)      # centre, face, edge, corner


def stencil9(nx, ny, row_start=0, row_end=None):
    """9-point stencil on a PERIODIC nx x ny grid (rows [row_start, row_end), global columns): every row stores exactly 9
    entries, so every full row block holds 2304 -- two passes.  Values by kind of neighbour (3)."""
    return _stencil((nx, ny), PAL9, row_start, row_end)


def stencil27(nx, ny, nz, row_start=0, row_end=None):
    """27-point stencil on a periodic nx x ny x nz grid: 27 entries per row, 6912 per full row block -- four passes.  Values
    by kind of neighbour (4)."""
    return _stencil((nx, ny, nz), PAL27, row_start, row_end)


def _stencil(dims, palette, row_start, row_end):
    assert all(d >= 3 for d in dims)                      # the wrapped neighbours of a point are all different points
    n = int(np.prod(dims))
    row_end = n if row_end is None else row_end
    i = np.arange(row_start, row_end, dtype=np.int64)
    coords, rest = [], i
    for d in dims:                                        # x fastest
        coords.append(rest % d)
        rest = rest // d
    offs = np.array(np.meshgrid(*[[-1, 0, 1]] * len(dims), indexing="ij")).reshape(len(dims), -1).T
    cols = np.zeros((len(i), len(offs)), dtype=np.int64)
    kind = np.abs(offs).sum(axis=1)
    stride = 1
    for k, d in enumerate(dims):
        cols += ((coords[k][:, None] + offs[None, :, k]) % d) * stride
        stride *= d
    vals = np.broadcast_to(np.asarray(palette)[kind][None, :], cols.shape)
    order = np.argsort(cols, axis=1, kind="stable")
    cols, vals = np.take_along_axis(cols, order, 1), np.take_along_axis(vals, order, 1)
    assert np.all(np.diff(cols, axis=1) > 0)
    rowptr = np.arange(len(i) + 1, dtype=np.int64) * len(offs)
    return rowptr, cols.reshape(-1).copy(), vals.reshape(-1).copy()


PAL_EDGES = (1.0 / 3.0, -0.7, 1.1, 2.0 / 7.0, -1.3, 0.9, 5.0 / 11.0)
PASS_TOTALS = (2047, 2048, 2049, 4096, 4097)
PASS_OFFSETS = (0, 3, 7)
LONG = 5000                    # entries of the rows that are longer than a whole pass


def _bounds(rng, m, total, must=(), avoid=()):
    """257 ascending row boundaries from m to total (relative to the octet-aligned start): every value of `must` is one (twice
    in `must`: an empty row there), none of `avoid` is."""
    allowed = np.setdiff1d(np.arange(m, total + 1), np.asarray(avoid, dtype=np.int64))
    inner = np.sort(rng.choice(allowed, size=RPB - 1, replace=True))
    taken = set()
    for v in must:
        k = min((k for k in range(RPB - 1) if k not in taken), key=lambda k: abs(int(inner[k]) - v))
        inner[k] = v
        taken.add(k)
    return np.concatenate([[m], np.sort(inner), [total]]).astype(np.int64)


def pass_edges():
    """Returns (rowptr, col, vals, info).  Row blocks whose entry counts FROM THE OCTET-ALIGNED START are exactly 2047, 2048,
    2049, 4096 and 4097, each at p0 % 8 = 0, 3 and 7 (a short filler block in front shifts p0 where needed), with rows that
    end on, begin on, sit empty on and straddle by one entry a pass boundary; two blocks whose first / last lane holds a row of
    5000 entries; a block of empty rows between two full ones; a ragged last block of 100 rows (its last two waves have no
    row) that still takes two passes.  ``info`` maps a name to the block (or (block, row)) that carries the property."""
    rng = np.random.default_rng(20260)
    lengths, info = [], {}

    def p_now():
        return int(sum(int(np.sum(L)) for L in lengths))

    def add(L):
        assert len(L) <= RPB
        lengths.append(np.asarray(L, dtype=np.int64))
        return len(lengths) - 1

    def shift_to(m):
        """a filler block (mostly empty rows) after which p0 % 8 == m"""
        if p_now() % OCTET == m:
            return
        cnt = (m - p_now()) % OCTET + OCTET * int(rng.integers(20, 60))
        L = np.zeros(RPB, dtype=np.int64)
        np.add.at(L, rng.integers(0, RPB, size=cnt), 1)
        add(L)
        assert p_now() % OCTET == m

    for m in PASS_OFFSETS:
        for total in PASS_TOTALS:
            shift_to(m)
            must, avoid = [], []
            if total >= 4096:
                must += [CHUNK, CHUNK, CHUNK]            # a row ends on the boundary, an empty row sits on it, a row begins there
                must += [2 * CHUNK - 1, 2 * CHUNK + 1] if total == 4097 else []
                avoid += [2 * CHUNK] if total == 4097 else []
            elif total == 2049:
                must, avoid = [CHUNK - 1], [CHUNK]       # the last row holds one entry on each side
            bnd = _bounds(rng, m, total, must, avoid)
            info[(total, m)] = add(np.diff(bnd))
    # a row longer than a whole pass in the first lane, then one in the last lane
    shift_to(3)
    L = np.diff(_bounds(rng, 0, 900))
    L[0] = LONG
    info["long_first"] = add(L)
    shift_to(7)
    L = np.diff(_bounds(rng, 0, 1000))                  # the long row begins before 1007 + 7: it ends inside pass 2
    L[RPB - 1] = LONG
    info["long_last"] = add(L)
    # full, empty, full
    full = rng.integers(7, 12, size=RPB)
    info["empty_between"] = add(full) + 1
    add(np.zeros(RPB, dtype=np.int64))
    add(rng.integers(7, 12, size=RPB))
    # ragged last block, two passes
    shift_to(3)
    info["ragged"] = add(rng.integers(20, 31, size=100))

    ln = np.concatenate(lengths)
    n = len(ln)
    assert n > LONG + 64
    row_cols = []
    for r, k in enumerate(ln.tolist()):
        if k == 0:
            row_cols.append(np.empty(0, dtype=np.int64))
            continue
        width = 2 * k + 16                               # k distinct columns out of a window of 2k + 16 around the diagonal
        w1 = min(n, max(0, r - k - 8) + width)
        w0 = max(0, w1 - width)
        row_cols.append(rng.choice(np.arange(w0, w1), size=k, replace=False))
    rowptr, col = _from_rows(row_cols, n)
    return rowptr, col, _pick(PAL_EDGES, len(col), rng), info


PAL_WINDOW = (0.3, -1.7, 2.0 / 3.0, 1.9, -0.45)


def window_edges(which):
    """Returns (rowptr, col, vals, n_own, bad_block).  The structure of _narrow_cols_cases.banded_edges (block 128 holds
    columns exactly at r0 - 32768 and r0 + 32767, both in one row too; 'past_low' / 'past_high' put a column one beyond into
    block 129) with values from a palette of 5.  'ghost' is 'edges' with one more entry in the last block whose column is
    n_own: inside that block's window, but not owned.  bad_block is the one block that is not packable (None for 'edges')."""
    rowptr, col, _ = banded_edges("edges" if which == "ghost" else which)
    n = len(rowptr) - 1
    bad = None if which == "edges" else 129
    if which == "ghost":
        r = n - 20
        bad = r // RPB
        col = np.insert(col, rowptr[r + 1], n)             # behind the row's last entry: columns stay ascending
        rowptr = rowptr.copy()
        rowptr[r + 1:] += 1
    vals = _pick(PAL_WINDOW, len(col), np.random.default_rng(31))
    return rowptr, col, vals, n, bad


def skip_every_third(nb):
    return [b for b in range(nb) if b % 3 != 2]


def shuffled(nb):
    """every block once, in no ascending order"""
    return [int(b) for b in np.random.default_rng(3).permutation(nb)]


PAL_OCTETS = (0.6, -1.0 / 3.0, 1.4, -0.8)


def neighbour_octets():
    """Returns (rowptr, col, vals, listed).  Six row blocks (n = 1536), none of which begins or ends on a multiple of 8, so
    every block shares its first octet with the block before and its last with the block after.  The last row of every block
    ends with eight columns in [n - 256, n - 2] and the first row of every block begins with eight columns in [1, 255]: read
    with the NEIGHBOUR's base (+-256), the first lie at or above n_own and the second below 0, so the kernel's clamp sends
    them to x[n_own - 1] and x[0].  No row stores column 0 or n - 1.  `listed` are the odd blocks."""
    rng = np.random.default_rng(77)
    nb = 6
    n = nb * RPB
    row_cols = []
    for r in range(n):
        near = [c for c in range(r - 2, r + 3) if 1 <= c < n - 1 and not (c <= 255 and r % RPB == 0) and not (c >= n - 256 and r % RPB == RPB - 1)]
        if r % 5 == 4:
            near = near[:-1]
        if r % RPB == 0:
            near = sorted(rng.choice(np.arange(1, 256), size=8, replace=False).tolist()) + near
        elif r % RPB == RPB - 1:
            near = near + sorted(rng.choice(np.arange(n - 256, n - 1), size=8, replace=False).tolist())
        elif r % RPB == 1:
            near = near[: 1 + (r // RPB) % 3]            # moves p0 % 8 from block to block
        row_cols.append(np.unique(np.asarray(near, dtype=np.int64)))
    p = 0
    for b in range(nb):                                   # no block may end on a multiple of 8: drop an entry of its third row
        cnt = sum(len(c) for c in row_cols[RPB * b:RPB * b + RPB])
        if (p + cnt) % OCTET == 0:
            row_cols[RPB * b + 2] = row_cols[RPB * b + 2][:-1]
            cnt -= 1
        p += cnt
    rowptr, col = _from_rows(row_cols, n)
    return rowptr, col, _pick(PAL_OCTETS, len(col), rng), [1, 3, 5]


DICT_ROWS = 41 * RPB           # 10 496 rows of 12 entries: 125 952 stored entries, 60 416 of them behind the seed sample
DICT_BAND = 12                 # 3072 entries per block: two passes
ROUNDS_LATE = 200


def dictionary(kind):
    """Returns (rowptr, col, vals, ndict).  A band of 12 entries per row (two passes per block, every block octet-aligned).
    'one': one value.  'full': 256 values in a fixed shuffle, so the largest (code 255) also lies in second passes.  'over':
    those 256 in the seed sample and a 257th value 5000 times behind it (ndict None: refused).  'flood': the seed sample holds
    one value, the 60 416 entries behind it three others.  'rounds': 3 values in the sample, behind it 200 others in runs of
    about 302 equal entries, so one round of the bounded list can name only some of them."""
    n = DICT_ROWS
    start = np.clip(np.arange(n) - DICT_BAND // 2, 0, n - DICT_BAND)
    col = (start[:, None] + np.arange(DICT_BAND)[None, :]).reshape(-1).astype(np.int64)
    rowptr = np.arange(n + 1, dtype=np.int64) * DICT_BAND
    nnz = len(col)
    late = nnz - SEED_SAMPLE
    assert late > 10 * MISS_CAP
    rng = np.random.default_rng(5)
    j = np.arange(nnz)
    if kind == "one":
        vals, nd = np.full(nnz, 0.3), 1
    elif kind in ("full", "over"):
        pal = 0.1 + 0.013 * rng.permutation(256)
        vals, nd = pal[j % 256], 256
        if kind == "over":
            vals[SEED_SAMPLE + 7 + 12 * np.arange(5000)] = 7.7
            nd = None
    elif kind == "flood":
        vals = np.full(nnz, 0.3)
        vals[SEED_SAMPLE:] = np.asarray([-1.1, 2.0 / 3.0, 1.7])[rng.integers(3, size=late)]
        nd = 4
    elif kind == "rounds":
        vals = np.asarray([0.3, -1.1, 2.0 / 3.0])[rng.integers(3, size=nnz)]
        vals[SEED_SAMPLE:] = 2.0 + 0.017 * rng.permutation(ROUNDS_LATE)[(np.arange(late) * ROUNDS_LATE) // late]
        nd = 3 + ROUNDS_LATE
    else:
        raise ValueError(kind)
    return rowptr, col, np.ascontiguousarray(vals), nd


def rectangular():
    """Returns (rowptr, col, vals, ncols): 1000 rows (a ragged fourth block) of 11 entries -- 2816 per full block, two passes
    -- over 1300 columns; row r stores columns r + 27 k, so the last rows reach the columns behind the square part."""
    n, ncols = 1000, 1300
    col = (np.arange(n)[:, None] + 27 * np.arange(11)[None, :]).astype(np.int64)
    assert col.max() < ncols and col.max() >= n
    rowptr = np.arange(n + 1, dtype=np.int64) * 11
    return rowptr, col.reshape(-1).copy(), _pick(PAL_OCTETS, n * 11, np.random.default_rng(9)), ncols


def fingerprint(y):
    """A digest of y's bits (for a child process to print and its parent to compare)."""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(y, dtype=np.float64).tobytes()).hexdigest()
