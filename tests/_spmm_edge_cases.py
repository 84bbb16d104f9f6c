"""Inputs, dispatch restatements and references for tests/test_gpu_spmm_edges.py, in plain numpy (no torch, no GPU): the
SpMM kernels of csrc/spmm.hip and the transposed product of csrc/spmm_t.hip at the constants they branch on.

* the constants themselves, read from the sources by regular expression (a pattern that no longer matches raises);
* `variant_of` / `spmm_t_variant_of`: which kernel instance `spmm_launch` / `spmm_t_impl` start under the default environment;
* `pass_matrix(CH)`: 64-row blocks whose record totals sit on, one below and one above the records a pass stages (CH = 512 or
  1536 for the vector kernel, CHUNK_MM for the generic one), with rows that end on, start on and straddle a pass boundary;
* `runs_cases()`: hand-built blocks on the limits of the run tiles (4 | 5 runs, 200 | 201 tile rows, 512 | 513 entries ...) and
  the host restatement of the run descriptors;
* `spmm_t_matrix(cpb)`: columns whose workgroup totals sit on the pass of the transposed product, `struct_cases()` for its
  structure kernels, `seq_transposed_ref` for its sums.

A's values are `order_sensitive` (magnitudes over 40 binades), B / X uniform in [-1, 1): a row (column) that straddles a pass
boundary gets values for which one running sum differs from "the sum of each pass, then added" and from the reversed order in
each of the first two columns of B (X), so a kernel that adds per-pass partial sums cannot give the oracle's bits at any width.
Checked on the CPU by tests/test_spmm_edge_cases.py, so that a failure on the GPU is the kernel's and not the test's."""
import numpy as np

from tests._grid_regimes import _ints, _pat
from tests._spgemm_edge_cases import order_sensitive

# ---- the constants, from the sources -------------------------------------------------------------------------------------------
TPB_MM, = _ints("spmm.hip", _pat("constexpr int TPB_MM = # ;"))
RPB_MM, = _ints("spmm.hip", _pat("constexpr int RPB_MM = # ;"))
CHUNK_MM, = _ints("spmm.hip", _pat("constexpr int CHUNK_MM = # ;"))
KT, = _ints("spmm.hip", _pat("constexpr int KT = # ;"))
RUNS_MAX, RUNS_TILE_ROWS, RUNS_EMAX = _ints("spmm.hip", _pat("constexpr int RUNS_MAX = # , RUNS_TILE_ROWS = # , RUNS_EMAX = # ;"))
CHUNK_V_SMALL, CHUNK_V_LARGE = _ints("spmm.hip", _pat("if ( small ) HPCLA_SPMM_VEC1 ( SP , # ) ; else HPCLA_SPMM_VEC1 ( SP , # ) ;"))
_small_env, SMALL_NNZ_PER_ROW = _ints("spmm.hip", _pat("const bool small = chunk_env ? chunk_env == # : nnz <= # * nrows ;"))
assert _small_env == CHUNK_V_SMALL
TPB_T, = _ints("spmm_t.hip", _pat("constexpr int TPB_T = # ;"))
CHUNK_T, = _ints("spmm_t.hip", _pat("constexpr int CHUNK_T = # ;"))
# the lines of spmm_launch / spmm_t_impl that variant_of / spmm_t_variant_of restate: they only have to be there
for _line in ("const bool c_colmajor = c_rs == 1 && c_cs != 1 && !accumulate && c_cs >= nrows ;",
              "const bool c_col = c_colmajor && k <= KT ;",
              "const bool odd_ok = ( k % 2 ) == 0 || ( b_rs > k && ( !split || !B_ghost || bg_rs > k ) && ( c_colmajor || c_rs > k ) ) ;",
              "const bool vec_ok = b_cs == 1 && ( c_colmajor || ( c_cs == 1 && ( c_rs % 2 ) == 0 ) ) && odd_ok && ( b_rs % 2 ) == 0 &&",
              "const int lpr = ( ke <= 8 && lpr_env != 4 && !c_col ) ? 2 : 4 ;",
              "const bool h64 = lpr == 4 && h64_env != 0 && ( ke % 16 ) == 0 ;",
              "const bool cstage = c_col || ( cst_env != 0 && ke <= 4 * lpr && c_rs == ke ) ;",
              "const bool k16 = h64 && cstage && ke == KT && b_rs == KT && ( !split || bg_rs == KT ) ;",
              "const bool tail2 = ( ke % 4 ) != 0 ;",
              "if ( split ) { if ( k <= 4 ) HPCLA_SPMM_GEN ( true , 4 ) ; else if ( k <= 8 ) HPCLA_SPMM_GEN ( true , 8 ) ; else "
              "HPCLA_SPMM_GEN ( true , 16 ) ; }"):
    _ints("spmm.hip", _pat(_line))
_ints("spmm_t.hip", _pat("const bool vec = x_cs == 1 && ( x_rs & 1 ) == 0 && ( m & 1 ) == 0 && ( ( uintptr_t ) X & 15 ) == 0 ;"))
_ints("spmm_t.hip", _pat("const int lpc = m <= 2 ? 1 : m <= 4 ? 2 : m <= 8 ? 4 : m <= 16 ? 8 : m <= 32 ? 16 : 32 ;"))
del _line

NCOLS = 4101                       # column space of the pass matrices (a row of 2 * CHUNK_MM + 7 entries fits)
N_OWN = 2731                       # own columns of the split products; columns N_OWN ... are rows of the ghost segment
BMAX = 40                          # widest B of the GPU tests; every narrower B is its first k columns


# ---- which kernel a call starts ------------------------------------------------------------------------------------------------
def variant_of(k, b_rs, b_cs, bg_rs, c_rs, c_cs, split, accumulate, nnz, nrows, aligned=True, block_list=False, ghost=None):
    """spmm_launch's dispatch under the default environment.  Returns (variant, launches): "spmv", ("generic", GRP) or
    ("vec", CH, LPR, HALF64, CSTAGE, K16, TAIL2, CCOL) and the list of kernel launches -- one, or for a column-major C wider
    than KT one per column tile (variant "tiles").  `aligned`: B, the ghost segment and C all start on 16 bytes; `ghost`:
    a ghost segment is passed (default: when split)."""
    ghost = bool(split) if ghost is None else ghost
    if k == 1 and not block_list and not accumulate and b_rs == 1 and c_rs == 1 and (not split or not ghost or bg_rs == 1):
        return "spmv", ["spmv"]
    c_colmajor = c_rs == 1 and c_cs != 1 and not accumulate and c_cs >= nrows
    c_col = c_colmajor and k <= KT
    odd_ok = k % 2 == 0 or (b_rs > k and (not split or not ghost or bg_rs > k) and (c_colmajor or c_rs > k))
    vec_ok = (b_cs == 1 and (c_colmajor or (c_cs == 1 and c_rs % 2 == 0)) and odd_ok and b_rs % 2 == 0 and
              (not split or bg_rs % 2 == 0) and aligned)
    if vec_ok and c_colmajor and not c_col:
        tiles = [variant_of(min(k - kt, KT), b_rs, b_cs, bg_rs, c_rs, c_cs, split, 0, nnz, nrows, aligned, block_list, ghost)[0]
                 for kt in range(0, k, KT)]
        return "tiles", tiles
    if not vec_ok:
        v = ("generic", 4 if k <= 4 else 8 if k <= 8 else 16)
        return v, [v]
    CH = CHUNK_V_SMALL if nnz <= SMALL_NNZ_PER_ROW * nrows else CHUNK_V_LARGE
    ke = k + (k & 1)
    lpr = 2 if ke <= 8 and not c_col else 4
    h64 = lpr == 4 and ke % 16 == 0
    cstage = c_col or (ke <= 4 * lpr and c_rs == ke)
    k16 = h64 and cstage and ke == KT and b_rs == KT and (not split or bg_rs == KT)
    tail2 = ke % 4 != 0
    if c_col:
        t = (4, True, True, True, False, True) if k16 else (4, False, True, False, tail2, True)
    elif lpr == 2:
        t = (2, False, cstage, False, tail2, False)
    elif k16:
        t = (4, True, True, True, False, False)
    elif h64:
        t = (4, True, cstage, False, False, False)
    else:
        t = (4, False, cstage, False, tail2, False)
    v = ("vec", CH) + t
    return v, [v]


# every (LPR, HALF64, CSTAGE, K16, TAIL2, CCOL) that the macros HPCLA_SPMM_VEC1 / _VEC / _VECC of spmm_launch instantiate:
# three CCOL forms; two lanes per row with and without CSTAGE and TAIL2; K16; HALF64 with and without CSTAGE; four lanes per
# row with and without CSTAGE and TAIL2
VEC_TUPLES = frozenset(
    [(4, True, True, True, False, True), (4, False, True, False, True, True), (4, False, True, False, False, True)] +
    [(2, False, cst, False, t2, False) for cst in (False, True) for t2 in (False, True)] +
    [(4, True, True, True, False, False), (4, True, True, False, False, False), (4, True, False, False, False, False)] +
    [(4, False, cst, False, t2, False) for cst in (False, True) for t2 in (False, True)])
assert len(VEC_TUPLES) == 14


def spmm_t_lpc(m):
    return 1 if m <= 2 else 2 if m <= 4 else 4 if m <= 8 else 8 if m <= 16 else 16 if m <= 32 else 32


def spmm_t_variant_of(m, x_row_major, ldx, w_col_major, aligned=True):
    """(LPC, VEC, WCOL) of spmm_t_impl."""
    x_rs, x_cs = (ldx, 1) if x_row_major else (1, ldx)
    vec = x_cs == 1 and x_rs % 2 == 0 and m % 2 == 0 and aligned
    return spmm_t_lpc(m), vec, bool(w_col_major)


SPMM_T_VARIANTS = frozenset((lpc, vec, wcol) for lpc in (1, 2, 4, 8, 16, 32) for vec in (False, True) for wcol in (False, True))


# ---- the case tables of the GPU tests ------------------------------------------------------------------------------------------
VEC_KS = (2, 3, 4, 6, 7, 8, 10, 12, 14, 15, 16, 18, 20, 32, 40)
GENERIC_KS = (3, 5, 7, 9, 15, 17, 33)
SPMM_T_MS = (1, 2, 4, 8, 16, 17, 18, 64, 65, 66, 130)    # 4, 8 and 18: the lane counts the other widths leave out, with even m


def vec_cases(nrows):
    """The calls of the vector-kernel test on a matrix of `nrows` (odd) rows: dicts entry ("csr" | "split" | "split_ccol" |
    "panel"), k, ldb, ldg (pitch of the ghost segment), ldc, ccol (C column-major).  B rows on the tight even pitch
    kp = k + (k & 1) and on kp + 2; a row-major C on B's pitch (and 18 at k = 16 on the pitch 16: HALF64 without CSTAGE; 16 on
    the B pitch 18: HALF64 and CSTAGE without K16), a column-major C on an odd and an even leading dimension.  The ghost
    segment of a split call has the pitch kp next to the tight B (K16 needs both at 16) and kp + 4 next to the padded one."""
    assert nrows % 2 == 1
    out = []
    for k in VEC_KS:
        kp = k + (k & 1)
        shapes = [(kp, kp, kp), (kp + 2, kp + 4, kp + 2)]
        if k == 16:
            shapes += [(16, 16, 18), (18, 18, 16)]
        for ldb, ldg, ldc in shapes:
            out.append(dict(entry="csr", k=k, ldb=ldb, ldg=ldg, ldc=ldc, ccol=False))
            out.append(dict(entry="split", k=k, ldb=ldb, ldg=ldg, ldc=ldc, ccol=False))
        for ldb, ldg, ldc in ((kp, kp, nrows), (kp + 2, kp + 4, nrows + 1)):
            out.append(dict(entry="csr", k=k, ldb=ldb, ldg=ldg, ldc=ldc, ccol=True))
            out.append(dict(entry="split_ccol", k=k, ldb=ldb, ldg=ldg, ldc=ldc, ccol=True))
        out.append(dict(entry="panel", k=k, ldb=kp, ldg=kp, ldc=kp, ccol=False))
    return out


def generic_cases(ncols):
    """The calls of the generic-kernel test: `how` = "odd" (row-major B and C on the tight odd pitch k), "colB" (column-major B,
    row-major C), "offset" (the even pitch k + 1, but B eight bytes past a 16-byte boundary)."""
    out = []
    for k in GENERIC_KS:
        for entry in ("csr", "split", "panel"):
            out.append(dict(entry=entry, how="odd", k=k, ldb=k, ldg=k, ldc=k, b_col=False, aligned=True))
            out.append(dict(entry=entry, how="offset", k=k, ldb=k + 1, ldg=k + 1, ldc=k + 1, b_col=False, aligned=False))
        out.append(dict(entry="csr", how="colB", k=k, ldb=ncols + 3, ldg=0, ldc=k, b_col=True, aligned=True))
    return out


def case_variant(case, nnz, nrows):
    """variant_of for one entry of vec_cases / generic_cases."""
    split = case["entry"] != "csr"
    b_rs, b_cs = (1, case["ldb"]) if case.get("b_col") else (case["ldb"], 1)
    c_rs, c_cs = (1, case["ldc"]) if case.get("ccol") else (case["ldc"], 1)
    return variant_of(case["k"], b_rs, b_cs, case["ldg"], c_rs, c_cs, split, 1 if case["entry"] == "panel" else 0, nnz, nrows,
                      aligned=case.get("aligned", True), block_list=case["entry"] in ("split", "split_ccol"))


# ---- order sensitivity -----------------------------------------------------------------------------------------------------
def running_sum(prod):
    """One running sum from 0.0 down the rows of `prod` (np.cumsum adds one after the other; np.sum is pairwise)."""
    prod = np.asarray(prod, dtype=np.float64)
    zero = np.zeros((1,) + prod.shape[1:])
    return np.cumsum(np.concatenate([zero, prod]), axis=0)[-1]


def per_pass_sum(prod, cuts):
    """What a kernel would give that summed each pass from 0.0 and added the pass sums: `cuts` = the positions in (0, len)
    at which a new pass begins."""
    edges = [0] + list(cuts) + [len(prod)]
    return running_sum(np.stack([running_sum(prod[a:b]) for a, b in zip(edges[:-1], edges[1:])]))


def discriminated(vals, dense_rows, cuts):
    """Per column of `dense_rows` (len x k): the running sum of vals * dense_rows differs from the per-pass sums AND from the
    reversed order."""
    prod = np.asarray(vals)[:, None] * np.asarray(dense_rows)
    one = running_sum(prod)
    return (one != per_pass_sum(prod, cuts)) & (one != running_sum(prod[::-1]))


def master_B(nrows=NCOLS, width=BMAX, seed=9):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (nrows, width))


def straddlers(ptr, CH, group):
    """[(index, cuts)] of the rows (columns) that a pass boundary cuts: `ptr` the row (column) pointer, `group` the rows
    (columns) per workgroup, whose first record is the pass origin; cuts relative to the row's first record."""
    out = []
    n = len(ptr) - 1
    for g0 in range(0, n, group):
        p0 = int(ptr[g0])
        for r in range(g0, min(g0 + group, n)):
            lo, hi = int(ptr[r]) - p0, int(ptr[r + 1]) - p0
            cuts = [c - lo for c in range((lo // CH + 1) * CH, hi, CH)]
            if cuts:
                out.append((r, cuts))
    return out


def _draw_values(vals, ptr, idx, dense, CH, group, seed):
    """The records of a straddling row (column) are drawn again until the row is told apart in column 0 and in column 1 of
    `dense` (whose rows `idx` names).  `vals`: order_sensitive values for every record, changed in place."""
    for r, cuts in straddlers(ptr, CH, group):
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        for attempt in range(200):
            if discriminated(vals[lo:hi], dense[idx[lo:hi], :2], cuts).all():
                break
            vals[lo:hi] = order_sensitive(np.random.default_rng([seed, r, attempt]), hi - lo)
        else:
            raise AssertionError(f"no order-sensitive draw for row {r}")
    return vals


# ---- pass matrices -----------------------------------------------------------------------------------------------------------
def _split(total, n):
    """`total` records over n rows, lengths differing by at most one (rows may be empty)."""
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


def _block_lens(CH, total, nr, pins=(), empty_first=False, empty_last=False):
    """Row lengths of one block: `pins` = [(start, end)], the record ranges that must be one row each; what lies between
    them is divided among the other rows.  No pass boundary may fall inside such a gap: a filler row never straddles."""
    pins = sorted(pins)
    segs, pos = [], 0                                             # (start, end, is_pin)
    for a, b in pins:
        assert pos <= a < b <= total
        if a > pos:
            segs.append((pos, a, False))
        segs.append((a, b, True))
        pos = b
    if pos < total:
        segs.append((pos, total, False))
    gaps = [(a, b) for a, b, pin in segs if not pin]
    for a, b in gaps:
        assert (b - 1) // CH == a // CH, f"a pass boundary inside the gap [{a}, {b})"
    free = nr - len(pins) - int(empty_first) - int(empty_last)
    assert free >= len(gaps)
    glen = sum(b - a for a, b in gaps)
    alloc = [1 + (free - len(gaps)) * (b - a) // glen for a, b in gaps]
    lens = [0] if empty_first else []
    gi = 0
    for a, b, pin in segs:
        if pin:
            lens.append(b - a)
        else:
            lens += _split(b - a, alloc[gi])
            gi += 1
    lens += [0] * (nr - len(lens))                                # what rounding left over: empty rows at the end
    assert len(lens) == nr and sum(lens) == total and (not empty_last or lens[-1] == 0)
    return lens


def pass_blocks(CH):
    """[(name, row lengths)] of the fixed blocks of pass_matrix(CH), the ragged last one excluded."""
    R = RPB_MM
    one = [0] * R
    one[17] = 1
    row63 = [0] * (R - 1) + [CH]
    # rows g, g + 16, g + 32, g + 48 (one lane group of the generic kernel at GRP = 16; g, g + 32 at GRP = 8) with lengths
    # 0, 1, odd and long
    group = [3] * R
    group[5], group[21], group[37], group[53] = 0, 1, 7, CH + 101
    return [
        ("empty", [0] * R),
        ("one", one),
        ("CH-1", _block_lens(CH, CH - 1, R, empty_first=True, empty_last=True)),
        ("CH in row 63", row63),
        ("CH+1", _block_lens(CH, CH + 1, R, [(CH - 7, CH), (CH, CH + 1)])),                      # ends at | starts at the boundary
        ("2CH", _block_lens(CH, 2 * CH, R, [(CH - 2, CH + 3)], empty_first=True, empty_last=True)),   # even | odd
        ("2CH+1", _block_lens(CH, 2 * CH + 1, R, [(CH - 3, CH + 3), (2 * CH - 5, 2 * CH), (2 * CH, 2 * CH + 1)])),   # odd | odd
        ("3CH+7", _block_lens(CH, 3 * CH + 7, R, [(CH - 4, 3 * CH + 3)])),                          # longer than 2 CH: two whole passes
        ("2CH+2", _block_lens(CH, 2 * CH + 2, R, [(CH - 4, CH + 4), (2 * CH - 3, 2 * CH + 2)])),      # even | even, odd | even
        ("lane group", group),
    ]


LAST_NR = 37                       # rows of the ragged last block (odd, < 64)
TOTALS = ("0", "1", "CH-1", "CH", "CH+1", "2CH", "2CH+1", "3CH+7")


def pass_matrix(CH, extra_entry=False, seed=5):
    """The pass matrix for passes of CH records.  CH = CHUNK_V_SMALL: blocks of short rows are added until
    nnz == SMALL_NNZ_PER_ROW * nrows exactly (the last size that selects the small pass); `extra_entry` adds one more entry
    to a short row (the first size that does not).  Any other CH: no short-row blocks, nnz > SMALL_NNZ_PER_ROW * nrows.
    Returns a dict: rowptr, colval (int64, 0-based, ascending and distinct per row), vals, nrows, ncols, n_own, CH, names (per
    block), and the rows the tests name: ends_at / starts_at (a pass boundary), long_row (> 2 CH), group_rows."""
    blocks = pass_blocks(CH)
    last = _block_lens(CH, CH + 1, LAST_NR, [(CH - 6, CH), (CH, CH + 1)])
    fillers = 0
    if CH == CHUNK_V_SMALL:
        fixed = sum(sum(l) for _, l in blocks) + sum(last)
        rows_fixed = RPB_MM * len(blocks) + LAST_NR
        while SMALL_NNZ_PER_ROW * (rows_fixed + RPB_MM * fillers) < fixed + 3 * RPB_MM * fillers or fillers == 0:
            fillers += 1                                         # until the short rows can average >= 3 entries
        short = _split(SMALL_NNZ_PER_ROW * (rows_fixed + RPB_MM * fillers) - fixed, RPB_MM * fillers)
        for f in range(fillers):
            blocks.append((f"short rows {f}", short[f::fillers]))
    lens = np.array([l for _, ls in blocks for l in ls] + last, dtype=np.int64)
    names = [n for n, _ in blocks] + ["ragged CH+1"]
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    nrows = len(lens)
    strad = dict(straddlers(rowptr, CH, RPB_MM))
    cols, vals = [], []
    for r, L in enumerate(lens.tolist()):
        rng = np.random.default_rng([seed, CH, r])
        c = np.sort(rng.choice(NCOLS, L, replace=False))
        force = [N_OWN] if L == 1 else [N_OWN - 1, N_OWN] if r in strad else []     # the first ghost column: offset -1
        for f in force:
            if f not in c:
                c[int(np.argmin(np.isin(c, force)))] = f         # replaces an entry that is not itself forced
                c = np.sort(c)
        assert len(np.unique(c)) == L
        cols.append(c)
        vals.append(order_sensitive(rng, L))
    colval = np.concatenate(cols).astype(np.int64)
    vals = _draw_values(np.concatenate(vals), rowptr, colval, master_B(), CH, RPB_MM, seed)
    if extra_entry:                                              # one more entry in a short row; nothing else changes
        assert fillers
        r = RPB_MM * (len(blocks) - 1) + 11
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        new = next(c for c in range(NCOLS // 2, NCOLS) if c not in colval[lo:hi])
        at = lo + int(np.searchsorted(colval[lo:hi], new))
        colval, vals = np.insert(colval, at, new), np.insert(vals, at, 0.8125 * 2.0 ** -7)
        lens[r] += 1
        rowptr = np.concatenate([[0], np.cumsum(lens)])
    b0 = {n: i * RPB_MM for i, n in enumerate(names)}

    def row_at(block, start=None, end=None):
        r0 = b0[block]
        p0 = rowptr[r0]
        for r in range(r0, min(r0 + RPB_MM, nrows)):
            if lens[r] and (start is None or rowptr[r] - p0 == start) and (end is None or rowptr[r + 1] - p0 == end):
                return r
        raise AssertionError((block, start, end))
    return dict(rowptr=rowptr, colval=colval, vals=vals, nrows=nrows, ncols=NCOLS, n_own=N_OWN, CH=CH, names=names,
                ends_at=[row_at("CH+1", end=CH), row_at("2CH+1", end=2 * CH), row_at("ragged CH+1", end=CH)],
                starts_at=[row_at("CH+1", start=CH), row_at("2CH+1", start=2 * CH), row_at("ragged CH+1", start=CH)],
                long_row=row_at("3CH+7", start=CH - 4), group_rows=[b0["lane group"] + g for g in (5, 21, 37, 53)])


def switch_pair():
    """Two matrices that differ by one entry: nnz == SMALL_NNZ_PER_ROW * nrows (small pass) and one more (large pass)."""
    return pass_matrix(CHUNK_V_SMALL), pass_matrix(CHUNK_V_SMALL, extra_entry=True)


def block_totals(M):
    rp, n = M["rowptr"], M["nrows"]
    return [int(rp[min(b + RPB_MM, n)] - rp[b]) for b in range(0, n, RPB_MM)]


def seq_spmm_ref(rowptr, colval, vals, B):
    """C = A * B, every C(r, c) one running sum from 0.0 in stored order, multiply and add rounded separately."""
    C = np.zeros((len(rowptr) - 1, B.shape[1]))
    for r in range(len(rowptr) - 1):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        if hi > lo:
            C[r] = running_sum(vals[lo:hi, None] * B[colval[lo:hi]])
    return C


def block_lists(M):
    """(interior, boundary): the blocks that touch no ghost column, and those that do (int32, ascending)."""
    rp, n = M["rowptr"], M["nrows"]
    touches = np.array([np.any(M["colval"][rp[b]:rp[min(b + RPB_MM, n)]] >= M["n_own"]) for b in range(0, n, RPB_MM)])
    return np.flatnonzero(~touches).astype(np.int32), np.flatnonzero(touches).astype(np.int32)


def panels_of(M, cuts=None):
    """The matrix as three column panels in panel order (own columns, then two ghost panels): [(rowptr, colval relative to the
    panel's buffer, vals, first column, one past the last)] -- the inputs of hpcla_spmm_panel_*."""
    c1 = M["n_own"]
    c2 = c1 + (M["ncols"] - c1) // 2 if cuts is None else cuts
    cv, n = M["colval"], M["nrows"]
    rowid = np.repeat(np.arange(n), np.diff(M["rowptr"]))
    out = []
    for lo, hi in ((0, c1), (c1, c2), (c2, M["ncols"])):
        sel = np.flatnonzero((cv >= lo) & (cv < hi))
        prp = np.concatenate([[0], np.cumsum(np.bincount(rowid[sel], minlength=n))]).astype(np.int64)
        out.append((prp, cv[sel] - lo, M["vals"][sel], lo, hi))
    return out


def panel_order_ref(M, B):
    """The product taken panel by panel, every C(r, c) ONE running sum that continues through the panels."""
    n = M["nrows"]
    C = np.zeros((n, B.shape[1]))
    for prp, pcv, pval, lo, _ in panels_of(M):
        for r in range(n):
            a, b = int(prp[r]), int(prp[r + 1])
            if b > a:
                C[r] = np.cumsum(np.concatenate([C[r:r + 1], pval[a:b, None] * B[pcv[a:b] + lo]]), axis=0)[-1]
    return C


# ---- run tiles -----------------------------------------------------------------------------------------------------------------
RUNS_NCOLS = 1400
RUNS_N_OWN = {"odd": 901, "even": 900, "all": RUNS_NCOLS}


def run_descriptors(rowptr, colval, nrows, n_own):
    """Host restatement of spmm_runs_build_kernel: per 64-row block (fits, starts, lens) -- the distinct 0-based columns as
    contiguous runs, cut where they stop being consecutive and at the own / ghost boundary; a block fits with at most
    RUNS_MAX runs, RUNS_TILE_ROWS distinct columns and RUNS_EMAX entries (an empty block fits: no runs)."""
    out = []
    for b in range(0, nrows, RPB_MM):
        lo, hi = int(rowptr[b]), int(rowptr[min(b + RPB_MM, nrows)])
        cols = np.unique(colval[lo:hi])
        if len(cols) == 0:
            out.append((True, cols, cols))
            continue
        brk = np.flatnonzero((np.diff(cols) != 1) | ((cols[:-1] < n_own) & (cols[1:] >= n_own))) + 1
        starts = np.concatenate([[0], brk])
        lens = np.diff(np.concatenate([starts, [len(cols)]]))
        ok = len(starts) <= RUNS_MAX and len(cols) <= RUNS_TILE_ROWS and hi - lo <= RUNS_EMAX
        out.append((bool(ok), cols[starts], lens))
    return out


def check_descriptors(d, n_fit, restated):
    """The device's descriptors `d` (blocks x 8 int32: start[4], len[4]) and its count against run_descriptors."""
    fit_ref = 0
    for b, (ok, starts, lens) in enumerate(restated):
        assert (d[b, RUNS_MAX] >= 0) == ok, (b, d[b], starts, lens)
        if ok:
            fit_ref += 1
            np.testing.assert_array_equal(d[b, :len(starts)], starts)
            np.testing.assert_array_equal(d[b, RUNS_MAX:RUNS_MAX + len(starts)], lens)
            assert (d[b, len(starts):RUNS_MAX] == 0).all() and (d[b, RUNS_MAX + len(starts):] == 0).all(), (b, d[b])
    assert n_fit == fit_ref, (n_fit, fit_ref)
    return fit_ref


def colmajor_fits(restated_block, n_own):
    """Whether spmm_runs_colmajor_kernel stages the block: it fits, its own runs widened to even bounds hold at most
    RUNS_TILE_ROWS rows, and no widened run ends past row n_own."""
    ok, starts, lens = restated_block
    if not ok:
        return False
    tpad = 0
    for s, l in zip(starts.tolist(), lens.tolist()):
        if s < n_own:
            a, e = s & ~1, (s + l + 1) & ~1
            if e > n_own:
                return False
            tpad += e - a
    return tpad <= RUNS_TILE_ROWS


def banded_count(rowptr, colval, nrows, n_own, max_runs):
    """hpcla_spmm_banded_blocks_*: blocks of at most RUNS_EMAX entries on at most `max_runs` runs."""
    count = 0
    for b, (_, starts, _) in zip(range(0, nrows, RPB_MM), run_descriptors(rowptr, colval, nrows, n_own)):
        total = int(rowptr[min(b + RPB_MM, nrows)] - rowptr[b])
        count += total <= RUNS_EMAX and len(starts) <= max_runs
    return count


def _runs_block(rng, runs, entries, nr):
    """Rows of a block whose distinct columns are exactly the union of `runs` [(start, len)] and that has `entries` entries:
    every column once (column j of the union in row j mod nr), then further (row, column) pairs."""
    if not runs:
        assert entries == 0
        return [np.zeros(0, dtype=np.int64) for _ in range(nr)]
    cols = np.concatenate([np.arange(s, s + l) for s, l in runs])
    T = len(cols)
    assert T <= entries <= nr * T
    have = np.zeros(nr * T, dtype=bool)
    have[(np.arange(T) % nr) * T + np.arange(T)] = True
    have[rng.choice(np.flatnonzero(~have), entries - T, replace=False)] = True
    have = have.reshape(nr, T)
    return [cols[np.flatnonzero(have[r])] for r in range(nr)]


def runs_blocks(N):
    """[(name, runs, entries, nr)]: the hand-built blocks, columns relative to the own / ghost boundary N where they say so."""
    R = RPB_MM
    e_runs = [(200, 20), (240, 15), (400, 5)]                     # 40 tile rows
    return [
        ("4 runs, one of length 1", [(10, 10), (30, 1), (50, 20), (100, 7)], 120, R),
        ("5 runs", [(10, 5), (20, 5), (30, 5), (40, 5), (50, 5)], 100, R),
        ("T=199", [(0, 64), (100, 66), (300, 69)], 320, R),        # T % 8 == 7
        ("T=200", [(0, 64), (100, 66), (300, 70)], 320, R),        # T % 8 == 0
        ("T=201", [(0, 64), (100, 66), (300, 71)], 320, R),
        ("T=9", [(5, 9)], 30, R),                                  # T % 8 == 1
        ("T=1", [(77, 1)], 40, R),
        ("E=256", e_runs, 256, R), ("E=257", e_runs, 257, R), ("E=511", e_runs, 511, R), ("E=512", e_runs, 512, R),
        ("E=513", e_runs, 513, R),
        ("300 columns in 400 entries", [(100, 300)], 400, R),
        ("run across N", [(N - 5, 10)], 64, R),
        ("own run to N-1", [(N - 12, 12)], 50, R),
        ("widened 200", [(1, 64), (101, 64), (200, 68)], 300, R),
        ("widened 202", [(1, 64), (101, 64), (200, 70)], 300, R),
        ("ghost run only", [(N + 20, 30)], 90, R),
        ("empty", [], 0, R),
        ("last, nr=1", [(40, 6)], 6, 1),
    ]


# what the names claim, per kind of n_own: {name: (fits, the column-major kernel stages it)}; a block not listed: (True, True)
RUNS_CLAIMS = {
    "5 runs": (False, False), "T=201": (False, False), "E=513": (False, False), "300 columns in 400 entries": (False, False),
    "widened 202": (True, False),
}
RUNS_CLAIMS_ODD = {"run across N": (True, False), "own run to N-1": (True, False)}   # the widened end N + 1 is past row N


def runs_claims(kind):
    claims = {name: (True, True) for name, *_ in runs_blocks(0)}
    claims.update(RUNS_CLAIMS)
    if kind == "odd":
        claims.update(RUNS_CLAIMS_ODD)
    return claims


def runs_cases(seed=11):
    """One matrix per kind of own / ghost boundary ("odd": n_own = 901, "even": 900, "all": every column owned, no ghost
    segment), all made of runs_blocks(901 | 900 | 901).  Dicts: kind, rowptr, colval, vals, nrows, ncols, n_own, names."""
    out = []
    for kind in ("odd", "even", "all"):
        N = RUNS_N_OWN["odd" if kind == "all" else kind]
        rng = np.random.default_rng([seed, N])
        rows, names = [], []
        for name, runs, entries, nr in runs_blocks(N):
            rows += _runs_block(rng, runs, entries, nr)
            names.append(name)
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        rowptr = np.concatenate([[0], np.cumsum(lens)])
        colval = np.concatenate(rows).astype(np.int64)
        out.append(dict(kind=kind, rowptr=rowptr, colval=colval, vals=order_sensitive(rng, len(colval)), nrows=len(lens),
                        ncols=RUNS_NCOLS, n_own=RUNS_N_OWN[kind], names=names))
    return out


# ---- the transposed product ----------------------------------------------------------------------------------------------------
T_ROWS = 2500                      # rows of A (a column of 2100 entries fits)
XMAX = 130                         # widest X; every narrower X is its first m columns


def spmm_t_col_lens(cpb):
    """Column lengths for workgroups of `cpb` columns: workgroup totals CHUNK_T - 1, CHUNK_T, CHUNK_T + 1 (its last column
    starts on the pass boundary), one above 3 CHUNK_T with a column longer than CHUNK_T and one longer than 2 CHUNK_T, and a
    last workgroup of nc < cpb columns whose first column straddles the boundary; the first and the last column are empty."""
    CH = CHUNK_T
    nc = cpb // 2 - 1                                             # (CHUNK_T + 3 * (nc - 1) entries: below 2 CHUNK_T)
    assert 3 <= nc and 3 * (nc - 1) < CH
    return ([0] + _split(CH - 1, cpb - 1) + _split(CH, cpb) + _split(CH, cpb - 1) + [1] +
            [CH + 76, 2 * CH + 52] + _split(60, cpb - 2) + [CH + 3] + [3] * (nc - 2) + [0])


def spmm_t_matrix(cpb, seed=21):
    """A (T_ROWS x ncols, CSR, ascending columns per row) with the column lengths spmm_t_col_lens(cpb).  Dict: rowptr, colval,
    vals, nrows, ncols, cpb, colptr (of the stored-order CSC), and perm / rowidx of csc_struct_ref."""
    lens = np.array(spmm_t_col_lens(cpb), dtype=np.int64)
    ncols = len(lens)
    rng = np.random.default_rng([seed, cpb])
    rows = np.concatenate([np.sort(rng.choice(T_ROWS, int(L), replace=False)) for L in lens])
    cols = np.repeat(np.arange(ncols), lens)
    colptr = np.concatenate([[0], np.cumsum(lens)])
    X = master_B(T_ROWS, XMAX, seed=13)
    vals_csc = _draw_values(order_sensitive(rng, len(rows)), colptr, rows, X, CHUNK_T, cpb, seed)
    order = np.lexsort((cols, rows))                               # CSR order: by row, then column
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=T_ROWS))]).astype(np.int64)
    M = dict(rowptr=rowptr, colval=cols[order].astype(np.int64), vals=vals_csc[order], nrows=T_ROWS, ncols=ncols, cpb=cpb)
    M["colptr"], M["rowidx"], M["perm"] = csc_struct_ref(M["rowptr"], M["colval"], ncols)
    assert np.array_equal(M["colptr"], colptr) and np.array_equal(M["rowidx"], rows)
    return M


def csc_struct_ref(rowptr, colval, ncols):
    """(colptr_t, rowidx_t, perm) of hpcla_spmm_t_struct_*: CSR positions sorted by column, stable."""
    perm = np.argsort(colval, kind="stable").astype(np.int64)
    colptr = np.searchsorted(colval[perm], np.arange(ncols + 1), side="left").astype(np.int64)
    rowid = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)).astype(np.int64)
    return colptr, rowid[perm], perm


def seq_transposed_ref(rowptr, colval, vals, X, ncols):
    """W = A^T X (ncols x m): per column of A one running sum from 0.0 in ascending-row stored order, multiply and add
    rounded separately."""
    colptr, rowidx, perm = csc_struct_ref(rowptr, colval, ncols)
    W = np.zeros((ncols, X.shape[1]))
    for c in range(ncols):
        lo, hi = int(colptr[c]), int(colptr[c + 1])
        if hi > lo:
            W[c] = running_sum(vals[perm[lo:hi], None] * X[rowidx[lo:hi]])
    return W


def transposed_csr(rowptr, colval, vals, ncols):
    """The explicit transpose as CSR (rows = columns of A, entries in ascending row order of A)."""
    colptr, rowidx, perm = csc_struct_ref(rowptr, colval, ncols)
    return colptr, rowidx, vals[perm]


def spmm_t_calls(m, ncols):
    """The calls of the transposed-product test at width m: dicts x_row (X row-major), ldx, w_col (W column-major), ldw.  X as
    rows on an even and on an odd padded pitch and as columns; W as rows on a padded pitch and as columns."""
    even = m + (m & 1) + 2
    return [dict(x_row=x_row, ldx=ldx, w_col=w_col, ldw=ncols + 1 if w_col else m + 3)
            for x_row, ldx in ((True, even), (True, even + 1), (False, T_ROWS + 3)) for w_col in (False, True)]


STRUCT_NCOLS = (1, 2, 3, 256, 257, 65536, 65537)    # key_bits on, one above and far from a power of two


def struct_cases(seed=17):
    """[(ncols, rowptr, colval)]: 300 rows with up to 1500 entries, an entry in the last column, empty rows."""
    out = []
    for ncols in STRUCT_NCOLS:
        rng = np.random.default_rng([seed, ncols])
        nrows = 300
        nnz = min(1500, nrows * ncols // 2 + 1)
        flat = np.unique(np.concatenate([rng.choice(nrows * ncols, nnz, replace=False), [(nrows - 7) * ncols + ncols - 1]]))
        flat = flat[(flat // ncols) % 13 != 4]                     # empty rows (not row nrows - 7 = 293)
        rows, cols = flat // ncols, flat % ncols
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrows))]).astype(np.int64)
        out.append((ncols, rowptr, cols.astype(np.int64)))
    return out
