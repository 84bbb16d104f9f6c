"""Cases, references and a restated dispatch for tests/test_gpu_dense_edges.py, in plain numpy (no torch, no GPU): the dense
mat-vec kernels of csrc/gemv.hip (A*x and transpose(A)*x) and the layout conversion hpcla_transpose_f64/_f32 of
csrc/spmm.hip, at the widths, pitches, alignments and chunk counts where their code takes another branch.  Checked on the CPU
by tests/test_dense_edge_cases.py -- the restated chunk count is tied to the library's own hpcla_gemv_t_work_bytes there -- so
that a failure on the GPU is the kernel's and not the test's.

Two kinds of input for every product.  "int": entries of A and x are integers in [-8, 8]; every product is at most 64 and
every partial sum at most 64 * 2e6 < 2^53, so any summation order, with or without FMA contraction, gives the same bits and
the int64 numpy product is the reference, compared for equality.  "real": uniform in [-0.5, 0.5); the reference is accumulated
in numpy's long double and the bound is RTOL_RED * sum|a||x| per output, which the longest add chain of each case (worked out
from the restated dispatch) stays an order of magnitude below."""
import numpy as np

RTOL_RED = 1e-12               # BASELINE.json: 1e-12 relative for fp64 reductions
UNIT_ROUNDOFF = 2.0 ** -53
MAX_BYTES = 30 * 10 ** 6       # no buffer of a test is larger
GUARD = 8                      # NaN elements before and after every output


def ceil_div(a, b):
    return -(-a // b)


# ---- transpose(A) * x: hpcla_gemv_t_rowmajor_f64 ------------------------------------------------------------------------

GEMVT_THREADS = 256            # stage 1
GEMVT2_THREADS = 1024          # stage 2


def gemv_t_W(ncols):
    W = 1
    while W < 64 and W < ncols:
        W <<= 1
    return W


def gemv_t_W2(ncols):
    W2 = 2
    while W2 < 128 and W2 < ncols:
        W2 <<= 1
    return W2


def gemv_t_rows_per_chunk(nrows, ncols):
    W = gemv_t_W(ncols)
    tiles = ceil_div(ncols, W)
    target = 1024 if ncols <= 32 else 2048
    want_chunks = max(1, ceil_div(target, max(tiles, 1)))
    return max(64, ceil_div(nrows, want_chunks))


def _strided_counts(total, step):
    """Elements that phases 0 .. step-1 visit when phase p takes p, p + step, ... below `total`."""
    return [ceil_div(total - p, step) if total > p else 0 for p in range(step)]


def gemv_t_dispatch(nrows, ncols, lda, aligned=True):
    """What hpcla_gemv_t_rowmajor_f64 launches for a block of nrows x ncols (both positive) on pitch lda; `aligned` says
    that A and work are both 16-byte aligned."""
    assert nrows > 0 and ncols > 0 and lda >= ncols
    vec2 = ncols % 2 == 0 and lda % 2 == 0 and aligned
    W = gemv_t_W(ncols)
    rpc = gemv_t_rows_per_chunk(nrows, ncols)
    nchunks = ceil_div(nrows, rpc)
    last_rows = nrows - (nchunks - 1) * rpc
    if vec2:
        tile_cols = gemv_t_W2(ncols)
        rstep = GEMVT_THREADS // (tile_cols // 2)
    else:
        tile_cols = W
        rstep = GEMVT_THREADS // W
    chunk_rows = sorted({min(rpc, nrows), last_rows})
    # a thread's rows r0 + rl, r0 + rl + rstep, ...: eight at a time while eight are left, then one at a time
    per_thread = [n for R in chunk_rows for n in _strided_counts(R, rstep)]
    CT = min(W, 64)
    nph = GEMVT2_THREADS // CT
    per_phase = _strided_counts(nchunks, nph)
    return {
        "kernel": "vec2" if vec2 else "scalar", "W": W, "tile_cols": tile_cols, "rstep": rstep, "rpc": rpc,
        "nchunks": nchunks, "last_rows": last_rows, "stage1_tiles": ceil_div(ncols, tile_cols),
        "stage1_main": any(n >= 8 for n in per_thread), "stage1_tail": any(n % 8 for n in per_thread),
        "CT": CT, "nph": nph, "stage2_workgroups": ceil_div(ncols, CT),
        "stage2_main": any(n >= 8 for n in per_phase), "stage2_tail": any(n % 8 for n in per_phase),
        # longest chain of roundings behind one output: the product, a thread's adds, the LDS phases, then stage 2's
        "chain": 1 + max(per_thread) + (rstep - 1) + max(per_phase) + (nph - 1),
        "work_bytes": nchunks * ncols * 8,
    }


GEMVT_BASELINE = [(5000, 16), (3001, 37), (257, 64), (40, 700), (1, 1), (100000, 3)]   # tests/test_gpu_parity.py

# group -> [(nrows, ncols, lda or None for ncols)]
GEMVT_GROUPS = {
    "baseline": [(m, n, None) for m, n in GEMVT_BASELINE],
    "stage2_main": [(14401, 32, None), (14401, 31, None), (7301, 64, None), (7301, 65, None), (7300, 130, None)],
    "stage1_main_16": [(230001, 16, None)],
    "stage1_main_3_4": [(460001, 3, None), (460001, 4, None)],
    "stage1_main_1_2": [(1900001, 1, None), (120001, 2, None)],
    "tile_edges": [(300, 128, None), (300, 129, None), (2000, 258, None), (65, 66, 70)],
    "few_rows_many_columns": [(16, 100001, None), (1, 70001, None), (3, 4097, None)],
}

GEMVT_FORMS = ("plain", "lda_plus_1", "A_off_8", "work_off_8")


def gemv_t_forms(nrows, ncols, lda):
    """[(form, lda, A offset in elements, work offset in elements)]: the four forms of a case; one whose A would not fit
    MAX_BYTES is left out."""
    lda = ncols if lda is None else lda
    out = []
    for form, l, a_off, w_off in (("plain", lda, 0, 0), ("lda_plus_1", lda + 1, 0, 0), ("A_off_8", lda, 1, 0),
                                  ("work_off_8", lda, 0, 1)):
        if (nrows * l + 2 * GUARD + 2) * 8 <= MAX_BYTES:
            out.append((form, l, a_off, w_off))
    return out


def gemv_t_cases():
    """Every (group, nrows, ncols, form, lda, a_off, w_off, dispatch)."""
    out = []
    for group, shapes in GEMVT_GROUPS.items():
        for nrows, ncols, lda in shapes:
            for form, l, a_off, w_off in gemv_t_forms(nrows, ncols, lda):
                out.append((group, nrows, ncols, form, l, a_off, w_off,
                            gemv_t_dispatch(nrows, ncols, l, aligned=(a_off == 0 and w_off == 0))))
    return out


def gemv_t_probe_rows(nrows, ncols, every=True, seed=0):
    """Rows i for the probes x = e_i: both sides of every chunk edge, row 0 and the last row.  every=False keeps the first and
    last eight and a seeded sample of 48 others."""
    rpc = gemv_t_rows_per_chunk(nrows, ncols)
    rows = {0, nrows - 1}
    for k in range(1, ceil_div(nrows, rpc)):
        rows |= {k * rpc - 1, k * rpc}
    rows = np.array(sorted(rows), dtype=np.int64)
    if not every and len(rows) > 64:
        mid = np.random.default_rng(seed).choice(rows[8:-8], size=48, replace=False)
        rows = np.unique(np.concatenate([rows[:8], mid, rows[-8:]]))
    return rows


# ---- A * x: hpcla_gemv_rowmajor_f64 -------------------------------------------------------------------------------------

SKINNY_PASSES = 16
SKINNY_MAX = 128


def skinny_L(ncols):
    L = 1
    while 2 * L < ncols:
        L <<= 1
    return L


def rows_per_wave(ncols):
    return (64 // skinny_L(ncols)) * SKINNY_PASSES


def gemv_dispatch(nrows, ncols, lda, a_off, split, xform):
    """What hpcla_gemv_rowmajor_f64 launches: A starts a_off elements (0 or 1) past a 16-byte boundary, x arrives as
    split = (n_lo, n_own, n_hi); xform "separate" gives every segment a 16-byte aligned buffer of its own, "ghost" puts x_lo
    and x_hi into one buffer, x_hi = ghost + 8 * n_lo."""
    n_lo, n_own, n_hi = split
    assert n_lo + n_own + n_hi == ncols > 0 and nrows > 0 and lda >= ncols and a_off in (0, 1)
    if ncols <= SKINNY_MAX:
        L = skinny_L(ncols)
        vec = lda % 2 == 0 and a_off == 0 and ncols >= 2            # the lanes that hold two columns take 16-byte loads
        return {"kernel": "skinny", "L": L, "rpw": (64 // L) * SKINNY_PASSES, "vec16": vec,
                "chain": 1 + 1 + int(np.log2(L))}                   # product, one add, log2(L) lane steps
    x_elem_off = (0, 0, n_lo % 2 if xform == "ghost" else 0)        # parity of each segment's x pointer
    starts = (0, n_lo, n_lo + n_own)
    paths, chain = set(), 0
    for row in range(min(nrows, 2)):                                # an odd pitch alternates with the row's parity
        adds = 0
        for s, n, xo in zip(starts, split, x_elem_off):
            if n == 0:
                continue
            vec = (a_off + row * lda + s) % 2 == 0 and xo == 0
            paths.add((vec, n % 2))
            adds += 2 * ceil_div(n // 2, 64) + (n % 2) if vec else ceil_div(n, 64)
            adds += 1                                               # acc += seg_dot(...)
        chain = max(chain, 1 + adds + 6)                            # product, a lane's adds, six shuffle steps
    return {"kernel": "rowmajor", "L": None, "rpw": 4, "vec16": None, "seg_paths": paths, "chain": chain}


def segment_splits(n):
    """{name: (n_lo, n_own, n_hi)} for a vector of n elements; a form that n is too short for is left out."""
    odd = lambda v: v if v % 2 else v - 1          # noqa: E731  (largest odd number <= v, v >= 1)
    out = {"all_own": (0, n, 0)}
    if n >= 2:
        out["own_odd_then_rest"] = (0, odd(max(1, n // 2)), n - odd(max(1, n // 2)))
        out["lo_1_own_0"] = (1, 0, n - 1)
        out["own_last_1"] = (n - 1, 1, 0)
    if n >= 3:
        a = odd(max(1, n // 3))
        out["odd_odd_rest"] = (a, a, n - 2 * a)
        out["single_first"] = (1, 1, n - 2)
        out["single_last"] = (n - 2, 1, 1)
    if n >= 4:
        out["edge_inside_pair"] = (3, n - 3, 0)     # between columns 2 and 3: inside the pair (2, 3) that one lane holds
        out["edge_between_pairs"] = (2, n - 2, 0)
    if n >= 7:
        out["even_even_rest"] = (4, 2, n - 6)
    assert all(sum(s) == n and min(s) >= 0 for s in out.values())
    return out


SKINNY_NCOLS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128)
ROWMAJOR_NCOLS = (129, 130, 131, 191, 192, 193, 256, 257, 1025, 4099)
ROWMAJOR_NROWS = (1, 3, 4, 5, 301)
LDA_PADS = (0, 1, 2, 7)
X_FORMS = ("separate", "ghost")
SWEEP_NROWS, SWEEP_NCOLS = 37, tuple(range(1, 131))
SPLITS_PER_BLOCK = 3           # (split, x form) pairs drawn for every (shape, pitch, offset) of A


def skinny_nrows(ncols):
    rpw = rows_per_wave(ncols)
    return (rpw - 1, rpw, rpw + 1, 4 * rpw - 1, 4 * rpw, 4 * rpw + 1, 8 * rpw + 3)


def gemv_shapes(group):
    """group: "skinny_L<L>" for one lane-group width, or "rowmajor"."""
    if group == "rowmajor":
        return [(m, n) for n in ROWMAJOR_NCOLS for m in ROWMAJOR_NROWS]
    L = int(group[len("skinny_L"):])
    return [(m, n) for n in SKINNY_NCOLS if skinny_L(n) == L for m in skinny_nrows(n)]


GEMV_GROUPS = tuple(f"skinny_L{L}" for L in (1, 2, 4, 8, 16, 32, 64)) + ("rowmajor",)


def gemv_cases(group):
    """[(nrows, ncols, lda, a_off, [(split name, split, x form), ...])]: every shape of the group with every pitch and both
    alignments of A; of the splits x forms of each, a seeded sample of SPLITS_PER_BLOCK (the full cross product is some
    20 000 launches).  tests/test_dense_edge_cases.py asserts that every value of every axis still meets every kernel."""
    rng = np.random.default_rng(sum(group.encode()))
    out = []
    for nrows, ncols in gemv_shapes(group):
        splits = segment_splits(ncols)
        pairs = [(name, splits[name], xf) for name in splits for xf in X_FORMS]
        for pad in LDA_PADS:
            for a_off in (0, 1):
                take = rng.choice(len(pairs), size=min(SPLITS_PER_BLOCK, len(pairs)), replace=False)
                out.append((nrows, ncols, ncols + pad, a_off, [pairs[t] for t in sorted(take)]))
    return out


def segment_edges(split):
    """Columns j for the probes x = e_j: first and last of every non-empty segment."""
    edges, s = set(), 0
    for n in split:
        if n:
            edges |= {s, s + n - 1}
        s += n
    return sorted(edges)


# ---- inputs and references ----------------------------------------------------------------------------------------------

def product_inputs(kind, nrows, ncols, nx, seed):
    """(A nrows x ncols, x of nx elements) as float64."""
    rng = np.random.default_rng([seed, nrows, ncols, 0 if kind == "int" else 1])
    if kind == "int":
        return (rng.integers(-8, 9, size=(nrows, ncols)).astype(np.float64), rng.integers(-8, 9, size=nx).astype(np.float64))
    return rng.random((nrows, ncols)) - 0.5, rng.random(nx) - 0.5


def int_terms_are_exact(terms):
    """`terms` products of at most 64 add up below 2^53 in any order."""
    return 64 * terms < 2 ** 53


def ref_int(A, x, transposed):
    """The int64 product of integer-valued A and x, as float64 (exact: see int_terms_are_exact)."""
    Ai, xi = A.astype(np.int64), x.astype(np.int64)
    assert np.array_equal(Ai, A) and np.array_equal(xi, x)
    return (Ai.T @ xi if transposed else Ai @ xi).astype(np.float64)


def ref_longdouble(A, x, transposed):
    """(product, sum |a||x|) accumulated in long double, rounded to float64 once."""
    Al, xl = A.astype(np.longdouble), x.astype(np.longdouble)
    if transposed:
        P = Al * xl[:, None]
        return P.sum(axis=0).astype(np.float64), np.abs(P).sum(axis=0).astype(np.float64)
    P = Al * xl[None, :]
    return P.sum(axis=1).astype(np.float64), np.abs(P).sum(axis=1).astype(np.float64)


def chain_bound(chain):
    """Relative to sum|a||x|, the error of a sum whose longest chain holds `chain` roundings (first order in u)."""
    return chain * UNIT_ROUNDOFF


# ---- layout conversion: hpcla_transpose_f64 / _f32 ----------------------------------------------------------------------

LAYOUT_ROW, LAYOUT_COL = 0, 1
RELAY_ROWS, RELAY_MAXC = 256, 32


def transpose_kernel(rows, cols, ld_src, src_layout, ld_dst, dst_layout):
    narrow = (cols <= RELAY_MAXC and rows >= RELAY_ROWS and src_layout == LAYOUT_COL and dst_layout == LAYOUT_ROW
              and ld_dst == cols and ld_src >= rows)
    return "narrow" if narrow else "generic"


def layout_index(layout, ld, rows, cols):
    """Flat index of every element (i, c) of a rows x cols matrix on leading dimension ld."""
    i, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return i * ld + c if layout == LAYOUT_ROW else i + c * ld


def layout_extent(layout, ld, rows, cols):
    return (rows if layout == LAYOUT_ROW else cols) * ld


def transpose_case(name, rows, cols, src_layout, ld_src, dst_layout, ld_dst, src_len=None, src_off=0, dst_len=None, dst_off=0):
    """A conversion of a rows x cols matrix that starts src_off elements into a source buffer of src_len elements and dst_off
    into a destination of dst_len (default: exactly the extents)."""
    c = dict(name=name, rows=rows, cols=cols, src_layout=src_layout, ld_src=ld_src, dst_layout=dst_layout, ld_dst=ld_dst,
             src_off=src_off, dst_off=dst_off)
    c["src_len"] = src_off + layout_extent(src_layout, ld_src, rows, cols) if src_len is None else src_len
    c["dst_len"] = dst_off + layout_extent(dst_layout, ld_dst, rows, cols) if dst_len is None else dst_len
    c["kernel"] = transpose_kernel(rows, cols, ld_src, src_layout, ld_dst, dst_layout)
    return c


def transpose_buffers(c, dtype):
    """(source buffer, expected destination buffer with GUARD elements of NaN on either side).  The matrix holds
    1, 2, 3, ... (every element distinct, exact in Float32); whatever else the buffers hold is NaN."""
    rows, cols = c["rows"], c["cols"]
    M = (np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) + 1).astype(dtype)
    assert rows * cols < 2 ** 24
    src = np.full(c["src_len"], np.nan, dtype=dtype)
    idx = c["src_off"] + layout_index(c["src_layout"], c["ld_src"], rows, cols)
    assert idx.max(initial=-1) < c["src_len"]
    src[idx] = M
    want = np.full(GUARD + c["dst_len"] + GUARD, np.nan, dtype=dtype)
    idx = c["dst_off"] + layout_index(c["dst_layout"], c["ld_dst"], rows, cols)
    assert idx.max(initial=-1) < c["dst_len"] and len(np.unique(idx)) == idx.size
    want[GUARD + idx] = M
    return src, want


def _ld_of(layout, rows, cols, pad):
    return (cols if layout == LAYOUT_ROW else rows) + pad


GENERIC_SIZES = (1, 31, 32, 33, 64, 65)
NARROW_ROWS = (255, 256, 257, 511, 512, 513, 1000)
NARROW_COLS = (1, 2, 15, 16, 17, 31, 32, 33)
LAYOUT_PAIRS = ((LAYOUT_ROW, LAYOUT_ROW), (LAYOUT_ROW, LAYOUT_COL), (LAYOUT_COL, LAYOUT_ROW), (LAYOUT_COL, LAYOUT_COL))


def transpose_cases(group):
    out = []
    if group == "generic":
        # all four layout pairs (ROW -> ROW and COL -> COL are strided copies), exact and padded leading dimensions
        for sl, dl in LAYOUT_PAIRS:
            for rows in GENERIC_SIZES:
                for cols in GENERIC_SIZES:
                    for sp, dp in ((0, 0), (3, 2)):
                        out.append(transpose_case(f"generic {rows}x{cols} {sl}->{dl} pads {sp},{dp}", rows, cols, sl,
                                                  _ld_of(sl, rows, cols, sp), dl, _ld_of(dl, rows, cols, dp)))
    elif group == "narrow":
        for rows in NARROW_ROWS:
            for cols in NARROW_COLS:
                for ld_src in (rows, rows + 3):
                    for ld_dst in (cols, cols + 1):          # a padded destination leaves the narrow kernel
                        out.append(transpose_case(f"narrow {rows}x{cols} ld_src {ld_src} ld_dst {ld_dst}", rows, cols,
                                                  LAYOUT_COL, ld_src, LAYOUT_ROW, ld_dst))
    elif group == "julia":
        # the SpMM operand: column-major nloc x k -> rows of pitch k + (k & 1)
        for k in (1, 3, 15, 16, 17):
            for nloc in (40, 257, 600):
                out.append(transpose_case(f"operand {nloc}x{k}", nloc, k, LAYOUT_COL, max(nloc, 1), LAYOUT_ROW, k + (k & 1)))
        # own rows lo .. hi-1 of a row-major m x k product -> column-major; the source starts (lo-1)*k elements in
        for m, k, lo, hi in ((40, 3, 6, 30), (300, 17, 4, 290), (64, 1, 2, 64), (50, 15, 2, 40)):
            assert ((lo - 1) * k) % 2 == 1
            out.append(transpose_case(f"own rows {lo}:{hi} of {m}x{k}", hi - lo, k, LAYOUT_ROW, k, LAYOUT_COL, hi - lo,
                                      src_len=m * k, src_off=(lo - 1) * k))
        # block placement, ROW -> ROW: a packed nloc x mq block into columns c0 .. c0+mq-1 of a row-major nloc x m matrix
        for nloc, m, c0, mq in ((37, 21, 5, 7), (300, 64, 33, 31), (5, 3, 1, 1), (65, 40, 7, 33)):
            assert c0 % 2 == 1 and c0 + mq <= m
            out.append(transpose_case(f"place {nloc}x{mq} at column {c0} of {m}", nloc, mq, LAYOUT_ROW, mq, LAYOUT_ROW, m,
                                      dst_len=nloc * m, dst_off=c0))
        # ... and from a strided source: columns of a wider send buffer
        out.append(transpose_case("place 33x9 from pitch 12 at column 3 of 20", 33, 9, LAYOUT_ROW, 12, LAYOUT_ROW, 20,
                                  src_len=33 * 12 + 1, src_off=1, dst_len=33 * 20, dst_off=3))
    else:
        raise KeyError(group)
    return out


TRANSPOSE_GROUPS = ("generic", "narrow", "julia")
