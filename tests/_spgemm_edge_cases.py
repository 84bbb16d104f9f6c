"""Inputs and references for tests/test_gpu_spgemm_edges.py, in plain numpy (no torch, no GPU): rows whose candidate
count ("upper bound", ub) sits on, one below and one above every bin cap of csrc/spgemm.hip, in three accumulation
regimes; rows with far more A entries than products; column ids at the documented 2^58 limit; strided columns; and
product lists for the streaming "mapped" kernel whose entries start, end and continue across its 1024-product passes.
Checked on the CPU by tests/test_spgemm_edge_cases.py, so that a failure on the GPU is the kernel's and not the test's.

A case is a dict: CSR A (a_rowptr, a_col, a_val; a_col indexes the rows of G), CSR G (g_rowptr, g_col int64 GLOBAL
columns ascending and distinct per row, g_val), per A row `ub` (candidate products) and `distinct` (result entries), and
`ncols` (the column space for the C oracle, None where it is too large to allocate)."""
import numpy as np

EPB = 256                      # result entries per workgroup of spgemm_mapped_kernel (csrc/spgemm.hip)
MCHUNK = 1024                  # products that kernel streams per pass (EPB * 4)
BIG_TOP = 2 ** 58 - 1          # the largest column id the numeric kernels document (include/hpcla_rocm.h: "< 2^58")


def order_sensitive(rng, n):
    """Values whose sum depends on the order it is taken in: magnitudes spread over 40 binades."""
    return rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, size=n)


def seq_sum(products):
    """First product assigned, the others added one by one: the reference's accumulation."""
    acc = products[0]
    for p in products[1:]:
        acc = acc + p
    return acc


def run_is_sensitive(products) -> bool:
    """A run of >= 16 products tells the sequential order from the reversed one; of >= 64 also from numpy's pairwise sum."""
    products = np.asarray(products, dtype=np.float64)
    n = len(products)
    if n < 16:
        return True
    fwd = seq_sum(products)
    if fwd == seq_sum(products[::-1]):
        return False
    return n < 64 or fwd != np.sum(products)


# ---- references ------------------------------------------------------------------------------------------------------

def gustavson_ref(a_rowptr, a_col, a_val, g_rowptr, g_col, g_val):
    """C = A * G row by row: k ascending, every product rounded on its own, the first product of a column assigned and
    the later ones added in arrival order.  Needs no array of the column space's size, so it also serves column ids near
    2^58.  Returns (c_rowptr, c_col, c_val) with ascending columns."""
    nrows = len(a_rowptr) - 1
    c_rowptr = np.zeros(nrows + 1, dtype=np.int64)
    cols, vals = [], []
    for i in range(nrows):
        acc = {}
        for p in range(int(a_rowptr[i]), int(a_rowptr[i + 1])):
            k, av = int(a_col[p]), a_val[p]
            for q in range(int(g_rowptr[k]), int(g_rowptr[k + 1])):
                j, prod = int(g_col[q]), g_val[q] * av
                acc[j] = acc[j] + prod if j in acc else prod
        for j in sorted(acc):
            cols.append(j)
            vals.append(acc[j])
        c_rowptr[i + 1] = len(cols)
    return c_rowptr, np.array(cols, dtype=np.int64), np.array(vals, dtype=np.float64)


def mapped_ref(pair_ptr, pairs, a_val, g_val):
    """Entry e = g_val[pairs[t, 1]] * a_val[pairs[t, 0]] for t in [pair_ptr[e], pair_ptr[e + 1]), each product rounded, added
    in list order (np.cumsum is sequential; np.sum and reduceat are pairwise and would not do)."""
    prod = g_val[pairs[:, 1]] * a_val[pairs[:, 0]]
    out = np.zeros(len(pair_ptr) - 1, dtype=np.float64)
    for e in range(len(out)):
        lo, hi = int(pair_ptr[e]), int(pair_ptr[e + 1])
        if hi > lo:
            out[e] = np.cumsum(prod[lo:hi])[-1]
    return out


# ---- row families ----------------------------------------------------------------------------------------------------

def _row_runs(a_vals, g_cols, g_vals):
    """{column: [products in k order]} of one row given per k its A value and G row."""
    runs = {}
    for av, cs, gv in zip(a_vals, g_cols, g_vals):
        for j, v in zip(cs.tolist(), (gv * av).tolist()):
            runs.setdefault(j, []).append(v)
    return runs


def _assemble(rows, seed, ncols):
    """`rows`: per A row the list (k ascending) of its G rows' column arrays (ascending, distinct, possibly empty).  Every
    (row, k) gets a G row of its own, so A's columns are consecutive.  Values are `order_sensitive`; a row is drawn again
    (next seed) until every run of its products is order-sensitive (run_is_sensitive)."""
    a_rowptr, a_val, g_len, g_col, g_val, ub, distinct = [0], [], [], [], [], [], []
    for r, gcols in enumerate(rows):
        gcols = [np.asarray(c, dtype=np.int64) for c in gcols]
        for attempt in range(200):
            rng = np.random.default_rng([seed, r, attempt])
            av = order_sensitive(rng, len(gcols))
            gv = [order_sensitive(rng, len(c)) for c in gcols]
            runs = _row_runs(av, gcols, gv)
            if all(run_is_sensitive(v) for v in runs.values()):
                break
        else:
            raise AssertionError(f"no order-sensitive draw for row {r}")
        a_val.append(av)
        a_rowptr.append(a_rowptr[-1] + len(gcols))
        g_len += [len(c) for c in gcols]
        g_col += gcols
        g_val += gv
        ub.append(sum(len(c) for c in gcols))
        distinct.append(len(runs))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)   # noqa: E731
    nk = a_rowptr[-1]
    return dict(a_rowptr=np.array(a_rowptr, dtype=np.int64), a_col=np.arange(nk, dtype=np.int64),
                a_val=cat(a_val, np.float64), g_rowptr=np.concatenate([[0], np.cumsum(g_len)]).astype(np.int64),
                g_col=cat(g_col, np.int64), g_val=cat(g_val, np.float64), ub=np.array(ub, dtype=np.int64),
                distinct=np.array(distinct, dtype=np.int64), ncols=ncols)


def cap_ubs(caps):
    """The upper bounds of cap_rows: 0, 1, every cap with its two neighbours -- but never a row above the last cap."""
    caps = [int(c) for c in caps]
    s = {0, 1, caps[-1] - 1, caps[-1]}
    for c in caps[:-1]:
        s |= {c - 1, c, c + 1}
    return sorted(s)


def _split(rng, total, longest):
    """`total` as a list of positive lengths <= longest, in random order."""
    parts = []
    while total > 0:
        n = int(min(total, rng.integers(1, longest + 1)))
        parts.append(n)
        total -= n
    return parts


def cap_rows(caps, regime):
    """One row per cap_ubs(caps) value, in a shuffled row order.
    "distinct":    every product has its own column (distinct == ub: at the last cap the 8192-slot table holds 6144 keys,
                   at 384 the 512-slot table 384); G rows of up to 300 entries, their columns interleaved over k.
    "one_column":  every referenced G row is [the same single column]: nk == ub, one result entry, ub products in k order.
    "few_columns": G rows of length 4 over the same 4 columns (one shorter G row, somewhere in the middle, when ub is no
                   multiple of 4): min(ub, 4) result entries fed by about ub / 4 products each."""
    ubs = cap_ubs(caps)
    rng = np.random.default_rng(58)
    order = rng.permutation(len(ubs))
    rows, ncols = [], 0
    for u in (ubs[i] for i in order):
        if regime == "distinct":
            lens = _split(rng, u, 300)
            cols = rng.permutation(3 * u + 7)[:u]
            cuts = np.cumsum([0] + lens)
            rows.append([np.sort(cols[cuts[i]:cuts[i + 1]]) for i in range(len(lens))])
            ncols = max(ncols, 3 * u + 7)
        elif regime == "one_column":
            rows.append([np.array([5])] * u)
            ncols = 9
        elif regime == "few_columns":
            four = np.array([2, 3, 11, 12])
            gc = [four] * (u // 4)
            if u % 4:
                gc.insert(len(gc) // 2, np.sort(rng.permutation(four)[:u % 4]))
            rows.append(gc)
            ncols = 13
        else:
            raise ValueError(regime)
    return _assemble(rows, {"distinct": 1, "one_column": 2, "few_columns": 3}[regime], ncols)


def many_empty_k(caps):
    """Rows with ub in {1, 16, 17, 64} and 65 or 200 A entries: most referenced G rows are empty, and the non-empty ones lie
    scattered among them.  At 16 lanes per row the expand loop of the register kernel runs ceil(200 / 16) = 13 rounds."""
    assert caps[0] == 16 and caps[2] == 64, "written for the 16 / 32 / 64 lane register kernel"
    rng = np.random.default_rng(13)
    rows = []
    for nk in (65, 200):
        for u in (1, 16, 17, 64):
            lens = _split(rng, u, 5)
            pos = np.sort(rng.permutation(nk)[:len(lens)])
            gc = [np.zeros(0, dtype=np.int64)] * nk
            for p, n in zip(pos, lens):
                gc[p] = np.sort(rng.permutation(12)[:n])
            rows.append(gc)
    return _assemble(rows, 4, 12)


def big_columns(caps):
    """One row per bin, at the bin's cap, over 40 % as many columns as products (so columns repeat), its last product in the
    case's largest column jmax; then every column j is mapped through the increasing j -> 2^58 - 1 - (jmax - j), which puts
    the largest at 2^58 - 1 = BIG_TOP: every row's last product slot, slot cap - 1, holds the largest id there is.  The case
    carries the unmapped one under "small" and jmax under "jmax"."""
    rng = np.random.default_rng(58 * 58)
    rows, top = [], (2 * int(caps[-1])) // 5 - 1
    for u in (int(c) for c in caps):
        width = max(2, (2 * u) // 5)
        lens = _split(rng, u, min(width, 70))
        gc = [np.sort(rng.permutation(width)[:n]) for n in lens]
        gc[-1][-1] = top                             # ascending stays ascending: the case's top column closes the row
        rows.append(gc)
    small = _assemble(rows, 5, int(max(c.max() for r in rows for c in r)) + 1)
    jmax = int(small["g_col"].max())
    big = dict(small, g_col=BIG_TOP - (jmax - small["g_col"]), ncols=None, small=small, jmax=jmax)
    return big


def strided_columns(caps):
    """A row at the cap of each hash bin (the last two bins) with distinct columns 4096 * j: the tables as full as they get,
    probed in another pattern than consecutive ids give."""
    rng = np.random.default_rng(4096)
    rows = []
    for u in (int(caps[-2]), int(caps[-1])):
        lens = _split(rng, u, 300)
        cols = 4096 * rng.permutation(2 * u)[:u]
        cuts = np.cumsum([0] + lens)
        rows.append([np.sort(cols[cuts[i]:cuts[i + 1]]) for i in range(len(lens))])
    return _assemble(rows, 6, None)


def bin_rows(caps, b, nrows):
    """`nrows` rows that belong to bin b itself (ub above the previous cap, at most min(cap, 1500)), columns repeating."""
    rng = np.random.default_rng(100 + b)
    lo = int(caps[b - 1]) + 1 if b else 1
    hi = min(int(caps[b]), 1500)
    rows = []
    for _ in range(nrows):
        u = int(rng.integers(lo, hi + 1))
        width = max(3, u // 3)
        rows.append([np.sort(rng.permutation(width)[:n]) for n in _split(rng, u, min(width, 90))])
    return _assemble(rows, 7 + b, max(3, hi // 3))


ROW_FAMILIES = {
    "cap_distinct": lambda caps: cap_rows(caps, "distinct"),
    "cap_one_column": lambda caps: cap_rows(caps, "one_column"),
    "cap_few_columns": lambda caps: cap_rows(caps, "few_columns"),
    "many_empty_k": many_empty_k,
    "big_columns": big_columns,
    "strided_columns": strided_columns,
}


def ub_case(nrows, seed):
    """(a_rowptr, a_col, g_rowptr) for the upper-bound kernel: A rows of 0..6 entries (about a third empty), G rows of 0..9."""
    rng = np.random.default_rng(seed)
    ng = 50
    g_rowptr = np.concatenate([[0], np.cumsum(rng.integers(0, 10, size=ng))]).astype(np.int64)
    lens = rng.integers(1, 7, size=nrows) * (rng.random(nrows) > 0.33)
    lens[nrows // 2] = 6                              # never an A without entries
    a_rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    a_col = np.concatenate([np.sort(rng.permutation(ng)[:n]) for n in lens]).astype(np.int64)
    return a_rowptr, a_col, g_rowptr


# ---- product lists for the mapped kernel -------------------------------------------------------------------------------

def _spread(rng, nent, total):
    """`nent` positive counts that sum to `total`."""
    return 1 + rng.multinomial(total - nent, np.full(nent, 1.0 / nent))


def mapped_lists():
    """(name, counts): counts[e] = number of products of result entry e.  A workgroup owns EPB consecutive entries and
    streams their products MCHUNK at a time, each pass in ceil(n / 256) rounds (mapped_pass<1..4>)."""
    rng = np.random.default_rng(1024)
    out = [(f"ones_{n}", np.ones(n, dtype=np.int64)) for n in (1, 255, 256, 257, 513)]
    for total in (256, 257, 512, 513, 768, 769, 1024, 1025, 2048 + 1, 2048 + 257, 2048 + 513, 2048 + 769):
        out.append((f"block_total_{total}", _spread(rng, EPB, total)))
    # entry 200 ends exactly at product 1024 of its block, entry 201 starts there
    c = np.ones(EPB, dtype=np.int64)
    c[:200] = 5
    c[200], c[201] = 24, 30
    out.append(("ends_and_starts_at_1024", c))
    # entry 100 holds products 1000 .. 3100 of its block: the passes 1024..2048 and 2048..3072 lie wholly inside it
    c = np.ones(EPB, dtype=np.int64)
    c[:98] = 10
    c[98] = 19
    c[100] = 2100
    assert c[:100].sum() == 1000 and c[99] == 1 and c[101] == 1
    out.append(("spans_two_whole_chunks", c))
    out.append(("one_entry_5000", np.array([5000], dtype=np.int64)))
    c = np.ones(EPB + 1, dtype=np.int64)
    c[EPB] = 1500
    out.append(("lone_entry_1500_in_last_block", c))
    return out


def mapped_case(name, counts):
    """Lists for `counts`: random pairs into 3000 A values and 4000 G values (`order_sensitive`); the pairs of an entry
    with 16 products or more are drawn again until its run is order-sensitive.  Returns pair_ptr (int64), pairs (int32
    [n, 2]), a_val, g_val."""
    counts = np.asarray(counts, dtype=np.int64)
    pair_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(pair_ptr[-1])
    rng = np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(name)), total])
    a_val, g_val = order_sensitive(rng, 3000), order_sensitive(rng, 4000)
    pairs = np.stack([rng.integers(0, 3000, size=total), rng.integers(0, 4000, size=total)], axis=1).astype(np.int32)
    for e in np.flatnonzero(counts >= 16):
        lo, hi = int(pair_ptr[e]), int(pair_ptr[e + 1])
        for _ in range(200):
            if run_is_sensitive(g_val[pairs[lo:hi, 1]] * a_val[pairs[lo:hi, 0]]):
                break
            pairs[lo:hi, 0] = rng.integers(0, 3000, size=hi - lo)
            pairs[lo:hi, 1] = rng.integers(0, 4000, size=hi - lo)
        else:
            raise AssertionError(f"no order-sensitive draw for entry {e} of {name}")
    return dict(pair_ptr=pair_ptr, pairs=pairs, a_val=a_val, g_val=g_val)


def block_passes(counts):
    """Per workgroup (EPB entries) the list of its passes' round counts R = ceil(n / 256), n = products in the pass."""
    counts = np.asarray(counts, dtype=np.int64)
    out = []
    for e0 in range(0, len(counts), EPB):
        total = int(counts[e0:e0 + EPB].sum())
        out.append([-(-min(MCHUNK, total - c) // 256) for c in range(0, total, MCHUNK)])
    return out
