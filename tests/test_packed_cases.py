"""CPU checks of what tests/test_gpu_packed_edges.py and tests/_multirank_packed_worker.py feed the GPU: every generator of
tests/_packed_cases.py has the properties its name claims (asserted on rowptr / col / vals), the geometry constants are the
ones csrc/packed.hip is compiled with, ``packed_walk`` -- the numpy restatement of the kernel's pass loop -- gives the
oracle's bits on every eligible case and under block lists, and each deliberate slip of the walk changes those bits."""
import os
import re
import sys
from functools import lru_cache

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _packed_cases as pc  # noqa: E402
from _packed_cases import CHUNK, HI, LO, OCTET, RPB, eligible_np  # noqa: E402


@lru_cache(maxsize=None)
def case(name, *args):
    out = getattr(pc, name)(*args)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _check_csr(rowptr, col, vals, ncols):
    n = len(rowptr) - 1
    assert rowptr.dtype == col.dtype == np.int64 and vals.dtype == np.float64
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(vals) and np.all(np.diff(rowptr) >= 0)
    assert col.min() >= 0 and col.max() < ncols and np.all(np.isfinite(vals)) and np.all(vals != 0)
    inner = np.ones(len(col), dtype=bool)
    inner[rowptr[:-1][np.diff(rowptr) > 0]] = False                      # first entry of each non-empty row
    assert np.all(np.diff(col)[inner[1:]] > 0), "columns ascend within every row"
    return n


def _x(orc, n):
    return orc.fill_uniform(0, n, orc.SEED_X) - 0.5


def _oracle(orc, rowptr, col, vals, x):
    return orc.spmv(rowptr.astype(np.int32), col.astype(np.int32), vals, x)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


# ---- the constants are the kernel's ------------------------------------------------------------------------------------------
def test_constants_are_the_ones_in_the_source():
    text = open(os.path.join(ROOT, "linearalgebrampi.jl_amd", "csrc", "packed.hip")).read()
    assert int(re.search(r"constexpr int P_RPB = (\d+);", text).group(1)) == RPB == pc.RPB == 256
    assert int(re.search(r"constexpr int P_CHUNK = P_RPB \* (\d+);", text).group(1)) == OCTET
    assert CHUNK == RPB * OCTET == 2048
    assert re.search(r"const int64_t pa = p0 & ~\(int64_t\)(\d+);", text).group(1) == str(OCTET - 1)
    assert re.search(r"const int e0 = tid \* (\d+);", text).group(1) == str(OCTET)
    shift = re.search(r"std::min<int64_t>\(nnz, 1 << (\d+)\)", text).group(1)
    assert 1 << int(shift) == pc.SEED_SAMPLE == 65536
    assert int(re.search(r"const int CAP = (\d+);", text).group(1)) == pc.MISS_CAP
    assert int(re.search(r"dict\.size\(\) > (\d+)", text).group(1)) == pc.MAX_DICT
    assert "const short *__restrict__ dcol" in text and (LO, HI) == (np.iinfo(np.int16).min, np.iinfo(np.int16).max)
    # the lines the slips of packed_walk stand for are still there
    for needle in ("double acc = 0.0;", "const int64_t g = pa + c + e0;", "block_list ? (int64_t)block_list[blockIdx.x]",
                   "& 0xff]", "int64_t idx = r0 + (int)dc[k];", "lo = (int)((int64_t)rowptr[r0 + tid] - base - pa);",
                   "const int a = lo > c ? lo : (int)c;", "const int e = hi < c + n ? hi : (int)(c + n);"):
        assert needle in text, needle


# ---- stencils ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dims,per_row,passes,kinds", [("stencil9", (40, 40), 9, 2, 3), ("stencil27", (12, 12, 12), 27, 4, 4)])
def test_stencils(orc, name, dims, per_row, passes, kinds):
    rowptr, col, vals = case(name, *dims)
    n = _check_csr(rowptr, col, vals, int(np.prod(dims)))
    assert n == int(np.prod(dims)) and n // RPB >= 6 and n % RPB != 0          # several full blocks and a ragged one
    assert np.all(np.diff(rowptr) == per_row)
    for b in range(n // RPB):
        p0, p1, pa, total = pc.block_span(rowptr, b)
        assert p1 - p0 == RPB * per_row == {9: 2304, 27: 6912}[per_row] and pc.n_passes(rowptr, b) == passes
    assert len(pc.bit_patterns(vals)) == kinds and eligible_np(rowptr, col, n)
    # symmetric with zero row sums off the palette: the centre value once per row
    centre = {9: pc.PAL9, 27: pc.PAL27}[per_row][0]
    assert np.all(vals[col == np.repeat(np.arange(n), per_row)] == centre)
    x = _x(orc, n)
    want = _oracle(orc, rowptr, col, vals, x)
    assert _same_bits(pc.packed_walk(rowptr, col, vals, x), want)
    # a row range of it is that range of the whole
    a, b = 300, 901
    rp, cl, vl = getattr(pc, name)(*dims, a, b)
    assert np.array_equal(rp, rowptr[a:b + 1] - rowptr[a]) and np.array_equal(cl, col[rowptr[a]:rowptr[b]])
    assert np.array_equal(vl, vals[rowptr[a]:rowptr[b]])


# ---- pass edges ----------------------------------------------------------------------------------------------------------------
def _rel(rowptr, b):
    """(lo, hi) of the rows of block b relative to its octet-aligned start, and the block's total from there."""
    n = len(rowptr) - 1
    r0, r1 = RPB * b, min(RPB * b + RPB, n)
    p0, p1, pa, total = pc.block_span(rowptr, b)
    return rowptr[r0:r1] - pa, rowptr[r0 + 1:r1 + 1] - pa, total


def test_pass_edges_properties():
    rowptr, col, vals, info = case("pass_edges")
    n = _check_csr(rowptr, col, vals, len(rowptr) - 1)
    nb = pc.n_blocks(n)
    assert 12 <= nb <= 40 and eligible_np(rowptr, col, n)
    assert 3 <= len(pc.bit_patterns(vals)) <= 8
    # every total at every offset, counted from the octet-aligned start
    for m in pc.PASS_OFFSETS:
        for total in pc.PASS_TOTALS:
            b = info[(total, m)]
            p0, p1, pa, t = pc.block_span(rowptr, b)
            assert p0 % OCTET == m and t == total and p1 - p0 == total - m
            assert pc.n_passes(rowptr, b) == {2047: 1, 2048: 1, 2049: 2, 4096: 2, 4097: 3}[total]
    found = {k: [] for k in ("ends_on", "begins_on", "empty_on", "straddles")}
    for b in range(nb):
        lo, hi, total = _rel(rowptr, b)
        for k in range(1, (total + CHUNK - 1) // CHUNK + 1):
            edge = k * CHUNK
            found["ends_on"] += [b] if np.any((hi == edge) & (lo < hi)) else []
            found["begins_on"] += [b] if np.any((lo == edge) & (lo < hi)) else []
            found["empty_on"] += [b] if np.any((lo == edge) & (hi == edge)) else []
            found["straddles"] += [b] if np.any((lo == edge - 1) & (hi == edge + 1)) else []
    for m in pc.PASS_OFFSETS:
        b = info[(4096, m)]
        assert b in found["ends_on"] and b in found["begins_on"] and b in found["empty_on"]
        assert info[(2049, m)] in found["straddles"] and info[(4097, m)] in found["straddles"]
        lo, hi, total = _rel(rowptr, info[(2048, m)])
        assert hi[-1] == CHUNK == total                                       # the block itself ends on the boundary
        lo, hi, total = _rel(rowptr, info[(4097, m)])
        assert np.any((lo == 2 * CHUNK - 1) & (hi == 2 * CHUNK + 1))          # ... the SECOND boundary straddled
    # rows longer than a whole pass: begin in pass 0, end in pass 2; first lane and last lane of a block
    for key, lane in (("long_first", 0), ("long_last", RPB - 1)):
        lo, hi, total = _rel(rowptr, info[key])
        assert hi[lane] - lo[lane] == pc.LONG > 2 * CHUNK and lo[lane] < CHUNK and 2 * CHUNK < hi[lane] <= 3 * CHUNK
        assert np.all(np.delete(hi - lo, lane) < 64)
    assert _rel(rowptr, info["long_first"])[0][0] % OCTET == 3 and rowptr[RPB * info["long_last"]] % OCTET == 7
    # a block of empty rows between two full ones
    e = info["empty_between"]
    assert pc.block_span(rowptr, e)[1] == pc.block_span(rowptr, e)[0]
    assert np.all(np.diff(rowptr)[RPB * (e - 1):RPB * e] >= 7) and np.all(np.diff(rowptr)[RPB * (e + 1):RPB * (e + 2)] >= 7)
    # ragged last block: 100 rows (waves 2 and 3 hold no row), two passes, not octet-aligned
    assert info["ragged"] == nb - 1 and n - RPB * (nb - 1) == 100 <= 2 * 64
    assert pc.n_passes(rowptr, nb - 1) == 2 and rowptr[RPB * (nb - 1)] % OCTET == 3
    assert 90_000 > len(col) > 50_000


def test_pass_edges_walk_and_block_lists(orc):
    rowptr, col, vals, info = case("pass_edges")
    n = len(rowptr) - 1
    x = _x(orc, n)
    want = _oracle(orc, rowptr, col, vals, x)
    assert _same_bits(pc.packed_walk(rowptr, col, vals, x), want)
    nb = pc.n_blocks(n)
    for blocks in (pc.skip_every_third(nb), pc.skip_every_third(nb)[::-1], pc.shuffled(nb)):
        assert 0 < len(blocks) <= nb and len(set(blocks)) == len(blocks)
        got = pc.packed_walk(rowptr, col, vals, x, blocks=blocks, sentinel=-7.0)
        listed = np.isin(np.arange(n) // RPB, blocks)
        assert _same_bits(got[listed], want[listed]) and np.all(got[~listed] == -7.0)
    assert pc.skip_every_third(nb) == [b for b in range(nb) if b % 3 != 2] and nb > 6
    assert np.any(np.diff(pc.shuffled(nb)) < 0) and sorted(pc.shuffled(nb)) == list(range(nb))    # the ragged block among them


# ---- window ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["edges", "past_low", "past_high", "ghost"])
def test_window_edges(orc, which):
    rowptr, col, vals, n_own, bad_block = case("window_edges", which)
    n = _check_csr(rowptr, col, vals, n_own + 1)
    assert n == n_own == 70_000 and len(pc.bit_patterns(vals)) == 5
    assert bad_block == (None if which == "edges" else pc.n_blocks(n) - 1 if which == "ghost" else 129)
    r0 = 128 * RPB
    seg = col[rowptr[r0]:rowptr[r0 + RPB]] - r0
    assert seg.min() == LO and seg.max() == HI                                 # both extremes in one block ...
    row = col[rowptr[r0 + 77]:rowptr[r0 + 78]] - r0
    assert row.min() == LO and row.max() == HI                                 # ... and in one row
    assert eligible_np(rowptr, col, n_own) == (which == "edges")
    x = _x(orc, n_own + 1)                                                     # one more for the oracle's read of the ghost
    want = _oracle(orc, rowptr, col, vals, x)
    if which == "edges":
        assert _same_bits(pc.packed_walk(rowptr, col, vals, x[:n_own]), want)
        return
    others = [b for b in range(pc.n_blocks(n)) if b != bad_block]
    assert eligible_np(rowptr, col, n_own, blocks=others) and not eligible_np(rowptr, col, n_own, blocks=[bad_block])
    bad = col[rowptr[RPB * bad_block]:rowptr[min(RPB * bad_block + RPB, n)]] - RPB * bad_block
    if which == "past_low":
        assert bad.min() == LO - 1 and bad.max() <= HI and col.max() < n_own
    elif which == "past_high":
        assert bad.max() == HI + 1 and bad.min() >= LO and col.max() < n_own
    else:                                                                      # inside the window, not owned: that rule alone
        assert (col >= n_own).sum() == 1 and bad.max() == n_own - RPB * bad_block <= HI and bad.min() >= LO
    got = pc.packed_walk(rowptr, col, vals, x[:n_own], n_own=n_own, blocks=others)
    listed = np.arange(n) // RPB != bad_block
    assert _same_bits(got[listed], want[listed]) and np.all(np.isnan(got[~listed]))


# ---- octets shared with the neighbouring blocks -----------------------------------------------------------------------------
def test_neighbour_octets(orc):
    rowptr, col, vals, listed = case("neighbour_octets")
    n = _check_csr(rowptr, col, vals, len(rowptr) - 1)
    nb = pc.n_blocks(n)
    assert n == nb * RPB and eligible_np(rowptr, col, n)
    assert not np.any(col == 0) and not np.any(col == n - 1)                   # no row stores either clamp target
    for b in range(nb):
        p0, p1, pa, total = pc.block_span(rowptr, b)
        r0 = RPB * b
        if b > 0:
            assert p0 % OCTET != 0
            foreign = col[pa:p0] - (r0 - RPB)                                   # the previous block's deltas ...
            assert len(foreign) and np.all(r0 + foreign >= n)                   # ... read with this block's base
        if b < nb - 1:
            assert p1 % OCTET != 0
            foreign = col[p1:(p1 + OCTET - 1) // OCTET * OCTET] - (r0 + RPB)
            assert len(foreign) and np.all(r0 + foreign < 0)
    assert listed == [1, 3, 5] and all(0 < b for b in listed) and any(b < nb - 1 for b in listed)
    x = _x(orc, n)
    x[0] = x[n - 1] = np.nan
    want = _oracle(orc, rowptr, col, vals, x)
    assert np.all(np.isfinite(want))
    assert _same_bits(pc.packed_walk(rowptr, col, vals, x), want)
    got = pc.packed_walk(rowptr, col, vals, x, blocks=listed, sentinel=-7.0)
    on = np.isin(np.arange(n) // RPB, listed)
    assert _same_bits(got[on], want[on]) and np.all(got[~on] == -7.0)
    assert not np.all(np.isfinite(pc.packed_walk(rowptr, col, vals, x, slip="lane0_from_pa")))


# ---- dictionary -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one", "full", "over", "flood", "rounds"])
def test_dictionary(orc, kind):
    rowptr, col, vals, nd = case("dictionary", kind)
    n = _check_csr(rowptr, col, vals, len(rowptr) - 1)
    nnz = len(col)
    assert eligible_np(rowptr, col, n) and 100_000 <= nnz <= 130_000 and nnz > pc.SEED_SAMPLE + 10 * pc.MISS_CAP
    assert all(pc.n_passes(rowptr, b) == 2 and rowptr[RPB * b] % OCTET == 0 for b in range(pc.n_blocks(n)))
    distinct = len(pc.bit_patterns(vals))
    head, tail = vals[:pc.SEED_SAMPLE], vals[pc.SEED_SAMPLE:]
    missed = ~np.isin(tail.view(np.int64), pc.bit_patterns(head))              # what the first encode round cannot find
    if kind == "one":
        assert distinct == nd == 1
    elif kind == "full":
        assert distinct == nd == 256 == len(pc.bit_patterns(head))
        at = np.flatnonzero(vals == vals.max()) % (RPB * pc.DICT_BAND)         # code 255 = the largest value
        assert np.any(at >= CHUNK) and np.any(at < CHUNK)
    elif kind == "over":
        assert distinct == 257 and nd is None and len(pc.bit_patterns(head)) == 256
        assert missed.sum() == 5000 > pc.MISS_CAP and len(pc.bit_patterns(tail[missed])) == 1
    elif kind == "flood":
        assert distinct == nd == 4 and len(pc.bit_patterns(head)) == 1
        assert missed.all() and len(tail) > 10 * pc.MISS_CAP and len(pc.bit_patterns(tail)) == 3
    elif kind == "rounds":
        assert distinct == nd == 203 and len(pc.bit_patterns(head)) == 3 and missed.all()
        _, counts = np.unique(tail, return_counts=True)
        assert len(counts) == pc.ROUNDS_LATE and 250 <= counts.min() and counts.max() <= 350
        # equal values lie in one run each: the first MISS_CAP misses in stored order name only a few of them
        assert np.count_nonzero(np.diff(tail)) == pc.ROUNDS_LATE - 1
        # every round of at most MISS_CAP listed misses names at least 11 new values: far fewer than 64 rounds
        assert -(-pc.ROUNDS_LATE // (pc.MISS_CAP // counts.max())) < 32
    if nd is None:
        with pytest.raises(AssertionError):
            pc.encode(rowptr, col, vals)
        return
    x = _x(orc, n)
    assert _same_bits(pc.packed_walk(rowptr, col, vals, x), _oracle(orc, rowptr, col, vals, x))


def test_rectangular(orc):
    rowptr, col, vals, ncols = case("rectangular")
    n = _check_csr(rowptr, col, vals, ncols)
    assert ncols > n and n % RPB != 0 and col.max() >= n and eligible_np(rowptr, col, ncols)
    assert all(pc.n_passes(rowptr, b) == 2 for b in range(n // RPB))
    x = _x(orc, ncols)
    assert _same_bits(pc.packed_walk(rowptr, col, vals, x, n_own=ncols), _oracle(orc, rowptr, col, vals, x))


# ---- each slip of the walk changes the bits of the case that is there for it ---------------------------------------------------
@pytest.mark.parametrize("slip,name,args,listed", [
    ("no_carry", "pass_edges", (), False), ("no_carry", "stencil9", (40, 40), False), ("no_carry", "stencil27", (12, 12, 12), False),
    ("p0_origin", "pass_edges", (), False),
    ("grid_index", "pass_edges", (), True),
    ("lane0_from_pa", "neighbour_octets", (), False),
    ("code7", "dictionary", ("full",), False),
    ("unsigned_delta", "window_edges", ("edges",), False),
])
def test_a_slip_in_the_walk_is_seen(orc, slip, name, args, listed):
    rowptr, col, vals = case(name, *args)[:3]
    n = len(rowptr) - 1
    x = _x(orc, n)
    want = _oracle(orc, rowptr, col, vals, x)
    blocks = pc.skip_every_third(pc.n_blocks(n)) if listed else None
    on = np.ones(n, dtype=bool) if blocks is None else np.isin(np.arange(n) // RPB, blocks)
    assert _same_bits(pc.packed_walk(rowptr, col, vals, x, blocks=blocks)[on], want[on])
    bad = pc.packed_walk(rowptr, col, vals, x, blocks=blocks, slip=slip)
    wrong = np.flatnonzero(bad[on].view(np.int64) != want[on].view(np.int64))
    assert len(wrong) > 0, f"{slip} ({pc.SLIPS[slip]}) goes unnoticed on {name}{args}"


def test_every_slip_has_a_case():
    marks = [m for m in test_a_slip_in_the_walk_is_seen.pytestmark if m.name == "parametrize"]
    assert {p[0] for p in marks[0].args[1]} == set(pc.SLIPS)
