"""CPU checks of what tests/test_gpu_spgemm_edges.py feeds the GPU: the generated matrices are well-formed CSR with the upper
bounds and distinct-column counts their names claim, both references (the dict-based Gustavson loop and the C oracle) agree
bit for bit, the product-list reference is the plain loop, every long run of products tells the reference's order from
another one, and the product lists reach every branch of the streaming kernel that they are meant to reach."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _spgemm_edge_cases import (BIG_TOP, EPB, MCHUNK, ROW_FAMILIES, bin_rows, block_passes, cap_ubs, gustavson_ref,  # noqa: E402
                                mapped_case, mapped_lists, mapped_ref, order_sensitive, seq_sum, ub_case)


@pytest.fixture(scope="module")
def caps(hp):
    """The bin caps are the library's to define (a host function: no device is touched)."""
    lib = hp._capi.load()
    out = []
    while lib.hpcla_spgemm_bin_cap(len(out)) >= 0:
        out.append(int(lib.hpcla_spgemm_bin_cap(len(out))))
    assert len(out) == 5 and out == sorted(set(out)) and lib.hpcla_spgemm_bin_cap(-1) == -1
    return tuple(out)


@pytest.fixture(scope="module")
def families(caps):
    return {name: make(caps) for name, make in ROW_FAMILIES.items()}


@pytest.fixture(scope="module")
def refs(families):
    return {name: gustavson_ref(c["a_rowptr"], c["a_col"], c["a_val"], c["g_rowptr"], c["g_col"], c["g_val"])
            for name, c in families.items()}


def _row_products(c, i):
    """{column: products in k order} of row i, written without the generator's helpers."""
    runs = {}
    for p in range(c["a_rowptr"][i], c["a_rowptr"][i + 1]):
        k = c["a_col"][p]
        for q in range(c["g_rowptr"][k], c["g_rowptr"][k + 1]):
            runs.setdefault(int(c["g_col"][q]), []).append(c["g_val"][q] * c["a_val"][p])
    return runs


def _check_case(c, top, caps):
    nrows, ng = len(c["a_rowptr"]) - 1, len(c["g_rowptr"]) - 1
    for rp, col, val in ((c["a_rowptr"], c["a_col"], c["a_val"]), (c["g_rowptr"], c["g_col"], c["g_val"])):
        assert rp.dtype == col.dtype == np.int64 and val.dtype == np.float64
        assert rp[0] == 0 and rp[-1] == len(col) == len(val) and np.all(np.diff(rp) >= 0)
        assert np.all(np.isfinite(val)) and np.all(val != 0)
        for r in range(len(rp) - 1):
            assert np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0)          # ascending and distinct
    assert len(c["a_col"]) > 0 and c["a_col"].min() >= 0 and c["a_col"].max() < ng
    assert c["g_col"].min() >= 0 and c["g_col"].max() <= top
    glen = np.diff(c["g_rowptr"])
    for i in range(nrows):
        ks = c["a_col"][c["a_rowptr"][i]:c["a_rowptr"][i + 1]]
        assert c["ub"][i] == glen[ks].sum()
        assert c["distinct"][i] == len(_row_products(c, i))
    assert c["ub"].max() <= caps[-1], "a row above the last cap never terminates in the hash kernel"


@pytest.mark.parametrize("name", list(ROW_FAMILIES))
def test_family_is_well_formed(families, caps, name):
    c = families[name]
    _check_case(c, BIG_TOP if c["ncols"] is None else c["ncols"] - 1, caps)


@pytest.mark.parametrize("regime", ["distinct", "one_column", "few_columns"])
def test_cap_rows_sit_on_the_caps(families, caps, regime):
    c = families["cap_" + regime]
    want = {0, 1, caps[-1] - 1, caps[-1]}
    for cap in caps[:-1]:
        want |= {cap - 1, cap, cap + 1}
    assert sorted(want) == cap_ubs(caps) and sorted(c["ub"].tolist()) == sorted(want)
    assert caps[-1] + 1 not in want
    nk = np.diff(c["a_rowptr"])
    glen = np.diff(c["g_rowptr"])
    if regime == "distinct":
        np.testing.assert_array_equal(c["distinct"], c["ub"])
        assert glen.max() > 256                                        # a G row longer than a workgroup has lanes
    elif regime == "one_column":
        np.testing.assert_array_equal(nk, c["ub"])
        np.testing.assert_array_equal(c["distinct"], np.minimum(c["ub"], 1))
        assert np.all(glen == 1) and len(np.unique(c["g_col"])) == 1
    else:
        np.testing.assert_array_equal(c["distinct"], np.minimum(c["ub"], 4))
        assert len(np.unique(c["g_col"])) == 4 and glen.max() == 4
        assert np.all((glen == 4).sum() >= (c["ub"] // 4).sum())
    assert np.any(np.diff(c["ub"]) < 0) and np.any(np.diff(c["ub"]) > 0)   # neither ascending nor descending


def test_many_empty_k(families, caps):
    c = families["many_empty_k"]
    nk = np.diff(c["a_rowptr"])
    assert sorted(zip(nk.tolist(), c["ub"].tolist())) == sorted((n, u) for n in (65, 200) for u in (1, 16, 17, 64))
    assert -(-200 // caps[0]) == 13
    glen = np.diff(c["g_rowptr"])
    for i in range(len(nk)):
        full = glen[c["a_col"][c["a_rowptr"][i]:c["a_rowptr"][i + 1]]] > 0
        if full.sum() > 1:                                             # empty G rows BETWEEN the non-empty ones
            first, last = np.flatnonzero(full)[[0, -1]]
            assert not full[first:last].all()
    assert np.any(c["distinct"] < c["ub"])


def test_big_columns(families, refs, caps):
    c = families["big_columns"]
    small = c["small"]
    np.testing.assert_array_equal(c["ub"], caps)
    assert c["g_col"].max() == BIG_TOP == 2 ** 58 - 1 and c["g_col"].min() == BIG_TOP - c["jmax"]
    np.testing.assert_array_equal(np.argsort(c["g_col"], kind="stable"), np.argsort(small["g_col"], kind="stable"))
    for i in range(len(caps)):                                         # the row's LAST product is in the top column
        k = c["a_col"][c["a_rowptr"][i + 1] - 1]
        assert c["g_col"][c["g_rowptr"][k + 1] - 1] == BIG_TOP
    assert np.all(c["distinct"] < c["ub"])
    rp, col, val = refs["big_columns"]
    rp_s, col_s, val_s = gustavson_ref(small["a_rowptr"], small["a_col"], small["a_val"], small["g_rowptr"], small["g_col"],
                                       small["g_val"])
    np.testing.assert_array_equal(rp, rp_s)
    np.testing.assert_array_equal(col, BIG_TOP - (c["jmax"] - col_s))
    np.testing.assert_array_equal(val.view(np.uint64), val_s.view(np.uint64))


def test_strided_columns(families, caps):
    c = families["strided_columns"]
    np.testing.assert_array_equal(c["ub"], caps[-2:])
    np.testing.assert_array_equal(c["distinct"], c["ub"])
    assert np.all(c["g_col"] % 4096 == 0)


def test_bin_rows_belong_to_their_bin(caps):
    for b in range(len(caps)):
        c = bin_rows(caps, b, 17)
        _check_case(c, c["ncols"] - 1, caps)
        assert len(c["ub"]) == 17 and c["ub"].max() <= caps[b] and c["ub"].min() > (caps[b - 1] if b else 0)
        assert np.any(c["distinct"] < c["ub"])


def test_gustavson_ref_equals_the_oracle(orc, families, refs, caps):
    cases = [(n, c) for n, c in families.items() if c["ncols"] is not None]
    cases += [("big_columns.small", families["big_columns"]["small"])] + [(f"bin_rows_{b}", bin_rows(caps, b, 17))
                                                                        for b in range(len(caps))]
    assert len(cases) >= 4 + 1 + len(caps)
    for name, c in cases:
        args = (c["a_rowptr"], c["a_col"], c["a_val"], c["g_rowptr"], c["g_col"], c["g_val"])
        rp, col, val = refs[name] if name in refs else gustavson_ref(*args)
        w_rp, w_col, w_val = orc.spgemm(*args, c["ncols"])
        np.testing.assert_array_equal(rp, w_rp, err_msg=name)
        np.testing.assert_array_equal(col, w_col, err_msg=name)
        np.testing.assert_array_equal(val.view(np.uint64), w_val.view(np.uint64), err_msg=name)
        np.testing.assert_array_equal(np.diff(rp), c["distinct"], err_msg=name)


def test_mapped_ref_is_the_plain_loop():
    for name, counts in mapped_lists():
        m = mapped_case(name, counts)
        got = mapped_ref(m["pair_ptr"], m["pairs"], m["a_val"], m["g_val"])
        for e in range(len(counts)):
            acc = None
            for t in range(m["pair_ptr"][e], m["pair_ptr"][e + 1]):
                prod = m["g_val"][m["pairs"][t, 1]] * m["a_val"][m["pairs"][t, 0]]
                acc = prod if acc is None else acc + prod
            assert got[e] == acc, (name, e)


def _assert_discriminates(products, what):
    products = np.asarray(products, dtype=np.float64)
    fwd = seq_sum(products)
    assert fwd != seq_sum(products[::-1]), f"{what}: {len(products)} products sum to the same bits backwards"
    if len(products) >= 64:
        assert fwd != np.sum(products), f"{what}: {len(products)} products sum to the same bits pairwise"


def test_long_runs_tell_the_order(families, caps):
    """A kernel that added a run of 16 products or more in another order than the reference's would give other bits."""
    n_runs = 0
    cases = list(families.items()) + [(f"bin_rows_{b}", bin_rows(caps, b, 17)) for b in range(len(caps))]
    for name, c in cases:
        for i in range(len(c["ub"])):
            for j, run in _row_products(c, i).items():
                if len(run) >= 16:
                    _assert_discriminates(run, f"{name} row {i} column {j}")
                    n_runs += 1
    # every one_column row from ub = 16 on, four runs in every few_columns row from ub = 64 on
    ubs = np.array(cap_ubs(caps))
    assert n_runs >= (ubs >= 16).sum() + 4 * (ubs >= 64).sum()
    n_runs = 0
    for name, counts in mapped_lists():
        m = mapped_case(name, counts)
        prod = m["g_val"][m["pairs"][:, 1]] * m["a_val"][m["pairs"][:, 0]]
        for e in np.flatnonzero(np.asarray(counts) >= 16):
            _assert_discriminates(prod[m["pair_ptr"][e]:m["pair_ptr"][e + 1]], f"{name} entry {e}")
            n_runs += 1
    assert n_runs >= 5


def test_order_sensitive_values_are_what_the_name_says(caps):
    """The measured rates behind the choice of values: sequential and reversed sums differ in most draws of 16 products and in
    every draw of a cap's worth."""
    rng = np.random.default_rng(0)
    differ = {n: sum(seq_sum(v) != seq_sum(v[::-1]) for v in (order_sensitive(rng, n) for _ in range(50)))
              for n in (16, 64, caps[-1])}
    assert differ[16] >= 25 and differ[64] >= 35 and differ[caps[-1]] == 50, differ


def test_mapped_lists_reach_every_branch():
    """mapped_pass<R> for R = 1..4 as a block's first pass and as its last; an entry that continues across a pass boundary,
    one that starts on a boundary and one that ends on it; trailing blocks of one entry; more than two passes."""
    assert (EPB, MCHUNK) == (256, 1024)
    lists = mapped_lists()
    first, last, nchunks = set(), set(), set()
    crosses = starts = ends = 0
    for name, counts in lists:
        counts = np.asarray(counts)
        assert counts.min() >= 1
        ptr = np.concatenate([[0], np.cumsum(counts)])
        for blk, passes in enumerate(block_passes(counts)):
            first.add(passes[0])
            last.add(passes[-1])
            nchunks.add(len(passes))
            e0, e1 = blk * EPB, min((blk + 1) * EPB, len(counts))
            p0, p1 = ptr[e0], ptr[e1]
            assert sum(passes) >= -(-(p1 - p0) // 256)
            for b in range(p0 + MCHUNK, p1, MCHUNK):                   # boundaries between two passes of this block
                lo, hi = ptr[e0:e1], ptr[e0 + 1:e1 + 1]
                crosses += int(((lo < b) & (b < hi)).sum())
                starts += int((lo == b).sum())
                ends += int((hi == b).sum())
    assert first == {1, 2, 3, 4} and last == {1, 2, 3, 4}, (first, last)
    assert crosses >= 1 and starts >= 1 and ends >= 1
    assert {1, 2, 3} <= nchunks and max(nchunks) >= 5
    names = dict(lists)
    assert {len(names[f"ones_{n}"]) for n in (1, 255, 256, 257, 513)} == {1, 255, 256, 257, 513}
    assert {int(names[f"block_total_{t}"].sum()) for t in (256, 257, 512, 513, 768, 769, 1024, 1025, 2049, 2305, 2561, 2817)} \
        == {256, 257, 512, 513, 768, 769, 1024, 1025, 2049, 2305, 2561, 2817}
    c = names["ends_and_starts_at_1024"]
    assert np.cumsum(c)[200] == MCHUNK and c[201] > 1
    c = names["spans_two_whole_chunks"]
    assert (np.cumsum(c)[99], np.cumsum(c)[100]) == (1000, 3100) and c[99] == c[101] == 1
    assert names["one_entry_5000"].tolist() == [5000]
    c = names["lone_entry_1500_in_last_block"]
    assert len(c) == EPB + 1 and c[EPB] == 1500 and np.all(c[:EPB] == 1)


@pytest.mark.parametrize("nrows", [1, 255, 256, 257])
def test_ub_case(nrows):
    a_rowptr, a_col, g_rowptr = ub_case(nrows, nrows)
    assert len(a_rowptr) == nrows + 1 and a_rowptr[-1] == len(a_col) > 0
    assert a_col.min() >= 0 and a_col.max() < len(g_rowptr) - 1
    if nrows > 1:
        assert np.any(np.diff(a_rowptr) == 0) and np.any(np.diff(g_rowptr) == 0)
