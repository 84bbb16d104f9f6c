"""CPU half of the index-set selection tests: the loop restatement of tests/_select_cases.py against scipy's own fancy
indexing, the per-rank results stitched back into the global selection for 1, 2 and 3 simulated ranks, the argument rules
that need no device, and the C ABI table against the header.  No tolerance anywhere: the operation moves bits."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import _select_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy(A):
    return sp.csr_matrix((A.data, A.indices, A.indptr), shape=A.shape)


def test_the_matrices_hold_what_the_cases_need():
    A = sc.matrix("edge")
    inside = sc.subset()
    lens = np.diff(A.indptr)
    kept = np.array([np.isin(A.indices[A.indptr[r]:A.indptr[r + 1]], inside).sum() for r in range(A.shape[0])])
    for k, L in enumerate(sc.EDGE_LENGTHS):
        assert kept[2 * k] == L and lens[2 * k] == L + sc.EDGE_OUTSIDE            # exact under a subset map
        assert lens[2 * k + 1] == L                                                # exact under a full map
    assert lens[1] == 0 and kept[0] == 0 and lens[0] > 0                           # a row without entries, a row all dropped
    assert {0, 1, sc.SHORT_CAP - 1, sc.SHORT_CAP, sc.SHORT_CAP + 1, sc.TILE - 1, sc.TILE, sc.TILE + 1, 2 * sc.TILE + 3} == set(
        sc.EDGE_LENGTHS)
    for r in range(A.shape[0]):
        assert np.all(np.diff(A.indices[A.indptr[r]:A.indptr[r + 1]]) > 0)         # the struct's invariant
    raw = sc.bits(A.data)
    for b in sc.SPECIAL_BITS:
        assert (raw == np.uint64(b)).any(), hex(b)
    nan_payloads = {int(x) for x in raw[np.isnan(A.data)]}
    assert len(nan_payloads) >= 4
    assert np.isfinite(sc.matrix("edge_finite").data).all()
    assert sc.matrix("band").shape[0] > sc.BAND_SELECTED == 2 * sc.SCAN_CHUNK + 1
    rows, cols = sc.case_lists([c for c in sc.CASES if c[0] == "band_chunks"][0])
    assert len(rows) == len(cols) == sc.BAND_SELECTED
    assert len(set(sc.IDS)) == len(sc.IDS)
    rep = sc.index_list("edge", "rows_repeats")
    assert len(set(rep.tolist())) < len(rep)
    uns = sc.index_list("edge", "cols_unsorted_subset")
    assert np.any(np.diff(uns) < 0) and np.array_equal(np.sort(uns), sc.subset())
    G = sc.matrix("grid33x31")
    assert G.shape == (1023, 1023) and np.array_equal(G.data, np.round(G.data))


@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_restatement_equals_scipy(case):
    _, key, _, _ = case
    A = sc.matrix(key + "_finite" if key == "edge" else key)
    rows, cols = sc.case_lists(case)
    m, n = A.shape
    S = _scipy(A)
    want = S[np.arange(m) if rows is None else rows]
    if cols is not None:
        want = want[:, cols]
    want = sp.csr_matrix(want)
    want.sort_indices()
    got = sc.restate(A, 0, m, rows, cols)
    assert np.array_equal(got["rowptr"], want.indptr)
    assert np.array_equal(got["cols"], want.indices)
    assert np.array_equal(sc.bits(got["vals"]), sc.bits(want.data))
    assert np.array_equal(got["col_indices"][got["colval"]], got["cols"])
    assert np.all(np.diff(got["col_indices"]) > 0)
    assert np.array_equal(sc.bits(A.data[got["src"]]), sc.bits(got["vals"]))
    for r in range(len(got["rowptr"]) - 1):                                        # columns ascend within every output row
        assert np.all(np.diff(got["cols"][got["rowptr"][r]:got["rowptr"][r + 1]]) > 0)
    # the same structure with the special values: the restatement moves their bits
    if key == "edge":
        B = sc.matrix("edge")
        again = sc.restate(B, 0, m, rows, cols)
        assert np.array_equal(again["src"], got["src"])
        assert np.array_equal(sc.bits(again["vals"]), sc.bits(B.data)[again["src"]])


@pytest.mark.parametrize("nranks", [1, 2, 3])
def test_stitched_rank_results_reproduce_the_global_selection(nranks):
    A = sc.matrix("edge")
    m, n = A.shape
    cols = sc.index_list("edge", "cols_unsorted_subset")
    parts = [sc.uniform_partition(m, nranks)] + ([sc.uneven_partition(m, nranks, 1)] if nranks > 1 else [])
    for part in parts:
        rng = np.random.default_rng(nranks)
        rows_by_rank = []
        for r in range(nranks):
            own = np.arange(part[r], part[r + 1])
            rows_by_rank.append(rng.permutation(np.concatenate([own, own[:2]])) if len(own) else own)
        cut = np.sort(rng.choice(len(cols) + 1, nranks - 1)) if nranks > 1 else np.empty(0, np.int64)
        cols_by_rank = np.split(cols, cut)
        ranks = [sc.expected_on_rank(A, part, r, rows_by_rank, cols_by_rank) for r in range(nranks)]
        glob = sc.restate(A, 0, m, np.concatenate(rows_by_rank), cols)
        assert np.array_equal(ranks[0]["row_partition"], np.concatenate([[0], np.cumsum([len(x) for x in rows_by_rank])]))
        assert np.array_equal(ranks[0]["col_partition"], np.concatenate([[0], np.cumsum([len(x) for x in cols_by_rank])]))
        counts = np.concatenate([np.diff(e["rowptr"]) for e in ranks])
        assert np.array_equal(np.concatenate([[0], np.cumsum(counts)]), glob["rowptr"])
        assert np.array_equal(np.concatenate([e["col_indices"][e["colval"]] for e in ranks]), glob["cols"])
        assert np.array_equal(sc.bits(np.concatenate([e["vals"] for e in ranks])), sc.bits(glob["vals"]))
        none = sc.expected_on_rank(A, part, 0, None, None)
        assert np.array_equal(none["row_partition"], part) and np.array_equal(none["col_partition"], sc.uniform_partition(n, nranks))


def test_take_and_put_restatements():
    rng = np.random.default_rng(9)
    vg = rng.standard_normal(50)
    vg[3], vg[4] = -0.0, np.nan
    idx = np.array([49, 3, 3, 0, 4, 17, 49], dtype=np.int64)
    assert np.array_equal(sc.bits(sc.take_of(vg, idx)), sc.bits(vg[idx]))
    own = np.array([5, 1, 44, 9], dtype=np.int64)
    src = np.array([1.5, -0.0, np.inf, 7.0])
    want = vg.copy()
    want[own] = src
    assert np.array_equal(sc.bits(sc.put_into(vg, own, src)), sc.bits(want))
    with pytest.raises(AssertionError):
        sc.put_into(vg, np.array([1, 1]), src[:2])


def test_argument_rules_that_need_no_device(hp):
    import sys
    import torch
    sel = sys.modules[hp.select.__module__]                        # the module: the package attribute of that name is the function
    cpu = torch.device("cpu")
    with pytest.raises(TypeError, match="select: rows must hold integers"):
        sel._index_tensor(np.array([0.5, 1.0]), "rows", "select", cpu)
    with pytest.raises(TypeError, match="select: cols must be int64"):
        sel._index_tensor(torch.zeros(3, dtype=torch.int32), "cols", "select", cpu)
    with pytest.raises(ValueError, match="take: idx must be one-dimensional"):
        sel._index_tensor(np.zeros((2, 2), dtype=np.int64), "idx", "take", cpu)
    with pytest.raises(IndexError, match="beyond int64"):
        sel._index_tensor(np.array([2 ** 63], dtype=np.uint64), "rows", "select", cpu)
    t = sel._index_tensor([3, 1, 2], "rows", "select", cpu)
    assert t.dtype == torch.int64 and t.tolist() == [3, 1, 2]
    assert sel._index_tensor([], "rows", "select", cpu).numel() == 0
    with pytest.raises(IndexError, match=r"select: 2 of the rows lie outside \[0, 5\); the first is -1 at position 1"):
        sel._check_range(torch.tensor([0, -1, 4, 5]), 5, "rows", "select")
    sel._check_range(torch.tensor([0, 4]), 5, "rows", "select")
    assert np.array_equal(sel._partition_of([2, 0, 3]), [0, 2, 2, 5])
    with pytest.raises(TypeError, match="select: an HPCSparseMatrix is required"):
        hp.select(np.eye(3), None, None)
    with pytest.raises(TypeError, match="take: an HPCVector is required"):
        hp.take(np.arange(3.0), [0])
    with pytest.raises(TypeError, match="put_: an HPCVector is required"):
        hp.put_(np.arange(3.0), [0], None)


def test_the_header_declares_every_selection_entry_of_the_binding(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    listed = [s for s in hp._capi.EXPORTED_SYMBOLS if s.startswith("hpcla_select_") or s == "hpcla_gather_b32_i64"]
    assert {"hpcla_select_short_cap", "hpcla_select_tile", "hpcla_select_work_bytes", "hpcla_select_structure_i32",
            "hpcla_select_structure_i64", "hpcla_select_fill_i32", "hpcla_select_fill_i64", "hpcla_gather_b32_i64",
            "hpcla_select_take_f64_i32", "hpcla_select_take_f64_i64", "hpcla_select_put_f64_i32",
            "hpcla_select_put_f64_i64"} == set(listed)
    for name in listed:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hpcla_rocm.h"
        nargs = 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1
        assert nargs == len(hp._capi._SIGNATURES[name]), (name, nargs)
    lib = hp._capi.load()
    assert lib.hpcla_select_short_cap() == sc.SHORT_CAP and lib.hpcla_select_tile() == sc.TILE
    assert lib.hpcla_submatrix_scan_chunk() == sc.SCAN_CHUNK
    assert lib.hpcla_select_work_bytes(-1, 0, 0) < 0 and lib.hpcla_select_work_bytes(0, 0, 0) > 0
    assert hp.select and hp.selection_plan and hp.SelectionPlan and hp.take and hp.put_ and hp.index_plan and hp.VectorIndexPlan
