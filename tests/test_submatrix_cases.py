"""CPU half of the range-indexing tests: the numpy restatement of tests/_submatrix_cases.py against scipy's own slicing, the
partition helpers against a literal transcription of the reference's `_compute_subpartition` (src/indexing.jl:38-62), the
per-rank results stitched back into the global cut for 1, 2, 3 and 8 simulated ranks, and the C ABI table against the header.
No tolerance anywhere: the operation copies bits."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import _submatrix_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy(A):
    return sp.csr_matrix((A.data, A.indices, A.indptr), shape=A.shape)


def test_the_matrices_hold_what_the_cases_need():
    A = sc.matrix("rand")
    lens = np.diff(A.indptr)
    for r, n in sc.PLANTED_LENGTHS.items():
        assert lens[r] == n
    assert {0, 63, 64, 65, 255, 256, 257} <= set(lens.tolist()) and lens.max() > 512 and lens.max() <= 701
    assert not ((A.indices >= sc.GAP_LO) & (A.indices < sc.GAP_HI)).any()
    assert {sc.GAP_LO - 10, sc.GAP_HI + 6, sc.GAP_LO - 1, sc.GAP_HI} <= set(A.indices.tolist())
    for r in range(A.shape[0]):
        assert np.all(np.diff(A.indices[A.indptr[r]:A.indptr[r + 1]]) > 0)         # the struct's invariant
    v = A.data
    assert np.isnan(v).sum() >= 30 and np.isposinf(v).sum() >= 30 and np.isneginf(v).sum() >= 30
    assert ((v == 0) & np.signbit(v)).sum() >= 30 and ((v == 0) & ~np.signbit(v)).sum() >= 30
    assert ((v != 0) & (np.abs(v) < np.finfo(np.float64).tiny)).sum() >= 30
    a, c, _ = A.rows(sc.WHOLE_ROW, sc.WHOLE_ROW + 1)
    assert len(c) and c.min() >= sc.BLOCK_A[0] and c.max() < sc.BLOCK_A[1]
    a, c, _ = A.rows(sc.OTHER_ROW, sc.OTHER_ROW + 1)
    assert len(c) and c.min() >= sc.BLOCK_B[0] and c.max() < sc.BLOCK_B[1]
    col = sc.column_of(A, 0, A.shape[0], sc.NEGZERO_COL)
    assert col[sc.NEGZERO_ROW] == 0 and np.signbit(col[sc.NEGZERO_ROW])
    assert sc.matrix("band").shape[0] == 68 * sc.SCAN_CHUNK + 369 and sc.matrix("p5").shape == (9216, 9216)
    assert np.isfinite(sc.matrix("rand_finite").data).all()
    names = [c[0] for c in sc.CASES]
    assert len(set(names)) == len(names)
    counts = {c[3] - c[2] for c in sc.CASES}
    assert {0, 1, 63, 64, 65, 255, 256, 257, 1000, 70001} <= counts
    # the two cases past the scan's first trip of chunk sums: more than SCAN_TRIP selected rows, more than SCAN_TRIP columns, and
    # entries (rows) / occurring columns on both sides of element SCAN_TRIP, with empty chunks before it
    assert sc.matrix(sc.BAND_LONG).shape == (sc.BAND_LONG_ROWS, sc.BAND_LONG_ROWS)
    long = {c[0]: c for c in sc.CASES if c[1] == sc.BAND_LONG}
    _, key, r0, r1, c0, c1 = long["band_long_rows"]
    got = sc.restate(sc.matrix(key), r0, r1, c0, c1)
    per_row = np.diff(got["rowptr"])
    assert r1 - r0 > sc.SCAN_TRIP and per_row[:sc.SCAN_TRIP].sum() > 0 and per_row[sc.SCAN_TRIP:].sum() > 0
    assert per_row[:sc.SCAN_CHUNK].sum() == 0 and c1 - c0 < sc.SCAN_TRIP
    _, key, r0, r1, c0, c1 = long["band_long_cols"]
    got = sc.restate(sc.matrix(key), r0, r1, c0, c1)
    assert c1 - c0 > sc.SCAN_TRIP and r1 - r0 < sc.SCAN_TRIP
    assert 0 < (got["col_indices"] < sc.SCAN_TRIP).sum() < len(got["col_indices"]) and got["col_indices"].min() > sc.SCAN_CHUNK


@pytest.mark.parametrize("case", sc.CASES, ids=[c[0] for c in sc.CASES])
def test_restatement_equals_scipy(case):
    _, key, r0, r1, c0, c1 = case
    A = sc.matrix(key)
    want = _scipy(A)[r0:r1, c0:c1]
    got = sc.restate(A, r0, r1, c0, c1)
    assert np.array_equal(got["rowptr"], want.indptr)
    assert np.array_equal(got["cols"], want.indices)
    assert np.array_equal(sc.bits(got["vals"]), sc.bits(want.data))                 # stored zeros, -0.0, NaN payloads included
    assert np.array_equal(got["col_indices"][got["colval"]], got["cols"])
    assert np.all(np.diff(got["col_indices"]) > 0)


@pytest.mark.parametrize("name,key,k", sc.COLUMN_CASES, ids=[c[0] for c in sc.COLUMN_CASES])
def test_column_restatement_equals_scipy(name, key, k):
    A = sc.matrix(key)
    got = sc.column_of(A, 0, A.shape[0], k)
    S = _scipy(A).tocsc()
    want = np.zeros(A.shape[0])
    a, b = S.indptr[k], S.indptr[k + 1]
    want[S.indices[a:b]] = S.data[a:b]
    assert np.array_equal(sc.bits(got), sc.bits(want))
    assert not np.signbit(got[np.setdiff1d(np.arange(A.shape[0]), S.indices[a:b])]).any()     # absent: exactly +0.0


def test_subpartition_equals_the_reference_transcription(hp):
    rng = np.random.default_rng(5)
    for trial in range(300):
        nranks = int(rng.integers(1, 9))
        sizes = rng.integers(0, 12, nranks)
        sizes[rng.random(nranks) < 0.3] = 0                                        # empty ranks
        part = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(part[-1])
        a = int(rng.integers(0, n + 1))
        b = int(rng.integers(a, n + 1))
        got = hp.subpartition(part, a, b)
        want = np.asarray(sc.reference_subpartition_1based([int(p) + 1 for p in part], a + 1, b)) - 1
        assert got.dtype == np.int64 and np.array_equal(got, want), (part, a, b)
        assert got[-1] == b - a
        for r in range(nranks):
            lo, hi = hp.local_window(part, r, a, b)
            assert hi - lo == got[r + 1] - got[r]
            if hi > lo:
                assert part[r] + lo == max(part[r], a) and part[r] + hi == min(part[r + 1], b)


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_stitched_rank_results_reproduce_the_global_cut(hp, nranks):
    for _, key, r0, r1, c0, c1 in sc.CASES:
        A = sc.matrix(key)
        parts = [sc.uniform_partition(A.shape[0], nranks)]
        if nranks > 1:
            parts.append(sc.uneven_partition(A.shape[0], nranks, nranks // 2))     # one rank without rows
        for part in parts:
            ranks = [sc.expected_on_rank(A, part, r, r0, r1, c0, c1) for r in range(nranks)]
            rowp, colp = ranks[0]["row_partition"], ranks[0]["col_partition"]
            assert np.array_equal(colp, hp.uniform_partition(c1 - c0, nranks))
            if r0 == r1 or c0 == c1:                                               # the quirk: uniform, not the sub-partition
                assert np.array_equal(rowp, hp.uniform_partition(r1 - r0, nranks))
            else:
                assert np.array_equal(rowp, hp.subpartition(part, r0, r1))
            glob = sc.restate(A, r0, r1, c0, c1)
            for r, e in enumerate(ranks):
                assert len(e["rowptr"]) - 1 == rowp[r + 1] - rowp[r]
                if not (r0 == r1 or c0 == c1):
                    lo, hi = hp.local_window(part, r, r0, r1)
                    assert len(e["rowptr"]) - 1 == hi - lo
            counts = np.concatenate([np.diff(e["rowptr"]) for e in ranks])
            assert np.array_equal(np.concatenate([[0], np.cumsum(counts)]), glob["rowptr"])
            assert np.array_equal(np.concatenate([e["col_indices"][e["colval"]] for e in ranks]), glob["cols"])
            assert np.array_equal(sc.bits(np.concatenate([e["vals"] for e in ranks])), sc.bits(glob["vals"]))


def test_the_header_declares_every_indexing_entry_of_the_binding(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    listed = [s for s in hp._capi.EXPORTED_SYMBOLS if s.startswith(("hpcla_submatrix_", "hpcla_sparse_column_"))]
    assert {"hpcla_submatrix_work_bytes", "hpcla_submatrix_structure_i32", "hpcla_submatrix_structure_i64",
            "hpcla_submatrix_fill_i32", "hpcla_submatrix_fill_i64", "hpcla_submatrix_values_i32",
            "hpcla_submatrix_values_i64", "hpcla_sparse_column_i32", "hpcla_sparse_column_i64"} <= set(listed)
    for name in listed:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hpcla_rocm.h"
        nargs = 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1
        assert nargs == len(hp._capi._SIGNATURES[name]), (name, nargs)
    lib = hp._capi.load()
    assert lib.hpcla_submatrix_scan_chunk() == sc.SCAN_CHUNK
    assert lib.hpcla_submatrix_work_bytes(-1, 0) < 0 and lib.hpcla_submatrix_work_bytes(0, 0) > 0
    assert hp.get_submatrix_plan and hp.SubmatrixPlan and hp.subpartition and hp.local_window
