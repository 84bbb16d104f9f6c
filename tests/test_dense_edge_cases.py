"""CPU checks of what tests/test_gpu_dense_edges.py feeds the GPU: the dispatch restated in tests/_dense_edge_cases.py gives
the library's own work size for every transpose(A)*x case, every branch of csrc/gemv.hip and of the layout conversion that the
GPU file is there for is reached by a named case (and by none of the six shapes the suite had before), the thinned A*x cross
product still pairs every axis value with every kernel, the two references agree where both are exact, and the rounding bound
of the longest add chain stays below the tolerance the GPU file asserts."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dense_edge_cases as dc  # noqa: E402


@pytest.fixture(scope="module")
def tcases():
    return dc.gemv_t_cases()


def _find(tcases, nrows, ncols, form="plain"):
    hit = [c for c in tcases if c[1] == nrows and c[2] == ncols and c[3] == form]
    assert len(hit) == 1, (nrows, ncols, form)
    return hit[0][7]


def test_restated_chunking_is_the_librarys(hp, tcases):
    """hpcla_gemv_t_work_bytes is a host function: no device is touched."""
    lib = hp._capi.load()
    assert len(tcases) == 4 * 23 - 2
    for group, nrows, ncols, form, lda, a_off, w_off, d in tcases:
        assert d["work_bytes"] == lib.hpcla_gemv_t_work_bytes(nrows, ncols), (nrows, ncols)
        assert d["nchunks"] <= 65535 and (d["nchunks"] - 1) * d["rpc"] < nrows <= d["nchunks"] * d["rpc"]
    for nrows, ncols in ((0, 5), (5, 0), (0, 0), (-1, 5), (5, -1)):
        assert lib.hpcla_gemv_t_work_bytes(nrows, ncols) == 8


def test_gemv_t_named_cases_reach_their_branches(tcases):
    d = _find(tcases, 14401, 32)
    assert (d["kernel"], d["nchunks"], d["CT"], d["last_rows"], d["stage2_main"]) == ("vec2", 226, 32, 1, True)
    d = _find(tcases, 14401, 31)
    assert (d["kernel"], d["nchunks"], d["CT"], d["stage2_main"]) == ("scalar", 226, 32, True)
    d = _find(tcases, 7301, 64)
    assert (d["kernel"], d["nchunks"], d["stage2_main"]) == ("vec2", 115, True) and 7 * d["nph"] == 112
    d = _find(tcases, 7301, 65)
    assert (d["kernel"], d["nchunks"], d["stage2_main"], d["stage1_tiles"]) == ("scalar", 115, True, 2)
    d = _find(tcases, 7300, 130)
    assert (d["kernel"], d["nchunks"], d["tile_cols"], d["stage1_tiles"], d["stage2_workgroups"]) == ("vec2", 115, 128, 2, 3)
    d = _find(tcases, 230001, 16)
    assert (d["kernel"], d["nchunks"], d["rstep"], d["stage1_main"], d["stage2_main"]) == ("vec2", 1023, 32, True, True)
    d = _find(tcases, 460001, 3)
    assert (d["kernel"], d["rstep"], d["stage1_main"]) == ("scalar", 64, True)
    d = _find(tcases, 1900001, 1)
    assert (d["kernel"], d["rstep"], d["stage1_main"], d["CT"], d["nph"]) == ("scalar", 256, True, 1, 1024)
    for shape in ((460001, 4), (120001, 2)):
        assert _find(tcases, *shape)["kernel"] == "vec2"
    assert _find(tcases, 460001, 4)["tile_cols"] == 4 and _find(tcases, 120001, 2)["tile_cols"] == 2
    assert (_find(tcases, 300, 128)["kernel"], _find(tcases, 300, 128)["stage1_tiles"]) == ("vec2", 1)
    assert (_find(tcases, 300, 129)["kernel"], _find(tcases, 300, 129)["stage1_tiles"]) == ("scalar", 3)
    assert (_find(tcases, 2000, 258)["kernel"], _find(tcases, 2000, 258)["stage1_tiles"]) == ("vec2", 3)
    d = _find(tcases, 65, 66)
    assert d["kernel"] == "vec2" and [c[4] for c in tcases if c[1:3] == (65, 66)] == [70, 71, 70, 70]
    for nrows, ncols in ((16, 100001), (1, 70001), (3, 4097)):                   # few rows, many columns of either parity
        d = _find(tcases, nrows, ncols)
        assert d["kernel"] == "scalar" and d["nchunks"] == 1 and d["stage2_workgroups"] == dc.ceil_div(ncols, 64)
    # the forms that must leave the 16-byte kernel do
    for group, nrows, ncols, form, lda, a_off, w_off, d in tcases:
        if form != "plain":
            assert d["kernel"] == "scalar", (nrows, ncols, form)
        elif ncols % 2 == 0:
            assert d["kernel"] == "vec2", (nrows, ncols)
    # the two forms that would pass 30 MB are the only ones left out (the scalar kernel's main loop at a padded pitch is
    # reached by 460001 x 3 and 460001 x 4 on lda + 1)
    have = {c[1:4] for c in tcases}
    missing = {(m, n, f) for shapes in dc.GEMVT_GROUPS.values() for m, n, _ in shapes for f in dc.GEMVT_FORMS} - have
    assert missing == {(230001, 16, "lda_plus_1"), (1900001, 1, "lda_plus_1")}
    for shape in ((460001, 3), (460001, 4)):
        d = _find(tcases, *shape, form="lda_plus_1")
        assert d["kernel"] == "scalar" and d["stage1_main"]


def test_gemv_t_every_branch_is_reached(tcases):
    for kernel in ("vec2", "scalar"):
        mine = [c[7] for c in tcases if c[7]["kernel"] == kernel]
        assert any(d["stage1_main"] for d in mine) and any(d["stage1_tail"] for d in mine), kernel
        assert any(d["stage1_tiles"] > 1 for d in mine), kernel
        assert any(d["stage2_main"] for d in mine) and any(d["stage2_tail"] for d in mine), kernel
        assert any(d["last_rows"] == 1 and d["nchunks"] > 1 for d in mine), kernel
        assert any(d["stage2_workgroups"] > 1 for d in mine), kernel
    assert {c[7]["CT"] for c in tcases} >= {1, 2, 4, 16, 32, 64}
    assert {c[7]["rstep"] for c in tcases if c[7]["stage1_main"]} >= {256, 64, 32, 16, 4}


def test_the_earlier_shapes_reach_neither_main_loop():
    """So that nobody takes the new cases for duplicates of tests/test_gpu_parity.py::test_dense_transpose_matvec."""
    nchunks = []
    for nrows, ncols in dc.GEMVT_BASELINE:
        d = dc.gemv_t_dispatch(nrows, ncols, ncols)
        nchunks.append(d["nchunks"])
        assert not d["stage2_main"], (nrows, ncols)
        if ncols <= 16:
            assert not d["stage1_main"], (nrows, ncols)
    assert nchunks == [79, 47, 5, 1, 1, 1021]


def test_gemv_t_probe_rows():
    for nrows, ncols in ((14401, 32), (230001, 16), (1, 1), (65, 66)):
        rpc = dc.gemv_t_rows_per_chunk(nrows, ncols)
        rows = dc.gemv_t_probe_rows(nrows, ncols)
        nchunks = dc.ceil_div(nrows, rpc)
        assert rows[0] == 0 and rows[-1] == nrows - 1 and np.all(np.diff(rows) > 0)
        assert set(rows) >= {k * rpc for k in range(nchunks)} | {k * rpc - 1 for k in range(1, nchunks)}
        few = dc.gemv_t_probe_rows(nrows, ncols, every=False)
        assert len(few) <= 64 and set(few) <= set(rows) and few[0] == 0 and few[-1] == nrows - 1


@pytest.fixture(scope="module")
def gcases():
    return {g: dc.gemv_cases(g) for g in dc.GEMV_GROUPS}


def test_gemv_groups_hold_the_shapes_they_name(gcases):
    seen_ncols, seen_L = set(), set()
    for group, cases in gcases.items():
        for nrows, ncols, lda, a_off, picks in cases:
            d = dc.gemv_dispatch(nrows, ncols, lda, a_off, picks[0][1], picks[0][2])
            if group == "rowmajor":
                assert d["kernel"] == "rowmajor" and ncols > 128
            else:
                assert d["kernel"] == "skinny" and f"skinny_L{d['L']}" == group and d["rpw"] == (64 // d["L"]) * 16
                seen_L.add(d["L"])
                assert nrows in {d["rpw"] + k for k in (-1, 0, 1)} | {4 * d["rpw"] + k for k in (-1, 0, 1)} | {8 * d["rpw"] + 3}
            seen_ncols.add(ncols)
    assert seen_L == {1, 2, 4, 8, 16, 32, 64}
    assert seen_ncols == set(dc.SKINNY_NCOLS) | set(dc.ROWMAJOR_NCOLS)
    assert dc.skinny_L(128) == 64 and dc.skinny_L(65) == 64 and dc.skinny_L(64) == 32 and dc.skinny_L(33) == 32
    assert [dc.skinny_L(n) for n in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert {n for _, n in dc.gemv_shapes("rowmajor")} == set(dc.ROWMAJOR_NCOLS)
    assert {m for m, _ in dc.gemv_shapes("rowmajor")} == set(dc.ROWMAJOR_NROWS)


def test_thinned_cross_product_keeps_every_axis_value_with_every_kernel(gcases):
    all_splits = set(dc.segment_splits(200))
    assert len(all_splits) == 10
    total = 0
    for group, cases in gcases.items():
        pads, offs, splits, xforms, vec16, seg_paths = set(), set(), set(), set(), set(), set()
        ghost_misaligned = False
        for nrows, ncols, lda, a_off, picks in cases:
            pads.add(lda - ncols)
            offs.add(a_off)
            for name, split, xf in picks:
                total += 1
                splits.add(name)
                xforms.add(xf)
                d = dc.gemv_dispatch(nrows, ncols, lda, a_off, split, xf)
                vec16.add(d["vec16"])
                seg_paths |= d.get("seg_paths", set())
                ghost_misaligned |= xf == "ghost" and split[0] % 2 == 1 and split[2] > 0
        assert pads == set(dc.LDA_PADS) and offs == {0, 1} and xforms == set(dc.X_FORMS), group
        assert ghost_misaligned, group
        if group == "skinny_L1":                                   # ncols 1 and 2 admit three of the splits
            assert splits == set(dc.segment_splits(2)) and vec16 == {True, False}
        elif group == "rowmajor":
            assert splits == all_splits
            assert seg_paths == {(True, 0), (True, 1), (False, 0), (False, 1)}     # both seg_dot paths, odd and even n
        else:
            assert splits == (all_splits if group != "skinny_L2" else set(dc.segment_splits(4))), group
            assert vec16 == {True, False}, group                   # the skinny 16-byte path on and off
    assert 3000 <= total <= 5000, total


def test_segment_splits_are_what_their_names_say():
    for n in (1, 2, 3, 4, 5, 7, 8, 129, 4099):
        s = dc.segment_splits(n)
        assert s["all_own"] == (0, n, 0)
        if n >= 2:
            assert s["own_odd_then_rest"][0] == 0 and s["own_odd_then_rest"][1] % 2 == 1
            assert s["lo_1_own_0"] == (1, 0, n - 1) and s["own_last_1"] == (n - 1, 1, 0)
        if n >= 3:
            lo, own, hi = s["odd_odd_rest"]
            assert lo % 2 == 1 and own % 2 == 1 and hi >= 1
            assert s["single_first"][:2] == (1, 1) and s["single_last"][1:] == (1, 1)
        if n >= 4:
            assert s["edge_inside_pair"][0] % 2 == 1 and s["edge_between_pairs"][0] % 2 == 0
    assert dc.segment_edges((3, 0, 4)) == [0, 2, 3, 6] and dc.segment_edges((0, 5, 0)) == [0, 4]
    assert dc.segment_edges((1, 1, 1)) == [0, 1, 2]


def test_references_agree_on_integer_inputs_and_integers_are_exact(tcases):
    for nrows, ncols, transposed in ((14401, 32, True), (3, 4097, True), (301, 257, False), (1027, 5, False), (1, 1, True)):
        A, x = dc.product_inputs("int", nrows, ncols, nrows if transposed else ncols, 7)
        assert np.abs(A).max() == (8 if A.size > 100 else 7) and np.abs(x).max() <= 8
        want = dc.ref_int(A, x, transposed)
        got, scale = dc.ref_longdouble(A, x, transposed)
        np.testing.assert_array_equal(got, want)
        assert np.all(scale >= np.abs(want))
    assert np.finfo(np.longdouble).nmant >= 63, "numpy's long double is no wider than float64 here"
    for group, nrows, ncols, form, lda, a_off, w_off, d in tcases:
        assert dc.int_terms_are_exact(nrows)
    assert all(dc.int_terms_are_exact(n) for n in dc.SKINNY_NCOLS + dc.ROWMAJOR_NCOLS + dc.SWEEP_NCOLS)
    A, x = dc.product_inputs("real", 50, 40, 40, 7)
    assert A.min() >= -0.5 and A.max() < 0.5 and x.min() >= -0.5 and x.max() < 0.5 and not np.array_equal(A, np.round(A))


def test_add_chains_stay_below_the_tolerance(tcases, gcases):
    longest = max(tcases, key=lambda c: c[7]["chain"])
    assert longest[1:3] == (1900001, 1) and 1200 < longest[7]["chain"] < 1400
    for c in tcases:
        assert dc.chain_bound(c[7]["chain"]) < dc.RTOL_RED / 5
    for cases in gcases.values():
        for nrows, ncols, lda, a_off, picks in cases:
            for name, split, xf in picks:
                assert dc.chain_bound(dc.gemv_dispatch(nrows, ncols, lda, a_off, split, xf)["chain"]) < dc.RTOL_RED / 50


def test_transpose_cases_reach_both_kernels_and_fit_their_buffers():
    kernels = {}
    for group in dc.TRANSPOSE_GROUPS:
        cases = dc.transpose_cases(group)
        kernels[group] = {c["kernel"] for c in cases}
        for c in cases:
            for dtype in (np.float64, np.float32):
                src, want = dc.transpose_buffers(c, dtype)
                inner = want[dc.GUARD:-dc.GUARD]
                assert len(src) == c["src_len"] and len(inner) == c["dst_len"]
                assert np.isnan(want[:dc.GUARD]).all() and np.isnan(want[-dc.GUARD:]).all()
                assert (~np.isnan(src)).sum() == (~np.isnan(inner)).sum() == c["rows"] * c["cols"]
                np.testing.assert_array_equal(np.sort(src[~np.isnan(src)]), np.arange(1, c["rows"] * c["cols"] + 1))
            assert len(src) * 8 <= dc.MAX_BYTES
    assert kernels == {"generic": {"generic"}, "narrow": {"narrow", "generic"}, "julia": {"narrow", "generic"}}
    for c in dc.transpose_cases("narrow"):
        assert c["kernel"] == ("narrow" if c["rows"] >= 256 and c["cols"] <= 32 and c["ld_dst"] == c["cols"] else "generic")
    narrow_cols = {c["cols"] for c in dc.transpose_cases("narrow") if c["kernel"] == "narrow"}
    assert narrow_cols == {1, 2, 15, 16, 17, 31, 32}               # 31 and 32 Float64 columns: more than 64 KiB of LDS
    pairs = {(c["src_layout"], c["dst_layout"]) for c in dc.transpose_cases("generic")}
    assert pairs == set(dc.LAYOUT_PAIRS)
    julia = dc.transpose_cases("julia")
    assert any(c["src_off"] % 2 == 1 and c["src_layout"] == dc.LAYOUT_ROW and c["dst_layout"] == dc.LAYOUT_COL for c in julia)
    assert any(c["dst_off"] % 2 == 1 and c["src_layout"] == c["dst_layout"] == dc.LAYOUT_ROW for c in julia)
    assert {c["ld_dst"] - c["cols"] for c in julia if c["name"].startswith("operand")} == {0, 1}
    # element (i, c) where the layouts say
    np.testing.assert_array_equal(dc.layout_index(dc.LAYOUT_ROW, 5, 2, 3), [[0, 1, 2], [5, 6, 7]])
    np.testing.assert_array_equal(dc.layout_index(dc.LAYOUT_COL, 4, 2, 3), [[0, 4, 8], [1, 5, 9]])
