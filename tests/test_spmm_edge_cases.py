"""tests/_spmm_edge_cases.py checked on the CPU: the matrices are what their names say, the case tables reach every kernel
instance, and every row (column) that a pass boundary cuts tells one running sum from per-pass partial sums -- so that a
failure of tests/test_gpu_spmm_edges.py is the kernel's and not the test's."""
import numpy as np
import pytest

from tests import _spmm_edge_cases as sc

I32 = np.int32
PASS_CH = (sc.CHUNK_V_SMALL, sc.CHUNK_V_LARGE, sc.CHUNK_MM)
CPBS = tuple(sorted({sc.TPB_T // sc.spmm_t_lpc(m) for m in sc.SPMM_T_MS}))


@pytest.fixture(scope="module")
def matrices():
    return {CH: sc.pass_matrix(CH) for CH in PASS_CH}


@pytest.fixture(scope="module")
def t_matrices():
    return {cpb: sc.spmm_t_matrix(cpb) for cpb in CPBS}


def _assert_csr(rowptr, colval, ncols):
    assert rowptr[0] == 0 and rowptr[-1] == len(colval) and np.all(np.diff(rowptr) >= 0)
    assert colval.min() >= 0 and colval.max() < ncols
    inner = np.ones(len(colval), dtype=bool)
    inner[rowptr[1:-1][rowptr[1:-1] < len(colval)]] = False        # the first entry of a row has no predecessor in it
    inner[0] = False
    assert np.all(np.diff(colval)[inner[1:]] > 0), "columns ascending and distinct in every row"


def test_constants_are_the_ones_the_cases_were_laid_out_for():
    assert (sc.RPB_MM, sc.TPB_MM, sc.KT) == (64, 256, 16)
    assert sc.CHUNK_V_SMALL < sc.CHUNK_V_LARGE < sc.CHUNK_MM and 2 * sc.CHUNK_MM + 7 <= sc.NCOLS
    assert sc.RUNS_EMAX == 2 * sc.TPB_MM and sc.RUNS_MAX == 4 and sc.RUNS_TILE_ROWS == 200
    assert 2 * sc.CHUNK_T + 52 <= sc.T_ROWS and CPBS == (8, 16, 32, 64, 128, 256)


@pytest.mark.parametrize("CH", PASS_CH)
def test_pass_matrix_is_what_its_names_say(matrices, CH):
    M = matrices[CH]
    rp, cv, n = M["rowptr"], M["colval"], M["nrows"]
    _assert_csr(rp, cv, M["ncols"])
    lens = np.diff(rp)
    totals = dict(zip(M["names"], sc.block_totals(M)))
    want = {"empty": 0, "one": 1, "CH-1": CH - 1, "CH in row 63": CH, "CH+1": CH + 1, "2CH": 2 * CH, "2CH+1": 2 * CH + 1,
            "3CH+7": 3 * CH + 7, "2CH+2": 2 * CH + 2, "ragged CH+1": CH + 1}
    assert {k: totals[k] for k in want} == want
    assert M["names"][-1] == "ragged CH+1" and n % sc.RPB_MM == sc.LAST_NR and sc.LAST_NR % 2 == 1
    # the side of the switch
    nnz = len(cv)
    if CH == sc.CHUNK_V_SMALL:
        assert nnz == sc.SMALL_NNZ_PER_ROW * n
    else:
        assert nnz > sc.SMALL_NNZ_PER_ROW * n
    # rows on the boundaries
    b0 = lambda r: rp[r - r % sc.RPB_MM]                           # noqa: E731
    for r in M["ends_at"]:
        assert lens[r] >= 2 and (rp[r + 1] - b0(r)) % CH == 0 and (rp[r] - b0(r)) // CH == (rp[r + 1] - 1 - b0(r)) // CH
    for r in M["starts_at"]:
        assert lens[r] >= 1 and (rp[r] - b0(r)) % CH == 0 and rp[r] > b0(r)
    assert lens[M["long_row"]] > 2 * CH
    strad = sc.straddlers(rp, CH, sc.RPB_MM)
    sides = set()
    for r, cuts in strad:
        first, last = cuts[0], lens[r] - cuts[-1]
        assert first >= 2 and last >= 2, f"row {r}: {first} | {last} entries beside the boundary prove nothing"
        sides.add((first % 2, last % 2))
    assert sides == {(0, 0), (0, 1), (1, 0), (1, 1)}, "even and odd counts on either side"
    assert any(len(cuts) >= 2 for _, cuts in strad), "a row that spans a whole pass"
    # empty rows in the first and the last slot of a block with entries; a block whose records all sit in row 63
    r0 = sc.RPB_MM * M["names"].index("2CH")
    assert lens[r0] == 0 and lens[r0 + sc.RPB_MM - 1] == 0
    r0 = sc.RPB_MM * M["names"].index("CH in row 63")
    assert lens[r0 + sc.RPB_MM - 1] == CH and lens[r0:r0 + sc.RPB_MM - 1].sum() == 0
    # the rows of one lane group of the generic kernel (GRP = 16: g + 16 s; GRP = 8: g + 32 s): 0, 1, odd, long
    g = M["group_rows"]
    assert [x - g[0] for x in g] == [0, 16, 32, 48]
    assert lens[g[0]] == 0 and lens[g[1]] == 1 and lens[g[2]] % 2 == 1 and lens[g[2]] > 1 and lens[g[3]] > CH
    # the first ghost column, offset -1 in the generic kernel's encoding: alone in a row, and in every straddling row
    assert cv[rp[g[1]]] == M["n_own"]
    for r, _ in strad:
        assert M["n_own"] in cv[rp[r]:rp[r + 1]] and M["n_own"] - 1 in cv[rp[r]:rp[r + 1]]
    interior, boundary = sc.block_lists(M)
    assert len(interior) >= 1 and len(boundary) >= 8 and len(interior) + len(boundary) == -(-n // sc.RPB_MM)


def test_switch_pair_differs_by_one_entry():
    a, b = sc.switch_pair()
    assert a["nrows"] == b["nrows"] and len(b["colval"]) == len(a["colval"]) + 1
    assert len(a["colval"]) == sc.SMALL_NNZ_PER_ROW * a["nrows"]
    _assert_csr(b["rowptr"], b["colval"], b["ncols"])
    changed = np.flatnonzero(np.diff(a["rowptr"]) != np.diff(b["rowptr"]))
    assert len(changed) == 1
    r = int(changed[0])
    at = int(np.flatnonzero(~np.isin(b["colval"][b["rowptr"][r]:b["rowptr"][r + 1]],
                                     a["colval"][a["rowptr"][r]:a["rowptr"][r + 1]]))[0]) + int(b["rowptr"][r])
    assert np.array_equal(np.delete(b["colval"], at), a["colval"]) and np.array_equal(np.delete(b["vals"], at), a["vals"])
    k = sc.KT
    va = sc.variant_of(k, k, 1, k, k, 1, False, 0, len(a["colval"]), a["nrows"])[0]
    vb = sc.variant_of(k, k, 1, k, k, 1, False, 0, len(b["colval"]), b["nrows"])[0]
    assert va[1] == sc.CHUNK_V_SMALL and vb[1] == sc.CHUNK_V_LARGE and va[2:] == vb[2:]
    assert max(sc.block_totals(b)) > sc.CHUNK_V_LARGE            # several passes on either side of the switch


def test_case_tables_reach_every_vector_kernel_instance(matrices):
    reached = set()
    for CH in (sc.CHUNK_V_SMALL, sc.CHUNK_V_LARGE):
        M = matrices[CH]
        assert max(sc.block_totals(M)) > 2 * CH                    # a multi-pass block
        for case in sc.vec_cases(M["nrows"]):
            v, launches = sc.case_variant(case, len(M["colval"]), M["nrows"])
            assert (v == "tiles") == (case["ccol"] and case["k"] > sc.KT), case
            assert len(launches) == -(-case["k"] // sc.KT) if v == "tiles" else launches == [v]
            for launch in launches:
                assert launch[0] == "vec" and launch[1] == CH, (case, launch)
                assert launch[2:] in sc.VEC_TUPLES, (case, launch)
                reached.add((CH, case["entry"] != "csr", launch[2:]))
    missing = {(CH, split, t) for CH in (sc.CHUNK_V_SMALL, sc.CHUNK_V_LARGE) for split in (False, True) for t in sc.VEC_TUPLES}
    assert not missing - reached, sorted(missing - reached)
    ks = {c["k"] for c in sc.vec_cases(5)}
    assert ks == set(sc.VEC_KS) and {2, 3, 4, 6, 7, 8, 10, 12, 14, 15, 16, 18, 20, 32, 40} <= ks
    # HALF64 without CSTAGE at k = 16 on ldc = 18
    assert sc.variant_of(16, 16, 1, 16, 18, 1, False, 0, 10 ** 6, 10)[0][2:] == (4, True, False, False, False, False)


def test_case_tables_reach_every_generic_kernel_instance(matrices):
    M = matrices[sc.CHUNK_MM]
    assert max(sc.block_totals(M)) > 3 * sc.CHUNK_MM
    reached = set()
    for case in sc.generic_cases(M["ncols"]):
        v, launches = sc.case_variant(case, len(M["colval"]), M["nrows"])
        assert v[0] == "generic" and launches == [v], (case, v)
        reached.add((v[1], case["entry"], case["how"]))
    for grp in (4, 8, 16):
        for entry in ("csr", "split", "panel"):
            assert {(grp, entry, "odd"), (grp, entry, "offset")} <= reached
        assert (grp, "csr", "colB") in reached
    assert {c["k"] for c in sc.generic_cases(9)} == {3, 5, 7, 9, 15, 17, 33}


def test_case_tables_reach_every_transposed_kernel_instance(t_matrices):
    reached = set()
    for m in sc.SPMM_T_MS:
        M = t_matrices[sc.TPB_T // sc.spmm_t_lpc(m)]
        totals = [int(M["colptr"][min(c + M["cpb"], M["ncols"])] - M["colptr"][c]) for c in range(0, M["ncols"], M["cpb"])]
        assert max(totals) > 2 * sc.CHUNK_T                        # !single
        for call in sc.spmm_t_calls(m, M["ncols"]):
            reached.add(sc.spmm_t_variant_of(m, call["x_row"], call["ldx"], call["w_col"]))
    assert reached == sc.SPMM_T_VARIANTS, sorted(sc.SPMM_T_VARIANTS - reached)
    assert {1, 2, 16, 17, 64, 65, 66, 130} <= set(sc.SPMM_T_MS)


@pytest.mark.parametrize("CH", PASS_CH)
def test_every_straddling_row_tells_a_running_sum_from_partial_sums(matrices, orc, CH):
    """NO straddling row may be left undiscriminated, in column 0 and in column 1 of B (so at every width k >= 1)."""
    M = matrices[CH]
    rp, cv, va = M["rowptr"], M["colval"], M["vals"]
    B = sc.master_B()
    strad = sc.straddlers(rp, CH, sc.RPB_MM)
    assert len(strad) == 6                                         # five pinned rows and the long row of the lane group
    for r, cuts in strad:
        lo, hi = int(rp[r]), int(rp[r + 1])
        told = sc.discriminated(va[lo:hi], B[cv[lo:hi], :2], cuts)
        assert told.all(), f"row {r} (cuts {cuts} of {hi - lo}): columns {np.flatnonzero(~told)} of B do not discriminate"
    # the numpy running sum is the oracle's sum
    want = orc.spmm(rp.astype(I32), cv.astype(I32), va, np.ascontiguousarray(B[:, :3]))
    np.testing.assert_array_equal(sc.seq_spmm_ref(rp, cv, va, B[:, :3]), want)
    np.testing.assert_array_equal(sc.panel_order_ref(M, B[:, :3]), want)    # ascending panels: the stored order


@pytest.mark.parametrize("cpb", CPBS)
def test_transposed_matrix_columns_and_their_order_sensitivity(t_matrices, orc, cpb):
    M = t_matrices[cpb]
    rp, cv, va, ncols = M["rowptr"], M["colval"], M["vals"], M["ncols"]
    _assert_csr(rp, cv, ncols)
    colptr, CH = M["colptr"], sc.CHUNK_T
    clen = np.diff(colptr)
    totals = [int(colptr[min(c + cpb, ncols)] - colptr[c]) for c in range(0, ncols, cpb)]
    assert totals[:3] == [CH - 1, CH, CH + 1] and totals[3] > 2 * CH and totals[4] > CH
    assert clen[0] == 0 and clen[-1] == 0 and 0 < ncols % cpb < cpb
    assert sorted(clen[3 * cpb:4 * cpb])[-2] > CH and clen[3 * cpb:4 * cpb].max() > 2 * CH
    assert colptr[3 * cpb - 1] - colptr[2 * cpb] == CH             # the last column of the CH + 1 workgroup starts on the boundary
    X = sc.master_B(sc.T_ROWS, sc.XMAX, seed=13)
    strad = sc.straddlers(colptr, CH, cpb)
    assert len(strad) >= 3 and any(len(cuts) >= 2 for _, cuts in strad)
    for c, cuts in strad:
        lo, hi = int(colptr[c]), int(colptr[c + 1])
        assert cuts[0] >= 2 and hi - lo - cuts[-1] >= 2
        told = sc.discriminated(va[M["perm"][lo:hi]], X[M["rowidx"][lo:hi], :2], cuts)
        assert told.all(), f"column {c}: X columns {np.flatnonzero(~told)} do not discriminate"
    # seq_transposed_ref is the oracle's product with the explicit transpose
    trp, tcv, tva = sc.transposed_csr(rp, cv, va, ncols)
    Xm = np.ascontiguousarray(X[:, :3])
    np.testing.assert_array_equal(sc.seq_transposed_ref(rp, cv, va, Xm, ncols), orc.spmm(trp.astype(I32), tcv.astype(I32), tva, Xm))


def test_run_tile_blocks_are_marked_as_their_names_claim():
    cases = sc.runs_cases()
    assert [c["kind"] for c in cases] == ["odd", "even", "all"]
    for case in cases:
        rp, cv, n, N = case["rowptr"], case["colval"], case["nrows"], case["n_own"]
        _assert_csr(rp, cv, case["ncols"])
        assert N % 2 == (1 if case["kind"] == "odd" else 0) and n % sc.RPB_MM == 1
        restated = sc.run_descriptors(rp, cv, n, N)
        claims = sc.runs_claims(case["kind"])
        by_name = dict(zip(case["names"], restated))
        totals = dict(zip(case["names"], (int(rp[min(b + sc.RPB_MM, n)] - rp[b]) for b in range(0, n, sc.RPB_MM))))
        for name, block in by_name.items():
            assert (block[0], sc.colmajor_fits(block, N)) == claims[name], (case["kind"], name, block)
        runs = {name: len(b[1]) for name, b in by_name.items()}
        rows = {name: int(b[2].sum()) for name, b in by_name.items()}
        assert runs["4 runs, one of length 1"] == 4 and 1 in by_name["4 runs, one of length 1"][2] and runs["5 runs"] == 5
        assert (rows["T=199"], rows["T=200"], rows["T=201"], rows["T=9"], rows["T=1"]) == (199, 200, 201, 9, 1)
        assert {rows[x] % 8 for x in ("T=199", "T=200", "T=9")} == {7, 0, 1}
        assert [totals[f"E={e}"] for e in (256, 257, 511, 512, 513)] == [256, 257, 511, 512, 513]
        assert totals["300 columns in 400 entries"] <= sc.RUNS_EMAX and rows["300 columns in 400 entries"] > sc.RUNS_TILE_ROWS
        assert runs["run across N"] == (1 if case["kind"] == "all" else 2)
        b = by_name["own run to N-1"]
        assert b[1][0] + b[2][0] == sc.RUNS_N_OWN["odd" if case["kind"] != "even" else "even"]
        widened = lambda blk: sum(((s + l + 1) & ~1) - (s & ~1) for s, l in zip(blk[1].tolist(), blk[2].tolist()))   # noqa: E731
        assert widened(by_name["widened 200"]) == 200 and widened(by_name["widened 202"]) == 202
        assert rows["widened 202"] <= sc.RUNS_TILE_ROWS
        assert totals["empty"] == 0 and by_name["empty"][0] and case["names"][-1] == "last, nr=1"
        if case["kind"] != "all":
            assert by_name["ghost run only"][1][0] >= N
        for max_runs in (3, 4, 5):
            assert 0 < sc.banded_count(rp, cv, n, N, max_runs) < len(restated)
        assert sc.banded_count(rp, cv, n, N, 3) < sc.banded_count(rp, cv, n, N, 4) < sc.banded_count(rp, cv, n, N, 5)


def test_structure_cases_put_an_entry_in_the_last_column():
    assert sc.STRUCT_NCOLS == (1, 2, 3, 256, 257, 65536, 65537)
    for ncols, rowptr, colval in sc.struct_cases():
        _assert_csr(rowptr, colval, ncols)
        assert colval.max() == ncols - 1 and np.any(np.diff(rowptr) == 0)
        colptr, rowidx, perm = sc.csc_struct_ref(rowptr, colval, ncols)
        assert colptr[-1] == len(colval) and np.all(np.diff(colptr) >= 0) and colptr[ncols] - colptr[ncols - 1] >= 1
        assert np.array_equal(np.sort(perm), np.arange(len(colval)))
        for c in (0, ncols - 1):
            assert np.all(np.diff(rowidx[colptr[c]:colptr[c + 1]]) > 0)     # stable: ascending rows within a column
