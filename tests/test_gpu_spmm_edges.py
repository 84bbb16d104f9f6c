"""The SpMM kernels of csrc/spmm.hip and the transposed product of csrc/spmm_t.hip at the constants they branch on, through
the raw C ABI, bit for bit against the oracle's column loop (orc.spmm: one running sum per C(r, c) in stored order, multiply
and add rounded separately).  Inputs, case tables and references come from tests/_spmm_edge_cases.py, which
tests/test_spmm_edge_cases.py checks on the CPU: block totals on, below and above the records a pass stages; rows that end on,
start on and straddle a pass boundary, with values for which per-pass partial sums give other bits than one running sum; run
tiles on 4 | 5 runs, 200 | 201 tile rows, 512 | 513 entries; columns of the transposed product on its 1024-record pass and
widths past one column tile.

Every output is prefilled with NaN and so is the padding of every input pitch: what a call must not write is NaN afterwards
(or, where the sources say so, the 0.0 that a whole-line store puts into the padding column of an odd k), and no NaN may reach
a result.

Which kernel instance a call starts is not observed on the GPU: it rests on the host restatement sc.variant_of and on the
presence of the restated `const bool` lines of spmm_launch in the source.  A change to the bodies of the launch macros
(HPCLA_SPMM_VEC1 / _VECC) that keeps those lines would lose coverage without a failure here.

Wall times on the MI355X (pytest's own figures, one run).  This module: 46 tests in 3.9 s; the slowest case is
test_vector_kernel_at_pass_edges[512-int32-0] at 1.9 s (the first HIP call of the process and the oracle's products are in
it), every other case at most 0.31 s (vector 0.06 - 0.12 s, generic 0.07 - 0.09 s, run tiles and transposed 0.01 - 0.02 s).
The modules around it, with this change | at the parent commit: test_gpu_kernel_variants 41.7 s | 37.5 s (the worker's new
checks add about 0.5 s to each of its eight children), test_gpu_parity 33.0 s | 30.3 s, test_gpu_colmajor 9.7 s and
test_gpu_dense_sparse 13.1 s (neither file changed; not timed at the parent).

Three mutations of the kernels, each built apart and run once against this module and the existing SpMM tests, none kept:
(a) `rows >= RUNS_TILE_ROWS` in spmm_runs_build_kernel: the six cases of test_run_tiles_at_their_limits fail at the block
    "T=200" -- and so do the two of the existing test_gpu_colmajor.py::test_spmm_run_tiles_on_colmajor_blocks, which already
    holds a 200-row block; 202 other tests pass.
(b) the sums a0, a1 of spmm_t_kernel declared before its column-tile loop: test_transposed_product_at_pass_and_tile_edges at
    m = 65, 66, 130 (both index types) and both operator cases fail; nothing else does, tests/test_gpu_dense_sparse.py included.
(c) the vector kernel's pass clip at `ch + n - 1` (the last record of every pass dropped): all eight cases of
    test_vector_kernel_at_pass_edges (CH = 512 under the default environment among them) and both of
    test_switch_between_the_two_pass_sizes fail, next to 100 existing SpMM tests of test_gpu_parity.py and
    test_gpu_colmajor.py."""
import ctypes

import numpy as np
import pytest

from tests import _spmm_edge_cases as sc

pytestmark = pytest.mark.gpu

I32, I64 = np.int32, np.int64
NAN = float("nan")
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _matrix(CH):
    return _memo(("pass", CH), lambda: sc.pass_matrix(CH))


def _want(orc, tag, M, k):
    """The oracle's product of M with the first k columns of the master B: computed once per (matrix, k), never changed."""
    def make():
        B = np.ascontiguousarray(_memo("B", sc.master_B)[:, :k])
        C = orc.spmm(M["rowptr"].astype(I32), M["colval"].astype(I32), M["vals"], B)
        C.setflags(write=False)
        return C
    return _memo(("want", tag, k), make)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _padded(M, pitch):
    out = np.full((M.shape[0], pitch), NAN)
    out[:, :M.shape[1]] = M
    return out


def _nan(*shape):
    import torch
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def _sfx(Ti):
    return "i32" if Ti == I32 else "i64"


def _check_row_major(got, want, k, what):
    np.testing.assert_array_equal(got[:, :k], want, err_msg=what)
    # the padding of C: untouched, or -- odd k on the pitch k + 1 <= 16 only, rows leaving as whole lines -- column k set to 0.0
    pad = got[:, k:]
    if k % 2 == 1 and got.shape[1] == k + 1 <= sc.KT:
        assert np.all(np.isnan(pad) | (pad == 0.0)), f"{what}: padding of C"
    else:
        assert np.all(np.isnan(pad)), f"{what}: padding of C"


def _check_col_major(got, want, n, what):
    np.testing.assert_array_equal(got[:, :n].T, want, err_msg=what)
    assert np.all(np.isnan(got[:, n:])), f"{what}: padding of C"


def _rows_of_blocks(blocks, n):
    return np.concatenate([np.arange(b * sc.RPB_MM, min((b + 1) * sc.RPB_MM, n)) for b in blocks])


def _run_cases(hp, orc, tag, M, cases, Ti, base):
    """Every call of `cases` (sc.vec_cases / sc.generic_cases) on the matrix M, against the oracle."""
    import torch
    sfx, s = _sfx(Ti), _stream()
    call = hp._capi.call
    ROW, COL = hp._capi.LAYOUT_ROW, hp._capi.LAYOUT_COL
    n, ncols, n_own, nnz = M["nrows"], M["ncols"], M["n_own"], len(M["colval"])
    d_rp, d_cv, d_nz = _t((M["rowptr"] + base).astype(Ti)), _t((M["colval"] + base).astype(Ti)), _t(M["vals"])
    lists = sc.block_lists(M)
    interior, boundary = (_t(x) for x in lists)
    interior_rows, boundary_rows = (_rows_of_blocks(x, n) for x in lists)
    panels = [(_t((prp + base).astype(Ti)), _t((pcv + base).astype(Ti)), _t(pval), lo, hi) for prp, pcv, pval, lo, hi in sc.panels_of(M)]
    Bm = _memo("B", sc.master_B)
    for case in cases:
        k, ldb, ldg, ldc, entry = case["k"], case["ldb"], case["ldg"], case["ldc"], case["entry"]
        what = f"{tag} {case} {sfx} base {base}"
        want = _want(orc, tag, M, k)
        B = Bm[:, :k]
        off = 0 if case.get("aligned", True) else 1          # B eight bytes past a 16-byte boundary

        def place(block, pitch, off=0):
            """(tensor kept alive, address): the rows of `block` on `pitch` behind `off` NaN doubles, NaN in the padding."""
            buf = _t(np.concatenate([np.full(off, NAN), _padded(block, pitch).ravel(), np.full(2, NAN)]))
            assert buf.data_ptr() % 16 == 0
            return buf, buf.data_ptr() + 8 * off
        ccol = case.get("ccol", False)
        dC = _nan(k, ldc) if ccol else _nan(n, ldc)
        if entry == "csr":
            if case.get("b_col"):
                keep, pB = place(B.T, ldb)                    # column-major B: k columns of ldb >= ncols doubles
            else:
                keep, pB = place(B, ldb, off)
            call(f"hpcla_spmm_csr_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), pB, ldb,
                 COL if case.get("b_col") else ROW, dC.data_ptr(), ldc, COL if ccol else ROW, n, nnz, k, base, s)
        elif entry in ("split", "split_ccol"):
            keep_o, pBo = place(B[:n_own], ldb, off)
            keep_g, pBg = place(B[n_own:], ldg)
            name = f"hpcla_spmm_split_f64_{sfx}" if entry == "split" else f"hpcla_spmm_split_ccol_f64_{sfx}"
            for step, blocks in enumerate((boundary, interior)):
                call(name, d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), pBo, ldb, pBg, ldg, n_own, dC.data_ptr(), ldc, n, nnz,
                     k, base, blocks.data_ptr(), blocks.numel(), s)
                if step == 0:                                # rows outside the list stay NaN
                    got = dC.cpu().numpy()
                    got = got[:, :n].T if ccol else got
                    assert np.all(np.isnan(got[interior_rows])), f"{what}: a block outside the list was written"
                    np.testing.assert_array_equal(got[boundary_rows][:, :k], want[boundary_rows], err_msg=what)
        else:                                                # panel order: own columns, then two ghost panels, one running sum
            keep_o, pBo = place(B[:n_own], ldb, off)
            keep_g = []
            for q, (prp, pcv, pval, lo, hi) in enumerate(panels):
                if q == 0:
                    pn_own, pBg = n_own, pBo                  # (no column of this panel is a ghost; the segment is not read)
                    keep_g.append(None)
                else:
                    kg, pBg = place(B[lo:hi], ldg)
                    keep_g.append(kg)
                    pn_own = 0                                # every column is a position in the panel's own buffer
                call(f"hpcla_spmm_panel_f64_{sfx}", prp.data_ptr(), pcv.data_ptr(), pval.data_ptr(), pBo, ldb, pBg if q else None,
                     ldg, pn_own, dC.data_ptr(), ldc, n, pval.numel(), k, base, 0 if q == 0 else 1, s)
        torch.cuda.synchronize()
        got = dC.cpu().numpy()
        if ccol:
            _check_col_major(got, want, n, what)
        else:
            _check_row_major(got, want, k, what)


# ---- the vector kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("Ti", [I32, I64])
@pytest.mark.parametrize("CH", [sc.CHUNK_V_SMALL, sc.CHUNK_V_LARGE])
def test_vector_kernel_at_pass_edges(hp, orc, CH, Ti, base):
    """spmm_rowblock_vec_kernel on pass_matrix(CH) -- CH = 512 has nnz == 8 * nrows, so the default environment stages 512
    records per pass and its 3 CH + 7 block holds a row that spans two whole passes -- through hpcla_spmm_csr_f64_* (row- and
    column-major C, one launch per 16-column tile when k > 16), hpcla_spmm_split_f64_* / _split_ccol_* (ghost segment on a pitch
    of its own, boundary blocks first: the interior blocks' rows stay NaN) and hpcla_spmm_panel_f64_* with accumulate = 1; every
    k of sc.VEC_KS on the tight and the padded even pitch: every kernel instance spmm_launch can start
    (tests/test_spmm_edge_cases.py)."""
    M = _matrix(CH)
    _run_cases(hp, orc, f"pass{CH}", M, sc.vec_cases(M["nrows"]), Ti, base)


# ---- the generic kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ti,base", [(I32, 0), (I32, 1), (I64, 0), (I64, 1)])
def test_generic_kernel_at_pass_edges(hp, orc, Ti, base):
    """spmm_rowblock_kernel (GRP = 4, 8, 16) on pass_matrix(CHUNK_MM), reached by a tight odd pitch, by a column-major B with a
    row-major C and by a B that starts eight bytes past a 16-byte boundary; unsplit, split with block lists, panel order.  The
    rows of one lane group have lengths 0, 1, 7 and CHUNK_MM + 101, and the first ghost column (offset -1 in the kernel's
    encoding) stands alone in a row and in every straddling row."""
    M = _matrix(sc.CHUNK_MM)
    _run_cases(hp, orc, f"pass{sc.CHUNK_MM}", M, sc.generic_cases(M["ncols"]), Ti, base)


# ---- nnz == 8 * nrows against 8 * nrows + 1 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ti", [I32, I64])
def test_switch_between_the_two_pass_sizes(hp, orc, Ti):
    """Two matrices that differ by one entry, on either side of `nnz <= 8 * nrows`: both give the oracle's bits."""
    a, b = _memo("pair", sc.switch_pair)
    for tag, M in (("switch 8n", a), ("switch 8n+1", b)):
        n = M["nrows"]
        cases = [dict(entry=e, k=k, ldb=ldb, ldg=ldb, ldc=n if ccol else ldb, ccol=ccol)
                 for k, ldb in ((16, 16), (6, 6), (15, 16), (40, 40)) for e, ccol in (("csr", False), ("csr", True), ("split", False))]
        _run_cases(hp, orc, tag, M, cases, Ti, 0)


# ---- run tiles ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ti", [I32, I64])
@pytest.mark.parametrize("kind", ["odd", "even", "all"])
def test_run_tiles_at_their_limits(hp, orc, kind, Ti):
    """hpcla_spmm_runs_build_* on the hand-built blocks of sc.runs_blocks: descriptors and n_fit against the host restatement
    (4 | 5 runs, 199 | 200 | 201 tile rows, 256 ... 513 entries, a run cut at an odd / even n_own); hpcla_spmm_banded_blocks_*
    at max_runs 3, 4, 5; the products of hpcla_spmm_runs_k16_f64_* and hpcla_spmm_runs_colmajor_k16_f64_* (widened runs of 200
    and 202 rows, an own run that ends at row n_own - 1) for fitting and marked blocks alike, natural and permuted order."""
    import torch
    case = next(c for c in _memo("runs", sc.runs_cases) if c["kind"] == kind)
    lib, call, sfx, s, k = hp._capi.load(), hp._capi.call, _sfx(Ti), _stream(), sc.KT
    rp, cv, va, n, ncols, n_own = case["rowptr"], case["colval"], case["vals"], case["nrows"], case["ncols"], case["n_own"]
    nnz, nblk = len(cv), -(-n // sc.RPB_MM)
    Bg = sc.master_B(ncols, k, seed=23)
    want = orc.spmm(rp.astype(I32), cv.astype(I32), va, Bg)
    restated = sc.run_descriptors(rp, cv, n, n_own)
    d_nz = _t(va)
    dB_own = _t(Bg[:n_own])                                              # row-major, 16 doubles per row
    dB_gh = _t(Bg[n_own:]) if n_own < ncols else None
    ldb = n_own + (n_own & 1) + 2                                        # column-major own block: even leading dimension
    dB_cm = _t(_padded(Bg[:n_own].T, ldb))
    ldg = k + 2
    dB_gh_cm = _t(_padded(Bg[n_own:], ldg)) if n_own < ncols else None
    ldc = n + 3
    perm = _t(np.random.default_rng(4).permutation(nblk).astype(I32))
    for base in (0, 1):
        d_rp, d_cv = _t((rp + base).astype(Ti)), _t((cv + base).astype(Ti))
        desc = torch.full((lib.hpcla_spmm_runs_desc_bytes(n),), 0xEE, dtype=torch.uint8, device="cuda")
        n_fit = ctypes.c_int64(-1)
        call(f"hpcla_spmm_runs_build_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), n, nnz, base, n_own, desc.data_ptr(), ctypes.byref(n_fit), s)
        d = desc.cpu().numpy().view(np.int32).reshape(nblk, 2 * sc.RUNS_MAX)
        fit = sc.check_descriptors(d, n_fit.value, restated)
        assert fit == sum(f for f, _ in sc.runs_claims(kind).values())
        for max_runs in (3, 4, 5):
            count = ctypes.c_int64(-1)
            call(f"hpcla_spmm_banded_blocks_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), n, nnz, base, n_own, max_runs, ctypes.byref(count), s)
            assert count.value == sc.banded_count(rp, cv, n, n_own, max_runs), (max_runs, count.value)
        for lst in (None, perm):
            what = f"{kind} {sfx} base {base} list {lst is not None}"
            C = _nan(n, k)
            call(f"hpcla_spmm_runs_k16_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), dB_own.data_ptr(),
                 dB_gh.data_ptr() if dB_gh is not None else None, n_own, C.data_ptr(), n, nnz, base, desc.data_ptr(),
                 lst.data_ptr() if lst is not None else None, nblk if lst is not None else 0, s)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(C.cpu().numpy(), want, err_msg="row-major run tiles " + what)
            C = _nan(k, ldc)
            call(f"hpcla_spmm_runs_colmajor_k16_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), dB_cm.data_ptr(), ldb,
                 dB_gh_cm.data_ptr() if dB_gh_cm is not None else None, ldg, n_own, C.data_ptr(), ldc, n, nnz, base, desc.data_ptr(),
                 lst.data_ptr() if lst is not None else None, nblk if lst is not None else 0, s)
            torch.cuda.synchronize()
            _check_col_major(C.cpu().numpy(), want, n, "column-major run tiles " + what)


# ---- the transposed product ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ti", [I32, I64])
def test_transposed_structure_at_key_widths(hp, Ti):
    """hpcla_spmm_t_struct_*: colptr_t, rowidx_t and perm against a stable numpy argsort, with ncols on, one above and far from
    a power of two (the key bits of the radix sort) and an entry in the last column."""
    import torch
    lib, sfx, s = hp._capi.load(), _sfx(Ti), _stream()
    tdt = torch.int32 if Ti == I32 else torch.int64
    for ncols, rowptr, colval in sc.struct_cases():
        nrows, nnz = len(rowptr) - 1, len(colval)
        colptr, rowidx, perm = sc.csc_struct_ref(rowptr, colval, ncols)
        d_rp, d_cv = _t(rowptr.astype(Ti)), _t(colval.astype(Ti))
        d_colptr = torch.full((ncols + 2,), -7, dtype=tdt, device="cuda")           # one guard element behind each output
        d_rowidx = torch.full((nnz + 1,), -7, dtype=tdt, device="cuda")
        d_perm = torch.full((nnz + 1,), -7, dtype=tdt, device="cuda")
        wb = lib.hpcla_spmm_t_struct_work_bytes(nnz, ncols, int(Ti == I64))
        assert wb > 0
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        hp._capi.call(f"hpcla_spmm_t_struct_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), nrows, nnz, ncols, d_colptr.data_ptr(),
                      d_rowidx.data_ptr(), d_perm.data_ptr(), work.data_ptr(), wb, s)
        torch.cuda.synchronize()
        for name, got, ref in (("colptr_t", d_colptr, colptr), ("rowidx_t", d_rowidx, rowidx), ("perm", d_perm, perm)):
            got = got.cpu().numpy()
            np.testing.assert_array_equal(got[:-1], ref, err_msg=f"{name} at ncols = {ncols} ({sfx})")
            assert got[-1] == -7, f"{name} at ncols = {ncols}: written past the end"


def _t_want(m):
    def make():
        M = _memo(("t", sc.TPB_T // sc.spmm_t_lpc(m)), lambda: sc.spmm_t_matrix(sc.TPB_T // sc.spmm_t_lpc(m)))
        X = np.ascontiguousarray(_memo("X", lambda: sc.master_B(sc.T_ROWS, sc.XMAX, seed=13))[:, :m])
        W = sc.seq_transposed_ref(M["rowptr"], M["colval"], M["vals"], X, M["ncols"])
        W.setflags(write=False)
        return M, X, W
    return _memo(("t_want", m), make)


@pytest.mark.parametrize("Ti", [I32, I64])
@pytest.mark.parametrize("m", sc.SPMM_T_MS)
def test_transposed_product_at_pass_and_tile_edges(hp, m, Ti):
    """hpcla_spmm_t_f64_* on sc.spmm_t_matrix: workgroups of 1023, 1024, 1025 and > 3072 records, columns longer than one and
    than two passes, empty first and last columns, a short last workgroup; X as rows on an even and an odd padded pitch and as
    columns, W as rows on a padded pitch and as columns: every (LPC, VEC, WCOL) instance.  m = 65, 66, 130 run a second and a
    third column tile, whose sums must start at 0.0 again.  Bit-equal to one running sum per column in ascending row order."""
    import torch
    M, X, want = _t_want(m)
    sfx, s, ncols = _sfx(Ti), _stream(), M["ncols"]
    ROW, COL = hp._capi.LAYOUT_ROW, hp._capi.LAYOUT_COL
    d_colptr, d_rowidx, d_perm, d_nz = _t(M["colptr"].astype(Ti)), _t(M["rowidx"].astype(Ti)), _t(M["perm"].astype(Ti)), _t(M["vals"])
    for c in sc.spmm_t_calls(m, ncols):
        what = f"m={m} {c} {sfx}"
        dX = _t(_padded(X, c["ldx"]) if c["x_row"] else _padded(X.T, c["ldx"]))
        assert dX.data_ptr() % 16 == 0
        dW = _nan(m, c["ldw"]) if c["w_col"] else _nan(ncols, c["ldw"])
        hp._capi.call(f"hpcla_spmm_t_f64_{sfx}", d_colptr.data_ptr(), d_rowidx.data_ptr(), d_perm.data_ptr(), d_nz.data_ptr(), ncols,
                      dX.data_ptr(), c["ldx"], ROW if c["x_row"] else COL, m, dW.data_ptr(), c["ldw"], COL if c["w_col"] else ROW, s)
        torch.cuda.synchronize()
        got = dW.cpu().numpy()
        if c["w_col"]:
            got = got.T                                      # (ldw, m): rows past ncols are padding
            np.testing.assert_array_equal(got[:ncols], want, err_msg=what)
            assert np.all(np.isnan(got[ncols:])), f"{what}: padding of W"
        else:
            np.testing.assert_array_equal(got[:, :m], want, err_msg=what)
            assert np.all(np.isnan(got[:, m:])), f"{what}: padding of W"


@pytest.mark.parametrize("m", [65, 130])
def test_transposed_product_through_the_operators_past_one_tile(hp, m):
    """transpose(X) @ A and X @ A with more than 64 columns of X: a second (and third) column tile per workgroup."""
    import scipy.sparse as sp
    M, X, want = _t_want(m)
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    S = sp.csr_matrix((M["vals"], M["colval"], M["rowptr"]), shape=(M["nrows"], M["ncols"]))
    A = hp.HPCSparseMatrix_from_global(S, backend)
    got = (hp.transpose(hp.HPCMatrix.from_global(X, backend)) @ A).gather()
    np.testing.assert_array_equal(got, want.T)
    got = (hp.HPCMatrix.from_global(np.ascontiguousarray(X.T), backend) @ A).gather()
    np.testing.assert_array_equal(got, want.T)
    del A
    hp.clear_plan_cache()
