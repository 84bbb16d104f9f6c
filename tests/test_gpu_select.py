"""Index-set selection on the device (csrc/select.hip, linearalgebrampi.jl_amd/select.py) against the loop restatement of
tests/_select_cases.py -- which tests/test_select_cases.py holds against scipy -- on one rank, and through
tests/_multirank_select_worker.py on 2 and 3 ranks sharing the GPU.

Every case runs through the raw C ABI (both index types, both index bases, outputs pre-filled with a sentinel and padded so
that an unwritten or an overrun entry shows; a second fill goes to outputs 1 element off a 16-byte boundary with the longest
row declared unknown, so the scalar stores and all three forms run) and through ``hp.select``.  Structure arrays are compared
with array_equal, values as integers: no tolerance appears, the operation moves bits.  Products over the result are compared
bitwise with the oracle's loops over the restated CSR (NaN where the oracle gives NaN): they show that columns ascend and
that the plan machinery accepts the result.

The edge matrix holds rows whose KEPT length is 0, 1 and cap - 1, cap, cap + 1 for both caps of the fill (read from the
library below) and 2 * tile + 3; the band cases select 2 * SCAN_CHUNK + 1 rows and columns, so both scans cross chunks."""
import ctypes
import os

import numpy as np
import pytest

from tests import _select_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_select_worker.py")

pytestmark = pytest.mark.gpu

SENT = -7
_cache = {}


def _torch():
    import torch
    return torch


def _backend(hp, Ti, T=np.float64):
    key = ("backend", np.dtype(Ti).name, np.dtype(T).name)
    if key not in _cache:
        _cache[key] = hp.backend_rocm_serial(T, Ti)
    return _cache[key]


def _csr(key, T=np.float64):
    A = sc.matrix(key)
    return A if T == np.float64 else A.with_values(A.data.astype(T))


def _matrix(hp, key, Ti, T=np.float64):
    """The case matrix on the device (built once per module) and integer snapshots of its three device arrays."""
    k = ("matrix", key, np.dtype(Ti).name, np.dtype(T).name)
    if k not in _cache:
        C = _csr(key, T)
        A = hp.HPCSparseMatrix_local(C.indptr, C.indices, C.data, C.shape[1], _backend(hp, Ti, T))
        torch = _torch()
        snap = (A.nzval.view(torch.int64 if T == np.float64 else torch.int32).clone(), A.rowptr_target.clone(),
                A.colval_target().clone())
        _cache[k] = (A, snap)
    return _cache[k]


def _unchanged(A, snap, T=np.float64):
    torch = _torch()
    return (torch.equal(A.nzval.view(torch.int64 if T == np.float64 else torch.int32), snap[0])
            and torch.equal(A.rowptr_target, snap[1]) and torch.equal(A.colval_target(), snap[2]))


def _expected(C, A, rows, cols):
    return sc.expected_on_rank(C, A.row_partition, 0, None if rows is None else [rows], None if cols is None else [cols],
                               col_partition=A.col_partition)


def _assert_matrix(B, e, Ti, what, hashed=False):
    assert np.array_equal(B.row_partition, e["row_partition"]) and np.array_equal(B.col_partition, e["col_partition"]), what
    assert B.rowptr.dtype == Ti and B.colval.dtype == Ti and B.col_indices.dtype == np.int64, what
    assert B.nrows_local == len(e["rowptr"]) - 1 and B.ncols_compressed == len(e["col_indices"]) and B.nnz == len(e["vals"]), what
    assert np.array_equal(B.rowptr, e["rowptr"]), what
    assert np.array_equal(B.col_indices, e["col_indices"]), what
    assert np.array_equal(B.colval, e["colval"]), what
    got = B.nzval.cpu().numpy()
    assert got.dtype == e["vals"].dtype and np.array_equal(sc.bits(got), sc.bits(e["vals"])), what
    assert np.array_equal(B.rowptr_target.cpu().numpy(), e["rowptr"]), what
    assert np.array_equal(B._col_indices_dev.cpu().numpy(), e["col_indices"]), what
    assert (B.structural_hash is not None) == hashed, what                # plain select hashes nothing: the hash is lazy


def _assert_product_bits(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(sc.bits(got)[~nan], sc.bits(want)[~nan]), what
    assert np.isnan(got[nan]).all(), what


def _products(hp, orc, B, e, Ti, T, what):
    """B @ x and B @ X (k = 3) against the oracle's loops over the restated CSR."""
    n = B.shape[1]
    xg = (1.0 + orc.fill_uniform(0, n, orc.SEED_X)).astype(T)
    Xg = np.ascontiguousarray(np.stack([xg, 0.5 - xg, xg * xg], axis=1)).astype(T)
    rp, cv = e["rowptr"].astype(Ti), e["colval"].astype(Ti)
    y = B @ hp.HPCVector.from_global(xg, B.backend)
    assert np.array_equal(y.partition, e["row_partition"]), what
    _assert_product_bits(y.local_values(), orc.spmv(rp, cv, e["vals"], xg[e["col_indices"]]), what + " B @ x")
    Y = B @ hp.HPCMatrix.from_global(Xg, B.backend)
    want = orc.spmm(rp, cv, e["vals"], np.ascontiguousarray(Xg[e["col_indices"]]))
    _assert_product_bits(Y.local_values().reshape(-1), want.reshape(-1), what + " B @ X")


def _upload(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def test_the_library_has_the_constants_the_cases_assume(hp):
    lib = hp._capi.load()
    assert lib.hpcla_select_short_cap() == sc.SHORT_CAP and lib.hpcla_select_tile() == sc.TILE
    assert lib.hpcla_submatrix_scan_chunk() == sc.SCAN_CHUNK


@pytest.mark.parametrize("Ti", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_select_matches_the_restatement(hp, orc, case, Ti):
    name, key = case[0], case[1]
    rows, cols = sc.case_lists(case)
    A, snap = _matrix(hp, key, Ti)
    e = _expected(sc.matrix(key), A, rows, cols)
    as_tensor = sc.IDS.index(name) % 2 == 1                               # every other case passes device tensors
    B = hp.select(A, _upload(rows) if as_tensor and rows is not None else rows,
                  _upload(cols) if as_tensor and cols is not None else cols)
    _assert_matrix(B, e, Ti, name)
    if B.shape[0] and B.shape[1]:
        _products(hp, orc, B, e, Ti, np.float64, name)
    assert _unchanged(A, snap), name + ": the input changed"


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("Ti", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_raw_abi_matches_the_restatement(hp, case, Ti, base):
    from hpcla_amd.vectors import current_stream_ptr, dptr
    torch = _torch()
    name, key = case[0], case[1]
    rows, cols = sc.case_lists(case)
    A, snap = _matrix(hp, key, Ti)
    C = sc.matrix(key)
    m, n = C.shape
    e = sc.restate(C, 0, m, rows, cols)
    sfx = "i64" if Ti == np.int64 else "i32"
    tdt = torch.int64 if Ti == np.int64 else torch.int32
    rowptr = _upload((A.rowptr + base).astype(Ti))
    colval = _upload((A.colval + base).astype(Ti))
    ci_src = _upload(A.col_indices + base)                        # 1-based global columns for a 1-based caller
    ncomp = len(A.col_indices)
    rows_d = None if rows is None else _upload(rows)              # positions: 0-based whatever the base
    nsel = m if rows is None else len(rows)
    if cols is None:
        sorted_cols = sorted_pos = None
        nsorted, width = -1, n
    else:
        order = np.argsort(cols, kind="stable")
        sorted_cols, sorted_pos = _upload(cols[order] + base), _upload(order.astype(np.int64))
        nsorted = width = len(cols)
    lib = hp._capi.load()
    work = torch.full((lib.hpcla_select_work_bytes(nsel, ncomp, width),), 0x5A, dtype=torch.uint8, device="cuda")
    cap = min(width, ncomp)
    rowptr_out = torch.full((nsel + 1 + 4,), SENT, dtype=tdt, device="cuda")
    ci_out = torch.full((cap + 4,), SENT, dtype=torch.int64, device="cuda")
    nnz_out, ncomp_out, max_row = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    s = current_stream_ptr()
    hp._capi.call(f"hpcla_select_structure_{sfx}", dptr(rowptr), dptr(colval), m, A.nnz, dptr(ci_src), ncomp, dptr(rows_d), nsel,
                  dptr(sorted_cols), dptr(sorted_pos), nsorted, width, base, dptr(rowptr_out), dptr(ci_out), ctypes.byref(nnz_out),
                  ctypes.byref(ncomp_out), ctypes.byref(max_row), dptr(work), s)
    assert nnz_out.value == len(e["vals"]) and ncomp_out.value == len(e["col_indices"]), name
    assert max_row.value == (int(np.diff(e["rowptr"]).max()) if nsel else 0), name
    rp = rowptr_out.cpu().numpy()
    assert np.array_equal(rp[:nsel + 1], e["rowptr"] + base) and np.all(rp[nsel + 1:] == SENT), name
    ci = ci_out.cpu().numpy()
    assert np.array_equal(ci[:ncomp_out.value], e["col_indices"] + base) and np.all(ci[ncomp_out.value:] == SENT), name
    nnz = nnz_out.value
    # aligned outputs with the longest row as returned; then 1 element off a 16-byte boundary with the longest row unknown
    for off, longest in ((0, max_row.value), (1, -1)):
        colval_out = torch.full((nnz + 9,), SENT, dtype=tdt, device="cuda")
        nzval_out = torch.full((nnz + 9,), float(SENT), dtype=torch.float64, device="cuda")
        src_out = torch.full((nnz + 9,), SENT, dtype=torch.int64, device="cuda")
        hp._capi.call(f"hpcla_select_fill_{sfx}", 8, dptr(rowptr), dptr(colval), dptr(A.nzval), m, A.nnz, ncomp, dptr(rows_d), nsel,
                      dptr(rowptr_out), nnz, longest, base, dptr(work), dptr(colval_out[off:]), dptr(nzval_out[off:]),
                      dptr(src_out[off:]), s)
        cv, nz, sr = colval_out.cpu().numpy(), nzval_out.cpu().numpy(), src_out.cpu().numpy()
        what = (name, off)
        assert np.array_equal(cv[off:off + nnz], e["colval"] + base), what
        assert np.array_equal(sc.bits(nz[off:off + nnz]), sc.bits(e["vals"])), what
        assert np.array_equal(sr[off:off + nnz], e["src"]), what
        for a in (cv, nz, sr):
            assert np.all(a[:off] == SENT) and np.all(a[off + nnz:] == SENT), what
    # the values pass: the gather of the library over the recorded positions
    again = torch.full((nnz + 4,), float(SENT), dtype=torch.float64, device="cuda")
    if nnz:
        hp._capi.call("hpcla_gather_f64_i64", dptr(A.nzval), dptr(src_out[1:]), None, dptr(again), nnz, 0, s)
    nz2 = again.cpu().numpy()
    assert np.array_equal(sc.bits(nz2[:nnz]), sc.bits(e["vals"])) and np.all(nz2[nnz:] == SENT), name
    assert _unchanged(A, snap), name + ": the input changed"


def test_float32_values_and_int64_indices_keep_their_types(hp, orc):
    T = np.float32
    torch = _torch()
    for Ti in (np.int32, np.int64):
        A, snap = _matrix(hp, "edge", Ti, T)
        C = _csr("edge", T)
        assert A.nzval.dtype == torch.float32
        for rspec, cspec in (("rows_repeats", "cols_unsorted_subset"), ("rows_perm", "cols_reversal"), ("none", "none")):
            rows, cols = sc.index_list("edge", rspec), sc.index_list("edge", cspec)
            e = _expected(C, A, rows, cols)
            B = hp.select(A, rows, cols)
            assert B.T == np.dtype(T) and B.Ti == np.dtype(Ti) and B.nzval.dtype == torch.float32
            _assert_matrix(B, e, Ti, "f32")
            _products(hp, orc, B, e, Ti, T, "f32")
        plan = hp.selection_plan(A, sc.index_list("edge", "rows_perm"), sc.index_list("edge", "cols_perm"))
        e = _expected(C, A, sc.index_list("edge", "rows_perm"), sc.index_list("edge", "cols_perm"))
        B2 = plan.extract(A)                                            # the 4-byte gather
        assert B2.nzval.dtype == torch.float32 and np.array_equal(sc.bits(B2.nzval.cpu().numpy()), sc.bits(e["vals"]))
        assert _unchanged(A, snap, T)


def test_a_symmetric_permutation_reproduces_the_product_exactly(hp):
    """Integer entries and an integer vector: every sum is exact, so the permuted product has the unpermuted one's bits."""
    C = sc.matrix("grid33x31")
    n = C.shape[0]
    b = _backend(hp, np.int32)
    A = hp.HPCSparseMatrix_local(C.indptr, C.indices, C.data, n, b)
    rng = np.random.default_rng(33)
    p = rng.permutation(n).astype(np.int64)
    xg = rng.integers(-9, 10, n).astype(np.float64)
    x = hp.HPCVector.from_global(xg, b)
    B = hp.select(A, p, p)
    assert A.structural_hash is None and B.structural_hash is None          # select hashes neither: the hashes are lazy
    lhs = hp.take(A @ x, p)
    assert np.array_equal(B.row_partition, B.col_partition) and B.shape == (n, n) and B.nnz == A.nnz
    rhs = B @ hp.take(x, p)
    assert np.array_equal(sc.bits(lhs.local_values()), sc.bits(rhs.local_values()))
    want = np.zeros(n)
    for r in range(n):
        for q in range(C.indptr[r], C.indptr[r + 1]):
            want[r] += C.data[q] * xg[C.indices[q]]
    assert np.array_equal(sc.bits(lhs.local_values()), sc.bits(want[p]))
    # and back: the inverse permutation restores A
    inv = np.empty(n, dtype=np.int64)
    inv[p] = np.arange(n)
    R = hp.select(B, inv, inv)
    assert np.array_equal(R.rowptr, C.indptr) and np.array_equal(R.col_indices[R.colval], C.indices)
    assert np.array_equal(sc.bits(R.nzval.cpu().numpy()), sc.bits(C.data))


def test_plan_extracts_values_only_and_shares_the_structure(hp, orc):
    A, snap = _matrix(hp, "edge", np.int32)
    C = sc.matrix("edge")
    rows, cols = sc.index_list("edge", "rows_repeats"), sc.index_list("edge", "cols_unsorted_subset")
    plan = hp.selection_plan(A, rows, cols)
    assert isinstance(plan, hp.SelectionPlan)
    e = _expected(C, A, rows, cols)
    B0 = plan.matrix
    _assert_matrix(B0, e, np.int32, "plan.matrix", hashed=True)
    other = C.data[::-1].copy()                                         # new value bits, the specials elsewhere
    A2 = hp.HPCSparseMatrix_local(C.indptr, C.indices, other, C.shape[1], A.backend)
    B2 = plan.extract(A2)
    assert B2.rowptr_target is B0.rowptr_target and B2._colval_target is B0._colval_target
    assert B2.col_indices is B0.col_indices and B2.structural_hash is B0.structural_hash
    assert B2.nzval is not B0.nzval
    e2 = _expected(C.with_values(other), A, rows, cols)
    assert np.array_equal(sc.bits(B2.nzval.cpu().numpy()), sc.bits(e2["vals"]))
    fresh = hp.select(A2, rows, cols)
    assert np.array_equal(sc.bits(B2.nzval.cpu().numpy()), sc.bits(fresh.nzval.cpu().numpy()))
    assert np.array_equal(fresh.rowptr, B2.rowptr) and np.array_equal(fresh.colval, B2.colval)
    assert np.array_equal(sc.bits(plan.extract(A).nzval.cpu().numpy()), sc.bits(e["vals"]))
    # downstream plans are cache hits: the second matrix of the structure builds no VectorPlan
    x = hp.HPCVector.from_global(1.0 + orc.fill_uniform(0, B0.shape[1], orc.SEED_X), A.backend)
    B0 @ x
    before = hp.cache_sizes()["vector_plan_cache"]
    B2 @ x
    assert hp.cache_sizes()["vector_plan_cache"] == before
    # another structure raises: another matrix, the same matrix with one stored column moved, other index or value types
    with pytest.raises(ValueError, match="SelectionPlan.extract: the matrix does not have the structure"):
        plan.extract(_matrix(hp, "band", np.int32)[0])
    idx = C.indices.copy()
    a = C.indptr[4]
    assert idx[a] > 0
    idx[a] -= 1
    moved = hp.HPCSparseMatrix_local(C.indptr, idx, C.data, C.shape[1], A.backend)
    assert moved.nnz == A.nnz
    with pytest.raises(ValueError):
        plan.extract(moved)
    with pytest.raises(ValueError):
        plan.extract(_matrix(hp, "edge", np.int64)[0])
    with pytest.raises(ValueError):
        plan.extract(_matrix(hp, "edge", np.int32, np.float32)[0])
    # the empty forms plan too
    pe = hp.selection_plan(A, np.empty(0, dtype=np.int64), cols)
    assert pe.extract(A2).nnz == 0 and np.array_equal(pe.matrix.row_partition, [0, 0])
    assert _unchanged(A, snap)


def test_dirichlet_elimination_matches_the_host_built_system(hp):
    """K_ff = K[free, free], f_f = f[free] - K[free, fixed] g[fixed], solve, u[free] = u_f, u[fixed] = g[fixed]: the same
    bits and iteration count as hp.cg on the reduced system cut out on the host with scipy and uploaded."""
    import scipy.sparse as sp
    C = sc.matrix("grid24x24")
    nx = 24
    n = C.shape[0]
    b = _backend(hp, np.int32)
    K = hp.HPCSparseMatrix_local(C.indptr, C.indices, C.data, n, b)
    idx = np.arange(n)
    on_edge = (idx % nx == 0) | (idx % nx == nx - 1) | (idx // nx == 0) | (idx // nx == nx - 1)
    fixed, free = idx[on_edge].astype(np.int64), idx[~on_edge].astype(np.int64)
    rng = np.random.default_rng(24)
    fg = rng.standard_normal(n)
    gg = np.where(on_edge, rng.standard_normal(n), 0.0)
    f, g = hp.HPCVector.from_global(fg, b), hp.HPCVector.from_global(gg, b)
    K_ff, K_fc = hp.select(K, free, free), hp.select(K, free, fixed)
    assert np.array_equal(K_ff.row_partition, K_ff.col_partition)
    rhs = hp.take(f, free) - K_fc @ hp.take(g, fixed)
    u_f, info = hp.cg(K_ff, rhs, rtol=1e-10)
    S = sp.csr_matrix((C.data, C.indices, C.indptr), shape=C.shape)
    S_ff, S_fc = sp.csr_matrix(S[free][:, free]), sp.csr_matrix(S[free][:, fixed])
    S_ff.sort_indices()
    S_fc.sort_indices()
    H_ff = hp.HPCSparseMatrix_local(S_ff.indptr, S_ff.indices, S_ff.data, len(free), b)
    H_fc = hp.HPCSparseMatrix_local(S_fc.indptr, S_fc.indices, S_fc.data, len(fixed), b)
    rhs_h = hp.HPCVector.from_global(fg[free], b) - H_fc @ hp.HPCVector.from_global(gg[fixed], b)
    assert np.array_equal(sc.bits(rhs.local_values()), sc.bits(rhs_h.local_values()))
    u_h, info_h = hp.cg(H_ff, rhs_h, rtol=1e-10)
    assert info.converged and info_h.converged and info.iterations == info_h.iterations > 0
    assert np.array_equal(sc.bits(u_f.local_values()), sc.bits(u_h.local_values()))
    u = hp.HPCVector.from_global(np.full(n, np.nan), b)
    assert hp.put_(u, free, u_f) is u
    hp.put_(u, fixed, hp.take(g, fixed))
    want = np.empty(n)
    want[free] = u_h.local_values()
    want[fixed] = gg[fixed]
    assert np.array_equal(sc.bits(u.local_values()), sc.bits(want))


def test_take_and_put(hp):
    torch = _torch()
    b = _backend(hp, np.int32)
    rng = np.random.default_rng(5)
    n = 3001
    vg = rng.standard_normal(n)
    vg[7], vg[8], vg[9] = -0.0, np.nan, np.inf
    v = hp.HPCVector.from_global(vg, b)
    idx = np.concatenate([[n - 1, 7, 7, 0, 8, 9, n - 1], rng.integers(0, n, 2500)]).astype(np.int64)     # out of order, repeats
    w = hp.take(v, idx)
    assert isinstance(w, hp.HPCVector) and np.array_equal(w.partition, [0, len(idx)]) and w.v.is_cuda
    assert w.structural_hash == hp.compute_partition_hash(w.partition)
    assert np.array_equal(sc.bits(w.local_values()), sc.bits(sc.take_of(vg, idx)))
    assert np.array_equal(sc.bits(hp.take(v, _upload(idx)).local_values()), sc.bits(vg[idx]))          # a device tensor
    assert np.array_equal(sc.bits(hp.take(v, torch.from_numpy(idx)).local_values()), sc.bits(vg[idx]))  # a host tensor
    out = hp.HPCVector.zeros(w.partition, b)
    assert hp.take(v, idx, out=out) is out and np.array_equal(sc.bits(out.local_values()), sc.bits(vg[idx]))
    with pytest.raises(ValueError, match="take: out must be"):
        hp.take(v, idx, out=hp.HPCVector.zeros(np.array([0, len(idx) + 1]), b))
    empty = hp.take(v, np.empty(0, dtype=np.int64))
    assert len(empty) == 0 and np.array_equal(empty.partition, [0, 0]) and empty.v.numel() == 0
    # a plan serves many vectors; on one rank no halo plan exists
    ip = hp.index_plan(idx, v.partition, b)
    assert isinstance(ip, hp.VectorIndexPlan) and not ip.has_halo and ip.n_ghost == 0
    v2 = hp.HPCVector.from_global(vg[::-1].copy(), b)
    assert np.array_equal(sc.bits(ip.take(v2).local_values()), sc.bits(vg[::-1][idx]))
    assert np.array_equal(sc.bits(ip.take(v).local_values()), sc.bits(vg[idx]))
    u, c = np.unique(idx, return_counts=True)
    for _ in range(2):                                                                                  # and the verdict is kept
        with pytest.raises(ValueError, match=f"put_: index {u[c > 1].min()} is listed more than once"):
            ip.put_(v, w)
    assert np.array_equal(sc.bits(v.local_values()), sc.bits(vg))
    # a misaligned view operand: local values 8 bytes off a 16-byte boundary
    base = torch.full((n + 1,), float(SENT), dtype=torch.float64, device="cuda")
    base[1:] = v.v
    vv = hp.HPCVector(v.structural_hash, v.partition, base[1:], b)
    assert vv.v.data_ptr() % 16 == 8
    assert np.array_equal(sc.bits(hp.take(vv, idx).local_values()), sc.bits(vg[idx]))
    own = rng.permutation(n)[:1700].astype(np.int64)
    sg = rng.standard_normal(len(own))
    sg[0], sg[1] = -0.0, np.nan
    src = hp.HPCVector.from_global(sg, b)
    assert hp.put_(vv, own, src) is vv
    got = base.cpu().numpy()
    assert got[0] == SENT and np.array_equal(sc.bits(got[1:]), sc.bits(sc.put_into(vg, own, sg)))
    assert np.array_equal(sc.bits(v.local_values()), sc.bits(vg))                                       # v itself is untouched
    with pytest.raises(ValueError, match="put_: src must be on the partition take returns"):
        hp.put_(v, own, hp.HPCVector.from_global(np.zeros(len(own) + 1), b))
    with pytest.raises(ValueError, match="put_: index 3 is listed more than once"):          # the smallest duplicate is named
        hp.put_(v, np.array([9, 5, 3, 5, 3]), hp.HPCVector.from_global(np.zeros(5), b))
    with pytest.raises(IndexError, match=rf"take: 2 of the indices lie outside \[0, {n}\); the first is {n} at position 1"):
        hp.take(v, np.array([0, n, -1]))
    with pytest.raises(IndexError, match=rf"put_: 1 of the indices lie outside \[0, {n}\); the first is {n} at position 0"):
        hp.put_(v, np.array([n]), hp.HPCVector.from_global(np.zeros(1), b))
    with pytest.raises(IndexError, match=rf"index_plan: 1 of the indices lie outside \[0, {n}\); the first is -3 at position 1"):
        hp.index_plan(np.array([0, -3]), v.partition, b)
    with pytest.raises(ValueError, match="take: the vector is not on the plan's partition"):
        ip.take(hp.HPCVector.from_global(np.zeros(5), b))
    b32 = _backend(hp, np.int32, np.float32)
    v32 = hp.HPCVector.from_global(vg.astype(np.float32), b32)
    with pytest.raises(TypeError, match="take: offered for Float64 backends only"):
        hp.take(v32, idx)
    with pytest.raises(TypeError, match="put_: offered for Float64 backends only"):
        hp.put_(v32, own, v32)
    with pytest.raises(TypeError, match="index_plan: offered for Float64 backends only"):
        hp.index_plan(idx, v32.partition, b32)


def test_argument_errors(hp):
    A, snap = _matrix(hp, "edge", np.int32)
    m, n = A.shape
    cols = sc.index_list("edge", "cols_perm")
    with pytest.raises(IndexError, match=rf"select: 2 of the rows lie outside \[0, {m}\); the first is {m} at position 1"):
        hp.select(A, np.array([0, m, 3, -2]), cols)
    with pytest.raises(IndexError, match=rf"select: 1 of the cols lie outside \[0, {n}\); the first is {n + 4} at position 2"):
        hp.select(A, None, np.array([0, 1, n + 4]))
    with pytest.raises(ValueError, match="select: column 11 is listed more than once; cols must be distinct"):
        hp.select(A, None, np.array([40, 11, 7, 40, 11, 3]))                # the smallest duplicated column is named
    with pytest.raises(ValueError, match="select: column 2 is listed more than once"):
        hp.select(A, None, _upload(np.array([2, 2], dtype=np.int64)))
    with pytest.raises(TypeError, match="select: rows must hold integers"):
        hp.select(A, np.array([0.0, 1.0]), None)
    with pytest.raises(TypeError, match="select: cols must be int64"):
        hp.select(A, None, _torch().zeros(3, dtype=_torch().int32))
    with pytest.raises(ValueError, match="select: rows must be one-dimensional"):
        hp.select(A, np.zeros((2, 2), dtype=np.int64), None)
    with pytest.raises(TypeError):
        A[([1, 2], slice(None))]                                            # __getitem__ keeps refusing index lists
    assert _unchanged(A, snap)


def test_a_result_that_does_not_fit_the_index_type_raises(hp):
    """The longest row of the edge matrix, repeated until the result passes 2^31 - 1 entries: Int32 refuses with the total,
    before anything is allocated by nnz and without handing out the wrapped rowptr; the structure pass alone runs.  The same
    list is accepted by the Int64 structure entry, and a shorter repeat succeeds on Int32."""
    from hpcla_amd.vectors import current_stream_ptr, dptr
    torch = _torch()
    C = sc.matrix("edge")
    lens = np.diff(C.indptr)
    r = int(np.argmax(lens))
    L = int(lens[r])
    reps = (2 ** 31 - 1) // L + 1
    total = reps * L
    assert total > 2 ** 31 - 1 and total - L <= 2 ** 31 - 1                   # the smallest repeat that does not fit
    rows = np.full(reps, r, dtype=np.int64)
    A32, snap = _matrix(hp, "edge", np.int32)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(OverflowError, match=f"select: the result's {total} entries do not fit the backend index type int32"):
        hp.select(A32, rows, None)
    assert torch.cuda.max_memory_allocated() - before < 4 * total // 8         # nothing of nnz entries was allocated
    assert _unchanged(A32, snap)
    B = hp.select(A32, rows[:1000], None)
    assert B.nnz == 1000 * L and np.array_equal(B.rowptr, np.arange(1001) * L)
    assert np.array_equal(sc.bits(B.nzval.cpu().numpy()), np.tile(sc.bits(C.data[C.indptr[r]:C.indptr[r + 1]]), 1000))
    # the raw entries: Int32 returns a status and the total, Int64 takes the same list
    lib = hp._capi.load()
    m, n = C.shape
    rows_d = _upload(rows)
    for Ti, want in ((np.int32, -5), (np.int64, 0)):
        A, _ = _matrix(hp, "edge", Ti)
        sfx = "i64" if Ti == np.int64 else "i32"
        ci_src = _upload(A.col_indices)
        ncomp = len(A.col_indices)
        work = torch.empty(lib.hpcla_select_work_bytes(reps, ncomp, n), dtype=torch.uint8, device="cuda")
        rowptr_out = torch.empty(reps + 1, dtype=A.rowptr_target.dtype, device="cuda")
        ci_out = torch.empty(ncomp, dtype=torch.int64, device="cuda")
        sizes = [ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)]
        status = getattr(lib, f"hpcla_select_structure_{sfx}")(
            dptr(A.rowptr_target), dptr(A.colval_target()), m, A.nnz, dptr(ci_src), ncomp, dptr(rows_d), reps, None, None, -1, n, 0,
            dptr(rowptr_out), dptr(ci_out), ctypes.byref(sizes[0]), ctypes.byref(sizes[1]), ctypes.byref(sizes[2]), dptr(work),
            current_stream_ptr())
        assert status == want, (sfx, status)
        assert sizes[0].value == total and sizes[1].value == L and sizes[2].value == L, sfx
        if want:
            assert f"the result's {total} entries do not fit the index type" in hp._capi.last_error()
        else:
            assert int(rowptr_out[-1].item()) == total and int(rowptr_out[1].item()) == L
        del work, rowptr_out


def test_bad_arguments_return_a_status(hp):
    from hpcla_amd.vectors import current_stream_ptr, dptr
    torch = _torch()
    lib = hp._capi.load()
    INVALID = -1
    s = current_stream_ptr()
    p = torch.zeros(64, dtype=torch.int64, device="cuda")
    f = torch.zeros(64, dtype=torch.float64, device="cuda")
    host = (ctypes.c_int64 * 3)()
    wk = torch.zeros(4096, dtype=torch.uint8, device="cuda")            # the sizes used below need < 400 B
    d, w, x, null = dptr(p), dptr(wk), dptr(f), None
    for sfx in ("i32", "i64"):
        st = getattr(lib, f"hpcla_select_structure_{sfx}")

        def structure(rowptr=d, colval=d, nrows=4, nnz=4, ci=d, ncomp=4, rows=d, nsel=4, sc_=d, sp_=d, nsorted=4, width=4, base=0,
                      rpo=d, cio=d, n_out=host, c_out=host, m_out=host, work=w):
            return st(rowptr, colval, nrows, nnz, ci, ncomp, rows, nsel, sc_, sp_, nsorted, width, base, rpo, cio, n_out, c_out, m_out,
                      work, s)

        for kw in (dict(nrows=-1), dict(nnz=-1), dict(ncomp=-1), dict(nsel=-1), dict(nsorted=-2), dict(width=-1), dict(base=2),
                   dict(base=-1), dict(rowptr=null), dict(colval=null), dict(ci=null), dict(sc_=null), dict(sp_=null),
                   dict(rpo=null), dict(cio=null), dict(n_out=null), dict(c_out=null), dict(m_out=null), dict(work=null)):
            assert structure(**kw) == INVALID, (sfx, kw)
            assert hp._capi.last_error()
        fl = getattr(lib, f"hpcla_select_fill_{sfx}")

        def fill(eb=8, rowptr=d, colval=d, nzval=x, nrows=4, nnz=4, ncomp=4, rows=d, nsel=4, rpo=d, nnz_out=4, longest=-1, base=0,
                 work=w, cvo=d, nzo=x, sro=d):
            return fl(eb, rowptr, colval, nzval, nrows, nnz, ncomp, rows, nsel, rpo, nnz_out, longest, base, work, cvo, nzo, sro, s)

        for kw in (dict(eb=2), dict(eb=16), dict(nrows=-1), dict(nnz=-1), dict(ncomp=-1), dict(nsel=-1), dict(nnz_out=-1),
                   dict(base=3), dict(rowptr=null), dict(colval=null), dict(nzval=null), dict(rpo=null), dict(work=null),
                   dict(cvo=null), dict(nzo=null), dict(sro=null)):
            assert fill(**kw) == INVALID, (sfx, kw)
        tk = getattr(lib, f"hpcla_select_take_f64_{sfx}")
        pt = getattr(lib, f"hpcla_select_put_f64_{sfx}")
        for args in ((x, -1, x, 0, d, 4, 0, x, s), (x, 4, x, -1, d, 4, 0, x, s), (x, 4, x, 0, d, -1, 0, x, s), (x, 4, x, 0, d, 4, 2, x, s),
                     (null, 4, x, 0, d, 4, 0, x, s), (x, 4, null, 4, d, 4, 0, x, s), (x, 4, x, 0, null, 4, 0, x, s),
                     (x, 4, x, 0, d, 4, 0, null, s)):
            assert tk(*args) == INVALID, (sfx, args)
        for args in ((x, -1, d, x, 4, 0, s), (x, 4, d, x, -1, 0, s), (x, 4, d, x, 4, 2, s), (null, 4, d, x, 4, 0, s),
                     (x, 4, null, x, 4, 0, s), (x, 4, d, null, 4, 0, s)):
            assert pt(*args) == INVALID, (sfx, args)
        # sizes of zero need no arrays
        assert structure(nrows=0, nnz=0, ncomp=0, nsel=0, nsorted=0, width=0, colval=null, ci=null, rows=null, sc_=null, sp_=null,
                         cio=null) == 0
        assert host[0] == 0 and host[1] == 0 and host[2] == 0
        assert fill(nsel=0, nnz_out=0, rowptr=null, colval=null, nzval=null, rows=null, rpo=null, work=null, cvo=null, nzo=null,
                    sro=null) == 0
        assert tk(null, 0, null, 0, null, 0, 0, null, s) == 0 and pt(null, 0, null, null, 0, 0, s) == 0
    g32 = lib.hpcla_gather_b32_i64
    for args in ((x, d, x, -1, 4, 0, s), (x, d, x, 4, -1, 0, s), (x, d, x, 4, 4, 2, s), (null, d, x, 4, 4, 0, s), (x, null, x, 4, 4, 0, s),
                 (x, d, null, 4, 4, 0, s)):
        assert g32(*args) == INVALID, args
    assert g32(null, null, null, 0, 0, 0, s) == 0
    assert lib.hpcla_select_work_bytes(-1, 4, 4) < 0 and lib.hpcla_select_work_bytes(4, -1, 4) < 0
    assert lib.hpcla_select_work_bytes(4, 4, -1) < 0
    torch.cuda.synchronize()


def test_a_temporary_handed_to_dptr_lives_as_long_as_its_pointer(hp):
    """``dptr(upload(a))`` inside an argument list: the tensor owns its block while the pointer object exists (until the entry
    point has been called) and is released with it."""
    import gc
    import weakref
    from hpcla_amd.vectors import dptr
    t = _upload(np.arange(5.0))
    alive = weakref.ref(t)
    p = dptr(t)
    del t
    assert alive() is not None and alive().data_ptr() == p.value
    assert np.array_equal(alive().cpu().numpy(), np.arange(5.0))
    del p
    gc.collect()
    assert alive() is None
    assert dptr(None).value is None


@pytest.mark.parametrize("nranks", [2, 3])
def test_select_across_ranks(nranks):
    """Ranks share the GPU; uneven row partitions, one with an empty rank; every rank's slice against the restatement, the
    gathered product against the one-rank product, take with and without a halo plan, the collective errors."""
    from hpcla_amd.launch import spawn_ranks
    assert spawn_ranks([WORKER], nranks, env_extra={"HPCLA_PUSH_TIMEOUT_S": "30"}, timeout=300, forward_rank0_stdout=False) == 0
