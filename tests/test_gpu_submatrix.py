"""Range indexing on the device (csrc/submatrix.hip, linearalgebrampi.jl_amd/indexing.py) against the numpy restatement of
tests/_submatrix_cases.py -- which tests/test_submatrix_cases.py holds against scipy -- on one rank, and through
tests/_multirank_submatrix_worker.py on 2 and 3 ranks sharing the GPU.

Every case runs through the raw C ABI (both index types, both index bases, outputs pre-filled with a sentinel and padded so
that an unwritten or an overrun entry shows) and through ``A[...]``.  Structure arrays are compared with array_equal, values
as integers (every bit, the sign of zeros and NaN payloads included): no tolerance appears, the operation copies bits.
Products over the result are compared bitwise with the oracle's loops over the restated CSR; where the oracle's own result
is a NaN the product must be a NaN (which NaN an Inf - Inf yields is the hardware's choice, not a copied bit).

The scan behind the new rowptr and col_indices works in chunks of SCAN_CHUNK = 1 024 elements (csrc/scan.h; asserted below
against the library); the 70 001-row band matrix crosses 68 chunk boundaries in both scans.  One workgroup scans the chunks'
sums 256 at a time with a carry between the trips: the two band_long cases (tests/_submatrix_cases.py) select more than
256 * 1 024 = 262 144 rows and a column range wider than that, with unequal chunk sums on both sides of the first carry."""
import ctypes
import os

import numpy as np
import pytest

from tests import _submatrix_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_submatrix_worker.py")

pytestmark = pytest.mark.gpu

SENT = -7
IDS = [c[0] for c in sc.CASES]
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
    assert (B.structural_hash is not None) == hashed, what                # plain A[r, c] hashes nothing: the hash is lazy


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


@pytest.mark.parametrize("Ti", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_getitem_matches_the_restatement(hp, orc, case, Ti):
    name, key, r0, r1, c0, c1 = case
    A, snap = _matrix(hp, key, Ti)
    part = A.row_partition
    e = sc.expected_on_rank(sc.matrix(key), part, 0, r0, r1, c0, c1)
    B = A[r0:r1, c0:c1]
    _assert_matrix(B, e, Ti, name)
    _products(hp, orc, B, e, Ti, np.float64, name)
    m, n = A.shape
    if c0 == 0 and c1 == n:
        _assert_matrix(A[r0:r1, :], e, Ti, name + " [r, :]")
    if r0 == 0 and r1 == m:
        _assert_matrix(A[:, c0:c1], e, Ti, name + " [:, c]")
        if c0 == 0 and c1 == n:
            _assert_matrix(A[:, :], e, Ti, name + " [:, :]")
    assert _unchanged(A, snap), name + ": the input changed"


def _upload(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("Ti", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_raw_abi_matches_the_restatement(hp, case, Ti, base):
    from hpcla_amd.vectors import current_stream_ptr, dptr
    torch = _torch()
    name, key, r0, r1, c0, c1 = case
    A, snap = _matrix(hp, key, Ti)
    C = sc.matrix(key)
    e = sc.restate(C, r0, r1, c0, c1)
    sfx = "i64" if Ti == np.int64 else "i32"
    tdt = torch.int64 if Ti == np.int64 else torch.int32
    rowptr = _upload((A.rowptr + base).astype(Ti))
    colval = _upload((A.colval + base).astype(Ti))
    ci_src = _upload(A.col_indices + base)                        # 1-based global columns for a 1-based caller
    j0, j1 = (int(j) for j in np.searchsorted(A.col_indices, [c0, c1]))
    nsel, width = r1 - r0, j1 - j0
    lib = hp._capi.load()
    assert lib.hpcla_submatrix_scan_chunk() == sc.SCAN_CHUNK
    work = torch.full((lib.hpcla_submatrix_work_bytes(nsel, width),), 0x5A, dtype=torch.uint8, device="cuda")
    src_start = torch.full((nsel + 4,), SENT, dtype=torch.int64, device="cuda")
    rowptr_out = torch.full((nsel + 1 + 4,), SENT, dtype=tdt, device="cuda")
    ci_out = torch.full((width + 4,), SENT, dtype=torch.int64, device="cuda")
    nnz_out, ncomp = ctypes.c_int64(-1), ctypes.c_int64(-1)
    s = current_stream_ptr()
    hp._capi.call(f"hpcla_submatrix_structure_{sfx}", dptr(rowptr), dptr(colval), A.nrows_local, A.nnz, r0, r1, j0, j1, base,
                  dptr(ci_src), c0, dptr(src_start), dptr(rowptr_out), dptr(ci_out), ctypes.byref(nnz_out), ctypes.byref(ncomp),
                  dptr(work), s)
    assert nnz_out.value == len(e["vals"]) and ncomp.value == len(e["col_indices"]), name
    rp = rowptr_out.cpu().numpy()
    assert np.array_equal(rp[:nsel + 1], e["rowptr"] + base) and np.all(rp[nsel + 1:] == SENT), name
    ci = ci_out.cpu().numpy()
    assert np.array_equal(ci[:ncomp.value], e["col_indices"] + base) and np.all(ci[ncomp.value:] == SENT), name
    ss = src_start.cpu().numpy()
    assert np.all(ss[nsel:] == SENT), name
    # the source start of every kept row: the first stored entry of the row with a column >= c0
    first = np.array([C.indptr[r] + np.searchsorted(C.indices[C.indptr[r]:C.indptr[r + 1]], c0) for r in range(r0, r1)],
                     dtype=np.int64)
    assert np.array_equal(ss[:nsel], first), name
    nnz = nnz_out.value
    colval_out = torch.full((nnz + 8,), SENT, dtype=tdt, device="cuda")
    nzval_out = torch.full((nnz + 8,), float(SENT), dtype=torch.float64, device="cuda")
    hp._capi.call(f"hpcla_submatrix_fill_{sfx}", 8, dptr(colval), dptr(A.nzval), A.nnz, dptr(src_start), dptr(rowptr_out), nsel,
                  nnz, j0, j1, base, dptr(work), dptr(colval_out), dptr(nzval_out), s)
    cv, nz = colval_out.cpu().numpy(), nzval_out.cpu().numpy()
    assert np.array_equal(cv[:nnz], e["colval"] + base) and np.all(cv[nnz:] == SENT), name
    assert np.array_equal(sc.bits(nz[:nnz]), sc.bits(e["vals"])) and np.all(nz[nnz:] == SENT), name
    # the values pass alone, into a misaligned output (8 bytes off a 16-byte boundary): the scalar path writes the same bits
    for off in (0, 1):
        again = torch.full((nnz + 9,), float(SENT), dtype=torch.float64, device="cuda")
        hp._capi.call(f"hpcla_submatrix_values_{sfx}", 8, dptr(A.nzval), A.nnz, dptr(src_start), dptr(rowptr_out), nsel, nnz, base,
                      dptr(again[off:]), s)
        nz2 = again.cpu().numpy()
        assert np.array_equal(sc.bits(nz2[off:off + nnz]), sc.bits(e["vals"])), name
        assert np.all(nz2[:off] == SENT) and np.all(nz2[off + nnz:] == SENT), name
    assert _unchanged(A, snap), name + ": the input changed"


@pytest.mark.parametrize("Ti", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("name,key,k", sc.COLUMN_CASES, ids=[c[0] for c in sc.COLUMN_CASES])
def test_column_matches_the_restatement(hp, name, key, k, Ti):
    from hpcla_amd.vectors import current_stream_ptr, dptr
    torch = _torch()
    A, snap = _matrix(hp, key, Ti)
    C = sc.matrix(key)
    want = sc.column_of(C, 0, C.shape[0], k)
    v = A[:, k]
    assert isinstance(v, hp.HPCVector) and np.array_equal(v.partition, A.row_partition)
    assert v.structural_hash == hp.compute_partition_hash(A.row_partition)
    got = v.local_values()
    assert np.array_equal(sc.bits(got), sc.bits(want)), name
    stored = np.zeros(C.shape[0], dtype=bool)
    rows = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr))
    stored[rows[C.indices == k]] = True
    assert np.all(sc.bits(got[~stored]) == 0), name                     # absent: exactly +0.0
    if name == "rand_negzero":
        assert got[sc.NEGZERO_ROW] == 0 and np.signbit(got[sc.NEGZERO_ROW])
    if name == "rand_gap_absent":
        assert not stored.any() and k not in A.col_indices
    # raw entry, both bases, sentinel behind the output
    jk = int(np.searchsorted(A.col_indices, k))
    if jk < len(A.col_indices) and A.col_indices[jk] == k:
        sfx = "i64" if Ti == np.int64 else "i32"
        for base in (0, 1):
            out = torch.full((A.nrows_local + 4,), float(SENT), dtype=torch.float64, device="cuda")
            hp._capi.call(f"hpcla_sparse_column_{sfx}", 8, dptr(_upload((A.rowptr + base).astype(Ti))),
                          dptr(_upload((A.colval + base).astype(Ti))), dptr(A.nzval), A.nrows_local, A.nnz, jk, base, dptr(out),
                          current_stream_ptr())
            o = out.cpu().numpy()
            assert np.array_equal(sc.bits(o[:A.nrows_local]), sc.bits(want)) and np.all(o[A.nrows_local:] == SENT), (name, base)
    assert _unchanged(A, snap)


def test_the_result_is_a_first_class_matrix(hp, orc):
    """B @ x, B @ X (in every case above), and here transpose(B) @ x, B + B and B.norm(): equal to the same operations on a
    matrix uploaded from the restated CSR."""
    for key, (r0, r1, c0, c1) in (("rand_finite", (95, 1095, 40, 4500)), ("p5", (97, 4100, 191, 4007))):
        C = sc.matrix(key)
        A = hp.HPCSparseMatrix_local(C.indptr, C.indices, C.data, C.shape[1], _backend(hp, np.int32))
        B = A[r0:r1, c0:c1]
        e = sc.restate(C, r0, r1, c0, c1)
        R = hp.HPCSparseMatrix_local(e["rowptr"], e["cols"], e["vals"], c1 - c0, _backend(hp, np.int32))
        assert B._ensure_hash() == R._ensure_hash()                     # the device-built structure hashes like the host-built one
        x = hp.HPCVector.from_global(1.0 + orc.fill_uniform(0, r1 - r0, 3), B.backend)
        assert np.array_equal((hp.transpose(B) @ x).local_values(), (hp.transpose(R) @ x).local_values())
        S = B + B
        assert np.array_equal(S.rowptr, e["rowptr"]) and np.array_equal(S.col_indices[S.colval], e["cols"])
        assert np.array_equal(S.nzval.cpu().numpy(), 2 * e["vals"])
        assert B.norm() == R.norm() and B.norm(1) == R.norm(1)


def test_plan_extracts_values_only_and_shares_the_structure(hp, orc):
    A, snap = _matrix(hp, "rand", np.int32)
    C = sc.matrix("rand")
    r0, r1, c0, c1 = 90, 1400, sc.GAP_LO - 300, sc.GAP_HI + 800
    plan = hp.get_submatrix_plan(A, slice(r0, r1), slice(c0, c1))
    e = sc.expected_on_rank(C, A.row_partition, 0, r0, r1, c0, c1)
    B0 = plan.matrix
    _assert_matrix(B0, e, np.int32, "plan.matrix", hashed=True)
    A2 = 2 * A
    doubled = A2.nzval.cpu().numpy()
    finite = np.isfinite(C.data)
    assert np.array_equal(doubled[finite], 2 * C.data[finite])
    B2 = plan.extract(A2)
    assert B2.rowptr_target is B0.rowptr_target and B2._colval_target is B0._colval_target
    assert B2.col_indices is B0.col_indices and B2.structural_hash is B0.structural_hash
    assert B2.nzval is not B0.nzval
    e2 = sc.restate(C.with_values(doubled), r0, r1, c0, c1)
    assert np.array_equal(sc.bits(B2.nzval.cpu().numpy()), sc.bits(e2["vals"]))
    assert np.array_equal(sc.bits(plan.extract(A).nzval.cpu().numpy()), sc.bits(e["vals"]))
    # downstream plans are cache hits: the second matrix of the structure builds no VectorPlan
    x = hp.HPCVector.from_global(1.0 + orc.fill_uniform(0, c1 - c0, orc.SEED_X), A.backend)
    y0 = B0 @ x
    before = hp.cache_sizes()["vector_plan_cache"]
    y2 = B2 @ x
    assert hp.cache_sizes()["vector_plan_cache"] == before
    fin = np.isfinite(y0.local_values())
    assert np.array_equal(y2.local_values()[fin], 2 * y0.local_values()[fin])
    # another structure raises: another matrix, and the same matrix with one stored column moved
    with pytest.raises(ValueError):
        plan.extract(_matrix(hp, "p5", np.int32)[0])
    idx = C.indices.copy()
    a = C.indptr[sc.WHOLE_ROW]
    idx[a] -= 1
    moved = hp.HPCSparseMatrix_local(C.indptr, idx, C.data, C.shape[1], A.backend)
    assert moved.nnz == A.nnz
    with pytest.raises(ValueError):
        plan.extract(moved)
    with pytest.raises(ValueError):
        plan.extract(_matrix(hp, "rand", np.int64)[0])
    # the empty forms plan too
    pe = hp.get_submatrix_plan(A, slice(5, 5), slice(None))
    assert pe.extract(A2).nnz == 0 and np.array_equal(pe.matrix.row_partition, [0, 0])
    assert _unchanged(A, snap)


def test_float32_backend(hp, orc):
    T, Ti = np.float32, np.int32
    A, snap = _matrix(hp, "rand", Ti, T)
    C = _csr("rand", T)
    assert A.nzval.dtype == _torch().float32
    for r0, r1, c0, c1 in ((95, 1095, 0, sc.NC), (50, 1700, sc.GAP_LO - 10, sc.GAP_LO + 5), (100, 109, 17, 4890)):
        e = sc.expected_on_rank(C, A.row_partition, 0, r0, r1, c0, c1)
        B = A[r0:r1, c0:c1]
        _assert_matrix(B, e, Ti, "f32")
        _products(hp, orc, B, e, Ti, T, "f32")
    want = sc.column_of(C, 0, C.shape[0], sc.NEGZERO_COL)
    got = A[:, sc.NEGZERO_COL].local_values()
    assert got.dtype == T and np.array_equal(sc.bits(got), sc.bits(want)) and np.signbit(got[sc.NEGZERO_ROW])
    plan = hp.get_submatrix_plan(A, slice(95, 1095), slice(0, sc.NC))
    e = sc.restate(C, 95, 1095, 0, sc.NC)
    assert np.array_equal(sc.bits(plan.extract(A).nzval.cpu().numpy()), sc.bits(e["vals"]))
    assert _unchanged(A, snap, T)


def test_vector_and_dense_ranges(hp):
    b = _backend(hp, np.int32)
    rng = np.random.default_rng(1)
    vg = rng.standard_normal(101)
    vg[7], vg[8] = -0.0, np.nan
    v = hp.HPCVector.from_global(vg, b)
    for a, z in ((0, 101), (5, 60), (7, 8), (100, 101)):
        w = v[a:z]
        assert np.array_equal(sc.bits(w.local_values()), sc.bits(vg[a:z])) and np.array_equal(w.partition, [0, z - a])
        assert w.structural_hash == hp.compute_partition_hash(w.partition) and w.v.is_cuda
    w = v[:]
    w.v.fill_(1.0)
    assert np.array_equal(sc.bits(v.local_values()), sc.bits(vg))                     # a copy, not a view
    assert len(v[9:9]) == 0 and np.array_equal(v[9:9].partition, [0, 0]) and v[9:9].v.numel() == 0
    assert np.array_equal(sc.bits(v[:10].local_values()), sc.bits(vg[:10])) and len(v[95:]) == 6
    Xg = rng.standard_normal((50, 7))
    X = hp.HPCMatrix.from_global(Xg, b)
    for key in ((slice(3, 40), slice(2, 6)), (slice(3, 40), slice(None)), (slice(None), slice(2, 6)), (slice(None), slice(None)),
                (slice(49, 50), slice(6, 7))):
        Y = X[key]
        assert isinstance(Y, hp.HPCMatrix) and Y.A.is_contiguous() and Y.A.is_cuda
        assert np.array_equal(Y.local_values(), Xg[key])
        assert np.array_equal(Y.row_partition, [0, Xg[key].shape[0]]) and np.array_equal(Y.col_partition, [0, Xg[key].shape[1]])
    Y = X[:, :]
    Y.A.fill_(0.0)
    assert np.array_equal(X.local_values(), Xg)
    for key, shape in (((slice(4, 4), slice(1, 5)), (0, 4)), ((slice(2, 9), slice(3, 3)), (7, 0))):
        Y = X[key]
        assert tuple(Y.A.shape) == shape and Y.shape == shape and np.array_equal(Y.row_partition, [0, shape[0]])
    assert np.array_equal(X[:, 3].local_values(), Xg[:, 3])                           # the existing form, as before
    with pytest.raises(IndexError, match="HPCMatrix column index out of bounds: k=7, ncols=7"):
        X[:, 7]


def test_key_errors(hp):
    A, _ = _matrix(hp, "p5", np.int32)
    m, n = A.shape
    b = _backend(hp, np.int32)
    v = hp.HPCVector.from_global(np.arange(10.0), b)
    X = hp.HPCMatrix.from_global(np.ones((6, 4)), b)
    for bad in ((slice(0, m + 1), slice(None)), (slice(5, 3), slice(None)), (slice(None), slice(0, n + 1)),
                (slice(None), slice(n, n - 1)), (slice(m + 1, m + 1), slice(None))):
        with pytest.raises(IndexError):
            A[bad]
    with pytest.raises(IndexError, match=f"HPCSparseMatrix column index out of bounds: k={n}, ncols={n}"):
        A[:, n]
    with pytest.raises(IndexError, match=f"HPCSparseMatrix column index out of bounds: k=-1, ncols={n}"):
        A[:, -1]
    for bad in ((slice(0, 8, 2), slice(None)), (slice(-1, 5), slice(None)), (slice(0, 5), slice(-3, None)), 3, (1, 2),
                ([1, 2], slice(None)), slice(0, 5), (slice(1.0, 3), slice(None)), (slice(0, 3), 5), (slice(None), 2.0),
                (slice(None), slice(None), slice(None)), (slice(None), True), (slice(0, 5, -1), slice(None))):
        with pytest.raises(TypeError):
            A[bad]
    for bad in (slice(0, 11), slice(6, 2)):
        with pytest.raises(IndexError):
            v[bad]
    for bad in (slice(0, 10, 2), slice(-1, None), 3, (slice(None), slice(None)), slice(None, -2), slice(0.0, 2)):
        with pytest.raises(TypeError):
            v[bad]
    for bad in ((slice(0, 7), slice(None)), (slice(None), slice(2, 5 + 1)), (slice(4, 2), slice(None))):
        with pytest.raises(IndexError):
            X[bad]
    for bad in ((slice(0, 4, 2), slice(None)), (slice(None), slice(-2, None)), (1, 2), 3, (slice(0, 2), 1)):
        with pytest.raises(TypeError):
            X[bad]
    assert A[0:m, 0:n].nnz == A.nnz and A[:m, :].nnz == A.nnz                           # the ends themselves are in bounds


def test_bad_arguments_return_a_status(hp):
    from hpcla_amd.vectors import current_stream_ptr, dptr
    torch = _torch()
    lib = hp._capi.load()
    INVALID = -1
    s = current_stream_ptr()
    p = torch.zeros(64, dtype=torch.int64, device="cuda")
    host = (ctypes.c_int64 * 2)()
    wk = torch.zeros(1024, dtype=torch.uint8, device="cuda")            # a work buffer of its own (sizes used below need < 200 B)
    d, w, null = dptr(p), dptr(wk), None
    for sfx in ("i32", "i64"):
        st = getattr(lib, f"hpcla_submatrix_structure_{sfx}")

        def structure(nrows=4, nnz=4, r0=0, r1=4, j0=0, j1=4, base=0, rowptr=d, colval=d, src=d, rpo=d, cio=d, n_out=host, c_out=host,
                      work=w):
            return st(rowptr, colval, nrows, nnz, r0, r1, j0, j1, base, d, 0, src, rpo, cio, n_out, c_out, work, s)

        for kw in (dict(nrows=-1), dict(nnz=-1), dict(j0=3, j1=2), dict(j0=-1), dict(r0=-1), dict(r1=5), dict(r0=3, r1=2),
                   dict(base=2), dict(base=-1), dict(rowptr=null), dict(colval=null), dict(src=null), dict(rpo=null),
                   dict(cio=null), dict(n_out=null), dict(c_out=null), dict(work=null)):
            assert structure(**kw) == INVALID, (sfx, kw)
            assert hp._capi.last_error()
        fl = getattr(lib, f"hpcla_submatrix_fill_{sfx}")

        def fill(eb=8, colval=d, nzval=d, nnz_src=4, src=d, rpo=d, nsel=4, nnz_out=4, j0=0, j1=4, base=0, work=w, cvo=d, nzo=d):
            return fl(eb, colval, nzval, nnz_src, src, rpo, nsel, nnz_out, j0, j1, base, work, cvo, nzo, s)

        for kw in (dict(eb=2), dict(eb=16), dict(nnz_src=-1), dict(nsel=-1), dict(nnz_out=-1), dict(nnz_out=5), dict(j0=2, j1=1),
                   dict(j0=-1), dict(base=3), dict(colval=null), dict(nzval=null), dict(src=null), dict(rpo=null), dict(work=null),
                   dict(cvo=null), dict(nzo=null)):
            assert fill(**kw) == INVALID, (sfx, kw)
        va = getattr(lib, f"hpcla_submatrix_values_{sfx}")

        def values(eb=8, nzval=d, nnz_src=4, src=d, rpo=d, nsel=4, nnz_out=4, base=0, nzo=d):
            return va(eb, nzval, nnz_src, src, rpo, nsel, nnz_out, base, nzo, s)

        for kw in (dict(eb=0), dict(nnz_src=-1), dict(nsel=-1), dict(nnz_out=-2), dict(nnz_out=9), dict(base=2), dict(nzval=null),
                   dict(src=null), dict(rpo=null), dict(nzo=null)):
            assert values(**kw) == INVALID, (sfx, kw)
        co = getattr(lib, f"hpcla_sparse_column_{sfx}")

        def column(eb=8, rowptr=d, colval=d, nzval=d, nrows=4, nnz=4, jk=0, base=0, out=d):
            return co(eb, rowptr, colval, nzval, nrows, nnz, jk, base, out, s)

        for kw in (dict(eb=3), dict(nrows=-1), dict(nnz=-1), dict(jk=-1), dict(base=2), dict(rowptr=null), dict(colval=null),
                   dict(nzval=null), dict(out=null)):
            assert column(**kw) == INVALID, (sfx, kw)
        # sizes of zero need no arrays
        assert structure(nrows=0, nnz=0, r0=0, r1=0, j0=0, j1=0, colval=null, src=null, cio=null) == 0
        assert host[0] == 0 and host[1] == 0
        assert fill(nsel=0, nnz_out=0, colval=null, nzval=null, src=null, rpo=null, cvo=null, nzo=null) == 0
        assert values(nsel=0, nnz_out=0, nzval=null, src=null, rpo=null, nzo=null) == 0
        assert column(nrows=0, nnz=0, rowptr=null, colval=null, nzval=null, out=null) == 0
    assert lib.hpcla_submatrix_work_bytes(-1, 4) < 0 and lib.hpcla_submatrix_work_bytes(4, -1) < 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("nranks", [2, 3])
def test_submatrix_across_ranks(nranks):
    """Ranks share the GPU; uneven row partition with one empty rank; ranges that put a rank wholly inside, wholly outside and
    partly inside; each rank against the restatement, the gathered product against the one-rank product."""
    from hpcla_amd.launch import spawn_ranks
    assert spawn_ranks([WORKER], nranks, env_extra={"HPCLA_PUSH_TIMEOUT_S": "30"}, timeout=300, forward_rank0_stdout=False) == 0
