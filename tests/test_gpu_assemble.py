"""COO assembly on the device (csrc/assemble.hip, linearalgebrampi.jl_amd/assemble.py) against the numpy restatement of
tests/_assemble_cases.py -- which tests/test_assemble_cases.py holds against scipy -- on one rank, and through
tests/_multirank_assemble_worker.py on 2 and 3 ranks sharing the GPU.

Every case runs through the raw C ABI (both position widths; outputs pre-filled with a sentinel and padded so that an
unwritten or an overrun entry shows) and through ``hp.assembly_plan`` on Int32 and Int64 backends.  Structure arrays are
compared with array_equal, values as integers, bit for bit: the kernel adds in the restatement's order, so no tolerance
appears anywhere in this file.

The constants of the kernels (chunk of the sum order, output entries per workgroup, contributions per LDS pass, elements per
scan chunk) are asserted against the library, so the cases below sit where they say they sit."""
import ctypes
import os

import numpy as np
import pytest

from tests import _assemble_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_assemble_worker.py")

pytestmark = pytest.mark.gpu

SENT = -7
PAD = 64
_cache = {}


def _torch():
    import torch
    return torch


def _backend(hp, Ti):
    key = np.dtype(Ti).name
    if key not in _cache:
        _cache[key] = hp.backend_rocm_serial(np.float64, Ti)
    return _cache[key]


def _padded(n, dtype, fill=SENT):
    """(whole, view of the n middle entries): PAD sentinels on both sides."""
    torch = _torch()
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + n]


def _pads_intact(whole, n, fill=SENT):
    return bool((whole[:PAD] == fill).all()) and bool((whole[PAD + n:] == fill).all())


def _raw_structure(hp, rows, cols, shape, sfx, row_lo=0, row_hi=None):
    """The plan-time kernels through the C ABI, sentinel-padded: keys, (torch's stable sort), segments, row_starts, columns."""
    torch = _torch()
    from hpcla_amd.vectors import current_stream_ptr, dptr
    lib = hp._capi.load()
    m, ncols = shape
    row_hi = m if row_hi is None else row_hi
    n = len(rows)
    pdt = torch.int64 if sfx == "i64" else torch.int32
    s = current_stream_ptr()
    r_d, c_d = torch.from_numpy(np.asarray(rows, dtype=np.int64)).cuda(), torch.from_numpy(np.asarray(cols, dtype=np.int64)).cuda()
    key_w, key = _padded(n, torch.int64)
    counts = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    hp._capi.call("hpcla_assemble_keys", dptr(r_d), dptr(c_d), n, row_lo, row_hi, m, ncols, 0, dptr(key), dptr(counts), s)
    assert _pads_intact(key_w, n)
    skey, perm = torch.sort(key.clone(), stable=True)
    seg_w, seg = _padded(n + 1, pdt)
    uk_w, uk = _padded(n, torch.int64)
    work = torch.empty(lib.hpcla_assemble_work_bytes(n), dtype=torch.uint8, device="cuda")
    nnz = ctypes.c_int64(-1)
    hp._capi.call(f"hpcla_assemble_segments_{sfx}", dptr(skey), n, dptr(seg), dptr(uk), ctypes.byref(nnz), dptr(work), s)
    nnz = nnz.value
    assert _pads_intact(seg_w, n + 1) and _pads_intact(uk_w, n)
    assert bool((seg[nnz + 1:] == SENT).all()) and bool((uk[nnz:] == SENT).all())       # nothing past the segments is written
    rp_w, rp = _padded(row_hi - row_lo + 1, torch.int64)
    ci_w, ci = _padded(nnz, torch.int64)
    hp._capi.call("hpcla_assemble_row_starts_i64", dptr(uk), nnz, row_hi - row_lo, ncols, 0, dptr(rp), s)
    hp._capi.call("hpcla_assemble_columns", dptr(uk), nnz, ncols, 0, dptr(ci), s)
    torch.cuda.synchronize()
    assert _pads_intact(rp_w, row_hi - row_lo + 1) and _pads_intact(ci_w, nnz)
    return dict(counts=counts.cpu().numpy(), key=key.cpu().numpy(), perm=perm.cpu().numpy(), seg_ptr=seg[:nnz + 1].cpu().numpy(),
                ukey=uk[:nnz].cpu().numpy(), rowptr=rp.cpu().numpy(), cols=ci.cpu().numpy(), nnz=nnz)


def _raw_values(hp, seg_ptr, perm, vals, sfx, max_len, split=None):
    """hpcla_assemble_values_f64_* on a sentinel-padded output.  ``split``: the value list is passed as [vals[:split] | ghost]."""
    torch = _torch()
    from hpcla_amd.vectors import current_stream_ptr, dptr
    lib = hp._capi.load()
    pdt = torch.int64 if sfx == "i64" else torch.int32
    nseg, n_in = len(seg_ptr) - 1, len(perm)
    sp = torch.from_numpy(np.asarray(seg_ptr)).to(pdt).cuda()
    pm = torch.from_numpy(np.asarray(perm)).to(pdt).cuda()
    v = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float64)).cuda()
    split = len(vals) if split is None else split
    own, ghost = v[:split].clone(), v[split:].clone()
    out_w, out = _padded(nseg, torch.float64, float(SENT))
    work = torch.empty(lib.hpcla_assemble_values_work_bytes(n_in), dtype=torch.uint8, device="cuda")
    hp._capi.call(f"hpcla_assemble_values_f64_{sfx}", dptr(sp), dptr(pm) if n_in else None, nseg, n_in,
                  dptr(own) if split else None, split, dptr(ghost) if len(vals) > split else None, len(vals) - split, max_len,
                  dptr(out), dptr(work), current_stream_ptr())
    torch.cuda.synchronize()
    assert _pads_intact(out_w, nseg, float(SENT))
    return out.cpu().numpy()


def _check_raw(hp, rows, cols, vals, shape, sfx):
    rowptr, c, v = ac.assemble_ref(rows, cols, vals, shape)
    perm, seg_ptr, uk = ac.inverted_index(np.asarray(rows, dtype=np.int64) * shape[1] + np.asarray(cols, dtype=np.int64))
    got = _raw_structure(hp, rows, cols, shape, sfx)
    assert got["counts"].tolist() == [0, -1, 0, -1]
    assert np.array_equal(got["perm"], perm) and np.array_equal(got["seg_ptr"], seg_ptr) and np.array_equal(got["ukey"], uk)
    assert np.array_equal(got["rowptr"], rowptr) and np.array_equal(got["cols"], c)
    L = int(np.diff(seg_ptr).max()) if len(seg_ptr) > 1 else 0
    for max_len in (L, -1):                                                # the plan's bound, and "unknown"
        out = _raw_values(hp, seg_ptr, perm, vals, sfx, max_len)
        assert np.array_equal(ac.bits(out), ac.bits(v)), (sfx, max_len)
    if len(vals) > 3:                                                      # the same list handed over in two pieces
        out = _raw_values(hp, seg_ptr, perm, vals, sfx, L, split=len(vals) // 3)
        assert np.array_equal(ac.bits(out), ac.bits(v)), (sfx, "split")
    return rowptr, c, v


def _check_plan(hp, Ti, rows, cols, vals, shape, device_inputs=True):
    torch = _torch()
    backend = _backend(hp, Ti)
    rowptr, c, v = ac.assemble_ref(rows, cols, vals, shape)
    if device_inputs:
        r_in, c_in = torch.from_numpy(np.asarray(rows, dtype=np.int64)).cuda(), torch.from_numpy(np.asarray(cols, dtype=np.int64)).cuda()
        v_in = torch.from_numpy(np.asarray(vals)).cuda()
    else:
        r_in, c_in, v_in = np.asarray(rows), np.asarray(cols), np.asarray(vals)
    plan = hp.assembly_plan(r_in, c_in, shape, backend)
    A = plan.assemble(v_in)
    assert plan.n_in == len(rows) and plan.nnz == len(v) and plan.n_routed == 0
    seg_ptr = ac.inverted_index(np.asarray(rows, dtype=np.int64) * shape[1] + np.asarray(cols, dtype=np.int64))[1]
    assert plan.max_duplicates == (int(np.diff(seg_ptr).max()) if len(rows) else 0)
    assert A.shape == tuple(shape) and A.rowptr_target.dtype == (torch.int64 if Ti == np.int64 else torch.int32)
    assert np.array_equal(A.rowptr, rowptr)
    assert np.array_equal(A.col_indices[A.colval.astype(np.int64)] if len(v) else np.zeros(0, dtype=np.int64), c)
    assert np.array_equal(ac.bits(A.nzval.cpu().numpy()), ac.bits(v))
    return plan, A


def test_constants_are_the_librarys(hp):
    lib = hp._capi.load()
    assert lib.hpcla_assemble_chunk() == ac.CH and lib.hpcla_assemble_run() == ac.RUN
    assert lib.hpcla_assemble_pass() == ac.PASS and lib.hpcla_submatrix_scan_chunk() == ac.SCAN_CHUNK


def _case(name):
    if name == "lengths":                                                  # 1, 2, 63..65, 255..257, CH - 1..CH + 1, 2 CH, 2 CH + 1, 5 000
        shape = (97, 113)
        rows, cols = ac.planted_lengths(ac.edge_lengths(), shape, 3)
    elif name == "lengths_sorted":                                         # the same lists, arriving already grouped
        shape = (97, 113)
        rows, cols = ac.planted_lengths(ac.edge_lengths(), shape, 3, shuffle=False)
    elif name == "hub":                                                    # all triplets on one entry: 5 chunks and a rest
        shape = (3, 5)
        rows, cols = np.full(5 * ac.CH + 77, 1, dtype=np.int64), np.full(5 * ac.CH + 77, 2, dtype=np.int64)
    elif name == "hub_first_of_run":                                       # a long list at a run's first and last entry
        shape = (1, 2 * ac.RUN)
        L = np.full(2 * ac.RUN, 2, dtype=np.int64)
        L[[0, ac.RUN - 1, ac.RUN]] = [ac.CH + 1, 3 * ac.CH, ac.CH + 5]
        rows, cols = np.zeros(int(L.sum()), dtype=np.int64), np.repeat(np.arange(2 * ac.RUN), L)
    elif name == "empty_rows":                                             # empty rows at the start, in the middle, at the end
        shape = (10, 6)
        rows, cols = np.array([2, 3, 7, 3, 2, 7, 7]), np.array([1, 0, 4, 0, 1, 2, 4])
    elif name.startswith("run_"):                                          # RUN - 1, RUN, RUN + 1 output entries, 3 PASS-crossing each
        nnz = ac.RUN + {"run_minus": -1, "run_exact": 0, "run_plus": 1}[name]
        shape = (37, 41)
        assert 3 * nnz > ac.PASS and nnz <= shape[0] * shape[1]
        rows, cols = ac.planted_lengths(np.full(nnz, 3), shape, 5)
    elif name == "scan_chunks":                                            # n_in and nnz cross many scan chunks, multiples of none
        shape = (300, 300)
        rows, cols = ac.random_coo(70001, shape, 17)
    elif name == "single":
        shape = (1, 1)
        rows, cols = np.array([0]), np.array([0])
    else:
        raise KeyError(name)
    return np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), shape


CASES = ["lengths", "lengths_sorted", "hub", "hub_first_of_run", "empty_rows", "run_minus", "run_exact", "run_plus", "scan_chunks",
         "single"]


@pytest.mark.parametrize("name", CASES)
def test_raw_abi_matches_the_restatement(hp, name):
    rows, cols, shape = _case(name)
    vals = ac.values_for(len(rows), 23)
    for sfx in ("i32", "i64"):
        rowptr, c, v = _check_raw(hp, rows, cols, vals, shape, sfx)
    if name == "scan_chunks":
        assert len(rows) % ac.SCAN_CHUNK and len(v) % ac.SCAN_CHUNK and len(v) > 8 * ac.SCAN_CHUNK
    if name.startswith("run_"):
        assert len(v) == ac.RUN + {"run_minus": -1, "run_exact": 0, "run_plus": 1}[name]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_plan_matches_the_restatement(hp, name, Ti):
    rows, cols, shape = _case(name)
    _check_plan(hp, Ti, rows, cols, ac.values_for(len(rows), 29), shape, device_inputs=(Ti == np.int32))


def test_empty_input_gives_an_empty_matrix(hp):
    z = np.zeros(0, dtype=np.int64)
    for Ti in (np.int32, np.int64):
        plan, A = _check_plan(hp, Ti, z, z, np.zeros(0), (5, 7))
        assert A.nnz == 0 and np.array_equal(A.rowptr, np.zeros(6, dtype=np.int64))
    for sfx in ("i32", "i64"):
        got = _raw_structure(hp, z, z, (5, 7), sfx)
        assert got["nnz"] == 0 and np.array_equal(got["seg_ptr"], [0]) and np.array_equal(got["rowptr"], np.zeros(6))


def test_unsorted_input_same_structure_own_order(hp):
    rows, cols = ac.random_coo(9001, (61, 67), 31)
    vals = ac.values_for(9001, 37)
    rng = np.random.default_rng(41)
    orders = [np.arange(9001), np.arange(9001)[::-1].copy(), rng.permutation(9001), rng.permutation(9001)]
    first = None
    for o in orders:
        plan, A = _check_plan(hp, np.int32, rows[o], cols[o], vals[o], (61, 67))      # each order's own restatement, bit for bit
        st = (A.rowptr.copy(), A.colval.copy(), A.col_indices.copy())
        if first is None:
            first = st
        assert all(np.array_equal(a, b) for a, b in zip(st, first))
    a = ac.assemble_ref(rows[orders[2]], cols[orders[2]], vals[orders[2]], (61, 67))[2]
    b = ac.assemble_ref(rows[orders[3]], cols[orders[3]], vals[orders[3]], (61, 67))[2]
    assert not np.array_equal(ac.bits(a), ac.bits(b))                      # the orders do differ in the last bits: the case bites


def test_special_values(hp):
    tiny = np.float64(5e-324)
    rows = np.array([0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 5, 6, 6, 7])
    cols = np.array([0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 5, 6, 6, 7])
    vals = np.array([-0.0, 1.5, -1.5, np.nan, 1.0, np.inf, 1.0, -np.inf, 2.0, tiny, tiny, 3 * tiny, np.inf, -np.inf, 2.5])
    for Ti in (np.int32, np.int64):
        plan, A = _check_plan(hp, Ti, rows, cols, vals, (8, 8))
        got = A.nzval.cpu().numpy()
        assert ac.bits(got)[0] == ac.bits(np.array([-0.0]))[0]             # a lone -0.0 is kept
        assert ac.bits(got)[1] == 0                                        # x + (-x) is +0.0
        assert np.isnan(got[2]) and got[3] == np.inf and got[4] == -np.inf and np.isnan(got[6])
        assert got[5] == 5 * tiny and got[7] == 2.5                        # denormals add exactly; the neighbours are untouched
    for sfx in ("i32", "i64"):
        _check_raw(hp, rows, cols, vals, (8, 8), sfx)


def test_vector_form(hp):
    torch = _torch()
    n = 3 * ac.RUN + 5
    rng = np.random.default_rng(43)
    idx = np.concatenate([[0, 0, n - 1], rng.integers(0, n, 2500), np.full(ac.CH + 3, 77), [n - 1, 5]]).astype(np.int64)
    idx = idx[(idx < 100) | (idx > 140)]                                   # a gap nothing contributes to
    vals = ac.values_for(len(idx), 47)
    idx, vals = np.concatenate([idx, [120]]), np.concatenate([vals, [-0.0]])            # a lone -0.0 inside the gap
    want = ac.assemble_vector_ref(idx, vals, n)
    assert ac.bits(want)[120] == ac.bits(np.array([-0.0]))[0] and ac.bits(want)[121] == 0
    for Ti in (np.int32, np.int64):
        backend = _backend(hp, Ti)
        vp = hp.assembly_plan(torch.from_numpy(idx).cuda(), None, (n,), backend)
        b = vp.assemble(vals)
        assert isinstance(b, hp.HPCVector) and np.array_equal(b.partition, [0, n]) and vp.nnz == n and vp.template is None
        assert vp.max_duplicates >= ac.CH + 3
        assert np.array_equal(ac.bits(b.local_values()), ac.bits(want))
        v2 = ac.values_for(len(idx), 53)
        before = b.v.data_ptr()
        assert vp.assemble_(b, v2) is b and b.v.data_ptr() == before
        assert np.array_equal(ac.bits(b.local_values()), ac.bits(ac.assemble_vector_ref(idx, v2, n)))
        with pytest.raises(ValueError, match="not a result of this plan"):
            vp.assemble_(hp.HPCVector.from_global(np.zeros(n + 1), backend), v2)
    # raw: seg_ptr with empty segments at both ends and in the middle
    seg = np.array([0, 0, 0, 2, 2, 3, 3, 3])
    out = _raw_values(hp, seg, np.array([2, 0, 1]), np.array([1.0, -0.0, 4.0]), "i32", 2)
    assert np.array_equal(ac.bits(out), ac.bits(np.array([0.0, 0.0, 5.0, 0.0, -0.0, 0.0, 0.0])))
    out = _raw_values(hp, np.zeros(ac.RUN + 2, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), "i64", 0)
    assert np.array_equal(ac.bits(out), np.zeros(ac.RUN + 1, dtype=np.int64))          # nothing contributes anywhere: +0.0


def test_structure_reuse(hp, orc):
    torch = _torch()
    backend = _backend(hp, np.int32)
    shape = (900, 900)
    rows, cols = ac.random_coo(30011, shape, 59)
    v1, v2 = ac.values_for(30011, 61), ac.values_for(30011, 67)
    plan, A = _check_plan(hp, np.int32, rows, cols, v1, shape)
    x = hp.HPCVector.from_global(1.0 + np.cos(np.arange(900.0)), backend)
    y = A @ x                                                              # builds the VectorPlan of this structure
    n_plans = hp.cache_sizes()["vector_plan_cache"]
    rp, cv, h, nz = A.rowptr_target, A.colval_target(), A._ensure_hash(), A.nzval.data_ptr()
    assert plan.assemble_(A, torch.from_numpy(v2).cuda()) is A
    assert A.rowptr_target is rp and A.colval_target() is cv and A._ensure_hash() is h and A.nzval.data_ptr() == nz
    rowptr, c, v = ac.assemble_ref(rows, cols, v2, shape)
    assert np.array_equal(ac.bits(A.nzval.cpu().numpy()), ac.bits(v))
    B = plan.assemble(v1)                                                  # a second result: the same structure objects
    assert B.rowptr_target is rp and B.colval_target() is cv and B._ensure_hash() is h and B.nzval.data_ptr() != nz
    hp.mul_(y, A, x)
    ci = np.unique(c)
    y_ref = orc.spmv(rowptr.astype(np.int32), np.searchsorted(ci, c).astype(np.int32), v, x.local_values()[ci])
    assert np.array_equal(ac.bits(y.local_values()), ac.bits(y_ref))
    assert hp.cache_sizes()["vector_plan_cache"] == n_plans                # the rewritten matrix found its plan
    assert np.array_equal(ac.bits(plan.assemble(v2).nzval.cpu().numpy()), ac.bits(v))   # two calls, the same bits


def test_the_chain_a_user_runs(hp):
    import scipy.sparse as sp
    torch = _torch()
    backend = _backend(hp, np.int32)
    nx, ny = 33, 31
    N = nx * ny
    rows, cols, vals = ac.p1_triplets(nx, ny)
    plan = hp.assembly_plan(rows, cols, (N, N), backend)
    A = plan.assemble(vals)
    S = sp.coo_matrix((vals, (rows, cols)), shape=(N, N)).tocsr()
    A0 = hp.HPCSparseMatrix_from_global(S, backend)
    assert np.array_equal(A.rowptr, A0.rowptr) and np.array_equal(A.colval, A0.colval)
    assert np.array_equal(A.col_indices, A0.col_indices)
    assert np.array_equal(ac.bits(A.nzval.cpu().numpy() + 0.0), ac.bits(A0.nzval.cpu().numpy() + 0.0))    # dyadic: every order is exact
    assert np.array_equal(ac.bits(A.nzval.cpu().numpy() + 0.0), ac.bits(ac.p1_expected(nx, ny).data + 0.0))
    b = hp.HPCVector.from_global(np.sin(np.arange(N, dtype=np.float64)), backend)
    it = [hp.cg(M_, b, M=hp.amg(M_))[1] for M_ in (A, A0)]
    assert it[0].converged and it[0].iterations == it[1].iterations
    # a new coefficient on the same structure, then ILU(0) refreshed on it: the factors of a freshly built matrix
    k = 1.0 + 0.5 * np.sin(np.arange(2 * (nx - 1) * (ny - 1), dtype=np.float64))
    vals2 = ac.p1_triplets(nx, ny, coeff=k)[2]
    M = hp.ilu0(A)
    plan.assemble_(A, vals2)
    M.update(A)
    rowptr, c, v = ac.assemble_ref(rows, cols, vals2, (N, N))
    assert np.array_equal(ac.bits(A.nzval.cpu().numpy()), ac.bits(v))
    fresh = hp.HPCSparseMatrix_local(rowptr, c, v, N, backend)
    assert np.array_equal(ac.bits(M.factors()[2]), ac.bits(hp.ilu0(fresh).factors()[2]))
    one = hp.sparse_from_coo(rows, cols, vals2, (N, N), backend)           # the one-shot form
    assert np.array_equal(ac.bits(one.nzval.cpu().numpy()), ac.bits(v)) and np.array_equal(one.rowptr, rowptr)


def test_errors(hp):
    torch = _torch()
    backend = _backend(hp, np.int32)
    r = torch.tensor([0, 5, 2, -1, 1], dtype=torch.int64, device="cuda")
    c = torch.tensor([0, 1, 9, 1, 1], dtype=torch.int64, device="cuda")
    with pytest.raises(IndexError, match=r"3 of the indices .*first is \(5, 1\) at position 1"):
        hp.assembly_plan(r, c, (5, 5), backend)
    with pytest.raises(IndexError, match="2 of the indices .*first is row 5 at position 1"):
        hp.assembly_plan(r, None, (5,), backend)
    got = _raw_structure(hp, r.cpu().numpy(), c.cpu().numpy(), (5, 5), "i32", row_lo=1, row_hi=3)
    assert got["counts"].tolist() == [3, 1, 1, 0]                          # three outside the matrix; (0, 0) inside, another rank's row
    assert got["key"].tolist() == [np.iinfo(np.int64).max] * 4 + [1]
    plan = hp.assembly_plan(r.clamp(0, 4), c.clamp(0, 4), (5, 5), backend)
    other = hp.assembly_plan(r.clamp(0, 4), c.clamp(0, 4), (5, 5), backend)
    A = plan.assemble(np.ones(5))
    with pytest.raises(ValueError, match="not a result of this plan"):
        other.assemble_(A, np.ones(5))
    with pytest.raises(ValueError, match="not a result of this plan"):
        plan.assemble_(hp.HPCSparseMatrix_local([0, 1], [0], [1.0], 1, backend), np.ones(5))
    assert plan.assemble_(A.copy(), np.ones(5)).nnz == A.nnz               # a copy shares the structure arrays
    with pytest.raises(ValueError, match="5 values"):
        plan.assemble(np.ones(4))
    with pytest.raises(TypeError, match="float64"):
        plan.assemble(torch.ones(5, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError, match="Float64 backends only"):
        hp.assembly_plan(r.clamp(0, 4), c.clamp(0, 4), (5, 5), hp.backend_rocm_serial(np.float32, np.int32))
    lib = hp._capi.load()
    assert lib.hpcla_assemble_values_f64_i32(None, None, 4, 0, None, 0, None, 0, 0, None, None, None) == -1
    assert "null" in hp._capi.last_error()
    assert lib.hpcla_assemble_keys(None, None, 3, 0, 2, 1, 1, 0, None, None, None) == -1
    assert lib.hpcla_assemble_row_starts_i64(None, 0, 2 ** 40, 2 ** 30, 0, None, None) == -1
    assert "63 bits" in hp._capi.last_error()


@pytest.mark.parametrize("nranks", [2, 3])
def test_assembly_across_ranks(nranks):
    """Ranks share the GPU; element-partitioned P1 triplets on uneven row partitions, one of them with an empty rank; each
    rank's slice against the restatement on its value list, the gathered matrix against the one-rank result."""
    from hpcla_amd.launch import spawn_ranks
    assert spawn_ranks([WORKER], nranks, env_extra={"HPCLA_PUSH_TIMEOUT_S": "30"}, timeout=300, forward_rank0_stdout=False) == 0
