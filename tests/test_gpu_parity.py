"""GPU parity tests (run with ``-m gpu`` on an MI355X): the HIP path, called through the C ABI and
through the host layer that mirrors the reference API, against the CPU oracle on identical inputs.

Bar: the SpMV/SpMM kernels accumulate each row sequentially in stored order with separately rounded
multiply and add, exactly like the reference loop (src/sparse.jl:2055-2066), so results must be
BIT-IDENTICAL to the oracle (np.array_equal), not merely within the 1e-12 relative tolerance of
BASELINE.json.  Reductions (dot/norm) use a different (tree) summation order than a sequential CPU
sum: tolerance 1e-12 relative, as BASELINE.json states.  Small fixtures additionally meet the
reference's own 1e-10 absolute (test/test_utils.jl:154-157).
"""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _grid_regimes as gr
from tests import _spmm_edge_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_REF = 1e-10      # reference absolute tolerance on its O(10) fixtures
RTOL_RED = 1e-12     # BASELINE.json: 1e-12 relative for fp64
CG_RTOL = 1e-12      # CG histories vs the oracle / fused vs unfused: BASELINE's 1e-12; measured 3.5e-15 (40 its, 24^3) and 8e-16


def _free_port():
    from hpcla_amd.launch import free_port
    return free_port()


def _t(a, dev="cuda"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _raw_spmv(hp, rowptr, colval, vals, x, Ti, base=0):
    """Call hpcla_spmv_csr_f64_{i32,i64} directly (the entry point a Julia @ccall binds)."""
    import torch
    sfx = "i32" if Ti == np.int32 else "i64"
    rp, cv = _t((rowptr + base).astype(Ti)), _t((colval + base).astype(Ti))
    nz, xd = _t(vals), _t(x)
    nrows = len(rowptr) - 1
    y = torch.full((max(nrows, 1),), float("nan"), dtype=torch.float64, device="cuda")
    hp._capi.call(f"hpcla_spmv_csr_f64_{sfx}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(),
                  xd.data_ptr(), y.data_ptr(), nrows, len(vals), base,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y[:nrows].cpu().numpy()


# ---------------------------------------------------------------------------------------------------
# golden fixtures through the raw C ABI and through the host layer
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spmv_tridiagonal", "spmv_nonsquare", "spmv_local_ctor",
                                  "laplacian2d_4x3", "laplacian2d_3x5"])
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
@pytest.mark.parametrize("base", [0, 1])
def test_spmv_golden_raw_abi(hp, orc, golden, gpu_backend_i32, name, Ti, base):
    case = golden[name]
    rows = orc.rows_from_coo(case["I"], case["J"], case["V"], case["m"], case["n"])
    ci, cv = orc.compress_columns(rows)
    y = _raw_spmv(hp, rows.rowptr, cv, rows.vals, np.array(case["x"])[ci], Ti, base)
    assert np.max(np.abs(y - np.array(case["y"]))) < TOL_REF
    np.testing.assert_array_equal(y, np.array(case["y"]))


@pytest.mark.parametrize("name", ["spmv_tridiagonal", "spmv_nonsquare", "spmv_local_ctor"])
@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_spmv_golden_host_layer(hp, golden, gpu_backend_i32, gpu_backend_i64, name, which, monkeypatch):
    """Reads like test/test_vector_multiplication.jl:42-118: HPCSparseMatrix(A, backend) * HPCVector.
    "i64": the reference's default Ti on a NARROWED plan (Int32 kernels); "i64wide": the Int64 kernels."""
    import scipy.sparse as sp
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    case = golden[name]
    A = sp.coo_matrix((case["V"], (np.array(case["I"]) - 1, np.array(case["J"]) - 1)),
                      shape=(case["m"], case["n"])).tocsr()
    Adist = hp.HPCSparseMatrix_from_global(A, backend)
    xdist = hp.HPCVector.from_global(np.array(case["x"]), backend)
    ydist = Adist @ xdist
    assert isinstance(ydist, hp.HPCVector) and ydist.backend is backend
    np.testing.assert_array_equal(ydist.partition, Adist.row_partition)
    # compared the way the reference's GPU tests compare (test/test_utils.jl:203-207): after
    # to_backend(y, cpu_version(backend)), on the host copy
    y_cpu = hp.to_backend(ydist, hp.cpu_version(backend))
    assert isinstance(y_cpu.backend.device, hp.DeviceCPU) and y_cpu.v.device.type == "cpu"
    assert y_cpu.structural_hash == ydist.structural_hash
    assert np.max(np.abs(y_cpu.v.numpy() - np.array(case["y"]))) < TOL_REF
    # mul!(y, A, x)  (test/test_vector_multiplication.jl:70-92)
    y2 = hp.HPCVector.zeros(Adist.row_partition, backend)
    hp.mul_(y2, Adist, xdist)
    np.testing.assert_array_equal(y2.local_values(), np.array(case["y"]))
    assert hp.cache_sizes()["vector_plan_cache"] >= 1


# ---------------------------------------------------------------------------------------------------
# randomised / structured parity, bit-exact
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(1, 1.0), (255, 0.05), (256, 0.05), (257, 0.05), (1000, 0.01),
                                 (10_000, 0.01), (5000, 0.0002)])
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_sprand_bit_exact(hp, orc, gpu_backend_i32, n, p, Ti):
    """configs[0]-like unstructured matrices incl. empty rows and ragged block tails."""
    rows = orc.sprand_rows(n, p, 0, n)
    ci, cv = orc.compress_columns(rows)
    x = orc.fill_uniform(0, n, orc.SEED_X)
    want = orc.spmv(rows.rowptr.astype(Ti), cv.astype(Ti), rows.vals, x[ci])
    got = _raw_spmv(hp, rows.rowptr, cv, rows.vals, x[ci], Ti)
    np.testing.assert_array_equal(got, want)


def test_spmv_long_rows_chunk_loop(hp, orc, gpu_backend_i32):
    """Rows much longer than the 2048-entry LDS chunk (carry across chunks) next to empty rows."""
    rng = np.random.default_rng(5)
    n = 20_000
    lens = np.zeros(300, dtype=np.int64)
    lens[[0, 7, 130, 131, 299]] = [9000, 2048, 2049, 1, 15000]
    lens[200:260] = 37
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    cols = np.concatenate([np.sort(rng.choice(n, size=l, replace=False)) for l in lens if l]).astype(np.int64)
    vals = rng.standard_normal(len(cols))
    x = rng.standard_normal(n)
    want = orc.spmv(rowptr.astype(np.int32), cols.astype(np.int32), vals, x)
    got = _raw_spmv(hp, rowptr, cols, vals, x, np.int32)
    np.testing.assert_array_equal(got, want)
    assert got[1] == 0.0 and got[298] == 0.0


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_whole_pass_rows_split_and_dot_epilogue(hp, orc, Ti):
    """Rows that own whole passes of a wave (round 5: the row-gather kernel multiplies such a pass out with all 64 lanes and
    the owner adds the parked products in stored order) in the forms the first test of this file does not reach: the SPLIT
    column space (own x + ghost segment, 1-based arrays, block lists) and the fused x.y epilogue -- rows of exactly one pass
    (464), one short of / one past it, several passes, a long row as the LAST row of a wave and as the first of the next.
    Same bits as the oracle."""
    import ctypes
    import torch
    rng = np.random.default_rng(77)
    n = 12_000                                        # square: the x.y epilogue pairs x[r] with y[r]
    lens = rng.integers(0, 9, n)
    for r, l in {0: 464, 1: 463, 2: 465, 63: 3000, 64: 2500, 200: 928, 255: 10_000, 256: 929, 699: 1857, n - 1: 700}.items():
        lens[r] = l
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.concatenate([np.sort(rng.choice(n, size=int(l), replace=False)) for l in lens if l]).astype(np.int64)
    vals = rng.standard_normal(len(cols))
    x = rng.standard_normal(n)
    want = orc.spmv(rowptr.astype(Ti), cols.astype(Ti), vals, x)
    sfx = "i32" if Ti == np.int32 else "i64"
    s = torch.cuda.current_stream().cuda_stream
    lib = hp._capi.load()
    try:
        n_own = 7_000
        rp, cv, nz = _t((rowptr + 1).astype(Ti)), _t((cols + 1).astype(Ti)), _t(vals)
        xo, xg = _t(x[:n_own]), _t(x[n_own:])
        nrows = len(lens)
        nblk = (nrows + lib.hpcla_spmv_rows_per_block() - 1) // lib.hpcla_spmv_rows_per_block()
        y = torch.full((nrows,), float("nan"), dtype=torch.float64, device="cuda")
        for blocks in (_t(np.arange(0, nblk, 2, dtype=np.int32)), _t(np.arange(1, nblk, 2, dtype=np.int32))):
            hp._capi.call(f"hpcla_spmv_split_f64_{sfx}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xo.data_ptr(), xg.data_ptr(), n_own,
                          y.data_ptr(), nrows, len(vals), 1, blocks.data_ptr(), blocks.numel(), s)
        np.testing.assert_array_equal(y.cpu().numpy(), want)
        # fused x.y epilogue, unsplit
        work = torch.empty(lib.hpcla_spmv_dot_work_bytes(nrows) // 8 + 1, dtype=torch.float64, device="cuda")
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        xs = _t(x)
        y.fill_(float("nan"))
        hp._capi.call(f"hpcla_spmv_dist_dot_f64_{sfx}", None, None, rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xs.data_ptr(), n,
                      y.data_ptr(), nrows, len(vals), 1, None, 0, None, 0, out.data_ptr(), work.data_ptr(), s)
        np.testing.assert_array_equal(y.cpu().numpy(), want)
        ref = float(np.dot(x, want))
        assert abs(out.item() - ref) <= 1e-12 * float(np.abs(x) @ np.abs(want))
    finally:
        pass


@pytest.mark.parametrize("nblk", gr.PARTIAL_BLOCKS)
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_dot_epilogue_at_the_branch_of_the_partial_sums(hp, orc, Ti, nblk):
    """The x.y epilogue of the fused SpMV leaves one partial per row block, which reduce_partials_sum adds in one stage up to
    4 * 256 = 1024 partials and in two above.  Row counts, with rpb rows per block: 1024 rpb is the last one-stage count (four
    full trips of the one workgroup); 1024 rpb + 1 the first two-stage count: 1025 partials, so one stage-1 workgroup whose
    lane 0 adds the odd last partial as the scalar tail; 2051 rpb + 1 gives 2052 partials on two stage-1 workgroups
    (tests/test_grid_regimes.py checks these counts against the branch).  A tridiagonal matrix with seeded random values, so
    every block's partial differs from the others; raw ABI, no plan and no block lists.  y: the oracle's bits; x.y: the project's
    margin for its reductions against math.fsum, relative to the sum of |x_i y_i|; two runs: the same bits."""
    import torch
    lib = hp._capi.load()
    rpb = lib.hpcla_spmv_rows_per_block()
    n = (nblk - 1) * rpb + (rpb if nblk == gr.PARTIAL_BLOCKS[0] else 1)
    assert (n + rpb - 1) // rpb == nblk
    rng = np.random.default_rng(1000 + nblk)
    lens = np.full(n, 3, dtype=np.int64)
    lens[0] = lens[-1] = 2
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = (np.repeat(np.arange(n, dtype=np.int64), 3) + np.tile(np.array([-1, 0, 1], dtype=np.int64), n))[1:-1]
    vals = rng.standard_normal(len(cols))
    x = rng.standard_normal(n)
    want = orc.spmv(rowptr.astype(Ti), cols.astype(Ti), vals, x)
    terms = x * want
    blocks = np.add.reduceat(terms, np.arange(0, n, rpb))
    assert len(blocks) == nblk and len(np.unique(blocks)) == nblk
    sfx = "i32" if Ti == np.int32 else "i64"
    s = torch.cuda.current_stream().cuda_stream
    rp, cv, nz, xs = _t(rowptr.astype(Ti)), _t(cols.astype(Ti)), _t(vals), _t(x)
    work = torch.empty(lib.hpcla_spmv_dot_work_bytes(n) // 8 + 1, dtype=torch.float64, device="cuda")
    got = []
    for _ in range(2):
        y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        work.fill_(float("nan"))
        hp._capi.call(f"hpcla_spmv_dist_dot_f64_{sfx}", None, None, rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xs.data_ptr(), n,
                      y.data_ptr(), n, len(vals), 0, None, 0, None, 0, out.data_ptr(), work.data_ptr(), s)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(y.cpu().numpy(), want)
        got.append(out.item())
    err = abs(got[0] - math.fsum(terms.tolist())) / float(np.abs(terms).sum())
    print(f"{sfx}, {nblk} partials: x.y off by {err:.2e} of the sum of |terms|")
    assert err <= RTOL_RED
    assert np.float64(got[0]).view(np.uint64) == np.float64(got[1]).view(np.uint64)


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_long_rows_opt_in(hp, orc, Ti):
    """OPT-IN long rows (hpcla_spmv_longrows_f64_*, HPCSparseMatrix.enable_long_rows): rows of >= min_len entries are summed
    in TREE order -- north_star's "__shfl / segmented-scan row reductions", where they are needed -- every other row keeps
    the reference's bits.  Bar for a long row r: |y_r - sequential| <= 1e-12 * (|A||x|)_r (SURVEY 8d's componentwise
    bound); bar for every other row: bit equality with the oracle.  Long rows at the start, across wave / block borders,
    next to each other, at the very end; a long row whose pieces are shorter than the minimum piece; split column space
    with a ghost segment through the raw ABI; the default path on the same matrix stays bit-exact."""
    import torch
    rng = np.random.default_rng(11)
    n = 300_000
    lens = rng.integers(0, 9, 1500)
    long_at = {0: 5000, 63: 4096, 64: 300_000, 65: 4100, 255: 9000, 256: 70_000, 700: 1_100_000 // 4, 1499: 12_345}
    for r, l in long_at.items():
        lens[r] = l
    lens[300:330] = 0
    lens[400] = 4095                                   # one short of the threshold: stays sequential
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.concatenate([np.sort(rng.choice(n, size=int(l), replace=False)) for l in lens if l]).astype(np.int64)
    vals = rng.standard_normal(len(cols))
    x = rng.standard_normal(n)
    want = orc.spmv(rowptr.astype(Ti), cols.astype(Ti), vals, x)
    bound = orc.spmv(rowptr.astype(Ti), cols.astype(Ti), np.abs(vals), np.abs(x))
    is_long = lens >= 4096
    assert is_long.sum() == len(long_at)
    # host layer: default = the oracle's bits on every row; opted in = bits on the short rows, the bound on the long ones
    backend = hp.backend_rocm_serial(np.float64, Ti)
    A = hp.HPCSparseMatrix_local(rowptr, cols, vals, n, backend)
    xv = hp.HPCVector.from_global(x, backend)
    np.testing.assert_array_equal((A @ xv).local_values(), want)
    assert A.enable_long_rows(4096) == len(long_at)
    got = (A @ xv).local_values()
    np.testing.assert_array_equal(got[~is_long], want[~is_long])
    assert np.all(np.abs(got[is_long] - want[is_long]) <= 1e-12 * bound[is_long]), np.abs(got - want)[is_long] / bound[is_long]
    assert np.array_equal((A @ xv).local_values(), got)                        # deterministic
    A.disable_long_rows()
    np.testing.assert_array_equal((A @ xv).local_values(), want)
    assert A.enable_long_rows(2_000_000) == 0                                  # nothing qualifies: the default path
    np.testing.assert_array_equal((A @ xv).local_values(), want)
    with pytest.raises(ValueError):
        A.enable_long_rows(100)
    # raw ABI, split column space: columns >= n_own come from a ghost segment; index base 1
    sfx = "i32" if Ti == np.int32 else "i64"
    n_own = 200_000
    s = torch.cuda.current_stream().cuda_stream
    rp, cv, nz = _t((rowptr + 1).astype(Ti)), _t((cols + 1).astype(Ti)), _t(vals)
    xo, xg = _t(x[:n_own]), _t(x[n_own:])
    rows = _t(np.flatnonzero(is_long).astype(np.int64))
    work = torch.empty(hp._capi.load().hpcla_spmv_longrows_work_bytes(int(rows.numel())) // 8, dtype=torch.float64, device="cuda")
    y = torch.full((len(lens),), float("nan"), dtype=torch.float64, device="cuda")
    hp._capi.call(f"hpcla_spmv_longrows_f64_{sfx}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xo.data_ptr(), xg.data_ptr(), n_own,
                  y.data_ptr(), len(lens), len(vals), 1, rows.data_ptr(), int(rows.numel()), 4096, work.data_ptr(), s)
    got = y.cpu().numpy()
    np.testing.assert_array_equal(got[~is_long], want[~is_long])
    assert np.all(np.abs(got[is_long] - want[is_long]) <= 1e-12 * bound[is_long])
    with pytest.raises(hp._capi.HPCLAError):                                   # a threshold below two wave passes is refused
        hp._capi.call(f"hpcla_spmv_longrows_f64_{sfx}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xo.data_ptr(), xg.data_ptr(), n_own,
                      y.data_ptr(), len(lens), len(vals), 1, rows.data_ptr(), int(rows.numel()), 100, work.data_ptr(), s)
    # round 6: a qualifying row the caller's list OMITS is summed by nobody -- its y must read NaN, not the value an
    # earlier product left there; every listed and every short row as before
    y.fill_(12345.0)
    fewer = rows[1:].contiguous()
    hp._capi.call(f"hpcla_spmv_longrows_f64_{sfx}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xo.data_ptr(), xg.data_ptr(), n_own,
                  y.data_ptr(), len(lens), len(vals), 1, fewer.data_ptr(), int(fewer.numel()), 4096, work.data_ptr(), s)
    got = y.cpu().numpy()
    omitted = int(rows[0].item())
    assert np.isnan(got[omitted])
    keep = np.ones(len(lens), bool)
    keep[omitted] = False
    np.testing.assert_array_equal(got[keep & ~is_long], want[keep & ~is_long])
    assert np.all(np.abs(got[keep & is_long] - want[keep & is_long]) <= 1e-12 * bound[keep & is_long])
    # unaligned colval / nzval (a view one entry into a larger buffer): the entry falls back to the default order -- every row
    # sequential, hence the oracle's bits on ALL rows -- instead of refusing the product
    pad_cv = torch.empty(len(vals) + 1, dtype=cv.dtype, device="cuda")
    pad_nz = torch.empty(len(vals) + 1, dtype=torch.float64, device="cuda")
    pad_cv[1:] = cv
    pad_nz[1:] = nz
    ucv, unz = pad_cv[1:], pad_nz[1:]
    assert unz.data_ptr() % 32 != 0
    y.fill_(float("nan"))
    hp._capi.call(f"hpcla_spmv_longrows_f64_{sfx}", rp.data_ptr(), ucv.data_ptr(), unz.data_ptr(), xo.data_ptr(), xg.data_ptr(), n_own,
                  y.data_ptr(), len(lens), len(vals), 1, rows.data_ptr(), int(rows.numel()), 4096, work.data_ptr(), s)
    np.testing.assert_array_equal(y.cpu().numpy(), want)


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_block_order_hint_is_a_bijection_with_the_same_bits(hp, orc, gpu_backend_i32, Ti):
    """hpcla_spmv_block_order_hint: XCD-grouped order of the row blocks.  Every group size must visit every row block
    exactly once -- y bit-identical to the natural order, incl. a ragged tail (block count not a multiple of 8 G),
    groups larger than the launch, and the fused x.y entry; a bad group is rejected; group 0 removes the hint."""
    import torch
    n = 256 * 1237 + 77                       # 1238 row blocks: ragged for every G
    rows = orc.poisson2d_rows(n // 50 + 1, 50, 0, n)
    x = orc.fill_uniform(0, (n // 50 + 1) * 50, orc.SEED_X)
    want = orc.spmv(rows.rowptr.astype(Ti), rows.colidx.astype(Ti), rows.vals, x)
    sfx = "i32" if Ti == np.int32 else "i64"
    rp, cv, nz, xd = _t(rows.rowptr.astype(Ti)), _t(rows.colidx.astype(Ti)), _t(rows.vals), _t(x)
    s = torch.cuda.current_stream().cuda_stream
    lib = hp._capi.load()
    work = torch.empty(lib.hpcla_spmv_dot_work_bytes(n) // 8 + 1, dtype=torch.float64, device="cuda")
    dots = []
    try:
        for G in (0, 2, 4, 64, 1024, 1):
            hp._capi.call("hpcla_spmv_block_order_hint", rp.data_ptr(), G)
            y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            hp._capi.call(f"hpcla_spmv_csr_f64_{sfx}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xd.data_ptr(), y.data_ptr(),
                          n, len(rows.vals), 0, s)
            np.testing.assert_array_equal(y.cpu().numpy(), want, err_msg=f"group {G}")
            y.fill_(float("nan"))
            d = torch.zeros(1, dtype=torch.float64, device="cuda")
            hp._capi.call(f"hpcla_spmv_dist_dot_f64_{sfx}", None, None, rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xd.data_ptr(),
                          n, y.data_ptr(), n, len(rows.vals), 0, None, 0, None, 0, d.data_ptr(), work.data_ptr(), s)
            np.testing.assert_array_equal(y.cpu().numpy(), want, err_msg=f"fused entry, group {G}")
            dots.append(float(d.item()))
        assert len(set(dots)) == 1               # the partials are indexed by ROW BLOCK, not by workgroup: same sum
        for bad in (3, -2, 2048):
            assert lib.hpcla_spmv_block_order_hint(ctypes.c_void_p(rp.data_ptr()), bad) != 0
        assert lib.hpcla_spmv_block_order_hint(None, 4) != 0
    finally:
        lib.hpcla_spmv_block_order_hint(ctypes.c_void_p(rp.data_ptr()), 0)


def test_plan_measures_block_order_once_per_structure(hp, orc, gpu_backend_i32):
    """hpcla_spmv_tune_block_order_* at plan time: the choice is one of the measured candidates, it is registered for
    the matrix, products are bit-identical under it and under the natural order, small matrices are not measured, and
    the hint dies with the matrix (host table only)."""
    import gc
    import torch
    from benchmarks.extra_workloads import device_stencil
    backend = gpu_backend_i32
    s = torch.cuda.current_stream().cuda_stream
    A3 = device_stencil(hp, torch, backend, (512, 512, 8), 0, 512 * 512 * 8)          # 8192 row blocks: measured
    x3 = hp.HPCVector.zeros(A3.row_partition, backend)
    hp._capi.call("hpcla_fill_uniform_f64", x3.v.data_ptr(), 0, A3.nrows_local, orc.SEED_X, s)
    plan3 = hp.get_vector_plan(A3, x3)
    assert plan3.block_group in (1, 8, 32, 64) and A3._block_order_hint == plan3.block_group
    y_plan = (A3 @ x3).v.clone()
    for G in (0, 64):
        hp._capi.call("hpcla_spmv_block_order_hint", A3.rowptr_target.data_ptr(), G)
        np.testing.assert_array_equal((A3 @ x3).v.cpu().numpy(), y_plan.cpu().numpy())
    # a second matrix of the same structure shares the plan and gets the same order registered for ITS arrays
    B3 = device_stencil(hp, torch, backend, (512, 512, 8), 0, 512 * 512 * 8)
    assert hp.get_vector_plan(B3, x3) is plan3 and B3._block_order_hint == plan3.block_group
    # the raw entry: small matrix -> natural, unmeasured; bad arguments -> error
    A2 = device_stencil(hp, torch, backend, (256, 256), 0, 256 * 256)
    x2 = hp.HPCVector.zeros(A2.row_partition, backend)
    assert hp.get_vector_plan(A2, x2).block_group == 1
    lib = hp._capi.load()
    chosen = ctypes.c_int(-1)
    assert lib.hpcla_spmv_tune_block_order_f64_i32(None, None, None, None, None, 0, None, 10, 10, 0, None, ctypes.byref(chosen)) != 0
    del A3, B3, plan3
    gc.collect()
    hp.clear_plan_cache()


def test_spmv_empty_and_zero_nnz(hp, gpu_backend_i32):
    got = _raw_spmv(hp, np.zeros(5, dtype=np.int64), np.empty(0, dtype=np.int64), np.empty(0), np.ones(3), np.int32)
    np.testing.assert_array_equal(got, np.zeros(4))
    got0 = _raw_spmv(hp, np.zeros(1, dtype=np.int64), np.empty(0, dtype=np.int64), np.empty(0), np.ones(3), np.int32)
    assert len(got0) == 0


@pytest.mark.parametrize("N", [64, 300, 1024])
def test_poisson2d_host_layer_bit_exact(hp, orc, gpu_backend_i32, N):
    rows = orc.poisson2d_rows(N, N, 0, N * N)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N * N, gpu_backend_i32)
    xg = orc.fill_uniform(0, N * N, orc.SEED_X)
    x = hp.HPCVector.from_global(xg, gpu_backend_i32)
    y = (A @ x).local_values()
    ci, cv = orc.compress_columns(rows)
    np.testing.assert_array_equal(A.col_indices, ci)
    np.testing.assert_array_equal(A.colval, cv)
    want = orc.spmv(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, xg[ci])
    np.testing.assert_array_equal(y, want)
    # componentwise bound of SURVEY section 8d holds trivially (difference is zero); also check linearity
    y2 = (A @ (x * 2.0)).local_values()
    np.testing.assert_array_equal(y2, 2.0 * want)     # scaling by 2 is exact in fp64


def test_poisson3d_host_layer_bit_exact(hp, orc, gpu_backend_i32):
    N = 48
    rows = orc.poisson3d_rows(N, N, N, 0, N ** 3)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N ** 3, gpu_backend_i32)
    xg = orc.fill_uniform(0, N ** 3, orc.SEED_X)
    y = (A @ hp.HPCVector.from_global(xg, gpu_backend_i32)).local_values()
    want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, xg)
    np.testing.assert_array_equal(y, want)


def test_full_size_config2_poisson4096(hp, orc, gpu_backend_i32):
    """BASELINE configs[1] at full size (n = 4096^2, nnz = 83 869 696): bit-exact against the oracle,
    plus size-independent properties (A*1 = boundary pattern, linearity)."""
    import torch
    N = 4096
    rows = orc.poisson2d_rows(N, N, 0, N * N)
    assert rows.nnz == 5 * N * N - 4 * N == 83_869_696
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N * N, gpu_backend_i32)
    xg = orc.fill_uniform(0, N * N, orc.SEED_X)
    x = hp.HPCVector.from_global(xg, gpu_backend_i32)
    y = (A @ x).local_values()
    want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, xg)
    np.testing.assert_array_equal(y, want)
    rel = np.linalg.norm(y - want) / np.linalg.norm(want)
    assert rel <= 1e-12
    ones = hp.HPCVector.from_global(np.ones(N * N), gpu_backend_i32)
    y1 = (A @ ones).local_values().reshape(N, N)
    assert np.all(y1[1:-1, 1:-1] == 0.0) and y1[0, 0] == 2.0 and y1[0, 5] == 1.0
    del A, x, ones
    hp.clear_plan_cache()
    torch.cuda.empty_cache()


def test_full_size_config4_share_poisson3d_cg_pieces(hp, orc, gpu_backend_i32):
    """BASELINE configs[3]'s per-GPU share (512 x 512 x 64 planes of the 7-point Laplacian,
    n = 16 777 216, nnz = 116 785 152): SpMV bit-exact against the oracle, the fused SpMV+dot equals
    the separate dot to reduction tolerance, and 3 CG iterations keep the Krylov identities
    (r_k orthogonal to r_{k-1} to rounding; residual norm equals ||b - A x||)."""
    import torch
    from hpcla_amd import workloads as wl
    nx, ny, nz = 512, 512, 64
    n = nx * ny * nz
    rp, ci, va = wl.poisson3d_rows(nx, ny, nz, 0, n)
    assert len(va) == 7 * n - 2 * (nx * ny + ny * nz + nx * nz) == 116_785_152
    A = hp.HPCSparseMatrix_local(rp, ci, va, n, gpu_backend_i32)
    bg = orc.fill_uniform(0, n, orc.SEED_RHS)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    y = A @ b
    want = orc.spmv(rp.astype(np.int32), ci.astype(np.int32), va, bg)
    np.testing.assert_array_equal(y.local_values(), want)
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    y2 = b.similar()
    hp.mul_dot_(y2, A, b, out)
    assert torch.equal(y2.v, y.v)
    ref = float(np.dot(bg, want))
    assert abs(out.item() - ref) <= RTOL_RED * float(np.dot(np.abs(bg), np.abs(want)))
    x, hist = hp.cg_fixed_iterations(A, b, 3)
    res = (b - A @ x)
    true_norm = hp.norm(res)
    assert abs(true_norm - hist[-1]) <= 1e-10 * hist[0]
    del A, b, y, y2, x, res
    hp.clear_plan_cache()
    torch.cuda.empty_cache()


def test_large_spmm_columns_equal_spmv_bitwise(hp, orc, gpu_backend_i32):
    """Size-independent property of the reference's SpMM (src/sparse.jl:2391-2413: one SpMV per column):
    column j of A*B is bit-identical to A*B[:,j], here at 1 048 576 rows, ~2.1e7 stored entries,
    k = 16 (config 5's access pattern: uniformly random columns)."""
    import torch
    n, k, per_row = 1 << 20, 16, 20
    rng = np.random.default_rng(5)
    cols = np.sort(rng.integers(0, n, size=(n, per_row), dtype=np.int64), axis=1)
    keep = np.ones_like(cols, dtype=bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]                       # drop duplicate columns within a row
    counts = keep.sum(axis=1)
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ci = cols[keep]
    va = rng.random(len(ci))
    A = hp.HPCSparseMatrix_local(rp, ci, va, n, gpu_backend_i32)
    Bg = rng.random((n, k))
    B = hp.HPCMatrix.from_global(Bg, gpu_backend_i32)
    C = hp.spmm(A, B)
    for j in (0, 7, 15):
        xj = B[:, j]                                                # getindex(::HPCMatrix, :, k), src/indexing.jl:385-393
        np.testing.assert_array_equal(xj.local_values(), Bg[:, j])
        yj = A @ xj
        assert torch.equal(C.A[:, j].contiguous(), yj.v), f"column {j}"
    want0 = orc.spmv(rp.astype(np.int32), ci.astype(np.int32), va, np.ascontiguousarray(Bg[:, 0]))
    np.testing.assert_array_equal(C.A[:, 0].cpu().numpy(), want0)
    del A, B, C
    hp.clear_plan_cache(); hp.clear_spmm_cache()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------
# distributed semantics on ONE GPU: every simulated rank's split-column SpMV with a hand-filled
# ghost segment + interior/boundary block lists == the reference pipeline for that rank
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nranks", [("poisson", 2), ("poisson", 4), ("sprand", 3)])
def test_split_spmv_per_rank_matches_reference_pipeline(hp, orc, gpu_backend_i32, kind, nranks):
    import torch
    if kind == "poisson":
        nx, ny = 512, 64 * nranks
        n = nx * ny
        gen = lambda lo, hi: orc.poisson2d_rows(nx, ny, lo, hi)
    else:
        n = 6000
        gen = lambda lo, hi: orc.sprand_rows(n, 0.004, lo, hi)
    rp = orc.uniform_partition(n, nranks)
    xp = rp
    x = orc.fill_uniform(0, n, orc.SEED_X)
    locs = [gen(int(rp[r]), int(rp[r + 1])) for r in range(nranks)]
    comp = [orc.compress_columns(l) for l in locs]
    plans = orc.vector_plans([c[0] for c in comp], xp)
    gathered = orc.execute_plans(plans, [x[xp[r]:xp[r + 1]] for r in range(nranks)])
    rpb = hp._capi.load().hpcla_spmv_rows_per_block()
    s = torch.cuda.current_stream().cuda_stream
    for r in range(nranks):
        rows, (ci, cv), pl = locs[r], comp[r], plans[r]
        want = orc.spmv(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, gathered[r])
        n_own = int(xp[r + 1] - xp[r])
        hplan = hp.HostVectorPlan(pl.send_rank_ids, pl.send_indices, pl.recv_rank_ids, pl.recv_perm,
                                  pl.local_src_indices, pl.local_dst_indices, pl.n_gathered, n_own)
        cmap = hp.split_column_map(hplan)
        ghost = (np.concatenate([gathered[r][p] for p in pl.recv_perm]) if pl.recv_perm else np.zeros(1))
        d_rp, d_cv = _t(rows.rowptr.astype(np.int32)), _t(cv.astype(np.int32))
        d_map, d_nz = _t(cmap.astype(np.int32)), _t(rows.vals)
        d_split = torch.empty_like(d_cv)
        hp._capi.call("hpcla_remap_i32", d_cv.data_ptr(), d_map.data_ptr(), d_split.data_ptr(), len(cv), 0, s)
        np.testing.assert_array_equal(d_split.cpu().numpy(), cmap[cv])
        nblk = (rows.nrows + rpb - 1) // rpb
        flags = torch.empty(nblk, dtype=torch.int32, device="cuda")
        hp._capi.call("hpcla_classify_blocks_i32", d_rp.data_ptr(), d_split.data_ptr(), rows.nrows, 0,
                      n_own, rpb, flags.data_ptr(), s)
        f = flags.cpu().numpy()
        f_ref = np.array([np.any(cmap[cv[rows.rowptr[b * rpb]:rows.rowptr[min((b + 1) * rpb, rows.nrows)]]] >= n_own)
                          for b in range(nblk)]).astype(np.int32)
        np.testing.assert_array_equal(f, f_ref)
        interior = _t(np.flatnonzero(f == 0).astype(np.int32))
        boundary = _t(np.flatnonzero(f != 0).astype(np.int32))
        d_x, d_g = _t(x[xp[r]:xp[r + 1]]), _t(ghost)
        y = torch.full((rows.nrows,), float("nan"), dtype=torch.float64, device="cuda")
        for lst in (interior, boundary):
            hp._capi.call("hpcla_spmv_split_f64_i32", d_rp.data_ptr(), d_split.data_ptr(), d_nz.data_ptr(),
                          d_x.data_ptr(), d_g.data_ptr(), n_own, y.data_ptr(), rows.nrows, rows.nnz, 0,
                          lst.data_ptr() if lst.numel() else None, lst.numel(), s)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(y.cpu().numpy(), want)
        if kind == "poisson" and nranks > 1:
            assert 0 < boundary.numel() <= 2 * (nx // rpb + 1) and interior.numel() > 0


def test_execute_plan_gathered_serial(hp, orc, gpu_backend_i32):
    """execute_plan! API parity: gathered == x[col_indices] (src/vectors.jl:394-463)."""
    n = 3000
    rows = orc.sprand_rows(n, 0.001, 0, n)            # many columns untouched -> real compression
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, gpu_backend_i32)
    xg = orc.fill_uniform(0, n, 3)
    x = hp.HPCVector.from_global(xg, gpu_backend_i32)
    plan = hp.get_vector_plan(A, x)
    assert plan is hp.get_vector_plan(A, x)           # memoized (src/sparse.jl:1992-2001)
    g = hp.execute_plan(plan, x).cpu().numpy()
    np.testing.assert_array_equal(g, xg[A.col_indices])
    assert A.ncols_compressed < n


@pytest.mark.parametrize("mode", ["serial", "overlap", "push"])
def test_rccl_halo_self_exchange_subprocess(mode):
    """The RCCL send/recv + side-stream + event code of hpcla_halo_begin/end and both orderings of the
    fused distributed SpMV (HPCLA_HALO_MODE: exchange on the caller's stream then one launch / exchange
    and boundary blocks on the side stream next to the interior blocks), exercised on one GPU with a
    one-rank RCCL communicator sending to itself (HPCLA_FORCE_RCCL=1)."""
    env = dict(os.environ, HPCLA_FORCE_RCCL="1", HPCLA_HALO_MODE=mode, HPCLA_PUSH_TIMEOUT_S="2")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_halo_self_worker.py")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "halo self-exchange OK" in out.stdout


# ---------------------------------------------------------------------------------------------------
# reductions and vector updates
# ---------------------------------------------------------------------------------------------------
def test_dot_norm_golden_and_random(hp, orc, golden, gpu_backend_i32):
    b = gpu_backend_i32
    d = golden["dot"]
    x, y = hp.HPCVector.from_global(np.array(d["x"]), b), hp.HPCVector.from_global(np.array(d["y"]), b)
    assert abs(hp.dot(x, y) - d["dot_xy"]) < TOL_REF and abs(hp.dot(x, x) - d["dot_xx"]) < TOL_REF
    nm = golden["norms"]
    v = hp.HPCVector.from_global(np.array(nm["x"]), b)
    assert abs(hp.norm(v) - nm["norm2"]) < TOL_REF
    assert abs(hp.norm(v, 1) - nm["norm1"]) < TOL_REF
    assert abs(hp.norm(v, math.inf) - nm["norminf"]) < TOL_REF
    assert abs(hp.norm(v, 3) - nm["norm3"]) < TOL_REF and abs(hp.norm(v, 1.5) - nm["norm1p5"]) < TOL_REF
    with pytest.raises(ValueError):
        hp.norm(v, -1)
    # 100 003: 49 partials; 4 000 001: 1954, a ragged eighth trip of reduce_stage2; 4 194 307: the cap of 2048 workgroups, each
    # lane in four grid-stride trips and lane 0 in a fifth, and odd (tests/_grid_regimes.py, tests/test_grid_regimes.py)
    for n in gr.PLAIN_F64:
        xg, yg = orc.fill_uniform(0, n, 1) - 0.5, orc.fill_uniform(0, n, 2) - 0.25
        xv, yv = hp.HPCVector.from_global(xg, b), hp.HPCVector.from_global(yg, b)
        scale = float(np.abs(xg) @ np.abs(yg))
        assert abs(hp.dot(xv, yv) - orc.dot([xg], [yg])) <= RTOL_RED * scale
        assert abs(hp.norm(xv) - orc.norm([xg], 2)) <= RTOL_RED * orc.norm([xg], 2)
        assert abs(hp.norm(xv, 1) - orc.norm([xg], 1)) <= RTOL_RED * orc.norm([xg], 1)
        assert hp.norm(xv, math.inf) == orc.norm([xg], math.inf)
        assert hp.maximum(xv) == xg.max() and hp.minimum(xv) == xg.min()            # src/vectors.jl:815-836
        assert abs(hp.vsum(xv) - xg.sum()) <= RTOL_RED * np.abs(xg).sum()           # src/vectors.jl:838-845
        want3 = float(np.sum(np.abs(xg) ** 3.0)) ** (1.0 / 3.0)                      # general p (src/vectors.jl:774-779)
        assert abs(hp.norm(xv, 3) - want3) <= 1e-11 * want3
        pg = 1.0 + 1e-3 * xg                                                          # prod(v), src/vectors.jl:853-858
        want_p = float(np.exp(np.sum(np.log(pg)))) if n > 64 else float(np.prod(pg))
        assert abs(hp.prod(hp.HPCVector.from_global(pg, b)) - want_p) <= (1e-9 if n > 64 else RTOL_RED) * abs(want_p)
    # the reference's own reductions case (test/test_vector_multiplication.jl:198-225): x = 1..8
    r8 = hp.HPCVector.from_global(np.arange(1.0, 9.0), b)
    assert hp.vsum(r8) == 36.0 and hp.prod(r8) == 40320.0 and hp.maximum(r8) == 8.0 and hp.minimum(r8) == 1.0
    # deterministic: two runs give the same bits
    assert hp.dot(xv, yv) == hp.dot(xv, yv)


@pytest.mark.parametrize("n,where", gr.PLAIN_F64_NAN)
def test_max_reductions_propagate_nan(hp, orc, gpu_backend_i32, n, where):
    """At n = 4 194 307 the grid is capped at 2048 workgroups, so a trip of stage 1 is 524 288 double2: element 4 194 303 is read
    by the last lane of the last workgroup in its last trip, 4 194 305 by lane 0 of workgroup 0 in a fifth trip of its own and
    4 194 306 is the scalar tail (tests/test_grid_regimes.py checks these positions against the grid).
    ADVICE r4: `v > s ? v : s` never selected a NaN, so norm(v, Inf) / maximum / minimum of a vector holding one NaN
    returned a finite number -- and with it the NaN rows an expired halo wait leaves in y.  Julia's maximum and
    norm(., Inf) return NaN (src/vectors.jl:769-772, 815-836)."""
    xg = orc.fill_uniform(0, n, 3) - 0.5
    xg[where] = np.nan
    v = hp.HPCVector.from_global(xg, gpu_backend_i32)
    assert math.isnan(hp.norm(v, math.inf)) and math.isnan(hp.maximum(v)) and math.isnan(hp.minimum(v))
    assert math.isnan(hp.norm(v)) and math.isnan(hp.norm(v, 1)) and math.isnan(hp.vsum(v))
    xg[where] = 0.25                                   # ... and without the NaN the same calls are exact again
    v = hp.HPCVector.from_global(xg, gpu_backend_i32)
    assert hp.norm(v, math.inf) == np.abs(xg).max() and hp.maximum(v) == xg.max() and hp.minimum(v) == xg.min()


def test_vector_ops_golden_and_random(hp, orc, golden, gpu_backend_i32):
    b = gpu_backend_i32
    c = golden["vector_ops"]
    u, v = hp.HPCVector.from_global(np.array(c["u"]), b), hp.HPCVector.from_global(np.array(c["v"]), b)
    np.testing.assert_array_equal((u + v).local_values(), c["add"])
    np.testing.assert_array_equal((u - v).local_values(), c["sub"])
    np.testing.assert_array_equal((-v).local_values(), c["neg"])
    np.testing.assert_array_equal((v * c["scale"]).local_values(), c["scaled"])
    np.testing.assert_array_equal((c["scale"] * v).local_values(), c["scaled"])
    np.testing.assert_array_equal((v / 2.0).local_values(), c["divided"])
    g = golden["broadcast"]
    vv, ww = hp.HPCVector.from_global(np.array(g["v"]), b), hp.HPCVector.from_global(np.array(g["w"]), b)
    np.testing.assert_array_equal((vv + ww).local_values(), g["add"])
    for n in (1, 2, 777, 1_000_001):
        xg, yg = orc.fill_uniform(0, n, 5), orc.fill_uniform(0, n, 6)
        xv, yv = hp.HPCVector.from_global(xg, b), hp.HPCVector.from_global(yg, b)
        want = yg.copy(); orc.axpy(0.37, xg, want)
        np.testing.assert_array_equal(yv.copy().axpy_(0.37, xv).local_values(), want)
        want = yg.copy(); orc.xpay(xg, -1.25, want)
        np.testing.assert_array_equal(yv.copy().xpay_(xv, -1.25).local_values(), want)
        np.testing.assert_array_equal((xv / 3.0).local_values(), xg / 3.0)
    with pytest.raises(ValueError):
        _ = hp.HPCVector.from_global(np.ones(8), b, partition=np.array([0, 8])) + \
            hp.HPCVector(hp.compute_partition_hash(np.array([0, 9])), np.array([0, 9]), xv.v[:8], b)


def test_device_fill_matches_oracle_generator(hp, orc, gpu_backend_i32):
    import torch
    v = torch.empty(100_001, dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_fill_uniform_f64", v.data_ptr(), 12345, v.numel(), orc.SEED_X,
                  torch.cuda.current_stream().cuda_stream)
    np.testing.assert_array_equal(v.cpu().numpy(), orc.fill_uniform(12345, v.numel(), orc.SEED_X))


# ---------------------------------------------------------------------------------------------------
# SpMM
# ---------------------------------------------------------------------------------------------------
def test_spmm_golden_host_layer(hp, golden, gpu_backend_i32):
    """test/test_new_operations.jl:43-59, 79-82."""
    import scipy.sparse as sp
    case = golden["spmm_sym"]
    A = sp.coo_matrix((case["V"], (np.array(case["I"]) - 1, np.array(case["J"]) - 1)), shape=(8, 8)).tocsr()
    Ad = hp.HPCSparseMatrix_from_global(A, gpu_backend_i32)
    Bd = hp.HPCMatrix.from_global(np.array(case["B"]), gpu_backend_i32)
    Cd = Ad @ Bd
    assert isinstance(Cd, hp.HPCMatrix)
    C = hp.to_backend(Cd, hp.cpu_version(gpu_backend_i32)).A.numpy()       # test/test_utils.jl:203-207
    assert np.max(np.abs(C - np.array(case["C"]))) < TOL_REF
    assert abs(np.linalg.norm(C) - case["C_fro"]) < TOL_REF


@pytest.mark.parametrize("dims,lo,hi", [((7, 5, 4), 0, 140), ((7, 5, 4), 33, 101), ((16, 16, 16), 1000, 4096),
                                        ((1, 1, 5), 0, 5), ((3, 1, 1), 0, 3), ((40, 30, 20), 11111, 24000)])
def test_device_poisson3d_generator_matches_oracle(hp, orc, dims, lo, hi):
    """hpcla_gen_poisson3d (closed-form rowptr, 7-point rows) against the oracle's C generator, any row range."""
    import torch
    nx, ny, nz = dims
    want = orc.poisson3d_rows(nx, ny, nz, lo, hi)
    assert hp._capi.load().hpcla_poisson3d_nnz(nx, ny, nz, lo, hi) == want.nnz
    rp = torch.empty(hi - lo + 1, dtype=torch.int64, device="cuda")
    ci = torch.full((max(want.nnz, 1),), -7, dtype=torch.int64, device="cuda")
    va = torch.full((max(want.nnz, 1),), float("nan"), dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_gen_poisson3d", nx, ny, nz, lo, hi, rp.data_ptr(), ci.data_ptr(), va.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rp.cpu().numpy(), want.rowptr)
    np.testing.assert_array_equal(ci.cpu().numpy()[:want.nnz], want.colidx)
    np.testing.assert_array_equal(va.cpu().numpy()[:want.nnz], want.vals)


def test_to_backend_round_trip(hp, orc, gpu_backend_i32):
    """to_backend (src/HPCLinearAlgebra.jl:337-378): device -> CPU -> device keeps every bit and the
    structure; the CPU copy shares partitions / hashes / host structure arrays, drops cached_transpose, and is
    refused by the operators (no CPU compute path in this build, by design)."""
    b = gpu_backend_i32
    cpu = hp.cpu_version(b)
    n = 3000
    rows = orc.sprand_rows(n, 0.01, 0, n)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, b)
    xg = orc.fill_uniform(0, n, orc.SEED_X)
    x = hp.HPCVector.from_global(xg, b)
    y = A @ x
    A.cached_transpose = object()                                  # pretend transpose(A) was materialised
    Ac, xc = hp.to_backend(A, cpu), hp.to_backend(x, cpu)
    assert Ac.backend is cpu and Ac.nzval.device.type == "cpu" and Ac.rowptr_target.device.type == "cpu"
    assert Ac.cached_transpose is None and Ac.col_indices is A.col_indices and Ac.structural_hash == A.structural_hash
    np.testing.assert_array_equal(Ac.nzval.numpy(), rows.vals)
    np.testing.assert_array_equal(xc.v.numpy(), xg)
    with pytest.raises((TypeError, ValueError)):
        Ac @ xc                                                    # CPU operands: an error, not a fallback
    with pytest.raises((TypeError, ValueError)):
        A @ xc                                                     # mixed backends (src/backends.jl:444-464)
    with pytest.raises(TypeError):
        hp.dot(xc, xc)
    A2, x2 = hp.to_backend(Ac, b), hp.to_backend(xc, b)
    assert A2.backend is b and A2.nzval.is_cuda and A2.rowptr_target.is_cuda
    np.testing.assert_array_equal((A2 @ x2).local_values(), y.local_values())
    M = hp.HPCMatrix.from_global(orc.fill_uniform(0, n * 4, 5).reshape(n, 4), b)
    Mc = hp.to_backend(M, cpu)
    assert Mc.A.device.type == "cpu"
    np.testing.assert_array_equal(hp.to_backend(Mc, b).local_values(), M.local_values())
    A.cached_transpose = None
    hp.clear_plan_cache()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 17, 18, 24, 32, 40])
@pytest.mark.parametrize("layout", ["row", "col"])
def test_spmm_bit_exact_raw_abi(hp, orc, gpu_backend_i32, k, layout):
    import torch
    n, m = 3000, 2500
    rows = orc.sprand_rows(m, 0.01, 0, n)
    ci, cv = orc.compress_columns(rows)
    B = orc.fill_uniform(0, len(ci) * k, 9).reshape(len(ci), k)
    if layout == "col":
        B = np.asfortranarray(B)
    want = orc.spmm(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, B)
    lay = hp._capi.LAYOUT_ROW if layout == "row" else hp._capi.LAYOUT_COL
    ldb = k if layout == "row" else len(ci)
    ldc = k if layout == "row" else n
    dB = _t(B.ravel(order="C" if layout == "row" else "F"))
    dC = torch.full((n * k,), float("nan"), dtype=torch.float64, device="cuda")
    d_rp, d_cv, d_nz = _t(rows.rowptr.astype(np.int32)), _t(cv.astype(np.int32)), _t(rows.vals)  # keep alive
    hp._capi.call("hpcla_spmm_csr_f64_i32", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(),
                  dB.data_ptr(), ldb, lay, dC.data_ptr(), ldc, lay, n, rows.nnz, k, 0,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    C = dC.cpu().numpy().reshape((n, k), order="C" if layout == "row" else "F")
    np.testing.assert_array_equal(C, want)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 7, 9, 13, 15, 16, 17, 31, 33])
@pytest.mark.parametrize("c_layout", ["row", "col"])
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmm_bit_exact_padded_pitch(hp, orc, gpu_backend_i32, k, c_layout, Ti):
    """Round 6: ODD k on the 16-byte vector kernel.  Row-major B rows on the pitch the converters of this boundary allocate
    (k + (k & 1), and a wider even one), C row-major on the same pitch or column-major: lanes own column pairs, the last pair's
    second half is the row's padding double -- read (here: NaN, so a leak into any real column would show), never stored
    into a real column (the padding of C stays NaN, or becomes 0.0 where the rows leave as whole lines).  Unsplit entry and split entry with a ghost segment of its own pitch and block lists.
    Bar: the oracle's bits (the reference's column loop, src/sparse.jl:2391-2413)."""
    import torch
    sfx = "i32" if Ti == np.int32 else "i64"
    n, m = 3000, 2500
    rows = orc.sprand_rows(m, 0.01, 0, n)
    ci, cv = orc.compress_columns(rows)
    nc = len(ci)
    B = orc.fill_uniform(0, nc * k, 9).reshape(nc, k) - 0.5
    want = orc.spmm(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, B)
    d_rp, d_cv, d_nz = _t(rows.rowptr.astype(Ti)), _t(cv.astype(Ti)), _t(rows.vals)
    ROW, COL = hp._capi.LAYOUT_ROW, hp._capi.LAYOUT_COL
    s = torch.cuda.current_stream().cuda_stream
    kp = k + (k & 1)

    def padded(M, pitch):
        out = np.full((M.shape[0], pitch), np.nan)
        out[:, :k] = M
        return out
    for ldb in (kp, kp + 2):
        dB = _t(padded(B, ldb))
        if c_layout == "row":
            ldc = ldb
            dC = torch.full((n, ldc), float("nan"), dtype=torch.float64, device="cuda")
            hp._capi.call(f"hpcla_spmm_csr_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), dB.data_ptr(), ldb, ROW,
                          dC.data_ptr(), ldc, ROW, n, rows.nnz, k, 0, s)
            got = dC.cpu().numpy()
            np.testing.assert_array_equal(got[:, :k], want)
            # the padding of C: untouched, or -- ldc == k + 1 <= 16: the rows leave as whole lines -- column k set to 0.0
            assert np.all(np.isnan(got[:, k:]) | (got[:, k:] == 0.0)) and np.all(np.isnan(got[:, k + 1:])), "padding of C"
        else:
            ldc = n + 2
            dC = torch.full((k, ldc), float("nan"), dtype=torch.float64, device="cuda")
            hp._capi.call(f"hpcla_spmm_csr_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), dB.data_ptr(), ldb, ROW,
                          dC.data_ptr(), ldc, COL, n, rows.nnz, k, 0, s)
            got = dC.cpu().numpy()
            np.testing.assert_array_equal(got[:, :n].T, want)
            assert np.all(np.isnan(got[:, n:]))
    # split form: own rows on pitch kp, ghost rows on pitch kp + 2, interior / boundary block lists
    n_own = (2 * nc) // 3
    dBo, dBg = _t(padded(B[:n_own], kp)), _t(padded(B[n_own:], kp + 2))
    rpb = hp._capi.load().hpcla_spmm_rows_per_block()
    nblk = (n + rpb - 1) // rpb
    rp = rows.rowptr
    touches = np.array([np.any(cv[rp[b * rpb]:rp[min((b + 1) * rpb, n)]] >= n_own) for b in range(nblk)])
    lists = [_t(np.flatnonzero(~touches).astype(np.int32)), _t(np.flatnonzero(touches).astype(np.int32))]
    if c_layout == "row":
        dC = torch.full((n, kp), float("nan"), dtype=torch.float64, device="cuda")
        for blocks in lists:
            if blocks.numel():
                hp._capi.call(f"hpcla_spmm_split_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), dBo.data_ptr(), kp,
                              dBg.data_ptr(), kp + 2, n_own, dC.data_ptr(), kp, n, rows.nnz, k, 0, blocks.data_ptr(), blocks.numel(), s)
        got = dC.cpu().numpy()
        np.testing.assert_array_equal(got[:, :k], want)
        assert np.all(np.isnan(got[:, k:]) | (got[:, k:] == 0.0))
    else:
        ldc = n + 4
        dC = torch.full((k, ldc), float("nan"), dtype=torch.float64, device="cuda")
        for blocks in lists:
            if blocks.numel():
                hp._capi.call(f"hpcla_spmm_split_ccol_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), dBo.data_ptr(), kp,
                              dBg.data_ptr(), kp + 2, n_own, dC.data_ptr(), ldc, n, rows.nnz, k, 0, blocks.data_ptr(), blocks.numel(), s)
        got = dC.cpu().numpy()
        np.testing.assert_array_equal(got[:, :n].T, want)
        assert np.all(np.isnan(got[:, n:]))


@pytest.mark.parametrize("k", [3, 7, 15, 17])
def test_spmm_host_layer_odd_k_runs_on_the_padded_pitch(hp, orc, gpu_backend_i32, k):
    """Round 6, host layer: ``A @ B`` with an odd k allocates its result on the even pitch k + 1 (spmm_plans.spmm_pitch) and
    multiplies B on that pitch too -- one copy for a B that arrives on the pitch k, none for a B that is itself such a
    result (the chained product below).  Bits of the oracle's column loop (src/sparse.jl:2391-2413) both times."""
    import torch
    n = 5000
    rng = np.random.default_rng(60 + k)
    lens = rng.integers(0, 14, n)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ci = np.concatenate([np.sort(rng.choice(n, int(l), replace=False)) for l in lens]).astype(np.int64)
    va = rng.random(len(ci)) - 0.5
    A = hp.HPCSparseMatrix_local(rp, ci, va, n, gpu_backend_i32)
    Bg = rng.random((n, k)) - 0.5
    C = A @ hp.HPCMatrix.from_global(Bg, gpu_backend_i32)
    assert tuple(C.A.shape) == (n, k) and C.A.stride(0) == k + 1 and C.A.stride(1) == 1
    want = orc.spmm(rp.astype(np.int32), ci.astype(np.int32), va, Bg)
    np.testing.assert_array_equal(C.local_values(), want)
    D = A @ C                                                     # C's block is a (n, k) view on the pitch k + 1: taken as it is
    np.testing.assert_array_equal(D.local_values(), orc.spmm(rp.astype(np.int32), ci.astype(np.int32), va, want))
    np.testing.assert_array_equal(C.local_values(), want)         # (the product read C, nothing wrote it)
    np.testing.assert_array_equal((C * 2.0).local_values(), want * 2.0)       # the other operators take the view too
    np.testing.assert_array_equal(C[:, k - 1].local_values(), want[:, k - 1])
    del A, C, D
    hp.clear_plan_cache(); hp.clear_spmm_cache()


@pytest.mark.parametrize("k", [16, 12, 6, 3, 1])
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmm_panel_accumulate_is_one_running_sum(hp, orc, gpu_backend_i32, k, Ti):
    """hpcla_spmm_panel_* with accumulate = 1 CONTINUES every C(r, c) from its current value, entry by entry.  A product
    taken panel by panel (own columns, then two ghost panels) is therefore the reference's sum in a different ORDER, not a
    sum of separately rounded partials: it must equal, BIT FOR BIT, a CPU loop that adds each row's terms in panel order --
    and the sequential product only to 1e-12 (asserted with the componentwise |A||B| bound of SURVEY 8d)."""
    import torch
    n, m = 1500, 1300
    rows = orc.sprand_rows(m, 0.012, 0, n)
    ci, cv = orc.compress_columns(rows)
    nc = len(ci)
    B = orc.fill_uniform(0, nc * k, 21).reshape(nc, k) - 0.5
    rp = rows.rowptr.astype(np.int64)
    # three column panels: "own" columns [0, c1), ghost panel A [c1, c2), ghost panel B [c2, nc); each ghost panel's
    # columns are positions in ITS buffer
    c1, c2 = nc // 3, (2 * nc) // 3
    pid = np.where(cv < c1, 0, np.where(cv < c2, 1, 2))
    rowid = np.repeat(np.arange(n), np.diff(rp))
    want_order = np.zeros((n, k))
    panels = []
    for q, base in ((0, 0), (1, c1), (2, c2)):
        sel = np.flatnonzero(pid == q)
        prp = np.concatenate([[0], np.cumsum(np.bincount(rowid[sel], minlength=n))])
        panels.append((prp.astype(Ti), (cv[sel] - base).astype(Ti), rows.vals[sel]))
        for r in range(n):                                   # the CPU loop in panel order: one running sum per entry of C
            for j in range(prp[r], prp[r + 1]):
                want_order[r] += rows.vals[sel][j] * B[cv[sel][j]]
    sfx = "i32" if Ti == np.int32 else "i64"
    s = torch.cuda.current_stream().cuda_stream
    dB_own, dB_g1, dB_g2 = _t(B[:c1].ravel()), _t(B[c1:c2].ravel()), _t(B[c2:].ravel())
    dC = torch.full((n * k,), float("nan"), dtype=torch.float64, device="cuda")
    keep = []
    for q, (prp, pcv, pval) in enumerate(panels):
        d = (_t(prp), _t(pcv), _t(pval))
        keep.append(d)
        n_own = c1 if q == 0 else 0                          # ghost panels: every column is a ghost position
        ghost = None if q == 0 else (dB_g1 if q == 1 else dB_g2).data_ptr()
        hp._capi.call(f"hpcla_spmm_panel_f64_{sfx}", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), dB_own.data_ptr(), k,
                      ghost, k, n_own, dC.data_ptr(), k, n, len(pval), k, 0, 0 if q == 0 else 1, s)
    torch.cuda.synchronize()
    C = dC.cpu().numpy().reshape(n, k)
    np.testing.assert_array_equal(C, want_order)             # one running sum in panel order: exact
    seq = orc.spmm(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, B)
    bound = orc.spmm(rows.rowptr.astype(np.int32), cv.astype(np.int32), np.abs(rows.vals), np.abs(B))
    assert np.all(np.abs(C - seq) <= 1e-12 * bound)
    assert np.linalg.norm(C - seq) <= 1e-12 * np.linalg.norm(seq)


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmm_block_order_is_a_bijection_with_the_same_bits(hp, orc, gpu_backend_i32, Ti):
    """hpcla_spmm_block_order_hint / hpcla_spmm_tune_block_order_*: XCD-grouped order of the 64-row blocks of an SpMM
    launch -- of a contiguous launch AND of the positions of a block list.  Every group size visits every block exactly
    once (ragged tail included), each C(r, c) is still one sequential sum: the reference's bits (src/sparse.jl:2391-2413)."""
    import ctypes
    import torch
    n, k = 64 * 301 + 17, 16
    rows = orc.sprand_rows(n, 6.0 / n, 0, n)
    ci, cv = orc.compress_columns(rows)
    B = orc.fill_uniform(0, n * k, 11).reshape(n, k)
    want = orc.spmm(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, np.ascontiguousarray(B[ci]))
    sfx = "i32" if Ti == np.int32 else "i64"
    s = torch.cuda.current_stream().cuda_stream
    rp, dcv, nz, dB = _t(rows.rowptr.astype(Ti)), _t(cv.astype(Ti)), _t(rows.vals), _t(np.ascontiguousarray(B[ci]).ravel())
    nblk = (n + 63) // 64
    perm = np.random.default_rng(2).permutation(nblk).astype(np.int32)          # an arbitrary block list
    lists = [None, _t(np.arange(nblk, dtype=np.int32)), _t(perm)]
    lib = hp._capi.load()
    try:
        for G in (0, 2, 16, 64, 256, 4096):
            hp._capi.call("hpcla_spmm_block_order_hint", rp.data_ptr(), G)
            for lst in lists:
                C = torch.full((n * k,), float("nan"), dtype=torch.float64, device="cuda")
                hp._capi.call(f"hpcla_spmm_split_f64_{sfx}", rp.data_ptr(), dcv.data_ptr(), nz.data_ptr(), dB.data_ptr(), k,
                              None, k, len(ci), C.data_ptr(), k, n, rows.nnz, k, 0,
                              lst.data_ptr() if lst is not None else None, nblk if lst is not None else 0, s)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(C.cpu().numpy().reshape(n, k), want)
        for bad in (3, -1, 8192):
            assert lib.hpcla_spmm_block_order_hint(ctypes.c_void_p(rp.data_ptr()), bad) != 0
        assert lib.hpcla_spmm_block_order_hint(None, 4) != 0
        # the tuner: below 4096 blocks it keeps the natural order unmeasured; odd k and k = 1 likewise
        chosen = ctypes.c_int(-1)
        C = torch.empty(n * k, dtype=torch.float64, device="cuda")
        hp._capi.call(f"hpcla_spmm_tune_block_order_f64_{sfx}", rp.data_ptr(), dcv.data_ptr(), nz.data_ptr(), dB.data_ptr(), k,
                      None, k, len(ci), C.data_ptr(), k, n, rows.nnz, k, 0, None, 0, s, ctypes.byref(chosen))
        assert chosen.value == 1
    finally:
        lib.hpcla_spmm_block_order_hint(ctypes.c_void_p(rp.data_ptr()), 0)


def test_spmm_plan_measures_block_order(hp, orc, gpu_backend_i32, gpu_backend_i64):
    """A structure large enough to be measured (>= 4096 blocks of 64 rows): the first product leaves a measured group
    from {1, 16, 64, 256} on the plan, every later product runs under it, and the bits stay the oracle's -- Int32 and a
    narrowed Int64 matrix alike."""
    import torch
    N = 640                                        # 409 600 rows = 6400 blocks
    rows = orc.poisson2d_rows(N, N, 0, N * N)
    k = 4
    Bg = orc.fill_uniform(0, N * N * k, 5).reshape(N * N, k)
    want = orc.spmm(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, Bg)
    for backend in (gpu_backend_i32, gpu_backend_i64):
        A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N * N, backend)
        B = hp.HPCMatrix.from_global(Bg, backend)
        assert hp.spmm_block_order_of(A, B) == 0
        C1 = (A @ B).local_values()
        g = hp.spmm_block_order_of(A, B)
        assert g in (1, 16, 64, 256), g
        C2 = (A @ B).local_values()
        np.testing.assert_array_equal(C1, want)
        np.testing.assert_array_equal(C2, want)
    hp.clear_spmm_cache()
    hp.clear_plan_cache()


def test_spmm_block_order_is_kept_per_k_on_one_structure(hp, orc, gpu_backend_i32, monkeypatch):
    """the library holds ONE SpMM order hint per rowptr array, the host layer measures one per (k, rowptr) -- a
    later k's measurement used to overwrite the order earlier k's launches ran under.  Orders forced through
    HPCLA_SPMM_BLOCK_ORDER (64 for k = 4, 16 for k = 6): every product puts its own k's order back in force first
    (bookkeeping checked on the plan), and the bits never depend on it."""
    from hpcla_amd.sparse import get_vector_plan
    N = 640
    rows = orc.poisson2d_rows(N, N, 0, N * N)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N * N, gpu_backend_i32)
    prod = {}
    for k, group in ((4, "64"), (6, "16")):
        Bg = orc.fill_uniform(0, N * N * k, 5 + k).reshape(N * N, k)
        prod[k] = (hp.HPCMatrix.from_global(Bg, gpu_backend_i32),
                   orc.spmm(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, Bg))
        monkeypatch.setenv("HPCLA_SPMM_BLOCK_ORDER", group)
        np.testing.assert_array_equal((A @ prod[k][0]).local_values(), prod[k][1])
        assert hp.spmm_block_order_of(A, prod[k][0]) == int(group)
    monkeypatch.delenv("HPCLA_SPMM_BLOCK_ORDER")
    plan = get_vector_plan(A, hp.HPCVector.from_global(np.zeros(N * N), gpu_backend_i32))
    ptr = plan.rowptr_of(A).data_ptr()
    assert plan._spmm_order_in_force[ptr] == 16                       # k = 6 was tuned last
    for k, group in ((4, 64), (6, 16), (6, 16), (4, 64)):
        np.testing.assert_array_equal((A @ prod[k][0]).local_values(), prod[k][1])
        assert plan._spmm_order_in_force[ptr] == group, (k, plan._spmm_order_in_force)
    hp.clear_spmm_cache()
    hp.clear_plan_cache()


def test_transpose_layout_conversion(hp, gpu_backend_i32):
    import torch
    # (the narrow column-major -> row-major kernel takes rows >= 256, cols <= 32; its LDS tile is sized from cols -- 31 / 32
    #  Float64 columns need more than 64 KiB of dynamic LDS)
    for rows, cols in ((1, 1), (33, 16), (1000, 16), (65, 70), (2000, 32), (777, 31), (300, 5), (256, 1), (513, 17)):
        M = np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) * 0.5
        src = _t(np.asfortranarray(M).ravel(order="F"))
        dst = torch.empty(rows * cols, dtype=torch.float64, device="cuda")
        hp._capi.call("hpcla_transpose_f64", src.data_ptr(), rows, hp._capi.LAYOUT_COL, dst.data_ptr(), cols,
                      hp._capi.LAYOUT_ROW, rows, cols, torch.cuda.current_stream().cuda_stream)
        np.testing.assert_array_equal(dst.cpu().numpy().reshape(rows, cols), M)
        back = torch.empty_like(dst)
        hp._capi.call("hpcla_transpose_f64", dst.data_ptr(), cols, hp._capi.LAYOUT_ROW, back.data_ptr(), rows,
                      hp._capi.LAYOUT_COL, rows, cols, torch.cuda.current_stream().cuda_stream)
        np.testing.assert_array_equal(back.cpu().numpy(), np.asfortranarray(M).ravel(order="F"))


# ---------------------------------------------------------------------------------------------------
# CG (config 4 building blocks)
# ---------------------------------------------------------------------------------------------------
def test_cg_matches_oracle(hp, orc, gpu_backend_i32):
    N = 24
    rows = orc.poisson3d_rows(N, N, N, 0, N ** 3)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N ** 3, gpu_backend_i32)
    bg = orc.fill_uniform(0, N ** 3, orc.SEED_RHS)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    x, hist = hp.cg_fixed_iterations(A, b, 40)
    xr, hist_ref = orc.cg(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, bg, 40)
    # dot products differ in summation order (tree on the GPU, sequential in the oracle: ~1e-16 relative per dot);
    # the recurrence feeds alpha / beta back into every later iterate, so the two histories drift apart as CG
    # converges (here the residual falls by > 100x in 40 iterations).  The deviation actually met is printed and
    # recorded in DESIGN.md section 5; CG_RTOL is that measurement with one order of magnitude of margin.
    hist, hist_ref = np.asarray(hist), np.asarray(hist_ref)
    dev_hist = float(np.max(np.abs(hist - hist_ref) / hist_ref))
    dev_x = float(np.max(np.abs(x.local_values() - xr)) / np.abs(xr).max())
    print(f"CG 40 iterations, 24^3: max relative residual-history deviation {dev_hist:.2e}, x deviation {dev_x:.2e}")
    assert dev_hist <= CG_RTOL and dev_x <= CG_RTOL, (dev_hist, dev_x)
    assert hist[-1] < 1e-2 * hist[0]


def test_error_convention(hp, gpu_backend_i32):
    import torch
    with pytest.raises(hp._capi.HPCLAError) as ei:
        hp._capi.call("hpcla_spmv_csr_f64_i32", None, None, None, None, None, 10, 5, 0, None)
    assert ei.value.status == -1 and "null" in str(ei.value)
    y = hp.HPCVector.from_global(np.ones(7), gpu_backend_i32)
    import scipy.sparse as sp
    A = hp.HPCSparseMatrix_from_global(sp.identity(8, format="csr"), gpu_backend_i32)
    with pytest.raises(ValueError):
        hp.mul_(y, A, hp.HPCVector.from_global(np.ones(8), gpu_backend_i32))


# ---------------------------------------------------------------------------------------------------
# more coverage: unaligned fallback kernel, distributed SpMM semantics, Int64 at moderate scale
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_unaligned_pointers_take_fallback_kernel(hp, orc, gpu_backend_i32, Ti):
    """colval/nzval views offset by one element are not 16/32-byte aligned: the element-per-lane
    kernel must be selected and give the same bits."""
    import torch
    n = 5000
    rows = orc.sprand_rows(n, 0.004, 0, n)
    x = orc.fill_uniform(0, n, orc.SEED_X)
    want = orc.spmv(rows.rowptr.astype(Ti), rows.colidx.astype(Ti), rows.vals, x)
    sfx = "i32" if Ti == np.int32 else "i64"
    d_rp = _t(rows.rowptr.astype(Ti))
    d_cv_pad = _t(np.concatenate([[0], rows.colidx]).astype(Ti))
    d_nz_pad = _t(np.concatenate([[0.0], rows.vals]))
    d_cv, d_nz = d_cv_pad[1:], d_nz_pad[1:]
    assert d_nz.data_ptr() % 32 != 0
    d_x = _t(x)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    hp._capi.call(f"hpcla_spmv_csr_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), d_x.data_ptr(),
                  y.data_ptr(), n, rows.nnz, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy(), want)


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
@pytest.mark.parametrize("nranks,k", [(2, 16), (3, 5), (2, 8), (3, 4), (2, 12), (2, 1), (2, 6), (3, 2), (2, 10)])
def test_split_spmm_per_rank_matches_reference_pipeline(hp, orc, gpu_backend_i32, nranks, k, Ti):
    """hpcla_spmm_split_f64_{i32,i64} (Int64 is the reference's default Ti, src/backends.jl:348) (own rows of B + ghost rows, interior/boundary block lists at SpMM
    granularity) == the reference's column loop over gathered B, for every simulated rank."""
    import torch
    sfx = "i32" if Ti == np.int32 else "i64"
    n = 4000
    rp = orc.uniform_partition(n, nranks)
    Bg = orc.fill_uniform(0, n * k, 21).reshape(n, k)
    locs = [orc.sprand_rows(n, 0.003, int(rp[r]), int(rp[r + 1])) for r in range(nranks)]
    comp = [orc.compress_columns(l) for l in locs]
    plans = orc.vector_plans([c[0] for c in comp], rp)
    rpb = hp._capi.load().hpcla_spmm_rows_per_block()
    s = torch.cuda.current_stream().cuda_stream
    for r in range(nranks):
        rows, (ci, cv), pl = locs[r], comp[r], plans[r]
        want = orc.spmm(rows.rowptr.astype(Ti), cv.astype(Ti), rows.vals, Bg[ci])
        n_own = int(rp[r + 1] - rp[r])
        hplan = hp.HostVectorPlan(pl.send_rank_ids, pl.send_indices, pl.recv_rank_ids, pl.recv_perm,
                                  pl.local_src_indices, pl.local_dst_indices, pl.n_gathered, n_own)
        cmap = hp.split_column_map(hplan)
        ghost_rows = np.concatenate([ci[p] for p in pl.recv_perm]) if pl.recv_perm else np.zeros(0, dtype=np.int64)
        d_rp, d_split = _t(rows.rowptr.astype(Ti)), _t(cmap[cv].astype(Ti))
        d_nz = _t(rows.vals)
        d_B, d_G = _t(Bg[rp[r]:rp[r + 1]]), _t(Bg[ghost_rows] if len(ghost_rows) else np.zeros((1, k)))
        nblk = (rows.nrows + rpb - 1) // rpb
        flags = torch.empty(nblk, dtype=torch.int32, device="cuda")
        hp._capi.call(f"hpcla_classify_blocks_{sfx}", d_rp.data_ptr(), d_split.data_ptr(), rows.nrows, 0, n_own, rpb,
                      flags.data_ptr(), s)
        f = flags.cpu().numpy()
        C = torch.full((rows.nrows, k), float("nan"), dtype=torch.float64, device="cuda")
        for sel in (np.flatnonzero(f == 0), np.flatnonzero(f != 0)):
            lst = _t(sel.astype(np.int32))
            if lst.numel() == 0:
                continue
            hp._capi.call(f"hpcla_spmm_split_f64_{sfx}", d_rp.data_ptr(), d_split.data_ptr(), d_nz.data_ptr(),
                          d_B.data_ptr(), k, d_G.data_ptr(), k, n_own, C.data_ptr(), k, rows.nrows, rows.nnz, k, 0,
                          lst.data_ptr(), lst.numel(), s)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(C.cpu().numpy(), want)


@pytest.mark.parametrize("narrow", [True, False])
def test_spmv_int64_moderate_scale(hp, orc, gpu_backend_i64, narrow, monkeypatch):
    """Int64 matrix (the reference's default Ti = Int, src/backends.jl:348,369).  narrow: the plan keeps Int32 copies of
    rowptr / split colval and launches the Int32 kernels (the matrix keeps its Int64 arrays); HPCLA_NARROW_INDICES=0:
    the Int64 kernels.  Indices are not results: the same bits either way."""
    import torch
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "1" if narrow else "0")
    N = 1500
    rows = orc.poisson2d_rows(N, N, 0, N * N)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N * N, gpu_backend_i64)
    assert A.rowptr.dtype == np.int64 and A.colval.dtype == np.int64
    xg = orc.fill_uniform(0, N * N, orc.SEED_X)
    x = hp.HPCVector.from_global(xg, gpu_backend_i64)
    y = (A @ x).local_values()
    want = orc.spmv(rows.rowptr, rows.colidx, rows.vals, xg)
    np.testing.assert_array_equal(y, want)
    plan = hp.get_vector_plan(A, x)
    assert plan.narrowed == narrow and plan.is_i64 == (not narrow)
    assert plan.colval_split.dtype == (torch.int32 if narrow else torch.int64)
    assert plan.rowptr_of(A).dtype == (torch.int32 if narrow else torch.int64)
    assert A.rowptr_target.dtype == torch.int64 and A.colval_target().dtype == torch.int64      # the matrix keeps its type
    if narrow:
        np.testing.assert_array_equal(plan.rowptr_of(A).cpu().numpy(), rows.rowptr)
    # a second matrix of the same structure shares the plan (and its Int32 rowptr copy), other values
    A2 = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, 2.0 * rows.vals, N * N, gpu_backend_i64)
    assert hp.get_vector_plan(A2, x) is plan
    np.testing.assert_array_equal((A2 @ x).local_values(), orc.spmv(rows.rowptr, rows.colidx, 2.0 * rows.vals, xg))
    # fused p.Ap and SpMM go through the same narrowed arrays
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    yy = x.similar()
    hp.mul_dot_(yy, A, x, out)
    np.testing.assert_array_equal(yy.local_values(), want)
    Bg = np.stack([xg, 0.5 - xg, xg * xg, 1.0 + xg], axis=1)
    C = A @ hp.HPCMatrix.from_global(Bg, gpu_backend_i64)
    Cw = orc.spmm(rows.rowptr, rows.colidx, rows.vals, np.ascontiguousarray(Bg))
    np.testing.assert_array_equal(C.local_values(), Cw)


def test_narrowing_entries_raw_abi(hp, gpu_backend_i32):
    """hpcla_remap_i64_to_i32 / hpcla_narrow_i64_to_i32: values, index_base, and the overflow word."""
    import ctypes
    import torch
    rng = np.random.default_rng(5)
    n, m = 100003, 777
    for base in (0, 1):
        cv = rng.integers(0, m, n).astype(np.int64) + base
        cmap = (rng.permutation(m).astype(np.int32) + base)
        d_in, d_map = torch.from_numpy(cv).cuda(), torch.from_numpy(cmap).cuda()
        d_out = torch.empty(n, dtype=torch.int32, device="cuda")
        hp._capi.call("hpcla_remap_i64_to_i32", d_in.data_ptr(), d_map.data_ptr(), d_out.data_ptr(), n, base, None)
        np.testing.assert_array_equal(d_out.cpu().numpy(), cmap[cv - base])
    src = torch.from_numpy(np.array([0, 5, 2**31 - 1, 17], dtype=np.int64)).cuda()
    dst = torch.empty(4, dtype=torch.int32, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    hp._capi.call("hpcla_narrow_i64_to_i32", src.data_ptr(), dst.data_ptr(), 4, ovf.data_ptr(), None)
    assert dst.cpu().tolist() == [0, 5, 2**31 - 1, 17] and int(ovf.item()) == 0
    src[1] = 2**31
    hp._capi.call("hpcla_narrow_i64_to_i32", src.data_ptr(), dst.data_ptr(), 4, ovf.data_ptr(), None)
    assert int(ovf.item()) == 1
    lib = hp._capi.load()
    assert lib.hpcla_remap_i64_to_i32(None, None, None, 5, 0, None) != 0
    assert lib.hpcla_remap_i64_to_i32(src.data_ptr(), dst.data_ptr(), dst.data_ptr(), 4, 2, None) != 0
    assert lib.hpcla_narrow_i64_to_i32(None, None, -1, None, None) != 0


def test_fused_spmv_dot_and_cg_update(hp, orc, gpu_backend_i32):
    """mul_dot_ (SpMV with the x.y partials in its epilogue) and cg_update_ vs the oracle."""
    import torch
    b = gpu_backend_i32
    for N in (37, 64, 200):
        rows = orc.poisson3d_rows(N, N, 3, 0, N * N * 3)
        n = rows.nrows
        A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, b)
        xg = orc.fill_uniform(0, n, 5) - 0.5
        x = hp.HPCVector.from_global(xg, b)
        y = hp.HPCVector.zeros(A.row_partition, b)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        hp.mul_dot_(y, A, x, out)
        want_y = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, xg)
        np.testing.assert_array_equal(y.local_values(), want_y)          # y still bit-exact
        want_d = orc.dot([xg], [want_y])
        assert abs(out.item() - want_d) <= RTOL_RED * float(np.abs(xg) @ np.abs(want_y))
        out2 = torch.zeros(1, dtype=torch.float64, device="cuda")
        hp.mul_dot_(y, A, x, out2)
        assert out.item() == out2.item()                                  # deterministic
        # cg_update_: x += s p ; r -= s Ap ; rr = sum r^2 with s = a*num/den from device scalars
        pg, apg = orc.fill_uniform(0, n, 6), orc.fill_uniform(0, n, 7)
        xx, rrv = orc.fill_uniform(0, n, 8), orc.fill_uniform(0, n, 9)
        num = torch.tensor([0.75], dtype=torch.float64, device="cuda")
        den = torch.tensor([1.5], dtype=torch.float64, device="cuda")
        s = 1.0 * 0.75 / 1.5
        X, R = hp.HPCVector.from_global(xx, b), hp.HPCVector.from_global(rrv, b)
        P, AP = hp.HPCVector.from_global(pg, b), hp.HPCVector.from_global(apg, b)
        rr = torch.zeros(1, dtype=torch.float64, device="cuda")
        hp.cg_update_(X, R, P, AP, 1.0, num, den, rr)
        wx = xx.copy(); orc.axpy(s, pg, wx)
        wr = rrv.copy(); orc.axpy(-s, apg, wr)
        np.testing.assert_array_equal(X.local_values(), wx)
        np.testing.assert_array_equal(R.local_values(), wr)
        assert abs(rr.item() - orc.dot([wr], [wr])) <= RTOL_RED * orc.dot([wr], [wr])
        # the deferred-x form: cg_residual_ (r -= s Ap ; rr) then cg_direction_ (x += s p ; p = r + t p) -- the
        # same per-element operations, so x / r / p must carry the same bits as the three separate updates
        X2, R2 = hp.HPCVector.from_global(xx, b), hp.HPCVector.from_global(rrv, b)
        P2 = hp.HPCVector.from_global(pg, b)
        rr2 = torch.zeros(1, dtype=torch.float64, device="cuda")
        hp.cg_residual_(R2, AP, 1.0, num, den, rr2)
        np.testing.assert_array_equal(R2.local_values(), wr)
        assert rr2.item() == rr.item()                                    # same reduction tree as cg_update_
        bnum = torch.tensor([0.3], dtype=torch.float64, device="cuda")
        bden = torch.tensor([0.7], dtype=torch.float64, device="cuda")
        hp.cg_direction_(X2, P2, R2, 1.0, num, den, 1.0, bnum, bden)
        np.testing.assert_array_equal(X2.local_values(), wx)
        wp = pg.copy(); orc.xpay(wr, 1.0 * 0.3 / 0.7, wp)                 # p = r + t p
        np.testing.assert_array_equal(P2.local_values(), wp)


@pytest.mark.parametrize("n", gr.CG_TRIO_ALONE)
def test_cg_update_trio_on_vectors_alone(hp, orc, gpu_backend_i32, n):
    """The cg_update_ / cg_residual_ / cg_direction_ block of test_fused_spmv_dot_and_cg_update without a matrix, at sizes that
    test's matrices do not reach (its largest has 120 000 rows: 59 partials, 235 elementwise workgroups).  1 is the scalar tail
    alone, 511 one workgroup of either grid with a tail, 2051 two partials and five elementwise workgroups, 614 403 gives 301
    partials (a ragged second trip of the second stage) and 1201 elementwise workgroups, 4 194 307 caps both grids (2048
    partials in five grid-stride trips, 4096 elementwise workgroups in three); all odd.  Elements: the bits of the oracle's
    axpy / xpay; the sum: the project's margin for its reductions, relative to the sum of the (positive) terms."""
    import torch
    b = gpu_backend_i32
    pg, apg = orc.fill_uniform(0, n, 6), orc.fill_uniform(0, n, 7)
    xx, rrv = orc.fill_uniform(0, n, 8), orc.fill_uniform(0, n, 9)
    dev = lambda v: torch.tensor([v], dtype=torch.float64, device="cuda")
    num, den, bnum, bden = dev(0.75), dev(1.5), dev(0.3), dev(0.7)
    s = 1.0 * 0.75 / 1.5
    X, R = hp.HPCVector.from_global(xx, b), hp.HPCVector.from_global(rrv, b)
    P, AP = hp.HPCVector.from_global(pg, b), hp.HPCVector.from_global(apg, b)
    rr = torch.zeros(1, dtype=torch.float64, device="cuda")
    hp.cg_update_(X, R, P, AP, 1.0, num, den, rr)
    wx = xx.copy(); orc.axpy(s, pg, wx)
    wr = rrv.copy(); orc.axpy(-s, apg, wr)
    np.testing.assert_array_equal(X.local_values(), wx)
    np.testing.assert_array_equal(R.local_values(), wr)
    want = math.fsum((wr * wr).tolist())
    err = abs(rr.item() - want) / want
    print(f"n = {n}: sum r^2 off by {err:.2e} of the sum of the terms")
    assert err <= RTOL_RED
    X2, R2, P2 = hp.HPCVector.from_global(xx, b), hp.HPCVector.from_global(rrv, b), hp.HPCVector.from_global(pg, b)
    rr2 = torch.zeros(1, dtype=torch.float64, device="cuda")
    hp.cg_residual_(R2, AP, 1.0, num, den, rr2)
    np.testing.assert_array_equal(R2.local_values(), wr)
    assert rr2.item() == rr.item()                                    # same reduction tree as cg_update_
    hp.cg_direction_(X2, P2, R2, 1.0, num, den, 1.0, bnum, bden)
    np.testing.assert_array_equal(X2.local_values(), wx)
    wp = pg.copy(); orc.xpay(wr, 1.0 * 0.3 / 0.7, wp)                 # p = r + t p
    np.testing.assert_array_equal(P2.local_values(), wp)


def test_cg_fused_equals_unfused(hp, orc, gpu_backend_i32):
    N = 20
    rows = orc.poisson3d_rows(N, N, N, 0, N ** 3)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N ** 3, gpu_backend_i32)
    b = hp.HPCVector.from_global(orc.fill_uniform(0, N ** 3, orc.SEED_RHS), gpu_backend_i32)
    x1, h1 = hp.cg_fixed_iterations(A, b, 30, fused=True)
    x2, h2 = hp.cg_fixed_iterations(A, b, 30, fused=False)
    h1, h2 = np.asarray(h1), np.asarray(h2)
    dev = float(np.max(np.abs(h1 - h2) / h2))
    dev_x = float(np.max(np.abs(x1.local_values() - x2.local_values())) / np.abs(x2.local_values()).max())
    print(f"CG fused vs unfused, 30 iterations, 20^3: history deviation {dev:.2e}, x deviation {dev_x:.2e}")
    assert dev <= CG_RTOL and dev_x <= CG_RTOL, (dev, dev_x)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("iters", [4, 11])
def test_cg_graph_replay_is_bit_identical_to_eager(hp, orc, gpu_backend_i32, fused, iters):
    """graph=True replays a captured pair of iterations (HIP graph): same kernels and arguments as the
    eager loop, so iterate and residual history must agree bit for bit (odd counts finish eagerly)."""
    N = 16
    rows = orc.poisson3d_rows(N, N, N, 0, N ** 3)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N ** 3, gpu_backend_i32)
    b = hp.HPCVector.from_global(orc.fill_uniform(0, N ** 3, orc.SEED_RHS), gpu_backend_i32)
    x1, h1 = hp.cg_fixed_iterations(A, b, iters, fused=fused, graph=False)
    x2, h2 = hp.cg_fixed_iterations(A, b, iters, fused=fused, graph=True)
    assert h1 == h2 and len(h2) == iters + 1
    np.testing.assert_array_equal(x1.local_values(), x2.local_values())


@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_cg_native_loop_same_bits_as_one_call_per_kernel(hp, orc, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    """hpcla_cg_iterations_f64_* enqueues k iterations in ONE host call (no Python / Julia in the loop): per
    iteration the launches of hpcla_spmv_dist_dot, hpcla_cg_residual and hpcla_cg_direction with the same
    arguments -- so iterate and residual history equal the three-calls-per-iteration loop bit for bit; a reused
    workspace and a solve continued in two pieces (7 + 6 iterations) change nothing either."""
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    N = 18
    rows = orc.poisson3d_rows(N, N, N, 0, N ** 3)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N ** 3, backend)
    b = hp.HPCVector.from_global(orc.fill_uniform(0, N ** 3, orc.SEED_RHS), backend)
    x_py, h_py = hp.cg_fixed_iterations(A, b, 13, native_loop=False)
    x_py = x_py.local_values()
    ws = hp.CGWorkspace(b, 20)
    for _ in range(2):                                   # second pass: the workspace is dirty from the first
        x_nat, h_nat = hp.cg_fixed_iterations(A, b, 13, workspace=ws)
        assert x_nat is ws.x and h_nat == h_py
        np.testing.assert_array_equal(x_nat.local_values(), x_py)
    plan, fused = hp.cg_setup(A, b, ws)
    assert fused
    hp.cg_iterate(A, ws, plan, fused, 7)
    hp.cg_iterate(A, ws, plan, fused, 6)
    assert ws.done == 13
    assert ws.hist[:14].sqrt().cpu().tolist() == h_py
    np.testing.assert_array_equal(ws.x.local_values(), x_py)
    with pytest.raises(ValueError):
        hp.cg_iterate(A, ws, plan, fused, 8)             # history array too short: refused, nothing enqueued
    # the oracle's restatement, at the tolerance the recurrence allows
    _, h_ref = orc.cg(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals,
                      orc.fill_uniform(0, N ** 3, orc.SEED_RHS), 13)
    assert np.allclose(h_nat, h_ref, rtol=CG_RTOL, atol=0)


def test_cg_iterations_entry_rejects_bad_arguments(hp, gpu_backend_i32):
    import torch
    z = torch.zeros(8, dtype=torch.float64, device="cuda")
    with pytest.raises(hp._capi.HPCLAError) as ei:
        hp._capi.call("hpcla_cg_iterations_f64_i32", None, None, None, None, None, 4, 0, 0, None, 0, None, 0,
                      z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, None, None, 3, None)
    assert ei.value.status == -1 and "null" in str(ei.value)
    with pytest.raises(hp._capi.HPCLAError):
        hp._capi.call("hpcla_cg_iterations_f64_i32", None, None, None, None, None, 4, 0, 0, None, 0, None, 0,
                      z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                      z.data_ptr(), -1, None)


def test_transpose_times_vector(hp, orc, gpu_backend_i32):
    """transpose(A) * x (test/test_new_operations.jl:73-76; src/sparse.jl:2375-2379): materialised,
    cached bidirectionally, result bit-identical to the row-sequential product with the explicit A^T."""
    import scipy.sparse as sp
    m, n = 700, 450
    rows = orc.sprand_rows(n, 0.02, 0, m)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, gpu_backend_i32)
    xg = orc.fill_uniform(0, m, 12)
    x = hp.HPCVector.from_global(xg, gpu_backend_i32)
    At = hp.transpose(A)
    assert At.shape == (n, m)
    y = (At @ x).local_values()
    AT = sp.csr_matrix((rows.vals, rows.colidx, rows.rowptr), shape=(m, n)).T.tocsr()
    AT.sort_indices()
    want = orc.spmv(AT.indptr.astype(np.int32), AT.indices.astype(np.int32), AT.data, xg)
    np.testing.assert_array_equal(y, want)
    Y = At.materialize()
    assert Y is A.cached_transpose and Y.cached_transpose is A and A.transpose().materialize() is Y
    np.testing.assert_array_equal(Y.row_partition, A.col_partition)
    # golden: S + S' + 2I is symmetric -> transpose(A)*x == A*x (test/test_new_operations.jl:43-50)
    # and (A^T)^T == A structurally
    Z = hp.TransposedHPCSparseMatrix(Y)
    Z.parent.cached_transpose = None
    back = Z.materialize()
    np.testing.assert_array_equal(back.rowptr, A.rowptr)
    np.testing.assert_array_equal(back.col_indices[back.colval], A.col_indices[A.colval])
    np.testing.assert_array_equal(back.nzval.cpu().numpy(), A.nzval.cpu().numpy())


def test_packed_csr_opt_in_bit_exact(hp, orc, gpu_backend_i32):
    """Opt-in packed copy (16-bit block-relative columns + 8-bit value codes): same bits as CSR."""
    import torch
    b = gpu_backend_i32
    for gen, n in ((lambda: orc.poisson2d_rows(700, 300, 0, 700 * 300), 700 * 300),
                   (lambda: orc.poisson3d_rows(20, 20, 50, 0, 20000), 20000)):
        rows = gen()
        A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, b)
        xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.3
        x = hp.HPCVector.from_global(xg, b)
        want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, xg)
        plan = hp.get_vector_plan(A, x)
        y_csr = (A @ x).local_values()
        assert A.enable_packed(x) is True
        y_pk = (A @ x).local_values()
        np.testing.assert_array_equal(y_csr, want)
        np.testing.assert_array_equal(y_pk, want)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        y = hp.HPCVector.zeros(A.row_partition, b)
        hp.mul_dot_(y, A, x, out)                                     # packed + fused dot epilogue
        np.testing.assert_array_equal(y.local_values(), want)
        assert abs(out.item() - orc.dot([xg], [want])) <= RTOL_RED * float(np.abs(xg) @ np.abs(want))
        nbytes, nd = ctypes.c_int64(), ctypes.c_int()
        hp._capi.call("hpcla_packed_info", A._packed[plan.key], ctypes.byref(nbytes), ctypes.byref(nd))
        assert nd.value == 2 and nbytes.value < 4 * rows.nnz
        A.disable_packed()
        np.testing.assert_array_equal((A @ x).local_values(), want)


def test_packed_csr_eligibility(hp, orc, gpu_backend_i32):
    import scipy.sparse as sp
    b = gpu_backend_i32
    # (1) > 256 distinct values -> not packable, CSR stays
    rows = orc.sprand_rows(3000, 0.01, 0, 3000)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, 3000, b)
    x = hp.HPCVector.from_global(np.ones(3000), b)
    assert A.enable_packed(x) is False and "distinct" in A.packed_reason
    # (2) columns outside the 16-bit window
    n = 100_000
    M = (sp.identity(n, format="csr") + sp.diags([np.ones(n - 40000)], [40000], format="csr")).tocsr()
    A2 = hp.HPCSparseMatrix_from_global(M, b)
    x2 = hp.HPCVector.from_global(np.arange(n, dtype=np.float64), b)
    assert A2.enable_packed(x2) is False and "window" in A2.packed_reason
    # (3) dictionary values that the 65 536-entry seed sample does not contain -> iterative extension;
    #     exactly 256 distinct values is still packable, 257 is not
    for ndist, ok in ((256, True), (257, False)):
        n3 = 40_000
        vals = np.ones(5 * n3)
        vals[-ndist + 1:] = 2.0 + np.arange(ndist - 1)              # late, outside the seed sample
        rowptr = np.arange(0, 5 * n3 + 1, 5)
        cols_b = np.minimum(np.repeat(np.arange(n3), 5) + np.tile(np.arange(5), n3), n3 - 1)   # banded
        A4 = hp.HPCSparseMatrix_local(rowptr, cols_b, vals, n3, b)
        x3g = orc.fill_uniform(0, n3, 4)
        x3 = hp.HPCVector.from_global(x3g, b)
        # A4 shares its structure -- and therefore its cached VectorPlan -- with the previous
        # iteration's matrix; the packed copy depends on the VALUES and must not be shared
        if not ok:
            assert A4.enable_packed(x3) is False and "distinct" in A4.packed_reason
            np.testing.assert_array_equal((A4 @ x3).local_values(),
                                          orc.spmv(rowptr.astype(np.int32), A4.colval, vals, x3g[A4.col_indices]))
            continue
        assert A4.enable_packed(x3) is True
        want = orc.spmv(rowptr.astype(np.int32), A4.colval, vals, x3g[A4.col_indices])
        np.testing.assert_array_equal((A4 @ x3).local_values(), want)
    hp.clear_plan_cache()


def test_spmv_randomised_structures(hp, orc, gpu_backend_i32):
    """Property test: arbitrary ragged CSR structures (empty rows, rows far longer than the LDS chunk,
    duplicate columns, nrows around the 256-row block size, both index types and bases) give the
    oracle's bits."""
    rng = np.random.default_rng(2024)
    for trial in range(40):
        nrows = int(rng.choice([1, 2, 63, 255, 256, 257, 511, 513, 1000, 3001]))
        ncols = int(rng.integers(1, 5000))
        kind = trial % 4
        if kind == 0:
            lens = rng.integers(0, 12, size=nrows)
        elif kind == 1:
            lens = rng.geometric(0.05, size=nrows) - 1
        elif kind == 2:
            lens = np.zeros(nrows, dtype=np.int64)
            lens[rng.integers(0, nrows, size=max(1, nrows // 50))] = rng.integers(1500, 7000)
        else:
            lens = rng.integers(0, 3, size=nrows) * rng.integers(0, 400, size=nrows)
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        nnz = int(rowptr[-1])
        cols = rng.integers(0, ncols, size=nnz)
        # ascending within each row (duplicates allowed), as the reference's construction yields
        rowid = np.repeat(np.arange(nrows), lens)
        order = np.lexsort((cols, rowid))
        cols = cols[order].astype(np.int64)
        vals = rng.standard_normal(nnz) * 10.0 ** rng.integers(-8, 8)
        x = rng.standard_normal(ncols)
        Ti = np.int32 if trial % 2 == 0 else np.int64
        base = (trial // 2) % 2
        want = orc.spmv(rowptr.astype(Ti), cols.astype(Ti), vals, x)
        got = _raw_spmv(hp, rowptr, cols, vals, x, Ti, base)
        np.testing.assert_array_equal(got, want, err_msg=f"trial {trial} kind {kind} nrows {nrows} nnz {nnz}")


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_pass_boundaries_of_the_straight_line_kernel(hp, orc, gpu_backend_i32, Ti):
    """Block totals around the pass limits of the round 1-3 quad kernel (retired in round 6) -- kept as a shape sweep of the row-gather
    kernel: waves with few / no entries, 2048-entry block totals followed by a short one, and the entry-by-entry pass for the last quad of the
    MATRIX when nnz is not a multiple of 4.  Block totals straddling every one of those limits, every nnz mod 4, split-column
    entry included."""
    import torch
    rng = np.random.default_rng(77)
    sfx = "i32" if Ti == np.int32 else "i64"
    totals = [0, 1, 3, 4, 5, 255, 256, 257, 1020, 1023, 1024, 1025, 1027, 1280, 2044, 2047, 2048, 2049, 2052, 3071, 3072, 4095,
              4096, 4097, 6143, 6150]
    for t0 in totals:
        for t1 in (t0, 7, 0):
            lens = np.zeros(512, dtype=np.int64)
            for blk, tot in enumerate((t0, t1)):
                cuts = np.sort(rng.integers(0, tot + 1, size=255))
                lens[blk * 256:(blk + 1) * 256] = np.diff(np.concatenate([[0], cuts, [tot]]))
            rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            nnz = int(rowptr[-1])
            ncols = 3000
            cols = rng.integers(0, ncols, size=nnz)
            rowid = np.repeat(np.arange(512), lens)
            cols = cols[np.lexsort((cols, rowid))].astype(np.int64)
            vals = rng.standard_normal(nnz)
            x = rng.standard_normal(ncols)
            want = orc.spmv(rowptr.astype(Ti), cols.astype(Ti), vals, x)
            got = _raw_spmv(hp, rowptr, cols, vals, x, Ti)
            np.testing.assert_array_equal(got, want, err_msg=f"block totals {t0}, {t1}")
            # the split-column kernel: columns >= n_own read the ghost segment
            n_own = 1700
            rp, cv, nz = _t(rowptr.astype(Ti)), _t(cols.astype(Ti)), _t(vals)
            xo, xg = _t(x[:n_own]), _t(x[n_own:])
            y = torch.full((512,), float("nan"), dtype=torch.float64, device="cuda")
            hp._capi.call(f"hpcla_spmv_split_f64_{sfx}", rp.data_ptr(), cv.data_ptr() if nnz else None, nz.data_ptr() if nnz else None,
                          xo.data_ptr(), xg.data_ptr(), n_own, y.data_ptr(), 512, nnz, 0, None, 0,
                          torch.cuda.current_stream().cuda_stream)
            np.testing.assert_array_equal(y.cpu().numpy(), want, err_msg=f"split, block totals {t0}, {t1}")


def test_spmv_x_partition_differs_from_row_partition(hp, orc, gpu_backend_i32):
    """A*x accepts any partition of x (the plan is keyed on it): simulated ranks
    with a non-uniform x partition, split-column map + ghost segment, bit-exact per rank."""
    import torch
    nranks, m, n = 3, 2000, 1500
    rp = orc.uniform_partition(m, nranks)
    xp = np.array([0, 200, 1300, n])
    x = orc.fill_uniform(0, n, 33)
    s = torch.cuda.current_stream().cuda_stream
    locs = [orc.sprand_rows(n, 0.01, int(rp[r]), int(rp[r + 1])) for r in range(nranks)]
    comp = [orc.compress_columns(l) for l in locs]
    plans = orc.vector_plans([c[0] for c in comp], xp)
    gathered = orc.execute_plans(plans, [x[xp[r]:xp[r + 1]] for r in range(nranks)])
    for r in range(nranks):
        rows, (ci, cv), pl = locs[r], comp[r], plans[r]
        n_own = int(xp[r + 1] - xp[r])
        hplan = hp.HostVectorPlan(pl.send_rank_ids, pl.send_indices, pl.recv_rank_ids, pl.recv_perm,
                                  pl.local_src_indices, pl.local_dst_indices, pl.n_gathered, n_own)
        cmap = hp.split_column_map(hplan)
        ghost = np.concatenate([gathered[r][p] for p in pl.recv_perm]) if pl.recv_perm else np.zeros(1)
        d_rp, d_split, d_nz = _t(rows.rowptr.astype(np.int32)), _t(cmap[cv].astype(np.int32)), _t(rows.vals)
        d_x, d_g = _t(x[xp[r]:xp[r + 1]]), _t(ghost)
        y = torch.full((rows.nrows,), float("nan"), dtype=torch.float64, device="cuda")
        hp._capi.call("hpcla_spmv_split_f64_i32", d_rp.data_ptr(), d_split.data_ptr(), d_nz.data_ptr(),
                      d_x.data_ptr(), d_g.data_ptr(), n_own, y.data_ptr(), rows.nrows, rows.nnz, 0, None, 0, s)
        torch.cuda.synchronize()
        want = orc.spmv(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, gathered[r])
        np.testing.assert_array_equal(y.cpu().numpy(), want)


@pytest.mark.parametrize("which", ["i32", "i64"])
def test_device_side_construction(hp, orc, gpu_backend_i32, gpu_backend_i64, which):
    """hpcla_gen_poisson2d + hpcla_compress_columns (device) == oracle generator + the reference's
    unique!(sort)/searchsortedfirst compression (host), for a row slice whose column window is wider
    than its rows, and for an unstructured matrix with untouched columns."""
    import torch
    b = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    s = torch.cuda.current_stream().cuda_stream
    lib = hp._capi.load()
    for nx, ny, lo, hi in ((300, 200, 0, 60000), (300, 200, 7777, 41234), (5, 3, 2, 13), (1, 9, 0, 9)):
        want = orc.poisson2d_rows(nx, ny, lo, hi)
        nnz = lib.hpcla_poisson2d_nnz(nx, ny, lo, hi)
        assert nnz == want.nnz
        rp = torch.empty(hi - lo + 1, dtype=torch.int64, device="cuda")
        ci = torch.empty(nnz, dtype=torch.int64, device="cuda")
        va = torch.empty(nnz, dtype=torch.float64, device="cuda")
        hp._capi.call("hpcla_gen_poisson2d", nx, ny, lo, hi, rp.data_ptr(), ci.data_ptr(), va.data_ptr(), s)
        np.testing.assert_array_equal(rp.cpu().numpy(), want.rowptr)
        np.testing.assert_array_equal(ci.cpu().numpy(), want.colidx)
        np.testing.assert_array_equal(va.cpu().numpy(), want.vals)
        A_dev = hp.HPCSparseMatrix_local_device(rp, ci, va, nx * ny, b)
        A_host = hp.HPCSparseMatrix_local(want.rowptr, want.colidx, want.vals, nx * ny, b)
        np.testing.assert_array_equal(A_dev.col_indices, A_host.col_indices)
        np.testing.assert_array_equal(A_dev.colval, A_host.colval)
        np.testing.assert_array_equal(A_dev.rowptr, A_host.rowptr)
        assert A_dev.colval.dtype == A_host.colval.dtype and A_dev._ensure_hash() == A_host._ensure_hash()
    # unstructured, sparse column usage; then multiply
    n = 4000
    rows = orc.sprand_rows(n, 0.0008, 0, n)
    A = hp.HPCSparseMatrix_local_device(_t(rows.rowptr), _t(rows.colidx), _t(rows.vals), n, b)
    ci_ref, cv_ref = orc.compress_columns(rows)
    np.testing.assert_array_equal(A.col_indices, ci_ref)
    np.testing.assert_array_equal(A.colval, cv_ref)
    assert A.ncols_compressed < n
    xg = orc.fill_uniform(0, n, 2)
    y = (A @ hp.HPCVector.from_global(xg, b)).local_values()
    Ti = np.int32 if which == "i32" else np.int64
    np.testing.assert_array_equal(y, orc.spmv(rows.rowptr.astype(Ti), cv_ref.astype(Ti), rows.vals, xg[ci_ref]))
    with pytest.raises(hp._capi.HPCLAError):
        hp.HPCSparseMatrix_local_device(_t(rows.rowptr), _t(rows.colidx), _t(rows.vals), n, b, col_window=(10, n - 1))


def _csr_of(M):
    """(rowptr, global cols, vals) of an HPCSparseMatrix' local rows, on the host."""
    return M.rowptr.astype(np.int64), M.col_indices[M.colval.astype(np.int64)], M.nzval.cpu().numpy()


@pytest.mark.parametrize("name", ["spgemm_tridiagonal", "spgemm_nonsquare"])
def test_spgemm_golden_host_layer(hp, golden, gpu_backend_i32, name):
    """test/test_matrix_multiplication.jl:38-88: HPCSparseMatrix * HPCSparseMatrix."""
    import scipy.sparse as sp
    c = golden[name]
    A = sp.coo_matrix((c["VA"], (np.array(c["IA"]) - 1, np.array(c["JA"]) - 1)), shape=(c["m"], c["k"])).tocsr()
    B = sp.coo_matrix((c["VB"], (np.array(c["IB"]) - 1, np.array(c["JB"]) - 1)), shape=(c["k"], c["n"])).tocsr()
    Ad = hp.HPCSparseMatrix_from_global(A, gpu_backend_i32)
    Bd = hp.HPCSparseMatrix_from_global(B, gpu_backend_i32)
    Cd = Ad @ Bd
    assert isinstance(Cd, hp.HPCSparseMatrix) and Cd.shape == (c["m"], c["n"])
    np.testing.assert_array_equal(Cd.row_partition, Ad.row_partition)
    np.testing.assert_array_equal(Cd.col_partition, Bd.col_partition)
    rp, col, val = _csr_of(Cd)
    for i, row in enumerate(c["C"]):
        assert (col[rp[i]:rp[i + 1]] + 1).tolist() == [j for j, _ in row]
        assert np.max(np.abs(val[rp[i]:rp[i + 1]] - np.array([v for _, v in row])), initial=0.0) < TOL_REF


@pytest.mark.parametrize("which", ["i32", "i64"])
def test_spgemm_bit_exact_vs_oracle(hp, orc, gpu_backend_i32, gpu_backend_i64, which):
    """Random and stencil products incl. every row-length bin (register kernel with 16/32/64 lanes per
    row, hash tables of 512/8192 slots), empty rows, rows with more A entries than products, and A*A of the 2-D Laplacian (the reference's only published SpGEMM benchmark case,
    tools/benchmark_vs_petsc_results.txt:3-11)."""
    import scipy.sparse as sp
    b = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    cases = []
    lap = orc.poisson2d_rows(100, 100, 0, 10_000)
    cases.append((lap, lap, 10_000))
    r1 = orc.sprand_rows(3000, 0.004, 0, 2500)                     # ~12 nnz/row
    r2 = orc.sprand_rows(2000, 0.02, 0, 3000)                      # ~40 nnz/row -> ub ~ 480 (bins 2-3)
    cases.append((r1, r2, 2000))
    # one very long row product (bin 3) next to empty rows
    rng = np.random.default_rng(3)
    lens = np.zeros(50, dtype=np.int64); lens[[3, 17]] = [60, 5]
    rp = np.concatenate([[0], np.cumsum(lens)])
    cols = np.concatenate([np.sort(rng.choice(400, size=l, replace=False)) for l in lens if l])
    Along = orc.LocalRows(rp, cols.astype(np.int64), rng.standard_normal(int(rp[-1])), 400)
    Bwide = orc.sprand_rows(5000, 0.016, 0, 400)                   # ~80 per row -> ub ~ 4800
    cases.append((Along, Bwide, 5000))
    # bin edges of the register expand-sort-combine kernel (16 / 32 / 64 products per row) and rows
    # with far more A entries than products (most referenced B rows are empty): row i of A has
    # i % 90 entries; only every 3rd row of B is non-empty, with (r % 7) + 1 entries in few columns
    nb, ncb = 300, 40
    blen = np.where(np.arange(nb) % 3 == 0, (np.arange(nb) % 7) + 1, 0)
    brp = np.concatenate([[0], np.cumsum(blen)])
    bcols = np.concatenate([np.sort(rng.choice(ncb, size=l, replace=False)) for l in blen if l])
    Bsparse = orc.LocalRows(brp, bcols.astype(np.int64), rng.standard_normal(int(brp[-1])), ncb)
    alen = np.arange(400) % 90
    arp = np.concatenate([[0], np.cumsum(alen)])
    empties = np.flatnonzero(blen == 0)
    acols = np.concatenate([np.sort(rng.choice(empties if (i % 50 == 5 or i % 50 == 45) else nb, size=l, replace=False))
                            for i, l in enumerate(alen) if l])       # rows 5, 45, 55, ...: products = 0, nk up to 55
    Aedge = orc.LocalRows(arp, acols.astype(np.int64), rng.standard_normal(int(arp[-1])), nb)
    cases.append((Aedge, Bsparse, ncb))
    for Ar, Br, ncols in cases:
        A = hp.HPCSparseMatrix_local(Ar.rowptr, Ar.colidx, Ar.vals, Ar.ncols_global, b)
        B = hp.HPCSparseMatrix_local(Br.rowptr, Br.colidx, Br.vals, Br.ncols_global, b)
        C = A @ B
        ci, cv = orc.compress_columns(Ar)
        g_rowptr = np.concatenate([[0], np.cumsum(np.diff(Br.rowptr)[ci])])
        sel = (np.concatenate([np.arange(Br.rowptr[r], Br.rowptr[r + 1]) for r in ci])
               if len(ci) else np.zeros(0, dtype=np.int64))
        w_rp, w_col, w_val = orc.spgemm(Ar.rowptr, cv, Ar.vals, g_rowptr, Br.colidx[sel], Br.vals[sel], ncols)
        rp_c, col_c, val_c = _csr_of(C)
        np.testing.assert_array_equal(rp_c, w_rp)
        np.testing.assert_array_equal(col_c, w_col)
        np.testing.assert_array_equal(val_c, w_val)               # bit-identical accumulation order
        # repeated product with new values on the cached structure: numeric kernels write the final
        # arrays directly (no upper-bound slots, no compaction) -- same structure, values scale exactly
        A2 = hp.HPCSparseMatrix_local(Ar.rowptr, Ar.colidx, Ar.vals * 2.0, Ar.ncols_global, b)
        rp_2, col_2, val_2 = _csr_of(A2 @ B)
        np.testing.assert_array_equal(rp_2, w_rp)
        np.testing.assert_array_equal(col_2, w_col)
        np.testing.assert_array_equal(val_2, 2.0 * w_val)
        # the third product on a structure builds the per-entry product lists (hpcla_spgemm_numeric_mapped_f64) and
        # runs on them, like every later one: new values in B, then in both -- still the oracle's bits (scaling by a
        # power of two is exact in every product and every sum)
        B4 = hp.HPCSparseMatrix_local(Br.rowptr, Br.colidx, Br.vals * 4.0, Br.ncols_global, b)
        rp_3, col_3, val_3 = _csr_of(A @ B4)
        np.testing.assert_array_equal(col_3, w_col)
        np.testing.assert_array_equal(val_3, 4.0 * w_val)
        np.testing.assert_array_equal(_csr_of(A2 @ B4)[2], 8.0 * w_val)
        from hpcla_amd.matmat import get_matrix_plan
        res = get_matrix_plan(A, B).cache["symbolic"]["result"]
        assert res.get("map") is not None or res["nnz"] == 0, "the product lists were not built"
        os.environ["HPCLA_SPGEMM_MAP"] = "0"                       # and without them (the numeric kernels): same bits
        try:
            from hpcla_amd.matmat import clear_matrix_plan_cache as _clear
            _clear()
            _csr_of(A @ B)
            np.testing.assert_array_equal(_csr_of(A2 @ B4)[2], 8.0 * w_val)
        finally:
            del os.environ["HPCLA_SPGEMM_MAP"]
        Cs = (sp.csr_matrix((Ar.vals, Ar.colidx, Ar.rowptr), shape=(Ar.nrows, Ar.ncols_global)) @
              sp.csr_matrix((Br.vals, Br.colidx, Br.rowptr), shape=(Br.nrows, Br.ncols_global))).tocsr()
        got = sp.csr_matrix((val_c, col_c, rp_c), shape=Cs.shape)
        assert abs(got - Cs).max() <= 1e-12 * max(abs(Cs).max(), 1.0)
        # the product is a first-class HPCSparseMatrix: multiply it with a vector
        xg = orc.fill_uniform(0, ncols, 8)
        y = (C @ hp.HPCVector.from_global(xg, b)).local_values()
        np.testing.assert_allclose(y, Cs @ xg, rtol=1e-12, atol=1e-12 * np.abs(Cs @ xg).max())
    from hpcla_amd.matmat import clear_matrix_plan_cache
    clear_matrix_plan_cache()


def test_dense_matvec(hp, orc, gpu_backend_i32):
    """HPCMatrix * HPCVector (src/dense.jl:614-658; test/test_dense_matrix.jl with dense_matrix
    A[i,j] = i+j, test/test_utils.jl:107-117): exact for small integers; random case within the
    stated 1e-12 relative (tree vs BLAS order); three-segment x (simulated ranks) through the raw ABI."""
    import torch
    b = gpu_backend_i32
    m, n = 8, 6
    A = np.array([[float(i + j) for j in range(1, n + 1)] for i in range(1, m + 1)])
    x = np.arange(1.0, n + 1)
    Ad, xd = hp.HPCMatrix.from_global(A, b), hp.HPCVector.from_global(x, b)
    y = Ad @ xd
    assert isinstance(y, hp.HPCVector)
    np.testing.assert_array_equal(y.local_values(), A @ x)             # exact in fp64
    np.testing.assert_array_equal(y.partition, Ad.row_partition)
    for m, n in ((1, 1), (5, 3), (300, 1025), (1000, 64), (64, 4099)):
        A = orc.fill_uniform(0, m * n, 3).reshape(m, n) - 0.5
        x = orc.fill_uniform(0, n, 4) - 0.5
        y = (hp.HPCMatrix.from_global(A, b) @ hp.HPCVector.from_global(x, b)).local_values()
        scale = np.abs(A) @ np.abs(x)
        assert np.all(np.abs(y - A @ x) <= RTOL_RED * scale + 1e-300)
        # raw ABI, x delivered as three segments (what a rank sees after the all-to-all halo)
        for n_lo, n_own in ((0, n), (n // 3, n // 3), (1, 0) if n > 1 else (0, n)):
            n_hi = n - n_lo - n_own
            dA, dy = _t(A), torch.empty(m, dtype=torch.float64, device="cuda")
            segs = [_t(x[:n_lo]) if n_lo else None, _t(x[n_lo:n_lo + n_own]) if n_own else None,
                    _t(x[n_lo + n_own:]) if n_hi else None]
            ptr = lambda t: t.data_ptr() if t is not None else None
            hp._capi.call("hpcla_gemv_rowmajor_f64", dA.data_ptr(), n, m, ptr(segs[0]), n_lo, ptr(segs[1]), n_own,
                          ptr(segs[2]), n_hi, dy.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.all(np.abs(dy.cpu().numpy() - A @ x) <= RTOL_RED * scale + 1e-300)
    hp.clear_dense_plan_cache()


def test_sparse_addition_and_subtraction(hp, orc, gpu_backend_i32):
    """A + B / A - B with different sparsity patterns (test/test_addition_different_sparsity.jl,
    src/sparse.jl:1405-1494): union structure with structural zeros kept, one rounding per entry."""
    import scipy.sparse as sp
    b = gpu_backend_i32
    n = 3000
    Ar, Br = orc.sprand_rows(n, 0.004, 0, n), orc.sprand_rows(n, 0.003, 0, n, seed_struct=77, seed_vals=78)
    # make some shared entries cancel exactly (structural zero must be kept)
    Br.vals[:50] = 1.0
    A = hp.HPCSparseMatrix_local(Ar.rowptr, Ar.colidx, Ar.vals, n, b)
    B = hp.HPCSparseMatrix_local(Br.rowptr, Br.colidx, Br.vals, n, b)
    As = sp.csr_matrix((Ar.vals, Ar.colidx, Ar.rowptr), shape=(n, n))
    Bs = sp.csr_matrix((Br.vals, Br.colidx, Br.rowptr), shape=(n, n))
    pattern = (abs(As) + abs(Bs)).tocsr(); pattern.sort_indices()
    for op, Cs in (("add", As + Bs), ("sub", As - Bs), ("self_sub", As - As)):
        C = (A + B) if op == "add" else ((A - B) if op == "sub" else (A - A))
        rp, col, val = _csr_of(C)
        want_pat = pattern if op != "self_sub" else As
        np.testing.assert_array_equal(rp, want_pat.indptr)             # structural zeros preserved
        np.testing.assert_array_equal(col, want_pat.indices)
        dense_want = Cs.toarray()
        got = sp.csr_matrix((val, col, rp), shape=(n, n)).toarray()
        np.testing.assert_array_equal(got, dense_want)                 # a+b / a-b / copies: exact
        np.testing.assert_array_equal(C.row_partition, A.row_partition)
    xg = orc.fill_uniform(0, n, 1)
    y = ((A + B) @ hp.HPCVector.from_global(xg, b)).local_values()
    np.testing.assert_allclose(y, (As + Bs) @ xg, rtol=1e-12, atol=1e-13)
    from hpcla_amd.addition import clear_addition_plan_cache
    clear_addition_plan_cache()


def test_repartition_serial_paths_and_range_exchange_errors(hp, orc, gpu_backend_i32):
    """repartition (src/vectors.jl:712-722, src/dense.jl:1798-1810, src/sparse.jl:4590-4600) on one rank:
    the only valid target is the current partition -> the object itself comes back; the C entry point
    performs the local-copy leg and rejects messages on a serial communicator (the RCCL leg runs in
    tests/_halo_self_worker.py, the plan lists in the gloo tests)."""
    import torch
    from hpcla_amd.repartition import exchange_ranges
    b = gpu_backend_i32
    n = 1000
    v = hp.HPCVector.from_global(orc.fill_uniform(0, n, 3), b)
    assert hp.repartition(v, np.array([0, n])) is v
    with pytest.raises(ValueError):
        hp.repartition(v, np.array([0, n - 1]))
    M = hp.HPCMatrix.from_global(orc.fill_uniform(0, n * 4, 4).reshape(n, 4), b)
    assert hp.repartition(M, np.array([0, n])) is M
    R = orc.sprand_rows(n, 0.01, 0, n)
    A = hp.HPCSparseMatrix_local(R.rowptr, R.colidx, R.vals, n, b)
    assert hp.repartition(A, np.array([0, n])) is A
    # local leg only, width 3
    src = torch.arange(30, dtype=torch.float64, device="cuda")
    dst = torch.zeros(30, dtype=torch.float64, device="cuda")
    exchange_ranges(b, src, dst, [], [], [], [], [], [], 2, 5, 4, 3)
    torch.cuda.synchronize()
    want = np.zeros(30); want[15:27] = np.arange(6, 18)
    np.testing.assert_array_equal(dst.cpu().numpy(), want)
    with pytest.raises(hp._capi.HPCLAError):
        exchange_ranges(b, src, dst, [0], [0], [4], [0], [0], [4], 0, 0, 0, 1)
    # dot / + with an operand of another length: explicit error before any launch
    w = hp.HPCVector.from_global(np.ones(n + 1), b)
    with pytest.raises(ValueError):
        hp.dot(v, w)


@pytest.mark.parametrize("shape", [(5000, 16), (3001, 37), (257, 64), (40, 700), (1, 1), (100000, 3)])
def test_dense_transpose_matvec(hp, orc, gpu_backend_i32, shape):
    """transpose(A) * x and transpose(v) * A for dense A (src/dense.jl:1210-1274,
    test/test_dense_matrix.jl transpose cases): BLAS + Allreduce order is unspecified in the
    reference, so tolerance parity: 1e-12 relative to |A|^T |x|."""
    b = gpu_backend_i32
    m, n = shape
    Ag = orc.fill_uniform(0, m * n, 21).reshape(m, n) - 0.5
    xg = orc.fill_uniform(0, m, 22) - 0.5
    A = hp.HPCMatrix.from_global(Ag, b)
    x = hp.HPCVector.from_global(xg, b)
    y = hp.transpose(A) @ x
    want = Ag.T @ xg
    scale = np.abs(Ag).T @ np.abs(xg) + 1e-300
    assert np.all(np.abs(y.local_values() - want) <= 1e-12 * scale)
    np.testing.assert_array_equal(y.partition, A.col_partition)
    yt = hp.transpose(x) @ A
    assert isinstance(yt, hp.TransposedHPCVector)
    np.testing.assert_array_equal(yt.parent.local_values(), y.local_values())    # same kernels: same bits
    with pytest.raises(ValueError):
        hp.transpose(A) @ hp.HPCVector.from_global(np.ones(m + 1), b)


def test_dense_scalar_ops_and_norms(hp, orc, golden, gpu_backend_i32):
    """a*A, A*a, A/a (src/dense.jl:1317-1327, 1818-1838) and norm(A, p) (src/dense.jl:1399-1420); the SpMM
    fixture's Frobenius norm (test/test_new_operations.jl:79-82) closes the loop on a reference value."""
    import math
    b = gpu_backend_i32
    Mg = orc.fill_uniform(0, 300 * 7, 9).reshape(300, 7) - 0.5
    M = hp.HPCMatrix.from_global(Mg, b)
    np.testing.assert_array_equal((2.5 * M).local_values(), 2.5 * Mg)
    np.testing.assert_array_equal((M * 2.5).local_values(), Mg * 2.5)
    np.testing.assert_array_equal((M / 3.0).local_values(), Mg / 3.0)
    assert abs(M.norm() - np.linalg.norm(Mg)) <= RTOL_RED * np.linalg.norm(Mg)
    assert abs(M.norm(1) - np.abs(Mg).sum()) <= RTOL_RED * np.abs(Mg).sum()
    assert M.norm(math.inf) == np.abs(Mg).max()
    c = golden["spmm_sym"]
    A = _from_coo(hp, c["I"], c["J"], c["V"], c["m"], c["n"], b)
    C = A @ hp.HPCMatrix.from_global(np.array(c["B"]), b)
    assert abs(C.norm() - c["C_fro"]) < TOL_REF


def test_sparse_scalar_ops_norm_and_transposed_products(hp, orc, gpu_backend_i32):
    """a*A, A*a, -A, copy (src/sparse.jl:2289-2315, 2458), norm(A, p) (:2172-2195) and the products with
    lazily transposed operands (:2342-2368): the structure arrays are shared, values exact."""
    import math
    import scipy.sparse as sp
    b = gpu_backend_i32
    Ar, Br = orc.sprand_rows(500, 0.02, 0, 400), orc.sprand_rows(500, 0.03, 0, 300, seed_struct=5, seed_vals=6)
    A = hp.HPCSparseMatrix_local(Ar.rowptr, Ar.colidx, Ar.vals, 500, b)          # 400 x 500
    Bm = hp.HPCSparseMatrix_local(Br.rowptr, Br.colidx, Br.vals, 500, b)         # 300 x 500
    As = sp.csr_matrix((Ar.vals, Ar.colidx, Ar.rowptr), shape=(400, 500))
    Bs = sp.csr_matrix((Br.vals, Br.colidx, Br.rowptr), shape=(300, 500))
    for M, want in ((2.5 * A, 2.5 * Ar.vals), (A * 2.5, Ar.vals * 2.5), (-A, -Ar.vals), (A.copy(), Ar.vals)):
        rp, col, val = _csr_of(M)
        np.testing.assert_array_equal(rp, Ar.rowptr); np.testing.assert_array_equal(col, Ar.colidx)
        np.testing.assert_array_equal(val, want)
        assert M._ensure_hash() == A._ensure_hash()
    nv = Ar.vals
    assert abs(A.norm() - np.linalg.norm(nv)) <= RTOL_RED * np.linalg.norm(nv)
    assert abs(A.norm(1) - np.abs(nv).sum()) <= RTOL_RED * np.abs(nv).sum() and A.norm(math.inf) == np.abs(nv).max()
    for got, want in ((A @ hp.transpose(Bm), As @ Bs.T), (hp.transpose(A) @ A, As.T @ As)):
        want = want.tocsr(); want.sort_indices()
        d = _dense_of(got, want.shape)
        assert np.max(np.abs(d - want.toarray())) <= 1e-12 * max(1.0, np.abs(want.toarray()).max())
    # A + lambda*I, A - lambda*I (src/sparse.jl:3925-3995): missing diagonal entries appear structurally
    Sq = orc.sprand_rows(300, 0.02, 0, 300, seed_struct=8, seed_vals=9)
    S = hp.HPCSparseMatrix_local(Sq.rowptr, Sq.colidx, Sq.vals, 300, b)
    Ss = sp.csr_matrix((Sq.vals, Sq.colidx, Sq.rowptr), shape=(300, 300))
    np.testing.assert_array_equal(_dense_of(hp.add_scaled_identity(S, 2.5), (300, 300)), (Ss + 2.5 * sp.identity(300)).toarray())
    np.testing.assert_array_equal(_dense_of(hp.add_scaled_identity(S, 2.5, subtract=True), (300, 300)),
                                  (Ss - 2.5 * sp.identity(300)).toarray())
    assert hp.add_scaled_identity(S, 1.0).nnz == len(np.unique(np.concatenate([Sq.colidx + 300 * np.repeat(np.arange(300), np.diff(Sq.rowptr)),
                                                                                  301 * np.arange(300)])))
    from hpcla_amd.matmat import clear_matrix_plan_cache
    clear_matrix_plan_cache(); hp.clear_transpose_plan_cache(); hp.clear_plan_cache()


def test_row_vector_algebra(hp, orc, gpu_backend_i32):
    """transpose(v) * A, a*vt, vt*a, vt/a, vt +/- wt (src/sparse.jl:2136-2142, src/vectors.jl:909-987,
    test/test_vector_multiplication.jl:141-160, 291-309)."""
    import scipy.sparse as sp
    b = gpu_backend_i32
    n, m = 900, 700
    R = orc.sprand_rows(m, 0.02, 0, n)
    A = hp.HPCSparseMatrix_local(R.rowptr, R.colidx, R.vals, m, b)
    As = sp.csr_matrix((R.vals, R.colidx, R.rowptr), shape=(n, m))
    vg, wg = orc.fill_uniform(0, n, 31), orc.fill_uniform(0, n, 32)
    v, w = hp.HPCVector.from_global(vg, b), hp.HPCVector.from_global(wg, b)
    vt = hp.transpose(v)
    assert hp.transpose(vt) is v and hp.adjoint(v).parent is v
    yt = vt @ A
    ref = hp.transpose(A) @ v                                    # bit-identical by construction ...
    np.testing.assert_array_equal(yt.parent.local_values(), ref.local_values())
    ATs = As.T.tocsr(); ATs.sort_indices()
    np.testing.assert_array_equal(ref.local_values(), orc.spmv(ATs.indptr, ATs.indices, ATs.data, vg))   # ... and to the oracle
    np.testing.assert_array_equal((2.5 * vt).parent.local_values(), 2.5 * vg)
    np.testing.assert_array_equal((vt * 2.5).parent.local_values(), vg * 2.5)
    np.testing.assert_array_equal((vt / 3.0).parent.local_values(), vg / 3.0)
    np.testing.assert_array_equal((vt + hp.transpose(w)).parent.local_values(), vg + wg)
    np.testing.assert_array_equal((vt - hp.transpose(w)).parent.local_values(), vg - wg)
    np.testing.assert_array_equal((-vt).parent.local_values(), -vg)
    assert abs(vt @ w - float(vg @ wg)) <= 1e-12 * float(np.abs(vg) @ np.abs(wg))


def _dense_of(M, shape):
    import scipy.sparse as sp
    rp, col, val = _csr_of(M)
    return sp.csr_matrix((val, col, rp), shape=shape).toarray()


def _from_coo(hp, I, J, V, m, n, backend):
    import scipy.sparse as sp
    return hp.HPCSparseMatrix_from_global(sp.coo_matrix((V, (np.array(I) - 1, np.array(J) - 1)), shape=(m, n)), backend)


def test_widened_rows_on_reference_fixtures(hp, golden, gpu_backend_i32):
    """The reference's own closed-form inputs for the SURVEY 8f rows, expected values in exact
    rational arithmetic (tests/golden/make_golden.py), reference tolerance 1e-10 absolute:
    transpose(A)*x (test/test_new_operations.jl:43-76), A+B / A-B with different sparsity and the
    D' * W * D product chains (test/test_addition_different_sparsity.jl:41-118)."""
    b = gpu_backend_i32
    c = golden["transpose_spmv"]
    A = _from_coo(hp, c["I"], c["J"], c["V"], c["m"], c["n"], b)
    y = (hp.transpose(A) @ hp.HPCVector.from_global(np.array(c["x"]), b)).local_values()
    assert np.max(np.abs(y - np.array(c["y"]))) < TOL_REF
    c = golden["add_different_sparsity"]
    n = c["n"]
    A = _from_coo(hp, c["IA"], c["JA"], c["VA"], n, n, b)
    B = _from_coo(hp, c["IB"], c["JB"], c["VB"], n, n, b)
    np.testing.assert_array_equal(_dense_of(A + B, (n, n)), np.array(c["sum"]))      # small integers / halves: exact
    np.testing.assert_array_equal(_dense_of(A - B, (n, n)), np.array(c["diff"]))
    c = golden["dtwd_products"]
    n = c["n"]
    dx = _from_coo(hp, c["Idx"], c["Jdx"], c["Vdx"], n, n, b)
    eye = _from_coo(hp, list(range(1, n + 1)), list(range(1, n + 1)), [1.0] * n, n, n, b)
    W = _from_coo(hp, list(range(1, n + 1)), list(range(1, n + 1)), c["w"], n, n, b)
    M1 = (hp.transpose(eye) @ W) @ dx
    M2 = (hp.transpose(dx) @ W) @ eye
    assert np.max(np.abs(_dense_of(M1 + M2, (n, n)) - np.array(c["M_sum"]))) < TOL_REF
    H = (hp.transpose(dx) @ W) @ dx
    H = H + (hp.transpose(eye) @ W) @ eye
    assert np.max(np.abs(_dense_of(H, (n, n)) - np.array(c["H"]))) < TOL_REF
    from hpcla_amd.addition import clear_addition_plan_cache
    from hpcla_amd.matmat import clear_matrix_plan_cache
    clear_addition_plan_cache(); clear_matrix_plan_cache(); hp.clear_plan_cache()


def test_host_collectives_on_mixed_gloo_nccl_group():
    """bench.py --gpus N initialises torch.distributed with "cpu:gloo,cuda:nccl" (that needs a GPU to be
    constructed, hence the gpu mark).  Two processes: comm_* primitives, index/value exchanges and
    build_host_vector_plan must work on that mixed group exactly as on the gloo-only group of the CPU tests."""
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "_mixed_pg_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("mixed-backend host collectives OK") == 2


def test_graft_entry_smoke():
    import __graft_entry__ as g
    g.smoke()


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmm_run_tiles_raw_abi(hp, orc, gpu_backend_i32, Ti):
    """hpcla_spmm_runs_build_* / hpcla_spmm_runs_k16_f64_* (RUN TILES): descriptors = the distinct columns of every
    64-row block as <= 4 contiguous runs, cut at the own / ghost boundary; blocks with more runs, > 200 rows or > 512
    entries are marked; the product is bit-identical to the oracle's column loop (src/sparse.jl:2391-2413) for fitting
    and for marked blocks alike, with and without a ghost segment, through block lists and in both index bases."""
    import ctypes
    import torch
    k = 16
    s = torch.cuda.current_stream().cuda_stream
    sfx = "i32" if Ti == np.int32 else "i64"
    lib = hp._capi.load()

    def run_case(rows, n_own, base, expect_fit=None, lists=True):
        n = rows.nrows
        ci, cv = orc.compress_columns(rows)
        ncomp = len(ci)
        Bg = orc.fill_uniform(0, ncomp * k, 21).reshape(ncomp, k)
        want = orc.spmm(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, Bg)
        rp, dcv, nz = _t((rows.rowptr + base).astype(Ti)), _t((cv + base).astype(Ti)), _t(rows.vals)
        dB_own = _t(Bg[:n_own].ravel()) if n_own else torch.zeros(16, dtype=torch.float64, device="cuda")
        dB_gh = _t(Bg[n_own:].ravel()) if n_own < ncomp else None
        desc = torch.empty(lib.hpcla_spmm_runs_desc_bytes(n), dtype=torch.uint8, device="cuda")
        n_fit = ctypes.c_int64(-1)
        hp._capi.call(f"hpcla_spmm_runs_build_{sfx}", rp.data_ptr(), dcv.data_ptr(), n, rows.nnz, base, n_own, desc.data_ptr(),
                      ctypes.byref(n_fit), s)
        nblk = (n + 63) // 64
        d = desc.cpu().numpy().view(np.int32).reshape(nblk, 8)
        # the descriptors against the host restatement (tests/_spmm_edge_cases.py)
        fit_ref = sc.check_descriptors(d, n_fit.value, sc.run_descriptors(rows.rowptr, cv, n, n_own))
        if expect_fit is not None:
            assert (fit_ref == nblk) == expect_fit, (fit_ref, nblk)
        perm = np.random.default_rng(4).permutation(nblk).astype(np.int32)
        for lst in ([None, _t(perm)] if lists else [None]):
            C = torch.full((n * k,), float("nan"), dtype=torch.float64, device="cuda")
            hp._capi.call(f"hpcla_spmm_runs_k16_f64_{sfx}", rp.data_ptr(), dcv.data_ptr(), nz.data_ptr(), dB_own.data_ptr(),
                          dB_gh.data_ptr() if dB_gh is not None else None, n_own, C.data_ptr(), n, rows.nnz, base, desc.data_ptr(),
                          lst.data_ptr() if lst is not None else None, nblk if lst is not None else 0, s)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(C.cpu().numpy().reshape(n, k), want)

    # 5-point matrix, every column owned: 3 runs of 64 / 66 / 64 rows per block; ragged last block
    nx, ny = 200, 37
    rows = orc.poisson2d_rows(nx, ny, 0, nx * ny)
    run_case(rows, nx * ny, 0, expect_fit=True)
    run_case(rows, nx * ny, 1, expect_fit=True, lists=False)
    # a rank's slab of it: ghost lines above and below; the own / ghost cut falls INSIDE a run of consecutive columns
    lo, hi = 5 * nx + 13, 21 * nx + 150
    slab = orc.poisson2d_rows(nx, ny, lo, hi)
    ci, _ = orc.compress_columns(slab)
    run_case(slab, int(np.searchsorted(ci, hi) - 0), 0)          # "own" = the compressed columns below hi (a split inside the space)
    # 7-point matrix: 5 runs per block -> every block marked, still the right product (slow path)
    r3 = orc.poisson3d_rows(24, 24, 6, 0, 24 * 24 * 6)
    run_case(r3, 24 * 24 * 6, 0, expect_fit=False, lists=False)
    # unstructured rows and a block with > 512 entries
    run_case(orc.sprand_rows(3000, 0.004, 0, 700), 2000, 0, lists=False)
    rng = np.random.default_rng(3)
    lens = np.full(130, 3, dtype=np.int64); lens[70] = 600
    rpx = np.concatenate([[0], np.cumsum(lens)])
    colsx = np.concatenate([np.sort(rng.choice(5000, size=l, replace=False)) for l in lens])
    run_case(orc.LocalRows(rpx, colsx.astype(np.int64), rng.standard_normal(int(rpx[-1])), 5000), 4000, 0, lists=False)
    assert lib.hpcla_spmm_runs_build_i32(None, None, 5, 5, 0, 5, None, None, None) != 0
    assert lib.hpcla_spmm_runs_k16_f64_i32(None, None, None, None, None, 0, None, 5, 5, 0, None, None, 0, None) != 0


def test_spmm_host_layer_takes_run_tiles_on_stencils_only(hp, orc, gpu_backend_i32, gpu_backend_i64, monkeypatch):
    """A * B with k = 16: the plan builds run descriptors once; a stencil matrix takes the run-tile kernel (every block
    fits), an unstructured one keeps the gather kernel; HPCLA_SPMM_RUNS=0 switches it off -- the same bits every way."""
    N, k = 300, 16
    rows = orc.poisson2d_rows(N, N, 0, N * N)
    Bg = orc.fill_uniform(0, N * N * k, 5).reshape(N * N, k)
    want = orc.spmm(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, Bg)
    for backend in (gpu_backend_i32, gpu_backend_i64):
        A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N * N, backend)
        B = hp.HPCMatrix.from_global(Bg, backend)
        assert hp.spmm_runs_fit_of(A, B) is None
        np.testing.assert_array_equal((A @ B).local_values(), want)
        fit, nb = hp.spmm_runs_fit_of(A, B)
        assert fit == nb == (N * N + 63) // 64
        np.testing.assert_array_equal((A @ B).local_values(), want)
    hp.clear_spmm_cache(); hp.clear_plan_cache()
    monkeypatch.setenv("HPCLA_SPMM_RUNS", "0")
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, N * N, gpu_backend_i32)
    B = hp.HPCMatrix.from_global(Bg, gpu_backend_i32)
    np.testing.assert_array_equal((A @ B).local_values(), want)
    assert hp.spmm_runs_fit_of(A, B) is None
    monkeypatch.delenv("HPCLA_SPMM_RUNS")
    n = 20000
    r2 = orc.sprand_rows(n, 0.001, 0, n)
    A2 = hp.HPCSparseMatrix_local(r2.rowptr, r2.colidx, r2.vals, n, gpu_backend_i32)
    B2g = orc.fill_uniform(0, n * k, 6).reshape(n, k)
    C2 = (A2 @ hp.HPCMatrix.from_global(B2g, gpu_backend_i32)).local_values()
    fit, nb = hp.spmm_runs_fit_of(A2, hp.HPCMatrix.from_global(B2g, gpu_backend_i32))
    assert fit < 0.5 * nb
    np.testing.assert_array_equal(C2, orc.spmm(r2.rowptr.astype(np.int32), r2.colidx.astype(np.int32), r2.vals, B2g))
    hp.clear_spmm_cache(); hp.clear_plan_cache()


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_kernel_forms_give_the_reference_bits(hp, orc, gpu_backend_i32, Ti):
    """The three forms of the row-gather SpMV (wave-private LDS copy of the A entries, every lane walks its own row) -- plain,
    split column space, fused x.y epilogue -- are the reference's row-sequential sum (src/sparse.jl:2055-2066): bits of the oracle
    on the golden-sized, sprand, long-row and empty-row shapes.  (Rounds 1-5 ran the retired quad kernel beside it here.)"""
    import torch
    lib = hp._capi.load()
    sfx = "i32" if Ti == np.int32 else "i64"
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(9)
    cases = [orc.poisson3d_rows(40, 40, 7, 0, 40 * 40 * 7), orc.poisson2d_rows(300, 41, 0, 300 * 41),
             orc.sprand_rows(5000, 0.004, 0, 5000)]
    lens = rng.integers(0, 12, 700)
    lens[[5, 300, 699]] = [1500, 449, 3000]                  # longer than one wave pass (448), across several
    lens[10:20] = 0
    rp = np.concatenate([[0], np.cumsum(lens)])
    cols = np.concatenate([np.sort(rng.choice(4000, size=l, replace=False)) for l in lens if l])
    cases.append(orc.LocalRows(rp, cols.astype(np.int64), rng.standard_normal(int(rp[-1])), 4000))
    try:
        for rows in cases:
            ci, cv = orc.compress_columns(rows)
            n, ncomp = rows.nrows, len(ci)
            xg = orc.fill_uniform(0, ncomp, 77) - 0.5
            want = orc.spmv(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, xg)
            n_own = ncomp // 2 + 3                               # split column space: own part, then "ghosts"
            d_rp, d_cv, d_nz = _t(rows.rowptr.astype(Ti)), _t(cv.astype(Ti)), _t(rows.vals)
            d_x, d_xo, d_xg = _t(xg), _t(xg[:n_own]), _t(xg[n_own:])
            got = {}
            for kind in (0,):
                y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                hp._capi.call(f"hpcla_spmv_csr_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), d_x.data_ptr(),
                              y.data_ptr(), n, rows.nnz, 0, s)
                y2 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                hp._capi.call(f"hpcla_spmv_split_f64_{sfx}", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), d_xo.data_ptr(),
                              d_xg.data_ptr(), n_own, y2.data_ptr(), n, rows.nnz, 0, None, 0, s)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(y.cpu().numpy(), want)
                np.testing.assert_array_equal(y2.cpu().numpy(), want)
                if ncomp == n:                                   # square: the fused x.y epilogue (x partitioned like the rows)
                    out = torch.zeros(1, dtype=torch.float64, device="cuda")
                    work = torch.empty(lib.hpcla_spmv_dot_work_bytes(n) // 8 + 1, dtype=torch.float64, device="cuda")
                    y3 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                    hp._capi.call(f"hpcla_spmv_dist_dot_f64_{sfx}", None, None, d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(),
                                  d_x.data_ptr(), n, y3.data_ptr(), n, rows.nnz, 0, None, 0, None, 0, out.data_ptr(),
                                  work.data_ptr(), s)
                    torch.cuda.synchronize()
                    np.testing.assert_array_equal(y3.cpu().numpy(), want)
                    got[kind] = float(out.item())
                    ref = float(np.dot(xg, want))
                    assert abs(got[kind] - ref) <= 1e-12 * float(np.abs(xg) @ np.abs(want))
    finally:
        pass


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_rowgather_wave_pass_boundaries(hp, orc, gpu_backend_i32, Ti):
    """The row-gather kernel's unit is a WAVE: 64 rows whose entry range -- from the quad-aligned entry at or before its
    first entry -- is streamed into LDS in passes of 464 entries.  Wave totals around every pass limit (one pass, one pass
    exactly, one entry over, two and three passes), every alignment of the wave's first entry (0..3 entries in front of
    it in its quad), empty waves, rows that span passes, a ragged last block, and the entry-by-entry pass at the end of the
    matrix for every nnz mod 4."""
    import torch
    rng = np.random.default_rng(2024)
    ncols = 5000
    lib = hp._capi.load()
    totals = [0, 1, 3, 4, 63, 64, 459, 460, 461, 462, 463, 464, 465, 468, 927, 928, 929, 1391, 1392, 1393, 2000]
    try:
        for shift in range(4):
            lens = []
            lens += [shift] + [0] * 63                           # a first wave that shifts everybody's alignment
            for tot in totals:
                if tot == 0:
                    w = np.zeros(64, dtype=np.int64)
                elif tot < 64:
                    w = np.zeros(64, dtype=np.int64)
                    w[rng.choice(64, size=tot, replace=False)] = 1
                else:
                    cuts = np.sort(rng.integers(0, tot + 1, size=63))
                    w = np.diff(np.concatenate([[0], cuts, [tot]]))
                lens += list(w)
            lens += [5] * 37                                     # ragged tail: the last block has 37 rows
            lens = np.array(lens, dtype=np.int64)
            n = len(lens)
            rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            nnz = int(rowptr[-1])
            rowid = np.repeat(np.arange(n), lens)
            cols = rng.integers(0, ncols, size=nnz)
            cols = cols[np.lexsort((cols, rowid))].astype(np.int64)
            vals = rng.standard_normal(nnz)
            x = rng.standard_normal(ncols)
            want = orc.spmv(rowptr.astype(Ti), cols.astype(Ti), vals, x)
            for kind in (0,):
                got = _raw_spmv(hp, rowptr, cols, vals, x, Ti)
                np.testing.assert_array_equal(got, want, err_msg=f"kernel {kind}, shift {shift}, nnz mod 4 = {nnz % 4}")
    finally:
        pass
