"""The plan's table of repeating block patterns (VectorPlan.patterns, csrc/patterns.hip, IndexPolicy<Pat16> of csrc/spmv.hip):
a row block whose index pattern is in the table reads its columns and row bounds from there instead of streaming cols16
and rowptr, and y keeps its bits.

Every product is compared with ``np.array_equal`` against the oracle's stored-order sum, against the same product on the
streamed 16-bit columns (``HPCLA_BLOCK_PATTERNS=0`` through the host layer, ``hpcla_spmv_cols16_f64_i32`` on the raw entry
points) and against ``hpcla_spmv_csr_f64_i32``.  What the info call must report (patterns kept, table bytes, blocks in the
table, or no handle at all) is computed in numpy by ``model_table``, independently of the device code.  Arrays handed to
the raw entry points END inside guarded buffers.  Generators and model are checked on the CPU in
tests/test_block_patterns_cases.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _narrow_cols_cases import eligible_np, long_and_empty_rows, tail_case  # noqa: E402
from _block_patterns_cases import (band_with_random_half, model_table, more_patterns_than_the_cap, one_column_off,  # noqa: E402
                                   pattern_keys_np, unstructured)

pytestmark = pytest.mark.gpu

RANK_WORKER = os.path.join(ROOT, "tests", "_block_patterns_rank_worker.py")
SELF_WORKER = os.path.join(ROOT, "tests", "_block_patterns_self_worker.py")
GUARD = 64


def _raw_products(hp, orc, rowptr, col, vals, xg, base, flags=0, expect_model=True):
    """Int32, cols16 and pattern products through the raw entry points with index_base `base`; asserts the bits and that
    the info call reports what the numpy model predicts.  Returns the info dict (None: the library created no handle)."""
    import torch
    lib = hp._capi.load()
    from hpcla_amd import sparse
    s = torch.cuda.current_stream().cuda_stream
    n, nnz = len(rowptr) - 1, len(col)
    assert eligible_np(rowptr, col, n)
    want = orc.spmv(rowptr.astype(np.int32), col.astype(np.int32), vals, xg)
    d_rp = torch.from_numpy((rowptr + base).astype(np.int32)).cuda()
    cbuf = torch.full((nnz + GUARD,), n - 1 + base, dtype=torch.int32, device="cuda")
    cbuf[:nnz] = torch.from_numpy((col + base).astype(np.int32)).cuda()
    vbuf = torch.full((nnz + GUARD,), float("nan"), dtype=torch.float64, device="cuda")     # nzval ENDS inside a NaN guard
    vbuf[:nnz] = torch.from_numpy(vals).cuda()
    xbuf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    xbuf[GUARD:GUARD + n] = torch.from_numpy(xg).cuda()
    d_cv, d_nz, d_x = cbuf[:nnz], vbuf[:nnz], xbuf[GUARD:GUARD + n]

    def fresh():
        return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    y32, y16, yp = fresh(), fresh(), fresh()
    hp._capi.call("hpcla_spmv_csr_f64_i32", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), d_x.data_ptr(), y32.data_ptr(),
                  n, nnz, base, s)
    c16 = torch.empty(lib.hpcla_cols16_padded_len(nnz), dtype=torch.int16, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    hp._capi.call("hpcla_cols16_encode_i32", d_rp.data_ptr(), d_cv.data_ptr(), n, nnz, n, base, None, 0, c16.data_ptr(),
                  bad.data_ptr(), s)
    assert int(bad.item()) == 0
    hp._capi.call("hpcla_spmv_cols16_f64_i32", d_rp.data_ptr(), c16.data_ptr(), d_nz.data_ptr(), d_x.data_ptr(), y16.data_ptr(),
                  n, nnz, base, None, 0, s)
    torch.cuda.synchronize()
    assert np.array_equal(y32.cpu().numpy(), want), "Int32 column stream differs from the oracle"
    assert np.array_equal(y16.cpu().numpy(), want), "streamed 16-bit columns differ from the oracle"

    h = ctypes.c_void_p()
    hp._capi.call("hpcla_block_patterns_create_i32", ctypes.byref(h), d_rp.data_ptr(), c16.data_ptr(), n, nnz, base, None, -1, 0,
                  flags, s)
    model = model_table(rowptr, col)
    if not h:
        assert model is None or not expect_model, "the library created no table where the model expects one"
        return None
    try:
        info = sparse.block_patterns_info(h)
        print(f"block patterns: {info} model: {model}")
        if expect_model:
            assert info == model, (info, model)
        assert info["table_bytes"] <= 256 * 1024 and 2 * info["patterned"] >= info["candidates"]
        for _ in range(2):
            hp._capi.call("hpcla_spmv_patterns_f64_i32", d_rp.data_ptr(), c16.data_ptr(), h, d_nz.data_ptr(), d_x.data_ptr(),
                          yp.data_ptr(), n, nnz, base, None, 0, s)
        torch.cuda.synchronize()
        got = yp.cpu().numpy()
        assert np.array_equal(got, want), f"pattern form differs from the oracle in {int((got != want).sum())} rows"
        assert np.array_equal(got, y16.cpu().numpy()) and np.array_equal(got, y32.cpu().numpy())
        # a listed subset of the blocks (every other one): the other rows keep what they held
        nblk = (n + 255) // 256
        some = torch.arange(0, nblk, 2, dtype=torch.int32, device="cuda")
        ys = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        hp._capi.call("hpcla_spmv_patterns_f64_i32", d_rp.data_ptr(), c16.data_ptr(), h, d_nz.data_ptr(), d_x.data_ptr(),
                      ys.data_ptr(), n, nnz, base, some.data_ptr(), some.numel(), s)
        torch.cuda.synchronize()
        listed = (np.arange(n) // 256) % 2 == 0
        assert np.array_equal(ys.cpu().numpy(), np.where(listed, want, -7.0))
        # the dot form (x.y epilogue; needs x partitioned like the rows: square matrices here)
        work = torch.empty(lib.hpcla_spmv_dot_work_bytes(n) // 8 + 1, dtype=torch.float64, device="cuda")
        dots = []
        for fn, extra in (("hpcla_spmv_dist_dot_patterns_f64_i32", (c16.data_ptr(), h)),
                          ("hpcla_spmv_dist_dot_cols16_f64_i32", (c16.data_ptr(),)), ("hpcla_spmv_dist_dot_f64_i32", ())):
            yd, out = fresh(), torch.zeros(1, dtype=torch.float64, device="cuda")
            hp._capi.call(fn, None, None, d_rp.data_ptr(), d_cv.data_ptr(), *extra, d_nz.data_ptr(), d_x.data_ptr(), n,
                          yd.data_ptr(), n, nnz, base, None, 0, None, 0, out.data_ptr(), work.data_ptr(), s)
            torch.cuda.synchronize()
            assert np.array_equal(yd.cpu().numpy(), want), fn
            dots.append(out.cpu().numpy().copy())
        assert np.array_equal(dots[0].view(np.int64), dots[1].view(np.int64)) and \
            np.array_equal(dots[0].view(np.int64), dots[2].view(np.int64)), "x.y differs in bits between the forms"
        # a handle of another structure is refused, never launched
        assert lib.hpcla_spmv_patterns_f64_i32(d_rp.data_ptr(), c16.data_ptr(), h, d_nz.data_ptr(), d_x.data_ptr(), yp.data_ptr(),
                                               n, nnz - 1, base, None, 0, s) != 0
        return info
    finally:
        hp._capi.call("hpcla_block_patterns_destroy", h)


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("nx,ny", [(4096, 24), (300, 300), (1000, 200), (512, 64), (701, 301)])
def test_five_point_grids_on_the_raw_entry_points(hp, orc, nx, ny, base):
    """A 4096-wide slab (the headline's patterns), widths that are no multiple of 256 with a ragged last block, a width whose
    phases cycle, and 701 x 301, whose patterns overflow the table: the most frequent are kept, the rest stream."""
    n = nx * ny
    rows = orc.poisson2d_rows(nx, ny, 0, n)
    xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.5
    info = _raw_products(hp, orc, rows.rowptr, rows.colidx, rows.vals, xg, base)
    assert info is not None
    if (nx, ny) == (701, 301):
        assert info["patterned"] < info["candidates"], "both kinds of block in one launch"
    else:
        assert info["patterned"] == info["candidates"]


@pytest.mark.parametrize("base", [0, 1])
def test_small_seven_point_grid(hp, orc, base):
    n = 32 * 32 * 40
    rows = orc.poisson3d_rows(32, 32, 40, 0, n)
    xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.5
    info = _raw_products(hp, orc, rows.rowptr, rows.colidx, rows.vals, xg, base)
    assert info is not None and info["patterned"] == n // 256


def test_half_stencil_half_random_band(hp, orc):
    """Patterned and streamed blocks in ONE launch; the share of patterned blocks is what the model says."""
    rowptr, col, vals = band_with_random_half()
    xg = orc.fill_uniform(0, len(rowptr) - 1, orc.SEED_X) - 0.5
    info = _raw_products(hp, orc, rowptr, col, vals, xg, 0)
    assert info is not None and 64 <= info["patterned"] <= 128
    print(f"half stencil / half random band: {info['patterned']} of {info['candidates']} blocks read the table")


def test_one_column_off_is_a_pattern_of_its_own_and_a_collision_never_changes_a_result(hp, orc):
    """Two blocks with equal row lengths and one column that differs by 1 do not share a pattern.  With the columns left out
    of the hash (HPCLA_BLOCK_PATTERNS_WEAK_HASH) the two DO collide: the exact comparison must put the odd block back on
    the streamed form -- one pattern and one patterned block fewer -- and y keeps its bits."""
    (rowptr, col, vals), blk = one_column_off()
    xg = orc.fill_uniform(0, len(rowptr) - 1, orc.SEED_X) - 0.5
    keys = pattern_keys_np(rowptr, col)
    assert keys[blk] != keys[blk - 1]
    info = _raw_products(hp, orc, rowptr, col, vals, xg, 0)
    assert info == {"patterns": 4, "table_bytes": info["table_bytes"], "candidates": 40, "patterned": 40}
    weak = _raw_products(hp, orc, rowptr, col, vals, xg, 0, flags=hp._capi.BLOCK_PATTERNS_WEAK_HASH, expect_model=False)
    assert weak is not None and weak["patterns"] == 3 and weak["patterned"] == 39, weak


def test_more_patterns_than_the_cap(hp, orc):
    (rowptr, col, vals), odd = more_patterns_than_the_cap()
    xg = orc.fill_uniform(0, len(rowptr) - 1, orc.SEED_X) - 0.5
    info = _raw_products(hp, orc, rowptr, col, vals, xg, 0)
    assert info is not None and info["patterned"] < 420 and info["table_bytes"] <= 256 * 1024


def test_unstructured_matrix_gets_no_handle(hp, orc):
    rowptr, col, vals = unstructured()
    xg = orc.fill_uniform(0, len(rowptr) - 1, orc.SEED_X) - 0.5
    assert _raw_products(hp, orc, rowptr, col, vals, xg, 0) is None


@pytest.mark.parametrize("base", [0, 1])
def test_rows_longer_than_a_pass_and_empty_rows(hp, orc, base):
    rowptr, col, vals = long_and_empty_rows()
    xg = orc.fill_uniform(0, len(rowptr) - 1, orc.SEED_X) - 0.5
    info = _raw_products(hp, orc, rowptr, col, vals, xg, base)
    assert info is not None and info["patterned"] == info["candidates"]


@pytest.mark.parametrize("short", range(8))
def test_last_pass_against_the_end_of_nzval(hp, orc, short):
    rowptr, col, vals = tail_case(short)
    xg = orc.fill_uniform(0, len(rowptr) - 1, orc.SEED_X) - 0.5
    assert _raw_products(hp, orc, rowptr, col, vals, xg, 0) is not None


# ---- host layer -------------------------------------------------------------------------------------------------------
def _legs(hp, monkeypatch, make):
    """[(y, A, x, plan)] of make() -> (A, x) for the default plan, HPCLA_BLOCK_PATTERNS=0 and HPCLA_NARROW_COLS=0."""
    out = []
    for env in ({}, {"HPCLA_BLOCK_PATTERNS": "0"}, {"HPCLA_NARROW_COLS": "0"}):
        monkeypatch.delenv("HPCLA_BLOCK_PATTERNS", raising=False)
        monkeypatch.delenv("HPCLA_NARROW_COLS", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        A, x = make()
        plan = hp.get_vector_plan(A, x)
        y = A @ x
        hp.mul_(y, A, x)
        out.append((y.local_values().copy(), A, x, plan))
    monkeypatch.delenv("HPCLA_BLOCK_PATTERNS", raising=False)
    monkeypatch.delenv("HPCLA_NARROW_COLS", raising=False)
    assert len({id(o[3]) for o in out}) == 3, "each switch is part of the plan cache key"
    assert out[0][3].patterns is not None and out[0][3].cols16 is not None
    assert out[1][3].patterns is None and out[1][3].cols16 is not None
    assert out[2][3].patterns is None and out[2][3].cols16 is None
    return out


@pytest.mark.parametrize("nx,ny", [(300, 300), (1024, 1024), (255, 131)])
def test_poisson2d_host_layer_three_legs(hp, orc, gpu_backend_i32, monkeypatch, nx, ny):
    import torch
    n = nx * ny
    rows = orc.poisson2d_rows(nx, ny, 0, n)
    xg = orc.fill_uniform(0, n, orc.SEED_X)
    want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, xg)

    def make():
        return (hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, gpu_backend_i32),
                hp.HPCVector.from_global(xg, gpu_backend_i32))
    legs = _legs(hp, monkeypatch, make)
    for y, *_ in legs:
        assert np.array_equal(y, want)
    from hpcla_amd.sparse import block_patterns_info
    assert block_patterns_info(legs[0][3].patterns) == model_table(rows.rowptr, rows.colidx)
    dots = []
    for _, A, x, plan in legs:
        y, out = x.similar(), torch.zeros(1, dtype=torch.float64, device="cuda")
        hp.mul_dot_(y, A, x, out)
        torch.cuda.synchronize()
        assert np.array_equal(y.local_values(), want)
        dots.append(out.cpu().numpy().copy())
    assert np.array_equal(dots[0].view(np.int64), dots[1].view(np.int64)) and np.array_equal(dots[0].view(np.int64), dots[2].view(np.int64))
    hp.clear_plan_cache()


def test_unstructured_matrix_keeps_the_cols16_plan(hp, orc, gpu_backend_i32):
    rowptr, col, vals = unstructured()
    n = len(rowptr) - 1
    xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.5
    A = hp.HPCSparseMatrix_local(rowptr, col, vals, n, gpu_backend_i32)
    x = hp.HPCVector.from_global(xg, gpu_backend_i32)
    plan = hp.get_vector_plan(A, x)
    assert plan.cols16 is not None and plan.patterns is None
    assert np.array_equal((A @ x).local_values(), orc.spmv(rowptr.astype(np.int32), col.astype(np.int32), vals, xg))
    hp.clear_plan_cache()


def test_values_are_read_live_shared_plan_and_in_place_updates(hp, orc, gpu_backend_i32):
    """Two matrices of one structure share the plan and its table with their own values; nzval modified in place after the
    plan was built is seen by the next product."""
    N = 200
    n = N * N
    rows = orc.poisson2d_rows(N, N, 0, n)
    rp, cv = rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32)
    xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.4
    v2 = rows.vals * (1.0 + orc.fill_uniform(0, rows.nnz, 5))
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, gpu_backend_i32)
    B = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, v2, n, gpu_backend_i32)
    x = hp.HPCVector.from_global(xg, gpu_backend_i32)
    plan = hp.get_vector_plan(A, x)
    assert plan.patterns is not None and hp.get_vector_plan(B, x) is plan
    assert np.array_equal((A @ x).local_values(), orc.spmv(rp, cv, rows.vals, xg))
    assert np.array_equal((B @ x).local_values(), orc.spmv(rp, cv, v2, xg))
    A.nzval.mul_(-1.5)
    A.nzval[::3] += 0.125
    v3 = rows.vals * -1.5
    v3[::3] += 0.125
    assert np.array_equal((A @ x).local_values(), orc.spmv(rp, cv, v3, xg))
    assert np.array_equal((B @ x).local_values(), orc.spmv(rp, cv, v2, xg))
    hp.clear_plan_cache()


def test_non_finite_values_and_signed_zeros(hp, orc, gpu_backend_i32, monkeypatch):
    """Inf, NaN, -0.0 and a denormal among the values and in x through the pattern form: the bits (NaN payloads aside: NaN where
    the oracle has NaN) of the oracle and of the streamed form."""
    N = 160
    n = N * N
    rows = orc.poisson2d_rows(N, N, 0, n)
    vals = rows.vals.copy()
    xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.5
    vals[7] = np.inf
    vals[1001] = -np.inf
    vals[5000] = np.nan
    vals[9000:9005] = -0.0
    vals[12000] = 5e-324
    xg[300] = np.inf
    xg[4000] = np.nan
    xg[8000:8300] = -0.0
    xg[9999] = 2.5e-310
    with np.errstate(invalid="ignore", over="ignore"):
        want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), vals, xg)
    assert np.isnan(want).sum() > 2 and np.isinf(want).sum() > 1

    def make():
        return (hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, vals, n, gpu_backend_i32),
                hp.HPCVector.from_global(xg, gpu_backend_i32))
    for y, *_ in _legs(hp, monkeypatch, make):
        assert np.array_equal(np.isnan(y), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(y[ok].view(np.int64), want[ok].view(np.int64)), "bits differ (signed zeros included)"
    hp.clear_plan_cache()


@pytest.mark.parametrize("nranks", [2, 3])
def test_push_transport_ranks_interior_patterned_boundary_int32(nranks):
    """Ranks sharing the GPU under the push transport: interior blocks in the pattern form, boundary blocks on Int32, bits
    equal to the per-rank oracle pipeline and to HPCLA_BLOCK_PATTERNS=0; no exchange timed out."""
    from hpcla_amd.launch import spawn_ranks
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([RANK_WORKER], nranks, env_extra={"HPCLA_PUSH_TIMEOUT_S": "30"}, timeout=600,
                       forward_rank0_stdout=False) == 0


@pytest.mark.parametrize("mode", ["serial", "overlap", "push"])
def test_self_exchange_orderings_with_patterned_interior(mode):
    """The three orderings of the distributed step with a patterned interior, on a one-rank communicator that exchanges
    with itself (tests/_block_patterns_self_worker.py)."""
    env = dict(os.environ, HPCLA_FORCE_RCCL="1", HPCLA_HALO_MODE=mode, HPCLA_PUSH_TIMEOUT_S="30")
    env.pop("HPCLA_NARROW_COLS", None)
    env.pop("HPCLA_BLOCK_PATTERNS", None)
    out = subprocess.run([sys.executable, SELF_WORKER], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "patterned self-exchange OK" in out.stdout
