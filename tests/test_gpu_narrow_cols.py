"""The plan's 16-bit block-relative column copy (VectorPlan.cols16, csrc/spmv.hip IndexPolicy<Cols16>): the SpMV streams
10 instead of 12 bytes per stored entry wherever a structure allows it, and y keeps its bits.

Every case is compared with ``np.array_equal`` against the oracle AND against the same product on the Int32 column
stream (``HPCLA_NARROW_COLS=0`` through the host layer, ``hpcla_spmv_csr_f64_i32`` on the raw entry points), and asserts
which path ran.  The expected eligibility of a case is computed here in numpy (``eligible_np``), independently of the
device encoder.  Arrays handed to the raw entry points END inside guarded buffers (NaN values, a far column), so an entry
read past the end poisons a row instead of passing unnoticed.  The generators and ``eligible_np`` are checked on the CPU
in tests/test_narrow_cols_cases.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _narrow_cols_cases import (banded_edges, eligible_np, long_and_empty_rows, tail_case)  # noqa: E402

pytestmark = pytest.mark.gpu

RANK_WORKER = os.path.join(ROOT, "tests", "_narrow_cols_rank_worker.py")
SELF_WORKER = os.path.join(ROOT, "tests", "_narrow_cols_self_worker.py")
GUARD = 64


def _raw_products(hp, orc, rowptr, col, vals, xg, base, expect):
    """Encode + multiply through the raw entry points with index_base `base`; returns after asserting the bits."""
    import torch
    lib = hp._capi.load()
    s = torch.cuda.current_stream().cuda_stream
    n, nnz = len(rowptr) - 1, len(col)
    assert eligible_np(rowptr, col, n) == expect
    want = orc.spmv(rowptr.astype(np.int32), col.astype(np.int32), vals, xg)
    d_rp = torch.from_numpy((rowptr + base).astype(np.int32)).cuda()
    # colval / nzval END inside guarded buffers; x sits between NaN guards
    cbuf = torch.full((nnz + GUARD,), n - 1 + base, dtype=torch.int32, device="cuda")
    cbuf[:nnz] = torch.from_numpy((col + base).astype(np.int32)).cuda()
    vbuf = torch.full((nnz + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    vbuf[:nnz] = torch.from_numpy(vals).cuda()
    xbuf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    xbuf[GUARD:GUARD + n] = torch.from_numpy(xg).cuda()
    d_cv, d_nz, d_x = cbuf[:nnz], vbuf[:nnz], xbuf[GUARD:GUARD + n]
    y32 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_spmv_csr_f64_i32", d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), d_x.data_ptr(), y32.data_ptr(),
                  n, nnz, base, s)
    torch.cuda.synchronize()
    assert np.array_equal(y32.cpu().numpy(), want), "Int32 column stream differs from the oracle"
    padded = lib.hpcla_cols16_padded_len(nnz)
    assert padded % 8 == 0 and padded >= nnz + 8
    # the library's own array is exactly `padded` long; behind it a guard of far deltas
    c16buf = torch.full((padded + GUARD,), 32767, dtype=torch.int16, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    hp._capi.call("hpcla_cols16_encode_i32", d_rp.data_ptr(), d_cv.data_ptr(), n, nnz, n, base, None, 0, c16buf.data_ptr(),
                  bad.data_ptr(), s)
    torch.cuda.synchronize()
    assert bool(bad.item() == 0) == expect, "the device encoder and the numpy rule disagree on eligibility"
    assert bool((c16buf[padded:] == 32767).all()), "the encoder wrote behind the padded length"
    if not expect:
        return
    assert bool((c16buf[nnz:padded] == 0).all()), "the pad is not zeroed"
    blk_of_entry = np.repeat(np.arange(n) // 256, np.diff(rowptr))
    assert np.array_equal(c16buf[:nnz].cpu().numpy().astype(np.int64), col - 256 * blk_of_entry)
    y16 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    for _ in range(2):
        hp._capi.call("hpcla_spmv_cols16_f64_i32", d_rp.data_ptr(), c16buf.data_ptr(), d_nz.data_ptr(), d_x.data_ptr(),
                      y16.data_ptr(), n, nnz, base, None, 0, s)
    torch.cuda.synchronize()
    got = y16.cpu().numpy()
    assert np.array_equal(got, want), f"narrow path differs from the oracle in {int((got != want).sum())} rows"
    assert np.array_equal(got, y32.cpu().numpy())


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("which", ["edges", "past_low", "past_high"])
def test_window_edges_on_the_raw_entry_points(hp, orc, which, base):
    """A column at r0 - 32768 and one at r0 + 32767 in the same block: eligible.  One past either edge: not eligible (the
    encoder says so; the Int32 product is the oracle's)."""
    rowptr, col, vals = banded_edges(which)
    xg = orc.fill_uniform(0, len(rowptr) - 1, orc.SEED_X) - 0.5
    _raw_products(hp, orc, rowptr, col, vals, xg, base, expect=(which == "edges"))


@pytest.mark.parametrize("base", [0, 1])
def test_rows_longer_than_a_pass_and_empty_rows(hp, orc, base):
    """Rows of 465 ... 3000 entries inside the window (the whole-pass branch: one row owns complete passes), rows of exactly
    one pass, empty rows and empty waves between them."""
    rowptr, col, vals = long_and_empty_rows()
    assert np.diff(rowptr).max() > 2 * 464 and (np.diff(rowptr) == 0).sum() > 300
    xg = orc.fill_uniform(0, len(rowptr) - 1, orc.SEED_X) - 0.5
    _raw_products(hp, orc, rowptr, col, vals, xg, base, expect=True)


@pytest.mark.parametrize("short", range(8))
def test_last_pass_against_the_end_of_nzval(hp, orc, short):
    """short = 0: the launch's last pass ends exactly at nnz, a multiple of 8 (vector loads right up to the end of the caller's
    nzval); 1 ... 7: it ends that far short of a multiple of 8 (staged entry by entry; only the 16-bit copy is padded)."""
    rowptr, col, vals = tail_case(short)
    assert (8 - len(col) % 8) % 8 == short
    xg = orc.fill_uniform(0, len(rowptr) - 1, orc.SEED_X) - 0.5
    _raw_products(hp, orc, rowptr, col, vals, xg, 0, expect=True)


def _both_paths(hp, monkeypatch, make, expect_narrow):
    """(y, plan) of make() -> (A, x) on the default path and under HPCLA_NARROW_COLS=0."""
    out = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("HPCLA_NARROW_COLS", "0")
        else:
            monkeypatch.delenv("HPCLA_NARROW_COLS", raising=False)
        A, x = make()
        plan = hp.get_vector_plan(A, x)
        assert (plan.cols16 is not None) == (expect_narrow and not off)
        if plan.cols16 is not None:
            import torch
            assert plan.cols16.dtype == torch.int16 and plan.cols16.numel() == hp._capi.load().hpcla_cols16_padded_len(A.nnz)
        y = A @ x
        hp.mul_(y, A, x)
        out.append((y.local_values().copy(), A, x, plan))
    monkeypatch.delenv("HPCLA_NARROW_COLS", raising=False)
    assert out[0][3] is not out[1][3], "the switch is part of the plan cache key"
    return out


@pytest.mark.parametrize("nx,ny", [(64, 64), (300, 300), (1024, 1024), (701, 301), (255, 131), (93, 1001)])
def test_poisson2d_host_layer_both_paths(hp, orc, gpu_backend_i32, monkeypatch, nx, ny):
    """The square grids N = 64, 300, 1024 (300^2 rows: no multiple of 256; their nnz = 5 N^2 - 4 N happens to be a multiple of
    8 for all three) and three rectangles whose row counts are no multiples of 64 and whose nnz % 8 != 0, so that the last
    pass of the launch is the one staged entry by entry."""
    n = nx * ny
    rows = orc.poisson2d_rows(nx, ny, 0, n)
    if nx != ny:
        assert rows.nnz % 8 != 0 and n % 64 != 0
    xg = orc.fill_uniform(0, n, orc.SEED_X)
    want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, xg)
    assert eligible_np(rows.rowptr, rows.colidx, n)

    def make():
        return (hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, gpu_backend_i32),
                hp.HPCVector.from_global(xg, gpu_backend_i32))
    (y_on, *_), (y_off, *_) = _both_paths(hp, monkeypatch, make, True)
    assert np.array_equal(y_on, want) and np.array_equal(y_off, want)
    hp.clear_plan_cache()


def test_mul_dot_same_bits_on_both_paths(hp, orc, gpu_backend_i32, monkeypatch):
    import torch
    N = 300
    n = N * N
    rows = orc.poisson2d_rows(N, N, 0, n)
    xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.3
    want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, xg)

    def make():
        return (hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, gpu_backend_i32),
                hp.HPCVector.from_global(xg, gpu_backend_i32))
    res = []
    for _, A, x, plan in _both_paths(hp, monkeypatch, make, True):
        y = x.similar()
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        hp.mul_dot_(y, A, x, out)
        torch.cuda.synchronize()
        res.append((y.local_values().copy(), out.cpu().numpy().copy()))
    assert np.array_equal(res[0][0], want) and np.array_equal(res[1][0], want)
    assert np.array_equal(res[0][1].view(np.int64), res[1][1].view(np.int64)), "p.Ap differs in bits between the paths"
    hp.clear_plan_cache()


def test_int64_matrix_narrowed_plan_is_eligible_wide_plan_is_not(hp, orc, gpu_backend_i64, monkeypatch):
    N = 300
    n = N * N
    rows = orc.poisson2d_rows(N, N, 0, n)
    xg = orc.fill_uniform(0, n, orc.SEED_X)
    want = orc.spmv(rows.rowptr.astype(np.int64), rows.colidx.astype(np.int64), rows.vals, xg)
    for wide in (False, True):
        monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if wide else "1")
        A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, gpu_backend_i64)
        x = hp.HPCVector.from_global(xg, gpu_backend_i64)
        plan = hp.get_vector_plan(A, x)
        assert plan.is_i64 == wide and plan.narrowed == (not wide)
        assert (plan.cols16 is not None) == (not wide)
        assert np.array_equal((A @ x).local_values(), want)
    hp.clear_plan_cache()


def test_seven_point_slab_512x512_is_not_eligible_and_unchanged(hp, orc, gpu_backend_i32):
    """+-262 144 between planes does not fit 16 bits: the plan keeps the Int32 column stream."""
    mx, my, mz = 512, 512, 8
    n = mx * my * mz
    rows = orc.poisson3d_rows(mx, my, mz, 0, n)
    assert not eligible_np(rows.rowptr, rows.colidx, n)
    A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, gpu_backend_i32)
    xg = orc.fill_uniform(0, n, orc.SEED_X)
    x = hp.HPCVector.from_global(xg, gpu_backend_i32)
    assert hp.get_vector_plan(A, x).cols16 is None
    want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, xg)
    assert np.array_equal((A @ x).local_values(), want)
    hp.clear_plan_cache()


def test_values_are_read_live_shared_plan_and_in_place_updates(hp, orc, gpu_backend_i32):
    """Two matrices of one structure share the plan (and its 16-bit columns) with their own values; nzval modified in place
    between two products is seen by the second -- the property the packed copy lacks."""
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
    assert plan.cols16 is not None and hp.get_vector_plan(B, x) is plan
    assert np.array_equal((A @ x).local_values(), orc.spmv(rp, cv, rows.vals, xg))
    assert np.array_equal((B @ x).local_values(), orc.spmv(rp, cv, v2, xg))
    A.nzval.mul_(-1.5)
    A.nzval[::3] += 0.125
    v3 = rows.vals * -1.5
    v3[::3] += 0.125
    assert np.array_equal((A @ x).local_values(), orc.spmv(rp, cv, v3, xg))
    assert np.array_equal((B @ x).local_values(), orc.spmv(rp, cv, v2, xg))
    hp.clear_plan_cache()


@pytest.mark.parametrize("nranks", [2, 3])
def test_push_transport_ranks_interior_narrow_boundary_int32(nranks):
    """Ranks sharing the GPU under the push transport: interior blocks on 16-bit columns, boundary blocks on Int32, bits equal
    to the per-rank oracle pipeline and to HPCLA_NARROW_COLS=0; no exchange timed out (tests/_narrow_cols_rank_worker.py)."""
    from hpcla_amd.launch import spawn_ranks
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([RANK_WORKER], nranks, env_extra={"HPCLA_PUSH_TIMEOUT_S": "30"}, timeout=600,
                       forward_rank0_stdout=False) == 0


@pytest.mark.parametrize("mode", ["serial", "overlap", "push"])
def test_self_exchange_orderings_with_narrow_interior(mode):
    """The three orderings of the distributed step with a 16-bit interior, on a one-rank communicator that exchanges with
    itself (tests/_narrow_cols_self_worker.py; the pattern of test_rccl_halo_self_exchange_subprocess)."""
    env = dict(os.environ, HPCLA_FORCE_RCCL="1", HPCLA_HALO_MODE=mode, HPCLA_PUSH_TIMEOUT_S="30")
    env.pop("HPCLA_NARROW_COLS", None)
    out = subprocess.run([sys.executable, SELF_WORKER], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "narrow self-exchange OK" in out.stdout
