"""CPU side of the converging CG solver: the public names, the C ABI tables, and the numpy restatement of the loop
(tests/_pcg_cases.py) against the oracle's textbook CG and on the shared cases."""
import math
import os
import re

import numpy as np

from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_sparse_diag_f64_i32", "hpcla_sparse_diag_f64_i64", "hpcla_pcg_residual_f64", "hpcla_pcg_direction_f64",
               "hpcla_pcg_iterations_f64_i32", "hpcla_pcg_iterations_f64_i64", "hpcla_pcg_work_bytes"]


def test_public_names_exist(hp):
    assert callable(hp.cg) and callable(hp.diag)
    info = hp.CGInfo(True, 3, "converged", [1.0, 0.5, 0.1, 0.0])
    assert info.converged and info.iterations == 3 and info.status == "converged" and len(info.residual_norms) == 4
    assert hp.PCGWorkspace


def test_header_declares_the_new_entries_and_ctypes_binds_them(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in hp._capi.EXPORTED_SYMBOLS, name
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hpcla_rocm.h"
        nargs = 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1
        assert nargs == len(hp._capi._SIGNATURES[name]), (name, nargs)
    lib = hp._capi.load()
    # two arrays of 2048 partials plus the 32-byte state
    assert lib.hpcla_pcg_work_bytes() == (2 * 2048 + 4) * 8
    # the Int32 loop takes the plan's 16-bit columns and pattern table on top of the Int64 one's arguments
    assert len(hp._capi._SIGNATURES["hpcla_pcg_iterations_f64_i32"]) == len(hp._capi._SIGNATURES["hpcla_pcg_iterations_f64_i64"]) + 2


def test_argument_errors_without_a_gpu(hp):
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    assert lib.hpcla_sparse_diag_f64_i32(None, None, None, -1, 0, 0, None, 0, 0, 0, None, None) == INVALID
    assert lib.hpcla_sparse_diag_f64_i64(None, None, None, 4, 0, 0, None, 0, 0, 0, None, None) == INVALID      # null arrays
    assert lib.hpcla_sparse_diag_f64_i32(None, None, None, 4, 0, 2, None, 0, 0, 0, None, None) == INVALID      # index_base
    assert lib.hpcla_sparse_diag_f64_i32(None, None, None, 0, 0, 0, None, 0, 0, 0, None, None) == 0            # zero sizes
    assert lib.hpcla_pcg_residual_f64(None, None, None, None, None, None, 4, 1, None, None, None, None) == INVALID
    assert lib.hpcla_pcg_direction_f64(None, None, None, None, None, None, None, None, -1, 1, None, None) == INVALID
    assert lib.hpcla_pcg_iterations_f64_i32(*([None] * 7), 4, 0, 0, None, 0, None, 0, *([None] * 9), 1, -1, None) == INVALID
    assert lib.hpcla_pcg_iterations_f64_i64(*([None] * 5), 4, 0, 0, None, 0, None, 0, *([None] * 9), 0, 1, None) == INVALID


def test_restatement_without_preconditioner_is_the_oracles_cg(orc):
    rowptr, colidx, vals, b = pc.scaled_poisson(orc, 24, 20)
    ones = np.ones(len(b))
    col_indices, colval = np.arange(len(b)), colidx                     # every column occurs: the compression is the identity
    _, h_ref = orc.cg(rowptr.astype(np.int32), colval.astype(np.int32), vals, b, 13)
    for dinv in (None, ones):
        _, its, status, h = pc.pcg(rowptr, colidx, vals, b, dinv=dinv, rtol=0.0, atol=0.0, maxiter=13)
        assert (its, status, len(h)) == (13, "maxiter", 14)
        dev = max(abs(a - c) / c for a, c in zip(h, h_ref))
        print(f"restatement vs orc.cg, 24x20, 13 iterations: max relative deviation {dev:.2e}")
        assert dev <= pc.CG_RTOL, dev


def test_restatement_converges_on_the_scaled_cases(orc):
    for nx, ny in pc.SIZES:
        rowptr, colidx, vals, b = pc.scaled_poisson(orc, nx, ny)
        # exactly symmetric
        n = len(b)
        dense = np.zeros((n, n))
        dense[np.repeat(np.arange(n), np.diff(rowptr)), colidx] = vals
        assert np.array_equal(dense, dense.T)
        d = pc.host_diag(rowptr, colidx, vals)
        assert np.array_equal(d, np.diag(dense)) and d.min() > 0
        counts = {}
        for name, dinv in (("jacobi", 1.0 / d), ("none", None)):
            x, its, status, h = pc.pcg(rowptr, colidx, vals, b, dinv=dinv, rtol=1e-8)
            assert status == "converged" and len(h) == its + 1
            true = np.linalg.norm(b - pc.matvec(rowptr, colidx, vals, x)) / np.linalg.norm(b)
            assert true <= 2e-8, (nx, ny, name, true)
            counts[name] = its
        print(f"{nx}x{ny}: iterations jacobi {counts['jacobi']}, unpreconditioned {counts['none']}")
        assert 2 * counts["jacobi"] <= counts["none"], counts


def test_restatement_on_the_freeze_and_breakdown_cases(orc):
    rowptr, colidx, d, b = pc.diagonal_case(orc)
    x, its, status, h = pc.pcg(rowptr, colidx, d, b, dinv=1.0 / d, rtol=1e-8, maxiter=50)
    assert (its, status, len(h)) == (1, "converged", 2)
    assert np.all(np.abs(x - b / d) <= 4 * np.spacing(np.abs(b / d)))
    # what the freeze is for: carried on (rtol = 0) the recurrence runs on rounding noise until rr is exactly 0
    _, its0, status0, h0 = pc.pcg(rowptr, colidx, d, b, dinv=1.0 / d, rtol=0.0, maxiter=50)
    print(f"diagonal case carried on with rtol = 0: {status0} at {its0}, last norms {h0[-3:]}")
    assert h0[1] <= 1e-14 * h0[0]
    # identity: r is exactly 0 after one iteration
    eye = pc.diag_matrix(np.ones(5))
    bi = orc.fill_uniform(0, 5, pc.SEED_RHS)
    x, its, status, h = pc.pcg(*eye, bi, rtol=0.0, atol=0.0)
    assert (its, status) == (1, "converged") and h[1] == 0.0 and np.array_equal(pc.bits(x), pc.bits(bi))
    # breakdown
    x, its, status, _ = pc.pcg(*pc.diag_matrix(-np.ones(5)), bi)
    assert (its, status) == (0, "breakdown") and not x.any()
    x, its, status, _ = pc.pcg(*pc.diag_matrix([1.0, -1.0, 2.0, 3.0]), np.array([1.0, 2.0, 1.0, 1.0]))
    assert (its, status) == (1, "breakdown") and np.all(np.isfinite(x)) and x.any()
    # b = 0
    x, its, status, h = pc.pcg(*eye, np.zeros(5))
    assert (its, status, h) == (0, "converged", [0.0]) and not x.any()
    assert math.isfinite(h[0])


def test_head_spread_at_the_large_size(orc):
    """65 x 63 (4095 rows, two reduction workgroups on the device): the first HEAD entries under the four summation orders of
    ``_bicgstab_cases.DOTS``.  CG_RTOL, which tests/test_gpu_pcg.py asks there, must be at least LARGE_MARGIN_FACTOR = 10 times the
    spread (measured: 6.9e-15 with Jacobi, 2.2e-14 without: 45 times)."""
    from tests import _bicgstab_cases as bc
    rowptr, colidx, vals, b = pc.scaled_poisson(orc, *pc.LARGE_SIZE)
    assert len(b) == 4095
    d = pc.host_diag(rowptr, colidx, vals)
    for name, dinv in (("jacobi", 1.0 / d), ("none", None)):
        hists = [pc.pcg(rowptr, colidx, vals, b, dinv=dinv, rtol=0.0, atol=0.0, maxiter=pc.HEAD, dot=dot)[3] for dot in bc.DOTS.values()]
        spread = max((max(col) - min(col)) / min(col) for col in zip(*[h[:pc.HEAD] for h in hists]))
        print(f"{pc.LARGE_SIZE} {name}: spread over the first {pc.HEAD} history entries {spread:.2e}")
        assert pc.LARGE_MARGIN_FACTOR * spread <= pc.CG_RTOL
