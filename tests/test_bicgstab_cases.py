"""CPU side of the BiCGStab solver: the public names, the C ABI tables, and the numpy restatement of the loop
(tests/_bicgstab_cases.py) against a direct solve, on the edge cases, and under four summation orders -- the measurement the
margins of tests/test_gpu_bicgstab.py rest on, re-run and printed here.

The first three tests need the feature (the public names, the new C entries).  The others exercise the restatement alone, as
the issue asks of this file: they check the yardstick of the GPU tests, not the library, and so pass without the feature."""
import math
import os
import re

import numpy as np
import pytest

from tests import _bicgstab_cases as bc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_bicgstab_work_bytes", "hpcla_bicg_dot_f64", "hpcla_bicg_s_f64", "hpcla_bicg_tts_f64", "hpcla_bicg_xr_f64",
               "hpcla_bicg_p_f64", "hpcla_bicgstab_iterations_f64_i32", "hpcla_bicgstab_iterations_f64_i64"]


@pytest.fixture(scope="module")
def orders(orc):
    """Every case x {jacobi, none} x the four summation orders, solved once: (x, iterations, status, history)."""
    out = {}
    for nx, ny in bc.SIZES:
        rowptr, colidx, vals, b = bc.convection_diffusion(orc, nx, ny)
        d = pc.host_diag(rowptr, colidx, vals)
        for name, dinv in (("jacobi", 1.0 / d), ("none", None)):
            for order, dot in bc.DOTS.items():
                out[(nx, ny), name, order] = bc.bicgstab(rowptr, colidx, vals, b, dinv=dinv, rtol=1e-8, dot=dot)
        out[(nx, ny), "case"] = (rowptr, colidx, vals, b)
    return out


def test_public_names_exist(hp):
    assert callable(hp.bicgstab) and hp.BiCGStabWorkspace
    assert hp.bicgstab.__module__.endswith("bicgstab")


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
    # three arrays of 2048 partials plus the 32-byte state
    assert lib.hpcla_bicgstab_work_bytes() == (3 * 2048 + 4) * 8
    sig = hp._capi._SIGNATURES
    assert len(sig["hpcla_bicgstab_iterations_f64_i32"]) == len(sig["hpcla_bicgstab_iterations_f64_i64"]) + 2


def test_argument_errors_without_a_gpu(hp):
    """Nulls, negative sizes, iteration / first_iter < 1 and misaligned vectors are refused on the host: nothing is launched
    (there is no GPU here to launch on)."""
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    buf = np.zeros(64)                                           # host memory: only ever looked at as an address
    a16 = buf.ctypes.data + (-buf.ctypes.data) % 16
    P, OFF = a16, a16 + 8                                        # an aligned and a misaligned non-null pointer
    # bicg_dot(comm, rhat, v, n, iter, rho, state, rv_out, work, stream)
    assert lib.hpcla_bicg_dot_f64(None, P, P, 4, 1, None, None, None, None, None) == INVALID         # null scalars
    assert lib.hpcla_bicg_dot_f64(None, None, None, 4, 1, P, P, P, P, None) == INVALID               # null vectors
    assert lib.hpcla_bicg_dot_f64(None, P, P, -1, 1, P, P, P, P, None) == INVALID
    assert lib.hpcla_bicg_dot_f64(None, P, P, 4, 0, P, P, P, P, None) == INVALID
    assert lib.hpcla_bicg_dot_f64(None, P, OFF, 4, 1, P, P, P, P, None) == INVALID
    # bicg_s(rho, rv, r, v, dinv, s, sh, n, iter, state, stream)
    assert lib.hpcla_bicg_s_f64(None, None, P, P, None, P, None, 4, 1, None, None) == INVALID
    assert lib.hpcla_bicg_s_f64(P, P, None, None, None, None, None, 4, 1, P, None) == INVALID
    assert lib.hpcla_bicg_s_f64(P, P, P, P, P, P, None, 4, 1, P, None) == INVALID                    # dinv without sh
    assert lib.hpcla_bicg_s_f64(P, P, P, P, None, P, None, -1, 1, P, None) == INVALID
    assert lib.hpcla_bicg_s_f64(P, P, P, P, None, P, None, 4, 0, P, None) == INVALID
    assert lib.hpcla_bicg_s_f64(P, P, P, OFF, None, P, None, 4, 1, P, None) == INVALID
    # bicg_tts(comm, t, s, n, iter, state, triple_out, work, stream)
    assert lib.hpcla_bicg_tts_f64(None, P, P, 4, 1, None, None, None, None) == INVALID
    assert lib.hpcla_bicg_tts_f64(None, None, None, 4, 1, P, P, P, None) == INVALID
    assert lib.hpcla_bicg_tts_f64(None, P, P, -1, 1, P, P, P, None) == INVALID
    assert lib.hpcla_bicg_tts_f64(None, P, P, 4, 0, P, P, P, None) == INVALID
    assert lib.hpcla_bicg_tts_f64(None, OFF, P, 4, 1, P, P, P, None) == INVALID
    # bicg_xr(comm, rho, rv, triple, ph, sh, s, t, rhat, x, r, n, iter, state, pair_out, work, stream)
    assert lib.hpcla_bicg_xr_f64(None, None, None, None, P, None, P, P, P, P, P, 4, 1, None, None, None, None) == INVALID
    assert lib.hpcla_bicg_xr_f64(None, P, P, P, None, None, None, None, None, None, None, 4, 1, P, P, P, None) == INVALID
    assert lib.hpcla_bicg_xr_f64(None, P, P, P, P, None, P, P, P, P, P, -1, 1, P, P, P, None) == INVALID
    assert lib.hpcla_bicg_xr_f64(None, P, P, P, P, None, P, P, P, P, P, 4, 0, P, P, P, None) == INVALID
    assert lib.hpcla_bicg_xr_f64(None, P, P, P, P, OFF, P, P, P, P, P, 4, 1, P, P, P, None) == INVALID
    # bicg_p(rho_new, rho, rv, triple, r, v, dinv, p, ph, n, iter, state, stream)
    assert lib.hpcla_bicg_p_f64(None, None, None, None, P, P, None, P, None, 4, 1, None, None) == INVALID
    assert lib.hpcla_bicg_p_f64(P, P, P, P, None, None, None, None, None, 4, 1, P, None) == INVALID
    assert lib.hpcla_bicg_p_f64(P, P, P, P, P, P, None, P, None, -1, 1, P, None) == INVALID
    assert lib.hpcla_bicg_p_f64(P, P, P, P, P, P, None, P, None, 4, 0, P, None) == INVALID
    assert lib.hpcla_bicg_p_f64(P, P, P, P, P, P, None, OFF, None, 4, 1, P, None) == INVALID
    # the loop: (plan, comm, rowptr, colval, [cols16, patterns,] nzval, nrows, nnz, base, interior, n, boundary, n, dinv,
    #            x, r, rhat, p, ph, v, s, sh, t, hist, scal, work, first_iter, iters, stream)
    for fn, lead in ((lib.hpcla_bicgstab_iterations_f64_i32, 7), (lib.hpcla_bicgstab_iterations_f64_i64, 5)):
        head = [None] * lead
        mid = [0, 0, None, 0, None, 0]
        vecs = [None, P, P, P, P, None, P, P, None, P]             # dinv, x, r, rhat, p, ph, v, s, sh, t
        assert fn(*head, 4, *mid, *([None] * 13), 1, 1, None) == INVALID                          # nulls
        assert fn(*head, 4, *mid, *vecs, None, None, None, 1, 1, None) == INVALID                 # null history / scalars / work
        assert fn(*head, -1, *mid, *vecs, P, P, P, 1, 1, None) == INVALID                         # negative size
        assert fn(*head, 4, *mid, *vecs, P, P, P, 1, -1, None) == INVALID                         # negative count
        assert fn(*head, 4, *mid, *vecs, P, P, P, 0, 1, None) == INVALID                          # first_iter < 1
        bad = list(vecs)
        bad[1] = OFF
        assert fn(*head, 4, *mid, *bad, P, P, P, 1, 1, None) == INVALID                           # misaligned x
        bad = list(vecs)
        bad[0] = P
        assert fn(*head, 4, *mid, *bad, P, P, P, 1, 1, None) == INVALID                           # dinv without ph / sh


def test_cases_are_not_symmetric(orc):
    for nx, ny in bc.SIZES:
        rowptr, colidx, vals, b = bc.convection_diffusion(orc, nx, ny)
        dense = bc.dense_of(rowptr, colidx, vals)
        assert not np.array_equal(dense, dense.T), (nx, ny)
        assert np.array_equal((dense != 0), (dense != 0).T)                    # the pattern is symmetric, the values are not
        d = pc.host_diag(rowptr, colidx, vals)
        assert np.array_equal(d, np.diag(dense)) and np.abs(d).min() > 0
    assert len(b) == 1023


def test_restatement_agrees_with_a_direct_solve(orc, orders):
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    for nx, ny in bc.SIZES:
        rowptr, colidx, vals, b = orders[(nx, ny), "case"]
        n = len(b)
        x_ref = spsolve(sp.csr_matrix((vals, colidx, rowptr), shape=(n, n)).tocsc(), b)
        for name in ("jacobi", "none"):
            x, its, status, h = orders[(nx, ny), name, "np.dot"]
            assert status == "converged" and len(h) == its + 1
            true = np.linalg.norm(b - pc.matvec(rowptr, colidx, vals, x)) / np.linalg.norm(b)
            err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
            print(f"{nx}x{ny} {name}: iterations {its}, true relative residual {true:.3e}, against spsolve {err:.3e}")
            assert err <= 1e-7, (nx, ny, name, err)
            assert true <= 2e-8, (nx, ny, name, true)
        # a start vector changes the path, not the answer
        d = pc.host_diag(rowptr, colidx, vals)
        x, its, status, _ = bc.bicgstab(rowptr, colidx, vals, b, dinv=1.0 / d, x0=np.full(n, 1e-3))
        assert status == "converged" and np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref) <= 1e-7


def test_spread_across_summation_orders_is_within_the_margins_of_the_gpu_tests(orders):
    """The device sums in yet another order.  What the order alone does, measured here with four orders on the CPU, bounds what
    the GPU tests may ask: iteration counts with Jacobi (+-2 there), 2 * jacobi <= none, the true residual (2e-8 there), and
    the first HEAD history entries (HIST_RTOL there).  BiCGStab amplifies rounding much faster than CG: the same spread is
    printed for entry 13, which the GPU tests therefore do not compare."""
    for size in bc.SIZES:
        rowptr, colidx, vals, b = orders[size, "case"]
        counts = {name: [orders[size, name, o][1] for o in bc.DOTS] for name in ("jacobi", "none")}
        for name in ("jacobi", "none"):
            for o in bc.DOTS:
                x, its, status, h = orders[size, name, o]
                assert status == "converged"
                true = np.linalg.norm(b - pc.matvec(rowptr, colidx, vals, x)) / np.linalg.norm(b)
                assert true <= 2e-8, (size, name, o, true)

        def spread(name, k):
            col = [orders[size, name, o][3][k] for o in bc.DOTS]
            return (max(col) - min(col)) / min(col)
        head = max(spread(name, k) for k in range(bc.HEAD) for name in ("jacobi", "none"))
        at13 = max(spread(name, 13) for name in ("jacobi", "none"))
        ratio = min(n_ / (2.0 * j_) for j_, n_ in zip(counts["jacobi"], counts["none"]))
        print(f"{size}: iterations jacobi {counts['jacobi']}, none {counts['none']} (none / 2 jacobi >= {ratio:.2f}); history "
              f"spread (jacobi and none) over the first {bc.HEAD} entries {head:.2e}, at entry 13 {at13:.2e}")
        assert max(counts["jacobi"]) - min(counts["jacobi"]) <= 2
        assert all(2 * j_ <= n_ for j_, n_ in zip(counts["jacobi"], counts["none"])), counts
        assert head <= bc.HIST_RTOL


def test_restatement_on_the_freeze_and_breakdown_cases(orc):
    rowptr, colidx, d, b = pc.diagonal_case(orc)
    x, its, status, h = bc.bicgstab(rowptr, colidx, d, b, dinv=1.0 / d, rtol=1e-8, maxiter=50)
    assert (its, status, len(h)) == (1, "converged", 2)
    assert np.all(np.abs(x - b / d) <= 4 * np.spacing(np.abs(b / d)))
    # identity: s is exactly 0 at the first half step, also with thr = 0; carried on it would be 0 / 0
    eye = pc.diag_matrix(np.ones(5))
    bi = orc.fill_uniform(0, 5, pc.SEED_RHS)
    x, its, status, h = bc.bicgstab(*eye, bi, rtol=0.0, atol=0.0)
    assert (its, status) == (1, "converged") and h[1] == 0.0 and np.array_equal(pc.bits(x), pc.bits(bi))
    # -I: CG breaks down on it, BiCGStab converges at the first half step
    x, its, status, h = bc.bicgstab(*pc.diag_matrix(-np.ones(5)), bi)
    assert (its, status, len(h)) == (1, "converged", 2) and np.array_equal(x, -bi)
    # breakdown in iteration 1: rhat.v = 0
    x, its, status, h = bc.bicgstab(*bc.ROT, bc.ROT_B)
    assert (its, status, h) == (0, "breakdown", [1.0]) and not x.any()
    # breakdown in iteration 2 after one full step
    x, its, status, h = bc.bicgstab(*bc.SINGULAR, bc.SINGULAR_B)
    assert (its, status) == (1, "breakdown") and np.array_equal(x, [1.0, 3.0]) and h == [math.sqrt(2.0), 1.0]
    # b = 0
    x, its, status, h = bc.bicgstab(*eye, np.zeros(5))
    assert (its, status, h) == (0, "converged", [0.0]) and not x.any()


def test_half_step_case_stops_at_gate_s_in_every_order(orc):
    """The case the rank test uses to see a half-step history entry: every summation order stops at gate S of iteration 8,
    the last entry is ||s_8|| (not ||r_8||), it meets the stop rule, and sqrt(2) times it would not -- so a sum of squares
    added up once more over two ranks cannot pass.  The spread of the whole history bounds what the GPU tests may ask."""
    rowptr, colidx, vals, b = bc.convection_diffusion(orc, *bc.HALF_SIZE)
    d = pc.host_diag(rowptr, colidx, vals)
    bnorm = math.sqrt(float(np.dot(b, b)))
    runs = [bc.bicgstab(rowptr, colidx, vals, b, dinv=1.0 / d, rtol=bc.HALF_RTOL, dot=dot) for dot in bc.DOTS.values()]
    full = bc.bicgstab(rowptr, colidx, vals, b, dinv=1.0 / d, rtol=0.0, atol=0.0, maxiter=bc.HALF_ITERATIONS)
    for x, its, status, h in runs:
        assert (its, status, len(h)) == (bc.HALF_ITERATIONS, "converged", bc.HALF_ITERATIONS + 1)
        assert 0.0 < h[-1] <= bc.HALF_RTOL * bnorm < math.sqrt(2.0) * h[-1]
    assert runs[0][3][:-1] == full[3][:-1] and runs[0][3][-1] != full[3][-1]           # ||s_8||, not ||r_8||
    spread = max((max(r[3][k] for r in runs) - min(r[3][k] for r in runs)) / min(r[3][k] for r in runs)
                 for k in range(bc.HALF_ITERATIONS + 1))
    print(f"half-step case: ||s_8|| / |b| = {runs[0][3][-1] / bnorm:.4f}, history spread across the orders {spread:.2e}")
    assert 20 * spread <= bc.HALF_HIST_RTOL


def test_head_spread_at_the_large_size(orc):
    """65 x 63 (4095 rows, two reduction workgroups on the device): the first HEAD entries under the four summation orders.
    HIST_RTOL, which tests/test_gpu_bicgstab.py asks there, must be at least 10 times the spread (measured: 3.3e-14 with Jacobi,
    4.7e-15 without: 30 times)."""
    rowptr, colidx, vals, b = bc.convection_diffusion(orc, *bc.LARGE_SIZE)
    assert len(b) == 4095
    d = pc.host_diag(rowptr, colidx, vals)
    for name, dinv in (("jacobi", 1.0 / d), ("none", None)):
        hists = [bc.bicgstab(rowptr, colidx, vals, b, dinv=dinv, rtol=0.0, atol=0.0, maxiter=8, dot=dot)[3] for dot in bc.DOTS.values()]
        spread = max((max(col) - min(col)) / min(col) for col in zip(*[h[:bc.HEAD] for h in hists]))
        print(f"{bc.LARGE_SIZE} {name}: spread over the first {bc.HEAD} history entries {spread:.2e}")
        assert pc.LARGE_MARGIN_FACTOR * spread <= bc.HIST_RTOL
