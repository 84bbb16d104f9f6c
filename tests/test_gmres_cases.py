"""CPU side of the restarted GMRES solver: the public names, the C ABI tables, the host's bookkeeping of the open cycle, and the
numpy restatement of the loop (tests/_gmres_cases.py) against a direct solve, on the exact cases, and under four summation
orders -- the measurement the margins of tests/test_gpu_gmres.py rest on, re-run and printed here.

The first four tests exercise the feature itself (the public names, the new C entries, the host's bookkeeping).  The others
exercise the restatement alone: they check the yardstick of the GPU tests, which means nothing without the solver it restates,
so the whole file asks for ``hp.gmres`` first."""
import math
import os
import re

import numpy as np
import pytest

from tests import _bicgstab_cases as bc
from tests import _gmres_cases as gc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_gmres_work_bytes", "hpcla_gmres_small_offset", "hpcla_gmres_dots_f64", "hpcla_gmres_update_f64",
               "hpcla_gmres_next_f64", "hpcla_gmres_solve_f64", "hpcla_gmres_xupdate_f64", "hpcla_gmres_residual_f64",
               "hpcla_gmres_finish_f64", "hpcla_gmres_iterations_f64_i32", "hpcla_gmres_iterations_f64_i64",
               "hpcla_gmres_restart_f64_i32", "hpcla_gmres_restart_f64_i64"]
ITERATIONS = {((16, 16), "jacobi"): (56, 102), ((16, 16), "none"): (228, 321),            # at restart 30 / 8
              ((24, 20), "jacobi"): (169, 135), ((24, 20), "none"): (297, 370),
              ((33, 31), "jacobi"): (262, 194), ((33, 31), "none"): (344, 573)}


@pytest.fixture(autouse=True)
def _the_solver_exists(hp):
    assert callable(getattr(hp, "gmres", None)), "hp.gmres is missing: there is nothing these figures are a yardstick of"


@pytest.fixture(scope="module")
def orders(orc):
    """Every case x {jacobi, none} x restart x the four summation orders, solved once: (x, iterations, status, history)."""
    out = {}
    for nx, ny in gc.SIZES:
        rowptr, colidx, vals, b = bc.convection_diffusion(orc, nx, ny)
        d = pc.host_diag(rowptr, colidx, vals)
        for name, dinv in (("jacobi", 1.0 / d), ("none", None)):
            for m in gc.RESTARTS:
                for order, dot in bc.DOTS.items():
                    out[(nx, ny), name, m, order] = gc.gmres(rowptr, colidx, vals, b, dinv=dinv, rtol=1e-8, restart=m, dot=dot)
            out[(nx, ny), name, "head"] = [gc.gmres(rowptr, colidx, vals, b, dinv=dinv, rtol=0.0, restart=gc.HEAD_RESTART,
                                                    maxiter=gc.HEAD + 3, dot=dot) for dot in bc.DOTS.values()]
        out[(nx, ny), "case"] = (rowptr, colidx, vals, b)
    return out


def test_public_names_exist(hp):
    assert callable(hp.gmres) and hp.GMRESWorkspace
    assert hp.gmres.__module__.endswith("gmres")


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
    # one array of 2048 partials per column, whole tiles of 8 columns, plus the 32-byte state
    assert [lib.hpcla_gmres_work_bytes(m) for m in (1, 8, 9, 30, 64)] == [(t * 8 * 2048 + 4) * 8 for t in (1, 1, 2, 4, 8)]
    assert lib.hpcla_gmres_work_bytes(0) == -1 == lib.hpcla_gmres_work_bytes(65)
    # R, c, s, g, h1, h2, col, y, nn, hn in one buffer
    for m in (1, 5, 64):
        offs = [lib.hpcla_gmres_small_offset(m, k) for k in range(11)]
        assert np.diff(offs).tolist() == [m * m, m, m, m + 1, m, m, m + 1, m, 1, 1], m
    assert lib.hpcla_gmres_small_offset(0, 0) == -1 == lib.hpcla_gmres_small_offset(5, 11)
    sig = hp._capi._SIGNATURES
    assert len(sig["hpcla_gmres_iterations_f64_i32"]) == len(sig["hpcla_gmres_iterations_f64_i64"]) + 2
    assert len(sig["hpcla_gmres_restart_f64_i32"]) == len(sig["hpcla_gmres_restart_f64_i64"]) + 2


def test_argument_errors_without_a_gpu(hp):
    """Nulls, negative sizes, an odd or short pitch, column counts outside the restart, iteration < 1 and misaligned vectors are
    refused on the host: nothing is launched (there is no GPU here to launch on)."""
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    buf = np.zeros(64)                                           # host memory: only ever looked at as an address
    a16 = buf.ctypes.data + (-buf.ctypes.data) % 16
    P, OFF = a16, a16 + 8                                        # an aligned and a misaligned non-null pointer
    # dots(comm, V, ldv, ncols, w, n, state, h_out, work, stream)
    assert lib.hpcla_gmres_dots_f64(None, P, 4, 1, P, 4, None, None, None, None) == INVALID           # null state / out / work
    assert lib.hpcla_gmres_dots_f64(None, None, 4, 1, None, 4, P, P, P, None) == INVALID              # null vectors
    assert lib.hpcla_gmres_dots_f64(None, P, 4, 1, P, -1, P, P, P, None) == INVALID
    assert lib.hpcla_gmres_dots_f64(None, P, 5, 1, P, 4, P, P, P, None) == INVALID                    # odd pitch
    assert lib.hpcla_gmres_dots_f64(None, P, 2, 1, P, 4, P, P, P, None) == INVALID                    # pitch < n
    assert lib.hpcla_gmres_dots_f64(None, P, 4, 0, P, 4, P, P, P, None) == INVALID
    assert lib.hpcla_gmres_dots_f64(None, P, 4, 65, P, 4, P, P, P, None) == INVALID
    assert lib.hpcla_gmres_dots_f64(None, P, 4, 1, OFF, 4, P, P, P, None) == INVALID
    # update(comm, V, ldv, ncols, h, w, n, iter, restart, small, hist_k, state, work, stream)
    assert lib.hpcla_gmres_update_f64(None, P, 4, 1, None, P, 4, 1, 5, None, None, None, None, None) == INVALID
    assert lib.hpcla_gmres_update_f64(None, None, 4, 1, P, None, 4, 1, 5, None, None, P, None, None) == INVALID
    assert lib.hpcla_gmres_update_f64(None, P, 4, 1, P, P, 4, 0, 5, None, None, P, None, None) == INVALID      # iteration < 1
    assert lib.hpcla_gmres_update_f64(None, P, 4, 1, P, P, 4, 1, 5, P, None, P, None, None) == INVALID         # small without hist / work
    assert lib.hpcla_gmres_update_f64(None, P, 4, 6, P, P, 4, 1, 5, P, P, P, P, None) == INVALID               # ncols > restart
    assert lib.hpcla_gmres_update_f64(None, P, 4, 1, P, P, 4, 1, 65, P, P, P, P, None) == INVALID
    assert lib.hpcla_gmres_update_f64(None, OFF, 4, 1, P, P, 4, 1, 5, None, None, P, None, None) == INVALID
    # next(w, hn, dinv, v_next, z, n, state, stream)
    assert lib.hpcla_gmres_next_f64(P, None, None, P, None, 4, None, None) == INVALID
    assert lib.hpcla_gmres_next_f64(None, P, None, None, None, 4, P, None) == INVALID
    assert lib.hpcla_gmres_next_f64(P, P, P, P, None, 4, P, None) == INVALID                          # dinv without z
    assert lib.hpcla_gmres_next_f64(P, P, None, P, None, -1, P, None) == INVALID
    assert lib.hpcla_gmres_next_f64(P, P, None, OFF, None, 4, P, None) == INVALID
    # solve(ncols, restart, small, state, stream)
    assert lib.hpcla_gmres_solve_f64(1, 5, None, P, None) == INVALID
    assert lib.hpcla_gmres_solve_f64(0, 5, P, P, None) == INVALID
    assert lib.hpcla_gmres_solve_f64(6, 5, P, P, None) == INVALID
    assert lib.hpcla_gmres_solve_f64(1, 0, P, P, None) == INVALID
    # xupdate(V, ldv, ncols, y, dinv, x, n, state, stream)
    assert lib.hpcla_gmres_xupdate_f64(P, 4, 1, None, None, P, 4, P, None) == INVALID
    assert lib.hpcla_gmres_xupdate_f64(None, 4, 1, P, None, None, 4, P, None) == INVALID
    assert lib.hpcla_gmres_xupdate_f64(P, 3, 1, P, None, P, 3, P, None) == INVALID                    # odd pitch
    assert lib.hpcla_gmres_xupdate_f64(P, 4, 1, P, OFF, P, 4, P, None) == INVALID
    # residual(comm, b, w, n, iter, restart, small, hist_k, state, work, stream)
    assert lib.hpcla_gmres_residual_f64(None, P, P, 4, 0, 5, None, None, None, None, None) == INVALID
    assert lib.hpcla_gmres_residual_f64(None, None, None, 4, 0, 5, P, P, P, P, None) == INVALID
    assert lib.hpcla_gmres_residual_f64(None, P, P, 4, -1, 5, P, P, P, P, None) == INVALID
    assert lib.hpcla_gmres_residual_f64(None, P, P, 4, 0, 0, P, P, P, P, None) == INVALID
    assert lib.hpcla_gmres_residual_f64(None, P, OFF, 4, 0, 5, P, P, P, P, None) == INVALID
    # finish(V, ldv, ncols, restart, small, dinv, x, n, stream): no open column is no work, whatever else is passed
    assert lib.hpcla_gmres_finish_f64(None, 0, 0, 5, None, None, None, 4, None) == 0
    assert lib.hpcla_gmres_finish_f64(P, 4, 6, 5, P, None, P, 4, None) == INVALID
    assert lib.hpcla_gmres_finish_f64(P, 4, 1, 5, None, None, P, 4, None) == INVALID
    # the loops: (plan, comm, rowptr, colval, [cols16, patterns,] nzval, nrows, nnz, base, interior, n, boundary, n, dinv,
    #             b, x, V, ldv, w, z, small, hist, work, restart, first_iter | iter, [iters,] stream)
    for lead, its, rst in ((7, lib.hpcla_gmres_iterations_f64_i32, lib.hpcla_gmres_restart_f64_i32),
                           (5, lib.hpcla_gmres_iterations_f64_i64, lib.hpcla_gmres_restart_f64_i64)):
        head = [None] * lead
        mid = [0, 0, None, 0, None, 0]
        for fn, tail, bad_tail in ((its, (1, 1, None), ((0, 1, None), (1, -1, None))), (rst, (0, None), ((-1, None),))):
            ok = [None, P, P, P, 4, P, None, P, P, P, 5]           # dinv, b, x, V, ldv, w, z, small, hist, work, restart
            assert fn(*head, 4, *mid, *([None] * 3), None, 4, *([None] * 5), 5, *tail) == INVALID       # nulls
            assert fn(*head, -1, *mid, *ok, *tail) == INVALID                                           # negative size
            for t in bad_tail:
                assert fn(*head, 4, *mid, *ok, *t) == INVALID                                           # first_iter < 1, count < 0
            for k, v in ((4, 5), (4, 2), (10, 0), (10, 65), (2, OFF), (0, P), (7, None)):
                bad = list(ok)                                     # odd pitch, short pitch, restart, misaligned x,
                bad[k] = v                                         # dinv without z, no small arrays
                assert fn(*head, 4, *mid, *bad, *tail) == INVALID, (k, v)


def test_open_columns_of_the_finish_call(hp):
    """The table of the cycle the host finishes: c columns by how the solve ended, against the restatement's bookkeeping."""
    from hpcla_amd.gmres import _check_restart, _open_columns
    m = 5
    assert [_open_columns(1, k, 99, m) for k in (1, 4, 5, 6, 10, 11)] == [1, 4, 5, 1, 5, 1]      # gate C at k
    assert [_open_columns(2, d, 99, m) for d in (0, 1, 4, 5, 6)] == [0, 1, 4, 0, 1]              # gate D, done_iter = d
    assert [_open_columns(0, 7, mx, m) for mx in (3, 5, 7, 10)] == [3, 0, 2, 0]                  # maxiter while running
    assert _open_columns(3, 5, 99, m) == 0                                                       # gate R
    assert [_check_restart(r) for r in (1, 30, 64)] == [1, 30, 64]
    for r in (0, 65, -3):
        with pytest.raises(ValueError):
            _check_restart(r)


def test_restatement_agrees_with_a_direct_solve(orc, orders):
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    for size in gc.SIZES:
        rowptr, colidx, vals, b = orders[size, "case"]
        n = len(b)
        x_ref = spsolve(sp.csr_matrix((vals, colidx, rowptr), shape=(n, n)).tocsc(), b)
        for name in ("jacobi", "none"):
            for m in gc.RESTARTS:
                x, its, status, h = orders[size, name, m, "np.dot"]
                assert status == "converged" and len(h) == its + 1
                true = np.linalg.norm(b - pc.matvec(rowptr, colidx, vals, x)) / np.linalg.norm(b)
                err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
                print(f"{size} {name} restart {m}: iterations {its}, true relative residual {true:.3e}, against spsolve {err:.3e}")
                assert (its == ITERATIONS[size, name][gc.RESTARTS.index(m)]), (size, name, m, its)
                assert err <= 1e-6, (size, name, m, err)
                assert true <= 1e-8 * (1 + 1e-6), (size, name, m, true)     # right preconditioning: the estimate IS the true residual
        d = pc.host_diag(rowptr, colidx, vals)
        x, its, status, _ = gc.gmres(rowptr, colidx, vals, b, dinv=1.0 / d, x0=np.full(n, 1e-3))
        assert status == "converged" and np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref) <= 1e-6


def test_spread_across_summation_orders_is_within_the_margins_of_the_gpu_tests(orders):
    """The device sums in yet another order.  What the order alone does, measured here with four orders on the CPU, bounds what
    the GPU tests may ask: iteration counts (+-2 there; identical here), fewer iterations with Jacobi at restart 30, the true
    residual (2 rtol there), the first HEAD history entries (HIST_RTOL there; the spread here must stay below HIST_RTOL / 10)
    and a history that never rises (RISE_RTOL there).  The spread of the whole history is printed: it is why only a head is
    compared."""
    for size in gc.SIZES:
        rowptr, colidx, vals, b = orders[size, "case"]
        for name in ("jacobi", "none"):
            for m in gc.RESTARTS:
                runs = [orders[size, name, m, o] for o in bc.DOTS]
                counts = [r[1] for r in runs]
                true = [np.linalg.norm(b - pc.matvec(rowptr, colidx, vals, r[0])) / np.linalg.norm(b) for r in runs]
                length = min(len(r[3]) for r in runs)
                whole = max((max(r[3][k] for r in runs) - min(r[3][k] for r in runs)) / min(r[3][k] for r in runs)
                            for k in range(length))
                rise = max((h[k + 1] - h[k]) / h[k] for r in runs for h in (r[3],) for k in range(len(h) - 1))
                print(f"{size} {name} restart {m}: iterations {counts}, true residual / rtol {min(true) / 1e-8:.3f} - "
                      f"{max(true) / 1e-8:.3f}, whole-history spread {whole:.2e}, largest relative rise {rise:.2e}")
                assert all(r[2] == "converged" for r in runs)
                assert max(counts) - min(counts) <= 1
                assert max(true) <= 1.5e-8
                assert rise <= gc.RISE_RTOL / 10
            head = max((max(r[3][k] for r in orders[size, name, "head"]) - min(r[3][k] for r in orders[size, name, "head"]))
                       / min(r[3][k] for r in orders[size, name, "head"]) for k in range(gc.HEAD))
            print(f"{size} {name}: spread of the first {gc.HEAD} entries at restart {gc.HEAD_RESTART}: {head:.2e}")
            assert head <= gc.HIST_RTOL / 10
            assert all(r[1:3] == (gc.HEAD + 3, "maxiter") and len(r[3]) == gc.HEAD + 4 for r in orders[size, name, "head"])
        assert all(orders[size, "jacobi", 30, o][1] < orders[size, "none", 30, o][1] for o in bc.DOTS)


def test_restatement_on_the_exact_cases(orc):
    # ROT: bicgstab's restatement breaks down on it, GMRES converges at step 2
    assert bc.bicgstab(*bc.ROT, bc.ROT_B)[2] == "breakdown"
    x, its, status, h = gc.gmres(*gc.ROT, gc.ROT_B)
    assert (its, status, h) == (2, "converged", [1.0, 1.0, 0.0]) and np.array_equal(x, [0.0, 1.0])
    # -I: one step, a residual of exactly 0
    bi = orc.fill_uniform(0, 5, pc.SEED_RHS)
    x, its, status, h = gc.gmres(*pc.diag_matrix(-np.ones(5)), bi)
    assert (its, status, len(h)) == (1, "converged", 2) and h[1] == 0.0 and np.allclose(x, -bi, rtol=1e-15, atol=0)
    # the diagonal case under Jacobi: A K = I, one step
    rowptr, colidx, d, b = pc.diagonal_case(orc)
    x, its, status, h = gc.gmres(rowptr, colidx, d, b, dinv=1.0 / d, rtol=1e-8, maxiter=50)
    assert (its, status, len(h)) == (1, "converged", 2) and h[1] <= 1e-8 * h[0]
    assert np.all(np.abs(x - b / d) <= 4 * np.spacing(np.abs(b / d)))
    # ZERO: gate D in step 1;  NILP: gate D in step 2
    x, its, status, h = gc.gmres(*gc.ZERO, gc.ZERO_B)
    assert (its, status, h) == (0, "breakdown", [math.sqrt(2.0)]) and not x.any()
    x, its, status, h = gc.gmres(*gc.NILP, gc.NILP_B)
    assert (its, status, h) == (1, "breakdown", [1.0, 1.0]) and not x.any()
    # b = 0
    x, its, status, h = gc.gmres(*pc.diag_matrix(np.ones(5)), np.zeros(5))
    assert (its, status, h) == (0, "converged", [0.0]) and not x.any()


def test_short_restarts_stagnate_to_maxiter(orc):
    rowptr, colidx, vals, b = bc.convection_diffusion(orc, 16, 16)
    d = pc.host_diag(rowptr, colidx, vals)
    for m in (1, 2):
        x, its, status, h = gc.gmres(rowptr, colidx, vals, b, dinv=1.0 / d, restart=m, maxiter=40)
        print(f"restart {m}: ||r_40|| / ||r_0|| = {h[-1] / h[0]:.4f}")
        assert (its, status, len(h)) == (40, "maxiter", 41) and np.all(np.isfinite(x))
        assert 0.99 <= h[-1] / h[0] <= 1.0


def test_head_spread_at_the_large_size(orc):
    """65 x 63 (4095 rows, two reduction workgroups on the device): the first HEAD entries at restart = HEAD_RESTART under the
    four summation orders.  HIST_RTOL, which tests/test_gpu_gmres.py asks there, must be at least 10 times the spread (measured:
    2.3e-15 with Jacobi, 8.8e-16 without: 430 times)."""
    rowptr, colidx, vals, b = bc.convection_diffusion(orc, *gc.LARGE_SIZE)
    assert len(b) == 4095
    d = pc.host_diag(rowptr, colidx, vals)
    for name, dinv in (("jacobi", 1.0 / d), ("none", None)):
        hists = [gc.gmres(rowptr, colidx, vals, b, dinv=dinv, rtol=0.0, atol=0.0, restart=gc.HEAD_RESTART, maxiter=gc.HEAD + 3,
                          dot=dot)[3] for dot in bc.DOTS.values()]
        spread = max((max(col) - min(col)) / min(col) for col in zip(*[h[:gc.HEAD] for h in hists]))
        print(f"{gc.LARGE_SIZE} {name}: spread over the first {gc.HEAD} history entries {spread:.2e}")
        assert pc.LARGE_MARGIN_FACTOR * spread <= gc.HIST_RTOL
