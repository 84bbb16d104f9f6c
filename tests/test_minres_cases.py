"""CPU side of the MINRES solver: the public names, the C ABI tables, and the numpy restatement of the loop
(tests/_minres_cases.py) against a dense solve and scipy's MINRES, on the exact and degenerate cases, against CG's breakdown on
the same matrices, and under four summation orders -- the measurement the margins of tests/test_gpu_minres.py rest on, re-run
and printed here.

The first three tests need the feature (the public names, the new C entries).  The others exercise the restatement alone:
they check the yardstick of the GPU tests, not the library, and so pass without the feature."""
import math
import os
import re

import numpy as np
import pytest

from tests import _minres_cases as mc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_minres_work_bytes", "hpcla_minres_r_f64", "hpcla_minres_xw_f64", "hpcla_minres_iterations_f64_i32",
               "hpcla_minres_iterations_f64_i64"]
EXPECTED = mc.EXPECTED


@pytest.fixture(scope="module")
def orders(orc):
    """Every case under the four summation orders, solved once: {key: (case, {order: result})}."""
    return {key: (case, {order: mc.minres(*case[:4], dinv=case[4], dot=dot) for order, dot in mc.DOTS.items()})
            for key, case in mc.all_cases(orc).items()}


def test_public_names_exist(hp):
    assert callable(hp.minres) and hp.MinresWorkspace
    assert hp.minres.__module__.endswith("minres")
    assert [f for f in hp.CGInfo.__dataclass_fields__] == ["converged", "iterations", "status", "residual_norms"]
    assert "M norm" in hp.minres.__doc__ and "hp.lsqr" in hp.minres.__doc__


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
    # one array of 2048 partials plus the 32-byte state
    assert lib.hpcla_minres_work_bytes() == (2048 + 4) * 8
    sig = hp._capi._SIGNATURES
    assert len(sig["hpcla_minres_iterations_f64_i32"]) == len(sig["hpcla_minres_iterations_f64_i64"]) + 2


def test_argument_errors_without_a_gpu(hp):
    """Nulls, negative sizes, iteration / first_iter < 1, a negative count, misaligned vectors and a written vector that
    aliases another are refused on the host: nothing is launched (there is no GPU here to launch on)."""
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    buf = np.zeros(256)                                          # host memory: only ever looked at as an address
    a16 = buf.ctypes.data + (-buf.ctypes.data) % 16
    P = [a16 + 64 * k for k in range(16)]                        # aligned, distinct non-null pointers
    OFF = a16 + 8                                                # a misaligned one
    # minres_r(comm, scal, t, r2, dinv, r1, yn, n, iter, state, pair_out, work, stream)
    r = lib.hpcla_minres_r_f64
    assert r(None, None, P[1], P[2], None, P[3], None, 4, 1, None, None, None, None) == INVALID     # null scalars / state / work
    assert r(None, P[0], None, None, None, None, None, 4, 1, P[5], None, P[6], None) == INVALID     # null vectors
    assert r(None, P[0], P[1], P[2], P[4], P[3], None, 4, 1, P[5], None, P[6], None) == INVALID     # dinv without yn
    assert r(None, P[0], P[1], P[2], None, P[3], None, -1, 1, P[5], None, P[6], None) == INVALID
    assert r(None, P[0], P[1], P[2], None, P[3], None, 4, 0, P[5], None, P[6], None) == INVALID
    assert r(None, P[0], OFF, P[2], None, P[3], None, 4, 1, P[5], None, P[6], None) == INVALID
    assert r(None, P[0], P[1], P[2], None, P[2], None, 4, 1, P[5], None, P[6], None) == INVALID     # r1 is r2
    assert r(None, P[0], P[1], P[2], P[4], P[3], P[3], 4, 1, P[5], None, P[6], None) == INVALID     # yn is r1
    # minres_xw(scal, y, w2, w1, x, n, iter, state, stream)
    xw = lib.hpcla_minres_xw_f64
    assert xw(None, P[1], P[2], P[3], P[4], 4, 1, None, None) == INVALID
    assert xw(P[0], None, None, None, None, 4, 1, P[5], None) == INVALID
    assert xw(P[0], P[1], P[2], P[3], P[4], -1, 1, P[5], None) == INVALID
    assert xw(P[0], P[1], P[2], P[3], P[4], 4, 0, P[5], None) == INVALID
    assert xw(P[0], P[1], OFF, P[3], P[4], 4, 1, P[5], None) == INVALID
    assert xw(P[0], P[1], P[2], P[2], P[4], 4, 1, P[5], None) == INVALID                            # w1 is w2
    # the loop: (plan, comm, rowptr, colval, (cols16, patterns,) nzval, nrows, nnz, base, interior, n, boundary, n, dinv,
    #            x, r_a, r_b, y_a, y_b, w_a, w_b, t, hist, scal, dot_work, work, first_iter, iters, stream)
    for fn, lead in ((lib.hpcla_minres_iterations_f64_i32, 7), (lib.hpcla_minres_iterations_f64_i64, 5)):
        def block(nrows):
            return [None] * lead + [nrows, 0, 0, None, 0, None, 0]
        vecs = [P[1], P[2], P[3], None, None, P[4], P[5], P[6]]      # x, r_a, r_b, y_a, y_b, w_a, w_b, t
        tail = [P[7], P[8], P[9], P[10]]                             # hist, scal, dot_work, work
        assert fn(*block(4), None, *([None] * 8), *tail, 1, 1, None) == INVALID                      # null vectors
        assert fn(*block(4), None, *vecs, None, None, None, None, 1, 1, None) == INVALID             # null history / scalars / work
        assert fn(*block(4), P[11], *vecs, *tail, 1, 1, None) == INVALID                             # dinv without y_a, y_b
        assert fn(*block(-1), None, *vecs, *tail, 1, 1, None) == INVALID                             # negative size
        assert fn(*block(4), None, *vecs, *tail, 1, -1, None) == INVALID                             # negative count
        assert fn(*block(4), None, *vecs, *tail, 0, 1, None) == INVALID                              # first_iter < 1
        for k in (0, 1, 2, 5, 6, 7):
            bad = list(vecs)
            bad[k] = OFF
            assert fn(*block(4), None, *bad, *tail, 1, 1, None) == INVALID                           # a misaligned vector


def test_cases_have_the_stated_shapes_and_spectra(orc):
    for (name, size, pre), (rowptr, colidx, vals, b, dinv) in mc.all_cases(orc).items():
        if pre and name == "shifted":
            continue
        dense = mc.dense_of(rowptr, colidx, vals)
        n = size[0] * size[1]
        assert dense.shape == ((n, n) if name == "shifted" else (2 * n, 2 * n)) and len(b) == dense.shape[0]
        assert np.array_equal(dense, dense.T)                                        # exactly symmetric
        assert all(np.all(np.diff(colidx[rowptr[i]:rowptr[i + 1]]) > 0) for i in range(len(b)))   # columns ascending
        ev = np.linalg.eigvalsh(dense)
        neg, cond = int((ev < 0).sum()), float(np.abs(ev).max() / np.abs(ev).min())
        print(f"{name} {size}: {neg} negative eigenvalues of {len(ev)}, condition number {cond:.2f}")
        if name == "saddle":
            assert neg == n and 7.5 <= cond <= 8.0
            K = dense[:n, :n]
            assert np.array_equal(dense[n:, n:], -K) and np.array_equal(dense[:n, n:], 0.5 * np.eye(n))
            assert np.all(np.diag(K) == 5.0)
        elif name == "scaled_saddle":
            assert neg == n
            d = np.diag(dense)
            assert (d > 0).sum() == n and d.max() / np.abs(d).min() > 50
        else:
            assert n == 1023 and neg == 21


def test_restatement_agrees_with_a_dense_solve_and_with_scipy(orders):
    """x against numpy.linalg.solve: the stop rule bounds the M-norm residual by rtol sqrt(b.M b), hence the error by
    rtol cond-ish; 1e-6 is asked (measured <= 7.4e-9).  The true residual in the tested norm stays within 2 thr^(1/2) (measured
    <= 0.97 of it).  scipy's MINRES stops by a different rule, so the solutions are compared, at the sum of both margins."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import minres as scipy_minres
    for key, (case, runs) in orders.items():
        rowptr, colidx, vals, b, dinv = case
        dense = mc.dense_of(rowptr, colidx, vals)
        x_ref = np.linalg.solve(dense, b)
        x, its, status, hist = runs["np.dot"]
        assert status == "converged" and len(hist) == its + 1
        assert all(h1 <= h0 for h0, h1 in zip(hist, hist[1:]))                       # the residual never rises
        err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
        limit = 1e-8 * mc.m_norm(b, dinv)
        true = mc.m_norm(b - dense @ x, dinv) / limit
        Mop = None if dinv is None else sp.diags(dinv)
        xs, flag = scipy_minres(sp.csr_matrix(dense), b, M=Mop, rtol=1e-10, maxiter=20 * len(b))
        vs = np.linalg.norm(x - xs) / np.linalg.norm(xs)
        print(f"{key}: converged at {its}, against solve {err:.2e}, true residual {true:.3f} of the limit, against scipy {vs:.2e}")
        assert err <= 1e-6 and true <= 2.0 and flag == 0 and vs <= 2e-6
        want, lo, hi = EXPECTED[key]                                                  # counts move with rounding: +-2, as on the GPU
        assert abs(its - want) <= 2, (key, its)


def test_spread_across_summation_orders_is_within_the_margins_of_the_gpu_tests(orders):
    """The device sums in yet another order.  What the order alone does, measured here with four orders on the CPU, bounds what
    the GPU tests may ask: iteration counts (the spread + 2 there) and the first HEAD history entries (HIST_RTOL there, which
    must be at least 100 times the spread)."""
    worst = 0.0
    for key, (case, runs) in orders.items():
        counts = [r[1] for r in runs.values()]
        assert {r[2] for r in runs.values()} == {"converged"}
        head = max((max(col) - min(col)) / min(col) for col in zip(*[r[3][:mc.HEAD] for r in runs.values()]))
        worst = max(worst, head)
        print(f"{key}: iterations {counts}; spread over the first {mc.HEAD} history entries {head:.2e}")
        want, lo, hi = EXPECTED[key]
        assert lo - 2 <= min(counts) and max(counts) <= hi + 2, (key, counts)
        assert 100 * head <= mc.HIST_RTOL
    print(f"largest head spread {worst:.2e}")


def test_cg_breaks_down_where_minres_converges(orc, orders):
    for key, (case, runs) in orders.items():
        if key[2]:
            continue
        _, its, status, _ = pc.pcg(*case[:4])
        assert status == "breakdown" and its <= 1, (key, its, status)
    _, its, status, _ = pc.pcg(*pc.diag_matrix(-np.ones(5)), orc.fill_uniform(0, 5, pc.SEED_RHS))
    assert (its, status) == (0, "breakdown")


def test_restatement_on_the_exact_and_degenerate_cases(orc):
    bi = orc.fill_uniform(0, 5, pc.SEED_RHS)
    for sign in (1.0, -1.0):
        # the literal loop forms t / beta - (alfa / beta) r2 and x = phi (y / beta): one iteration, x to rounding
        x, its, status, hist = mc.minres(*pc.diag_matrix(sign * np.ones(5)), bi)
        assert (its, status) == (1, "converged") and np.all(np.abs(x - sign * bi) <= 1e-15)
        assert hist[1] <= 1e-15 * hist[0]
    x, its, status, hist = mc.minres(*pc.diag_matrix([1.0, -1.0, 2.0, 3.0]), np.array([1.0, 2.0, 1.0, 1.0]))
    assert status == "converged" and its <= 4 and np.all(np.abs(x - [1.0, -2.0, 0.5, 1.0 / 3.0]) <= 1e-8)
    # singular and consistent: rn = 0 exactly, beta' = 0, sn = 0: the lucky termination
    x, its, status, hist = mc.minres(*pc.diag_matrix([1.0, 0.0]), np.array([1.0, 0.0]))
    assert (x.tolist(), its, status, hist) == ([1.0, 0.0], 1, "converged", [1.0, 0.0])
    x, its, status, hist = mc.minres(*pc.diag_matrix([1.0, math.nan]), np.array([1.0, 1.0]))
    assert (its, status, hist) == (0, "breakdown", [math.sqrt(2.0)]) and not x.any()
    x, its, status, hist = mc.minres(*pc.diag_matrix(np.ones(5)), np.zeros(5))
    assert (its, status, hist) == (0, "converged", [0.0]) and not x.any()
    x, its, status, hist = mc.minres(*pc.diag_matrix(np.ones(5)), bi, maxiter=0)
    assert (its, status, len(hist)) == (0, "maxiter", 1) and not x.any()
    # a start vector near the solution stops sooner, and its threshold still refers to b
    rowptr, colidx, vals, b = mc.saddle(orc, 16, 16)
    x_ref = np.linalg.solve(mc.dense_of(rowptr, colidx, vals), b)
    _, its0, _, _ = mc.minres(rowptr, colidx, vals, b)
    x, its, status, hist = mc.minres(rowptr, colidx, vals, b, x0=x_ref * (1.0 + 1e-4))
    assert status == "converged" and its < its0 and hist[-1] <= 1e-8 * np.linalg.norm(b) < hist[-2] <= hist[0]


def test_head_spread_at_the_large_size(orc):
    """65 x 63 (8190 rows for the saddle cases: four reduction workgroups on the device; 4095 shifted: two): the first HEAD
    entries under the four summation orders.  HIST_RTOL, which tests/test_gpu_minres.py asks there, must be at least 10 times the
    spread (measured: saddle 6.3e-15, scaled saddle 1.1e-14, shifted 9.1e-15: 90 times)."""
    for name, case, dinv in mc.large_cases(orc):
        hists = [mc.minres(*case, dinv=dinv, rtol=0.0, maxiter=mc.HEAD, dot=dot)[3] for dot in mc.DOTS.values()]
        spread = max((max(col) - min(col)) / min(col) for col in zip(*[h[:mc.HEAD] for h in hists]))
        print(f"{name} {mc.LARGE_SIZE} ({len(case[3])} rows): spread over the first {mc.HEAD} history entries {spread:.2e}")
        assert pc.LARGE_MARGIN_FACTOR * spread <= mc.HIST_RTOL
