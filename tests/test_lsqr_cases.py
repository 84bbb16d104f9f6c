"""CPU side of the least-squares solver: the public names, the C ABI tables, and the numpy restatement of the loop
(tests/_lsqr_cases.py) against a dense least-squares solve, on the exact and degenerate cases, and under four summation
orders -- the measurement the margins of tests/test_gpu_lsqr.py rest on, re-run and printed here.

The first three tests need the feature (the public names, the new C entries).  The others exercise the restatement alone:
they check the yardstick of the GPU tests, not the library, and so pass without the feature."""
import math
import os
import re

import numpy as np
import pytest

from tests import _lsqr_cases as lc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_lsqr_work_bytes", "hpcla_lsqr_u_f64", "hpcla_lsqr_v_f64", "hpcla_lsqr_xw_f64",
               "hpcla_lsqr_iterations_f64_i32", "hpcla_lsqr_iterations_f64_i64"]
# np.dot's (status, iterations) at damp = 0 and damp = 0.3, as the issue records them
EXPECTED = {("tall", (16, 16)): ("least_squares", 78, "least_squares", 73), ("tall", (24, 20)): ("least_squares", 85, "least_squares", 79),
            ("tall", (33, 31)): ("least_squares", 86, "least_squares", 80), ("wide", (16, 16)): ("converged", 91, "least_squares", 76),
            ("wide", (24, 20)): ("converged", 99, "least_squares", 83), ("wide", (33, 31)): ("converged", 102, "least_squares", 84)}


@pytest.fixture(scope="module")
def orders(orc):
    """Every case x damp x the four summation orders, solved once."""
    out = {}
    for kind, make in lc.CASES.items():
        for size in lc.SIZES:
            case = make(orc, *size)
            out[kind, size, "case"] = case
            for damp in lc.DAMPS:
                for order, dot in lc.DOTS.items():
                    out[kind, size, damp, order] = lc.lsqr(*case, damp=damp, dot=dot)
    return out


def test_public_names_exist(hp):
    assert callable(hp.lsqr) and hp.LSQRWorkspace and hp.LSQRInfo
    assert hp.lsqr.__module__.endswith("lsqr")
    assert [f for f in hp.LSQRInfo.__dataclass_fields__] == ["converged", "iterations", "status", "residual_norms",
                                                            "normal_residual_norms", "anorm"]
    assert [f for f in hp.CGInfo.__dataclass_fields__] == ["converged", "iterations", "status", "residual_norms"]


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
    assert lib.hpcla_lsqr_work_bytes() == (2048 + 4) * 8
    sig = hp._capi._SIGNATURES
    assert len(sig["hpcla_lsqr_iterations_f64_i32"]) == len(sig["hpcla_lsqr_iterations_f64_i64"]) + 4


def test_argument_errors_without_a_gpu(hp):
    """Nulls, negative sizes, iteration / first_iter < 1, a negative count and misaligned vectors are refused on the host:
    nothing is launched (there is no GPU here to launch on)."""
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    buf = np.zeros(64)                                           # host memory: only ever looked at as an address
    a16 = buf.ctypes.data + (-buf.ctypes.data) % 16
    P, OFF = a16, a16 + 8                                        # an aligned and a misaligned non-null pointer
    # lsqr_u(comm, scal, tu, uh, n, iter, state, work, stream)
    assert lib.hpcla_lsqr_u_f64(None, None, P, P, 4, 1, None, None, None) == INVALID                 # null scalars / state / work
    assert lib.hpcla_lsqr_u_f64(None, P, None, None, 4, 1, P, P, None) == INVALID                    # null vectors
    assert lib.hpcla_lsqr_u_f64(None, P, P, P, -1, 1, P, P, None) == INVALID
    assert lib.hpcla_lsqr_u_f64(None, P, P, P, 4, 0, P, P, None) == INVALID
    assert lib.hpcla_lsqr_u_f64(None, P, OFF, P, 4, 1, P, P, None) == INVALID
    # lsqr_v(comm, scal, tv, vh, n, iter, state, pair_out, work, stream)
    assert lib.hpcla_lsqr_v_f64(None, None, P, P, 4, 1, None, P, None, None) == INVALID
    assert lib.hpcla_lsqr_v_f64(None, P, None, None, 4, 1, P, P, P, None) == INVALID
    assert lib.hpcla_lsqr_v_f64(None, P, P, P, -1, 1, P, P, P, None) == INVALID
    assert lib.hpcla_lsqr_v_f64(None, P, P, P, 4, 0, P, P, P, None) == INVALID
    assert lib.hpcla_lsqr_v_f64(None, P, P, OFF, 4, 1, P, P, P, None) == INVALID
    # lsqr_xw(scal, vh, x, w, n, iter, state, stream)
    assert lib.hpcla_lsqr_xw_f64(None, P, P, P, 4, 1, None, None) == INVALID
    assert lib.hpcla_lsqr_xw_f64(P, None, None, None, 4, 1, P, None) == INVALID
    assert lib.hpcla_lsqr_xw_f64(P, P, P, P, -1, 1, P, None) == INVALID
    assert lib.hpcla_lsqr_xw_f64(P, P, P, P, 4, 0, P, None) == INVALID
    assert lib.hpcla_lsqr_xw_f64(P, P, OFF, P, 4, 1, P, None) == INVALID
    # the loop: (comm, [plan, rowptr, colval, (cols16, patterns,) nzval, nrows, nnz, base, interior, n, boundary, n] twice,
    #            x, uh, vh, w, tu, tv, hist, scal, work, first_iter, iters, stream)
    for fn, lead in ((lib.hpcla_lsqr_iterations_f64_i32, 6), (lib.hpcla_lsqr_iterations_f64_i64, 4)):
        def block(nrows):
            return [None] * lead + [nrows, 0, 0, None, 0, None, 0]
        vecs = [P] * 6                                           # x, uh, vh, w, tu, tv
        assert fn(None, *block(4), *block(4), *([None] * 9), 1, 1, None) == INVALID                       # nulls
        assert fn(None, *block(4), *block(4), *vecs, None, None, None, 1, 1, None) == INVALID             # null history / scalars / work
        assert fn(None, *block(-1), *block(4), *vecs, P, P, P, 1, 1, None) == INVALID                     # negative size (A)
        assert fn(None, *block(4), *block(-1), *vecs, P, P, P, 1, 1, None) == INVALID                     # negative size (At)
        assert fn(None, *block(4), *block(4), *vecs, P, P, P, 1, -1, None) == INVALID                     # negative count
        assert fn(None, *block(4), *block(4), *vecs, P, P, P, 0, 1, None) == INVALID                      # first_iter < 1
        for k in range(6):
            bad = list(vecs)
            bad[k] = OFF
            assert fn(None, *block(4), *block(4), *bad, P, P, P, 1, 1, None) == INVALID                   # a misaligned vector


def test_cases_have_the_stated_shapes_and_condition(orc):
    for size in lc.SIZES:
        rowptr, colidx, vals, n, b = lc.tall(orc, *size)
        dense = lc.dense_of(rowptr, colidx, vals, n)
        assert dense.shape == (2 * n, n) and len(b) == 2 * n
        cond = np.linalg.cond(dense)
        print(f"tall {size}: condition number {cond:.2f}")
        assert 10.8 <= cond <= 11.2
        rt, ct, vt, n2, bw = lc.wide(orc, *size)
        assert n2 == 2 * n and len(bw) == n
        assert np.array_equal(lc.dense_of(rt, ct, vt, n2), dense.T)
        assert all(np.all(np.diff(ct[rt[i]:rt[i + 1]]) > 0) for i in range(n))      # columns ascending within a row
    assert n == 1023


def test_restatement_agrees_with_a_dense_least_squares_solve(orders):
    for kind in lc.CASES:
        for size in lc.SIZES:
            rowptr, colidx, vals, ncols, b = orders[kind, size, "case"]
            dense = lc.dense_of(rowptr, colidx, vals, ncols)
            got = []
            for damp in lc.DAMPS:
                x, its, status, hr, hn, anorm = orders[kind, size, damp, "np.dot"]
                assert len(hr) == len(hn) == its + 1
                Ab, bb = lc.augmented(dense, b, damp)
                x_ref = np.linalg.lstsq(Ab, bb, rcond=None)[0]
                err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
                rbar = bb - Ab @ x
                rn = float(np.linalg.norm(rbar))
                line = f"{kind} {size} damp {damp}: {status} at {its}, against lstsq {err:.2e}"
                assert err <= 1e-6, (kind, size, damp, err)
                if status == "converged":                                        # the consistent cases
                    true = np.linalg.norm(b - dense @ x) / np.linalg.norm(b)
                    line += f", true relative residual {true:.2e}"
                    assert true <= 2e-8
                else:
                    normal = np.linalg.norm(Ab.T @ rbar) / (np.linalg.norm(Ab) * rn)
                    rel = abs(hr[-1] - rn) / rn
                    line += f", true normal residual {normal:.2e} of |Abar|_F |rbar|, last history entry off by {rel:.2e}"
                    assert normal <= 2e-8
                    assert rel <= 1e-11
                print(line)
                got += [status, its]
            want = EXPECTED[kind, size]                                       # counts move with rounding: +-2, as on the GPU
            assert (got[0], got[2]) == (want[0], want[2]), (kind, size, got)
            assert abs(got[1] - want[1]) <= 2 and abs(got[3] - want[3]) <= 2, (kind, size, got)


def test_spread_across_summation_orders_is_within_the_margins_of_the_gpu_tests(orders):
    """The device sums in yet another order.  What the order alone does, measured here with four orders on the CPU, bounds what
    the GPU tests may ask: iteration counts (+-2 there) and the first HEAD entries of both histories (HIST_RTOL there).  The
    tail of normal_residual_norms is rounding-dominated near the stop: its spread at the last common entry is printed and not
    compared, here or on the GPU."""
    worst_head = 0.0
    for kind in lc.CASES:
        for size in lc.SIZES:
            for damp in lc.DAMPS:
                runs = [orders[kind, size, damp, o] for o in lc.DOTS]
                counts = [r[1] for r in runs]
                assert len({r[2] for r in runs}) == 1
                assert max(counts) - min(counts) <= 2, (kind, size, damp, counts)

                def spread(which, k):
                    col = [r[which][k] for r in runs]
                    return (max(col) - min(col)) / min(col)
                head = max(spread(which, k) for which in (3, 4) for k in range(lc.HEAD))
                last = spread(4, min(counts))
                worst_head = max(worst_head, head)
                print(f"{kind} {size} damp {damp}: iterations {counts}; spread over the first {lc.HEAD} entries of both histories "
                      f"{head:.2e}; of the last normal residual {last:.2e} (not compared)")
                assert 20 * head <= lc.HIST_RTOL
    print(f"largest head spread {worst_head:.2e}")


def test_restatement_on_the_exact_and_degenerate_cases(orc):
    # gate U: uh is exactly 0 in iteration 1; the step ends the solve with thr = 0 and ntol = 0
    x, its, status, hr, hn, _ = lc.lsqr(*lc.DIAG20, [1.0, 0.0], rtol=0.0, ntol=0.0)
    assert (x.tolist(), its, status, hr, hn) == ([0.5, 0.0], 1, "converged", [1.0, 0.0], [2.0, 0.0])
    # b orthogonal to range(A)
    x, its, status, hr, hn, _ = lc.lsqr(*lc.DIAG10, [0.0, 1.0])
    assert (x.tolist(), its, status, hr, hn) == ([0.0, 0.0], 0, "least_squares", [1.0], [0.0])
    # an inconsistent singular system: one iteration
    x, its, status, hr, hn, _ = lc.lsqr(*lc.DIAG10, [1.0, 1.0])
    assert (its, status, hr) == (1, "least_squares", [math.sqrt(2.0), 1.0000000000000002])
    assert hn[1] <= 1e-15
    # x = (1, 0) to rounding: t1 = (c phibar) / rho carries three roundings, the literal loop gives x_0 = 1 + 2 ulp; the bound
    # is the one the next case states
    assert x[1] == 0.0 and abs(x[0] - 1.0) <= 1e-15
    x, its, status, hr, hn, _ = lc.lsqr(*lc.THREE_BY_TWO, [1.0, 2.0, 0.0])
    assert (its, status) == (2, "least_squares") and np.all(np.abs(x - [0.0, 1.0]) <= 1e-15)
    bi = orc.fill_uniform(0, 5, pc.SEED_RHS)
    x, its, status, hr, hn, _ = lc.lsqr(*lc.identity(5), bi)
    assert (its, status) == (1, "converged") and np.all(np.abs(x - bi) <= 4 * np.spacing(bi))
    x, its, status, hr, hn, _ = lc.lsqr(*lc.DIAG1NAN, [1.0, 1.0])
    assert (its, status) == (0, "breakdown") and not x.any()
    x, its, status, hr, hn, _ = lc.lsqr(*lc.identity(5), np.zeros(5))
    assert (its, status, hr) == (0, "converged", [0.0]) and not x.any()
    # a start vector changes the path, not the answer (consistent system, minimum norm is lost: only the residual is asked)
    case = lc.wide(orc, 16, 16)
    x, its, status, hr, hn, _ = lc.lsqr(*case, x0=np.full(case[3], 1e-3))
    dense = lc.dense_of(*case[:4])
    assert status == "converged" and np.linalg.norm(case[4] - dense @ x) <= 2e-8 * np.linalg.norm(case[4])


def test_head_spread_at_the_large_size(orc):
    """The tall case at 65 x 63 (8190 x 4095: four and two reduction workgroups on the device): the first HEAD entries of both
    histories under the four summation orders.  HIST_RTOL, which tests/test_gpu_lsqr.py asks there, must be at least 10 times
    the spread (measured: 1.2e-14 at damp 0, 1.0e-14 at damp 0.3: 80 times)."""
    case = lc.tall(orc, *lc.LARGE_SIZE)
    assert (len(case[0]) - 1, case[3]) == (8190, 4095)
    for damp in lc.DAMPS:
        runs = [lc.lsqr(*case, damp=damp, rtol=0.0, ntol=0.0, maxiter=lc.HEAD, dot=dot) for dot in lc.DOTS.values()]
        spread = max((max(col) - min(col)) / min(col) for which in (3, 4) for col in zip(*[r[which][:lc.HEAD] for r in runs]))
        print(f"tall {lc.LARGE_SIZE} damp {damp}: spread over the first {lc.HEAD} entries of both histories {spread:.2e}")
        assert pc.LARGE_MARGIN_FACTOR * spread <= lc.HIST_RTOL
