"""CPU side of the eigensolver (``hp.eigsh``): the public names, the C ABI tables, the argument errors that need no device, the
pure-numpy host functions of eigsh.py (selection by ``which``, the choice of p, the assembly of T, the estimates), and the numpy
restatement of the loop (tests/_eigsh_cases.py) against the dense spectrum and under four summation orders -- the measurement
the margins of tests/test_gpu_eigsh.py rest on, re-run and printed here.

The restatement's tests check the yardstick of the GPU tests, which means nothing without the solver it restates, so the whole
file asks for ``hp.eigsh`` first."""
import os
import re
import sys

import numpy as np
import pytest

from tests import _bicgstab_cases as bc
from tests import _eigsh_cases as ec
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_eigsh_small_offset", "hpcla_eigsh_update_f64", "hpcla_eigsh_rotate_f64", "hpcla_eigsh_steps_f64_i32",
               "hpcla_eigsh_steps_f64_i64"]
# (steps, cycles) of the restatement at tol = 1e-10: the figures the GPU tests' margins come from
STEPS = {(("plain", (24, 20)), 4, 20, "LA"): (148, 17), (("plain", (24, 20)), 4, 20, "SA"): (156, 18),
         (("plain", (24, 20)), 1, 8, "LA"): (184, 45), (("plain", (33, 31)), 6, 32, "LA"): (214, 15),
         (("scaled", (33, 31)), 4, 24, "LA"): (84, 7)}


@pytest.fixture(autouse=True)
def _the_solver_exists(hp):
    assert callable(getattr(hp, "eigsh", None)), "hp.eigsh is missing: there is nothing these figures are a yardstick of"


@pytest.fixture(scope="module")
def matrices(orc):
    return ec.matrices(orc)


def test_public_names_exist(hp):
    assert callable(hp.eigsh) and hp.EigshWorkspace and hp.EigshInfo
    assert hp.eigsh.__module__.endswith("eigsh")


def test_header_declares_the_new_entries_and_ctypes_binds_them(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in hp._capi.EXPORTED_SYMBOLS, name
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hpcla_rocm.h"
        assert m.group(1).count(",") + 1 == len(hp._capi._SIGNATURES[name]), name
    lib = hp._capi.load()
    for m in (1, 5, 20, 64):                                     # T, beta, h1, h2, nn, hn in one buffer
        offs = [lib.hpcla_eigsh_small_offset(m, k) for k in range(7)]
        assert np.diff(offs).tolist() == [m * m, m, m, m, 1, 1], m
    assert lib.hpcla_eigsh_small_offset(0, 0) == -1 == lib.hpcla_eigsh_small_offset(65, 0)
    assert lib.hpcla_eigsh_small_offset(5, 7) == -1 == lib.hpcla_eigsh_small_offset(5, -1)
    sig = hp._capi._SIGNATURES
    assert len(sig["hpcla_eigsh_steps_f64_i32"]) == len(sig["hpcla_eigsh_steps_f64_i64"]) + 2


def test_c_entries_refuse_bad_arguments_without_a_gpu(hp):
    """Nulls, negative sizes, an odd or short pitch, p and m outside 1 <= p <= m <= 64, misaligned vectors: refused on the host,
    nothing is launched."""
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    buf = np.zeros(64)                                           # host memory: only ever looked at as an address
    a16 = buf.ctypes.data + (-buf.ctypes.data) % 16
    P, OFF = a16, a16 + 8
    # update(comm, V, ldv, ncols, h, w, n, iter, ncv, small, state, work, stream)
    assert lib.hpcla_eigsh_update_f64(None, P, 4, 1, None, P, 4, 1, 5, P, P, P, None) == INVALID
    assert lib.hpcla_eigsh_update_f64(None, P, 4, 1, P, P, 4, 1, 5, None, P, P, None) == INVALID
    assert lib.hpcla_eigsh_update_f64(None, P, 4, 1, P, P, 4, 1, 5, P, None, P, None) == INVALID
    assert lib.hpcla_eigsh_update_f64(None, P, 4, 1, P, P, 4, 1, 5, P, P, None, None) == INVALID
    assert lib.hpcla_eigsh_update_f64(None, None, 4, 1, P, None, 4, 1, 5, P, P, P, None) == INVALID
    assert lib.hpcla_eigsh_update_f64(None, P, 4, 1, P, P, 4, 0, 5, P, P, P, None) == INVALID          # iteration < 1
    assert lib.hpcla_eigsh_update_f64(None, P, 4, 6, P, P, 4, 1, 5, P, P, P, None) == INVALID          # ncols > ncv
    assert lib.hpcla_eigsh_update_f64(None, P, 4, 1, P, P, 4, 1, 65, P, P, P, None) == INVALID
    assert lib.hpcla_eigsh_update_f64(None, P, 5, 1, P, P, 4, 1, 5, P, P, P, None) == INVALID          # odd pitch
    assert lib.hpcla_eigsh_update_f64(None, P, 2, 1, P, P, 4, 1, 5, P, P, P, None) == INVALID          # pitch < n
    assert lib.hpcla_eigsh_update_f64(None, P, 4, 1, P, OFF, 4, 1, 5, P, P, P, None) == INVALID
    # rotate(V, ldv, m, p, S, move_last, out, out_row_stride, out_col_stride, n, stream)
    assert lib.hpcla_eigsh_rotate_f64(None, 4, 2, 1, P, 0, None, 0, 0, 4, None) == INVALID
    assert lib.hpcla_eigsh_rotate_f64(P, 4, 2, 1, None, 0, None, 0, 0, 4, None) == INVALID
    assert lib.hpcla_eigsh_rotate_f64(P, 4, 2, 1, P, 0, None, 0, 0, -1, None) == INVALID
    assert lib.hpcla_eigsh_rotate_f64(P, 5, 2, 1, P, 0, None, 0, 0, 4, None) == INVALID                # odd pitch
    assert lib.hpcla_eigsh_rotate_f64(P, 2, 2, 1, P, 0, None, 0, 0, 4, None) == INVALID                # pitch < n
    assert lib.hpcla_eigsh_rotate_f64(P, 4, 2, 0, P, 0, None, 0, 0, 4, None) == INVALID                # p < 1
    assert lib.hpcla_eigsh_rotate_f64(P, 4, 2, 3, P, 0, None, 0, 0, 4, None) == INVALID                # p > m
    assert lib.hpcla_eigsh_rotate_f64(P, 4, 65, 1, P, 0, None, 0, 0, 4, None) == INVALID
    assert lib.hpcla_eigsh_rotate_f64(OFF, 4, 2, 1, P, 0, None, 0, 0, 4, None) == INVALID
    assert lib.hpcla_eigsh_rotate_f64(P, 4, 2, 1, P, 0, P, 0, 1, 4, None) == INVALID                   # out with a zero stride
    assert lib.hpcla_eigsh_rotate_f64(P, 4, 2, 1, P, 1, P, 1, 1, 4, None) == INVALID                   # out with move_last
    assert lib.hpcla_eigsh_rotate_f64(P, 4, 2, 1, P, 0, None, 0, 0, 0, None) == 0                      # no rows: no work
    # steps_i64(plan, comm, rowptr, colval, nzval, nrows, nnz, base, interior, ni, boundary, nb, V, ldv, w, small, work, ncv,
    #           first_col, count, first_iter, stream)
    steps = lambda **kw: lib.hpcla_eigsh_steps_f64_i64(*[{**dict(
        plan=None, comm=None, rowptr=P, colval=P, nzval=P, nrows=4, nnz=4, base=0, interior=P, ni=0, boundary=P, nb=0, V=P, ldv=4,
        w=P, small=P, work=P, ncv=5, first_col=0, count=0, first_iter=1, stream=None), **kw}[key] for key in (
        "plan", "comm", "rowptr", "colval", "nzval", "nrows", "nnz", "base", "interior", "ni", "boundary", "nb", "V", "ldv", "w",
        "small", "work", "ncv", "first_col", "count", "first_iter", "stream")])
    assert steps() == 0                                          # count = 0 enqueues nothing
    for bad in (dict(nrows=-1), dict(ncv=0), dict(ncv=65), dict(first_col=-1), dict(count=-1), dict(first_col=3, count=3),
                dict(first_iter=0), dict(ldv=5), dict(ldv=2), dict(small=None), dict(work=None), dict(V=None), dict(w=OFF)):
        assert steps(**bad) == INVALID, bad


def test_argument_errors_that_need_no_device(hp):
    mod = sys.modules[hp.eigsh.__module__]                       # hp.eigsh is the function; its module holds the host functions
    assert mod.check_arguments(480, 6, "LA", None, None) == (6, 20, 4800)
    assert mod.check_arguments(480, 12, "SA", None, 7) == (12, 25, 7)
    assert mod.check_arguments(480, 40, "LM", None, None)[1] == 64
    assert mod.check_arguments(12, 3, "LA", None, None)[1] == 12
    assert mod.check_arguments(12, 3, "LA", 4, None)[1] == 4      # ncv = k + 1
    with pytest.raises(ValueError, match="shift-invert"):
        mod.check_arguments(480, 6, "SM", None, None)
    for bad in (dict(which="BE"), dict(which="la"), dict(k=0), dict(k=-1), dict(ncv=6), dict(ncv=5), dict(ncv=65),
                dict(n=30, ncv=31), dict(maxiter=-1)):
        args = {**dict(n=480, k=6, which="LA", ncv=None, maxiter=None), **bad}
        with pytest.raises(ValueError):
            mod.check_arguments(args["n"], args["k"], args["which"], args["ncv"], args["maxiter"])


def test_selection_by_which_and_ties(hp):
    mod = sys.modules[hp.eigsh.__module__]                       # hp.eigsh is the function; its module holds the host functions
    theta = np.array([-5.0, -1.0, 0.5, 2.0, 5.0, 3.0])
    assert mod.wanted_order(theta, "LA").tolist() == [4, 5, 3, 2, 1, 0]
    assert mod.wanted_order(theta, "SA").tolist() == [0, 1, 2, 3, 5, 4]
    assert mod.wanted_order(theta, "LM").tolist() == [4, 0, 5, 3, 1, 2]          # |-5| = |5|: the larger value first
    assert mod.wanted_order(np.array([2.0, -2.0, 2.0]), "LM").tolist() == [0, 2, 1]   # equal values: the lower index first
    for which in ("LA", "SA", "LM"):                             # the package's order is the restatement's
        assert mod.wanted_order(theta, which).tolist() == ec.order(theta, which).tolist()
    S = np.linalg.qr(np.arange(36.0).reshape(6, 6) + np.eye(6))[0]
    idx, vals, rho, anorm = mod.select(theta, S, 0.25, 3, "LM")
    assert idx.tolist() == [0, 5, 4] and vals.tolist() == [-5.0, 3.0, 5.0] and anorm == 5.0     # ascending in the value
    assert np.array_equal(rho, np.abs(0.25 * S[5, [0, 5, 4]]))
    assert np.array_equal(mod.estimates(-2.0, S, np.array([1])), np.abs(-2.0 * S[5, [1]]))


def test_choice_of_p(hp):
    mod = sys.modules[hp.eigsh.__module__]                       # hp.eigsh is the function; its module holds the host functions
    assert mod.kept_count(4, 20) == 12 and mod.kept_count(6, 32) == 19 and mod.kept_count(1, 8) == 4
    assert mod.kept_count(29, 64) == 46
    for k in range(1, 64):
        assert mod.kept_count(k, k + 1) == k                     # ncv = k + 1: only the wanted pairs are kept
        for m in range(k + 1, 65):
            assert k <= mod.kept_count(k, m) < m


def test_assembly_of_T_and_an_invariant_stop_with_fewer_columns_than_k(hp):
    mod = sys.modules[hp.eigsh.__module__]                       # hp.eigsh is the function; its module holds the host functions
    m = 5
    T_dev = np.arange(1.0, 26.0).reshape(m, m)                   # T_dev[j] is column j; entries below the diagonal are scratch
    T = mod.assemble_T(T_dev, np.zeros(0), 0, m)                 # the first cycle
    assert np.array_equal(T, T.T) and all(T[i, j] == T_dev[j, i] for j in range(m) for i in range(j + 1))
    kept = np.array([7.0, -3.0])
    T = mod.assemble_T(T_dev, kept, 2, m)                        # after a restart with p = 2: the arrow column is the device's
    assert np.array_equal(T, T.T) and np.array_equal(T[:2, :2], np.diag(kept))
    assert all(T[i, j] == T_dev[j, i] for j in range(2, m) for i in range(j + 1))
    assert np.array_equal(T, ec.symmetric_T(T_dev.T, kept, 2, m))
    T3 = mod.assemble_T(T_dev, kept, 2, 3)                       # an invariant stop with c = 3 finished columns
    assert np.array_equal(T3, T[:3, :3])
    theta, S = np.linalg.eigh(T3)
    idx, vals, rho, anorm = mod.select(theta, S, 0.0, 4, "LA")   # k = 4 > c = 3: the 3 pairs found, exact
    assert len(idx) == 3 and np.array_equal(vals, theta) and not rho.any() and anorm == np.abs(theta).max()


def test_restatement_meets_the_dense_spectrum(matrices):
    """Every convergence case of the GPU tests: converged, eigenvalues within 1e-13 anorm of numpy.linalg.eigvalsh, X orthonormal
    to 1e-13, and the true residual within 1.01 tol anorm: the stop rule bounds the estimate by tol anorm, and with full
    reorthogonalisation the true residual differs from it by rounding alone, about 1e-14 anorm = 1e-4 tol anorm (so the GPU
    tests' 2 tol anorm is a margin of 2)."""
    for name, k, ncv, whiches in ec.CONVERGENCE:
        rowptr, colidx, vals = matrices[name]
        ev = ec.dense_eigenvalues(rowptr, colidx, vals)
        for which in whiches:
            got, X, info = ec.eigsh(rowptr, colidx, vals, k=k, which=which, ncv=ncv)
            err = np.abs(got - ec.reference_values(ev, k, which)).max() / info["anorm"]
            AX = np.stack([pc.matvec(rowptr, colidx, vals, X[:, i]) for i in range(k)], axis=1)
            res = np.linalg.norm(AX - X * got, axis=0).max() / (ec.TOL * info["anorm"])
            orth = np.abs(X.T @ X - np.eye(k)).max()
            est = np.abs(np.linalg.norm(AX - X * got, axis=0) - info["residual_norms"]).max() / info["anorm"]
            print(f"{name} k {k} ncv {ncv} {which}: {info['iterations']} steps ({info['restarts'] + 1} cycles), eigenvalue error "
                  f"{err:.1e} anorm, true residual {res:.2f} tol anorm, orthogonality {orth:.1e}, estimate vs true residual "
                  f"{est:.1e} anorm")
            assert est <= 1e-13                                  # pair by pair: the estimates are aligned with the values
            assert info["status"] == "converged" and info["converged"]
            assert err <= 1e-13 and res <= 1.01 and orth <= 1e-13
            assert np.all(info["residual_norms"] <= ec.TOL * info["anorm"]) and len(info["history"]) == info["restarts"] + 1
            if (name, k, ncv, which) in STEPS:
                assert (info["iterations"], info["restarts"] + 1) == STEPS[name, k, ncv, which]


def test_spread_over_four_summation_orders(matrices):
    """The first cycle's T and beta, the eigenvalues and the step counts under the four orders of ``bc.DOTS``: the spreads the
    GPU tests' margins (T_RTOL and VAL_RTOL = 1e-12) are 10 times above at least; the counts agree.  The spread of T is bounded
    RELATIVE to max|T| of the case, on purpose: that is the measure the GPU test uses, and rounding scales with the matrix (the
    plain and saddle cases spread by 1.8e-15 .. 6.2e-15 absolute at max|T| = 4.2 .. 5.5, the scaled case by 2.6e-13 at
    max|T| = 274: all about 1e-15 of max|T|).  The absolute figures are printed next to it."""
    worst_T = worst_v = 0.0
    for name, k, ncv, whiches in ec.CONVERGENCE:
        rowptr, colidx, vals = matrices[name]
        for which in whiches:
            runs = []
            for dot in bc.DOTS.values():
                first = {}
                got, _, info = ec.eigsh(rowptr, colidx, vals, k=k, which=which, ncv=ncv, dot=dot, first_T=first)
                runs.append((got, info, first))
            assert len({(r[1]["iterations"], r[1]["restarts"], r[1]["status"]) for r in runs}) == 1, (name, k, which)
            scale = np.abs(runs[0][2]["T"]).max()
            sT = max(max(np.abs(r[2]["T"] - runs[0][2]["T"]).max(), np.abs(r[2]["beta"] - runs[0][2]["beta"]).max()) for r in runs)
            sv = max(np.abs(r[0] - runs[0][0]).max() for r in runs) / runs[0][1]["anorm"]
            print(f"{name} k {k} ncv {ncv} {which}: first-cycle T spread {sT:.1e} (max|T| {scale:.3g}), eigenvalue spread {sv:.1e} anorm")
            worst_T, worst_v = max(worst_T, sT / scale), max(worst_v, sv)
    print(f"worst: T {worst_T:.1e} relative, eigenvalues {worst_v:.1e} relative")
    assert worst_T <= ec.SPREAD and worst_v <= ec.SPREAD


def test_restatement_on_the_exact_cases():
    rowptr, colidx, d = pc.diag_matrix(np.arange(1.0, 13.0))
    e3 = np.zeros(12)
    e3[2] = 1.0
    got, X, info = ec.eigsh(rowptr, colidx, d, k=1, ncv=8, v0=e3)
    assert (info["status"], info["converged"], info["iterations"]) == ("invariant", True, 1) and got.tolist() == [3.0]
    got, X, info = ec.eigsh(rowptr, colidx, d, k=2, ncv=8, v0=e3)
    assert (info["status"], info["converged"], info["iterations"]) == ("invariant", False, 1) and got.tolist() == [3.0]
    assert X.shape == (12, 1)
    for which, want in (("LA", [10, 11, 12]), ("SA", [1, 2, 3]), ("LM", [10, 11, 12])):
        got, X, info = ec.eigsh(rowptr, colidx, d, k=3, ncv=12, which=which)
        assert (info["status"], info["iterations"], info["restarts"]) == ("converged", 12, 0)
        assert np.abs(got - want).max() <= 1e-12 * 12
    bad = d.copy()
    bad[5] = np.nan
    got, X, info = ec.eigsh(rowptr, colidx, bad, k=2, ncv=8)
    assert info["status"] == "breakdown" and got.shape == (2,) and X.shape == (12, 2)
    got, X, info = ec.eigsh(*pc.diag_matrix(np.arange(1.0, 61.0)), k=4, ncv=20, maxiter=5)       # maxiter inside the first cycle
    assert (info["status"], info["converged"], info["iterations"], info["restarts"]) == ("maxiter", False, 20, 0)
    assert len(info["history"]) == 1 and got.shape == (4,) and X.shape == (60, 4)


def test_first_cycle_spread_at_the_large_size(orc):
    """Plain Poisson at 65 x 63 (4095 rows, two reduction workgroups on the device), ncv = 20, one cycle: T and beta under the
    four summation orders.  T_RTOL, which tests/test_gpu_eigsh.py asks there, must be at least 10 times the spread relative to
    max|T| (measured: T 1.3e-15, beta 1.4e-15: 700 times)."""
    rowptr, colidx, vals = ec.plain_poisson(orc, *ec.LARGE_SIZE)
    assert len(rowptr) - 1 == 4095
    Ts, betas = [], []
    for dot in bc.DOTS.values():
        first = {}
        _, _, info = ec.eigsh(rowptr, colidx, vals, k=4, ncv=20, maxiter=1, dot=dot, first_T=first)
        assert (info["status"], info["iterations"], info["restarts"]) == ("maxiter", 20, 0)
        Ts.append(np.triu(first["T"]))
        betas.append(first["beta"])
    scale = np.abs(Ts[0]).max()
    sT = (np.max(Ts, axis=0) - np.min(Ts, axis=0)).max() / scale
    sb = (np.max(betas, axis=0) - np.min(betas, axis=0)).max() / scale
    print(f"plain {ec.LARGE_SIZE}: first-cycle T spread {sT:.1e}, beta {sb:.1e} (relative to max|T| = {scale:.3g})")
    assert pc.LARGE_MARGIN_FACTOR * max(sT, sb) <= ec.T_RTOL
