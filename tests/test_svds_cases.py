"""CPU side of the truncated SVD (``hp.svds``): the public names, the C ABI tables, the argument errors that need no device, the
pure-numpy host functions of svds.py (which gate stopped, the assembly of B), and the numpy restatement of the loop
(tests/_svds_cases.py) against the dense SVD and under four summation orders -- the measurement the margins of
tests/test_gpu_svds.py rest on, re-run and printed here.

The restatement's tests check the yardstick of the GPU tests, which means nothing without the solver it restates, so the whole
file asks for ``hp.svds`` first."""
import os
import re
import sys

import numpy as np
import pytest

from tests import _bicgstab_cases as bc
from tests import _pcg_cases as pc
from tests import _svds_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_svds_small_offset", "hpcla_svds_update_f64", "hpcla_svds_steps_f64_i32", "hpcla_svds_steps_f64_i64"]
# steps of the restatement at tol = 1e-10 on 24 x 20: the figures the GPU tests' step-count margins refer to
STEPS = {("tall", 4, 20): 100, ("tall", 1, 8): 112, ("tall", 16, 64): 160, ("wide", 4, 20): 108, ("wide", 1, 8): 112,
         ("wide", 16, 64): 160, ("plain", 4, 20): 108, ("plain", 1, 8): 112, ("plain", 16, 64): 160}


@pytest.fixture(autouse=True)
def _the_solver_exists(hp):
    assert callable(getattr(hp, "svds", None)), "hp.svds is missing: there is nothing these figures are a yardstick of"


@pytest.fixture(scope="module")
def matrices(orc):
    return sc.matrices(orc)


def test_public_names_exist(hp):
    assert callable(hp.svds) and hp.SvdsWorkspace and hp.SvdsInfo
    assert hp.svds.__module__.endswith("svds")
    assert "descending" in hp.svds.__doc__.lower()


def test_header_declares_the_new_entries_and_ctypes_binds_them(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in hp._capi.EXPORTED_SYMBOLS, name
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hpcla_rocm.h"
        assert m.group(1).count(",") + 1 == len(hp._capi._SIGNATURES[name]), name
    lib = hp._capi.load()
    for m in (1, 5, 20, 64):                                     # B, beta, g1, g2, h1, h2, aa, bb, dv in one buffer
        offs = [lib.hpcla_svds_small_offset(m, k) for k in range(10)]
        assert np.diff(offs).tolist() == [m * m, m, m, m, m, m, 1, 1, 1], m
    assert lib.hpcla_svds_small_offset(0, 0) == -1 == lib.hpcla_svds_small_offset(65, 0)
    assert lib.hpcla_svds_small_offset(5, 10) == -1 == lib.hpcla_svds_small_offset(5, -1)
    sig = hp._capi._SIGNATURES
    assert len(sig["hpcla_svds_steps_f64_i32"]) == len(sig["hpcla_svds_steps_f64_i64"]) + 4
    assert len(sig["hpcla_svds_steps_f64_i32"]) == len(sig["hpcla_lsqr_iterations_f64_i32"]) + 1


def test_c_entries_refuse_bad_arguments_without_a_gpu(hp):
    """Nulls, negative sizes, an odd or short pitch, a column count outside the side's range, misaligned vectors: refused on the
    host, nothing is launched."""
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    buf = np.zeros(64)                                           # host memory: only ever looked at as an address
    a16 = buf.ctypes.data + (-buf.ctypes.data) % 16
    P, OFF = a16, a16 + 8
    # update(comm, W, ldw, ncols, h, w, n, iter, ncv, side, small, state, work, stream)
    upd = lambda **kw: lib.hpcla_svds_update_f64(*[{**dict(
        comm=None, W=P, ldw=4, ncols=1, h=P, w=P, n=4, iter=1, ncv=5, side=0, small=P, state=P, work=P, stream=None), **kw}[key]
        for key in ("comm", "W", "ldw", "ncols", "h", "w", "n", "iter", "ncv", "side", "small", "state", "work", "stream")])
    for bad in (dict(h=None), dict(small=None), dict(state=None), dict(work=None), dict(W=None), dict(w=None), dict(iter=0),
                dict(ncv=0), dict(ncv=65), dict(ldw=5), dict(ldw=2), dict(n=-1), dict(w=OFF), dict(W=OFF), dict(side=2),
                dict(side=-1), dict(ncols=-1), dict(ncols=5),                  # left: 0 .. ncv - 1
                dict(side=1, ncols=0), dict(side=1, ncols=6)):                 # right: 1 .. ncv
        assert upd(**bad) == INVALID, bad
    # steps_i64(comm, [plan, rowptr, colval, nzval, nrows, nnz, base, interior, ni, boundary, nb] x 2, U, ldu, V, ldv, u, v,
    #           small, work, ncv, first_col, count, first_iter, stream)
    keys = ("comm", "plan", "rowptr", "colval", "nzval", "nrows", "nnz", "base", "interior", "ni", "boundary", "nb", "plan_t",
            "rowptr_t", "colval_t", "nzval_t", "nrows_t", "nnz_t", "base_t", "interior_t", "ni_t", "boundary_t", "nb_t", "U", "ldu",
            "V", "ldv", "u", "v", "small", "work", "ncv", "first_col", "count", "first_iter", "stream")
    steps = lambda **kw: lib.hpcla_svds_steps_f64_i64(*[{**dict(
        comm=None, plan=None, rowptr=P, colval=P, nzval=P, nrows=6, nnz=4, base=0, interior=P, ni=0, boundary=P, nb=0, plan_t=None,
        rowptr_t=P, colval_t=P, nzval_t=P, nrows_t=4, nnz_t=4, base_t=0, interior_t=P, ni_t=0, boundary_t=P, nb_t=0, U=P, ldu=6,
        V=P, ldv=4, u=P, v=P, small=P, work=P, ncv=5, first_col=0, count=0, first_iter=1, stream=None), **kw}[key] for key in keys])
    assert len(keys) == len(hp._capi._SIGNATURES["hpcla_svds_steps_f64_i64"])
    assert steps() == 0                                          # count = 0 enqueues nothing
    for bad in (dict(nrows=-1), dict(nrows_t=-1), dict(nnz_t=-1), dict(ncv=0), dict(ncv=65), dict(first_col=-1), dict(count=-1),
                dict(first_col=3, count=3), dict(first_iter=0), dict(ldu=7), dict(ldu=4), dict(ldv=5), dict(ldv=2),
                dict(small=None), dict(work=None), dict(U=None), dict(V=None), dict(u=None), dict(v=OFF), dict(U=OFF)):
        assert steps(**bad) == INVALID, bad


def test_argument_errors_that_need_no_device(hp):
    mod = sys.modules[hp.svds.__module__]                        # hp.svds is the function; its module holds the host functions
    assert mod.check_arguments(960, 480, 6, "LM", None, None) == (6, 20, 4800)
    assert mod.check_arguments(480, 960, 12, "LM", None, 7) == (12, 25, 7)
    assert mod.check_arguments(960, 480, 40, "LM", None, None)[1] == 64
    assert mod.check_arguments(30, 12, 3, "LM", None, None)[1] == 12
    assert mod.check_arguments(12, 30, 3, "LM", 4, None)[1] == 4  # ncv = k + 1
    with pytest.raises(ValueError, match="harmonic Ritz restarts or shift-invert"):
        mod.check_arguments(960, 480, 6, "SM", None, None)
    for bad in (dict(which="LA"), dict(which="lm"), dict(k=0), dict(k=-1), dict(ncv=6), dict(ncv=5), dict(ncv=65),
                dict(M=30, ncv=31), dict(N=30, ncv=31), dict(maxiter=-1)):
        args = {**dict(M=960, N=480, k=6, which="LM", ncv=None, maxiter=None), **bad}
        with pytest.raises(ValueError):
            mod.check_arguments(args["M"], args["N"], args["k"], args["which"], args["ncv"], args["maxiter"])


def test_which_gate_stopped_and_the_assembly_of_B(hp):
    mod = sys.modules[hp.svds.__module__]
    m = 5
    beta = np.array([0.5, 0.25, 0.0, 7.0, 7.0])
    assert mod.finished_columns(0, 0, 10, 2, m, beta) == (m, False)              # running: the whole cycle
    assert mod.finished_columns(4, 13, 10, 0, m, beta) == (3, False)             # Z' at column 2: beta[2] == 0
    assert mod.finished_columns(4, 12, 10, 0, m, beta) == (2, True)              # Z at column 2: beta[1] != 0
    assert mod.finished_columns(4, 10, 10, 3, m, beta) == (3, True)              # Z in a cycle's first left half: c == p
    assert mod.finished_columns(2, 11, 10, 0, m, beta) == (1, False)             # breakdown
    B_dev = np.arange(1.0, 26.0).reshape(m, m)                   # B_dev[j] is column j; entries below the diagonal are scratch
    B = mod.assemble_B(B_dev, np.zeros(0), 0, m, m)              # the first cycle
    assert not np.tril(B, -1).any() and all(B[i, j] == B_dev[j, i] for j in range(m) for i in range(j + 1))
    kept = np.array([7.0, 3.0])
    B = mod.assemble_B(B_dev, kept, 2, m, m)                     # after a restart with p = 2: the arrow column is the device's
    assert np.array_equal(B[:2, :2], np.diag(kept)) and not np.tril(B, -1).any()
    assert all(B[i, j] == B_dev[j, i] for j in range(2, m) for i in range(j + 1))
    assert np.array_equal(B, sc.projected(B_dev.T, kept, 2, m, m))
    B3 = mod.assemble_B(B_dev, kept, 2, 3, 4)                    # gate Z with c = 3: the 3 x 4 block with column 3
    assert B3.shape == (3, 4) and np.array_equal(B3, B[:3, :4]) and np.array_equal(B3, sc.projected(B_dev.T, kept, 2, 3, 4))
    assert np.array_equal(mod.assemble_B(B_dev, kept, 2, 2, 3), B[:2, :3])       # gate Z at c == p


def test_restatement_meets_the_dense_svd(matrices):
    """Every convergence case of the GPU tests: converged, singular values within 1e-13 anorm of numpy.linalg.svd, U and V
    orthonormal to 1e-13, u_i' A v_i > 0, A v - s u within 1e-13 anorm, and the true residual ||A' u - s v|| within 1.01 tol
    anorm: the stop rule bounds the estimate by tol anorm, and with full reorthogonalisation the true residual differs from it by
    rounding alone, about 1e-14 anorm = 1e-4 tol anorm (so the GPU tests' 2 tol anorm is a margin of 2)."""
    for name, k, ncv in sc.CONVERGENCE:
        M = matrices[name]
        U, s, V, info = sc.svds(*M, k=k, ncv=ncv)
        f = sc.figures(*M, U, s, V, info, sc.dense_singular_values(*M))
        print(f"{name} k {k} ncv {ncv}: {info['iterations']} steps ({info['restarts'] + 1} cycles), value error {f['err']:.1e} "
              f"anorm, true residual {f['res']:.2f} tol anorm, A v - s u {f['left']:.1e} anorm, orthogonality {f['orth']:.1e}, "
              f"estimate vs true residual {f['est']:.1e} anorm")
        assert info["status"] == "converged" and info["converged"]
        assert s.shape == (k,) and np.all(np.diff(s) < 0) and U.shape == (len(M[0]) - 1, k) and V.shape == (M[3], k)
        assert f["err"] <= 1e-13 and f["res"] <= 1.01 and f["orth"] <= 1e-13 and f["left"] <= 1e-13 and f["est"] <= 1e-13
        assert f["sign"] > 0
        assert np.all(info["residual_norms"] <= sc.TOL * info["anorm"]) and len(info["history"]) == info["restarts"] + 1
        p = k + (ncv - k) // 2
        assert info["iterations"] == ncv + info["restarts"] * (ncv - p) == STEPS[name, k, ncv]


def test_spread_over_four_summation_orders(matrices):
    """The first cycle's B and beta, the singular values and the step counts under the four orders of ``bc.DOTS``: the spreads
    the GPU tests' margins (T_RTOL and VAL_RTOL = 1e-12) are 10 times above at least; the counts are identical."""
    worst_B = worst_v = 0.0
    for name, k, ncv in sc.CONVERGENCE:
        M = matrices[name]
        runs = []
        for dot in bc.DOTS.values():
            first = {}
            _, s, _, info = sc.svds(*M, k=k, ncv=ncv, dot=dot, first_B=first)
            runs.append((s, info, first))
        assert len({(r[1]["iterations"], r[1]["restarts"], r[1]["status"]) for r in runs}) == 1, (name, k, ncv)
        scale = np.abs(runs[0][2]["B"]).max()
        sB = max(max(np.abs(r[2]["B"] - runs[0][2]["B"]).max(), np.abs(r[2]["beta"] - runs[0][2]["beta"]).max()) for r in runs)
        sv = max(np.abs(r[0] - runs[0][0]).max() for r in runs) / runs[0][1]["anorm"]
        print(f"{name} k {k} ncv {ncv}: first-cycle B and beta spread {sB:.1e} (max|B| {scale:.3g}), value spread {sv:.1e} anorm")
        worst_B, worst_v = max(worst_B, sB / scale), max(worst_v, sv)
    print(f"worst: B {worst_B:.1e} relative, singular values {worst_v:.1e} relative")
    assert worst_B <= sc.SPREAD and worst_v <= sc.SPREAD


def test_restatement_on_the_exact_cases():
    D = (*pc.diag_matrix(np.arange(1.0, 13.0)), 12)
    e3 = np.zeros(12)
    e3[2] = 1.0
    U, s, V, info = sc.svds(*D, k=1, ncv=8, v0=e3)               # A e_3 = 3 e_3, A' e_3 = 3 e_3: gate Z' in the first step
    assert (info["status"], info["converged"], info["iterations"]) == ("invariant", True, 1) and s.tolist() == [3.0]
    assert np.array_equal(np.abs(U[:, 0]), e3) and np.array_equal(np.abs(V[:, 0]), e3) and info["residual_norms"].tolist() == [0.0]
    U, s, V, info = sc.svds(*D, k=2, ncv=8, v0=e3)
    assert (info["status"], info["converged"], info["iterations"]) == ("invariant", False, 1) and s.tolist() == [3.0]
    assert U.shape == (12, 1) and V.shape == (12, 1)
    U, s, V, info = sc.svds(*D, k=3, ncv=12)                     # ncv = min(M, N): the whole wanted set after one cycle
    assert (info["status"], info["iterations"], info["restarts"]) == ("converged", 12, 0)
    assert np.abs(s - [12, 11, 10]).max() <= 1e-12 * 12
    U, s, V, info = sc.svds(*sc.rank_deficient(), k=1, ncv=3, v0=sc.RANK_DEFICIENT_V0)
    assert (info["status"], info["converged"], info["iterations"]) == ("invariant", True, 1)      # gate Z at column 1
    assert abs(s[0] - 4.0) <= 4e-15 and info["residual_norms"].tolist() == [0.0] and U.shape == (6, 1) and V.shape == (4, 1)
    assert np.array_equal(np.abs(U[:, 0]), np.eye(6)[0]) and np.abs(np.abs(V[:, 0]) - np.eye(4)[0]).max() <= 1e-15
    _, s, _, info = sc.svds(*sc.rank_deficient(), k=2, ncv=3, v0=sc.RANK_DEFICIENT_V0)
    assert (info["status"], info["converged"], info["iterations"], len(s)) == ("invariant", False, 1, 1)
    U, s, V, info = sc.svds(*sc.rank_deficient(), k=1, ncv=3, v0=np.eye(4)[1])                    # a start inside the null space
    assert (info["status"], info["converged"], info["iterations"], info["anorm"]) == ("invariant", False, 0, 0.0)
    assert s.shape == (0,) and U.shape == (6, 0) and V.shape == (4, 0)
    bad = np.arange(1.0, 13.0)
    bad[5] = np.nan
    U, s, V, info = sc.svds(*pc.diag_matrix(bad), 12, k=2, ncv=8)
    assert info["status"] == "breakdown" and s.shape == (2,) and np.isnan(s).all() and U.shape == (12, 2) and not U.any()
    U, s, V, info = sc.svds(*pc.diag_matrix(np.arange(1.0, 61.0)), 60, k=4, ncv=20, maxiter=5)   # maxiter inside the first cycle
    assert (info["status"], info["converged"], info["iterations"], info["restarts"]) == ("maxiter", False, 20, 0)
    assert len(info["history"]) == 1 and s.shape == (4,) and U.shape == (60, 4)


def test_first_cycle_spread_at_the_large_size(orc):
    """``tall`` at 65 x 63 (8190 x 4095: an odd local length on the right side, two reduction workgroups on the device),
    ncv = 20, one cycle: B and beta under the four summation orders.  T_RTOL, which tests/test_gpu_svds.py asks there, must be
    at least 10 times the spread relative to max|B|."""
    M = sc.matrix(orc, "tall", sc.LARGE_SIZE)
    assert (len(M[0]) - 1, M[3]) == (8190, 4095)
    Bs, betas = [], []
    for dot in bc.DOTS.values():
        first = {}
        _, _, _, info = sc.svds(*M, k=4, ncv=20, maxiter=1, dot=dot, first_B=first)
        assert (info["status"], info["iterations"], info["restarts"]) == ("maxiter", 20, 0)
        Bs.append(np.triu(first["B"]))
        betas.append(first["beta"])
    scale = np.abs(Bs[0]).max()
    sB = (np.max(Bs, axis=0) - np.min(Bs, axis=0)).max() / scale
    sb = (np.max(betas, axis=0) - np.min(betas, axis=0)).max() / scale
    print(f"tall {sc.LARGE_SIZE}: first-cycle B spread {sB:.1e}, beta {sb:.1e} (relative to max|B| = {scale:.3g})")
    assert pc.LARGE_MARGIN_FACTOR * max(sB, sb) <= sc.T_RTOL
