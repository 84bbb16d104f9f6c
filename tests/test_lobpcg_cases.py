"""CPU tests of the block eigensolver: the public names, the header and the binding, the C entries' argument checks (no launch),
the host's Rayleigh-Ritz step on hand-built Gram matrices, the argument rules, and the numpy restatement of the whole solve
(tests/_lobpcg_cases.py) on every convergence case -- with the figures the margins of tests/test_gpu_lobpcg.py are derived from,
re-measured and printed here:

  * iterations, true residuals, |vals - eigvalsh|, ||X'X - I|| and the drift |residual_norms - true residual| on every case;
  * their spread over four summation orders of the Gram matrices and over additive Gram noise of 1e-16, 1e-15 and 1e-14
    (relative to sqrt(G_ii G_jj)): no outcome changes; the iteration count moves by 3 % on the 16 x 16 grid and on the random
    matrix, and from 16 to between 15 and 23 on the Jacobi case (where a drop decision of the Rayleigh-Ritz step flips), which
    the cap of the GPU test, 1.5 x + 5, contains and which this file asserts with the same cap."""
import os
import re

import numpy as np
import pytest

from tests import _lobpcg_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_lobpcg_chunk_rows", "hpcla_lobpcg_work_bytes", "hpcla_lobpcg_residual_f64", "hpcla_lobpcg_combine_f64"]


@pytest.fixture(autouse=True)
def _the_solver_exists(hp):
    assert callable(getattr(hp, "lobpcg", None)), "hp.lobpcg is missing: there is nothing these figures are a yardstick of"


@pytest.fixture(scope="module")
def mats(orc):
    dense = lc.dense_matrices(orc)
    return dense, {name: np.linalg.eigvalsh(A) for name, A in dense.items()}


def test_public_names_exist(hp):
    assert callable(hp.lobpcg) and hp.LobpcgWorkspace and hp.LobpcgInfo
    assert hp.lobpcg.__module__.endswith("lobpcg")
    mod = lc.host()
    assert (mod.MAX_K, mod.RR_DROP, mod.WHICH) == (16, 1e-12, ("SA", "LA"))
    assert "lobpcg" in (hp.eigsh.__doc__ or "")                  # the limitation paragraph points to the remedy


def test_header_declares_the_new_entries_and_ctypes_binds_them(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in hp._capi.EXPORTED_SYMBOLS, name
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hpcla_rocm.h"
        assert m.group(1).count(",") + 1 == len(hp._capi._SIGNATURES[name]), name
    lib = hp._capi.load()
    rows = lib.hpcla_lobpcg_chunk_rows(1)
    assert rows == lib.hpcla_lobpcg_chunk_rows(rows) and rows >= 64
    assert lib.hpcla_lobpcg_work_bytes(rows, 3) == 8 * 3 and lib.hpcla_lobpcg_work_bytes(rows + 1, 16) == 8 * 16 * 2
    assert lib.hpcla_lobpcg_work_bytes(16 * rows + 1, 1) == 8 * 17
    big = 1 << 22                                                 # the chunk grows with n: the partial count stays bounded
    assert lib.hpcla_lobpcg_work_bytes(big, 16) == 8 * 16 * -(-big // lib.hpcla_lobpcg_chunk_rows(big)) <= 8 * 16 * 2048
    assert lib.hpcla_lobpcg_work_bytes(0, 4) == 8 == lib.hpcla_lobpcg_work_bytes(10, 17)


def test_c_entries_refuse_bad_arguments_without_a_gpu(hp):
    """Nulls, negative sizes, short pitches, k outside 1..16, c_rest outside {0, k, 2k}, misaligned arrays: refused on the
    host, nothing is launched."""
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    buf = np.zeros(64)                                           # host memory: only ever looked at as an address
    a16 = buf.ctypes.data + (-buf.ctypes.data) % 16
    P, OFF = a16, a16 + 4
    # residual(comm, X, ldx, AX, ldax, theta, minv, W, ldw, W2, ldw2, n, k, rn2, work, stream)
    res = lambda **kw: lib.hpcla_lobpcg_residual_f64(*[{**dict(
        comm=None, X=P, ldx=4, AX=P, ldax=4, theta=P, minv=None, W=P, ldw=4, W2=None, ldw2=0, n=4, k=4, rn2=P, work=P, stream=None),
        **kw}[key] for key in ("comm", "X", "ldx", "AX", "ldax", "theta", "minv", "W", "ldw", "W2", "ldw2", "n", "k", "rn2", "work",
                               "stream")])
    for bad in (dict(k=0), dict(k=17), dict(n=-1), dict(ldx=3), dict(ldax=3), dict(ldw=3), dict(W2=P, ldw2=3), dict(rn2=None),
                dict(rn2=OFF), dict(X=None), dict(AX=None), dict(W=None), dict(theta=None), dict(work=None), dict(X=OFF),
                dict(AX=OFF), dict(W=OFF), dict(W2=OFF, ldw2=4), dict(minv=OFF), dict(theta=OFF), dict(work=OFF)):
        assert res(**bad) == INVALID, bad
    # combine(S, lds, AS, ldas, C, k, c_rest, n, stream)
    comb = lambda **kw: lib.hpcla_lobpcg_combine_f64(*[{**dict(S=P, lds=12, AS=P, ldas=12, C=P, k=4, c_rest=4, n=4, stream=None),
                                                        **kw}[key] for key in ("S", "lds", "AS", "ldas", "C", "k", "c_rest", "n",
                                                                               "stream")])
    for bad in (dict(k=0), dict(k=17), dict(c_rest=1), dict(c_rest=12), dict(c_rest=-4), dict(n=-1), dict(lds=11), dict(ldas=11),
                dict(c_rest=0, lds=3), dict(C=None), dict(S=None), dict(S=OFF), dict(AS=OFF), dict(C=OFF)):
        assert comb(**bad) == INVALID, bad
    assert comb(n=0, S=None, AS=None) == 0                       # no rows: no work
    assert comb(n=0, c_rest=0, lds=4, ldas=4) == 0


# ---- the host's Rayleigh-Ritz step -----------------------------------------------------------------------------------------------
def _check_rr(S, A, k, which, kept):
    RR = lc.host().rayleigh_ritz
    theta, C, every = RR(S.T @ A @ S, S.T @ S, k, which)
    assert len(every) == kept and C.shape == (S.shape[1], min(k, kept)) and np.all(np.diff(theta) >= 0)
    Y = S @ C
    assert np.abs(Y.T @ Y - np.eye(C.shape[1])).max() <= 1e-12
    assert np.abs(Y.T @ A @ Y - np.diag(theta)).max() <= 1e-12 * np.abs(A).max() * S.shape[0]
    want = every[:len(theta)] if which == "SA" else every[len(every) - len(theta):]
    assert np.array_equal(theta, want)
    return theta, C, every


def test_rayleigh_ritz_on_hand_built_grams():
    rng = np.random.default_rng(1)
    n = 40
    A = rng.uniform(-1, 1, (n, n))
    A = A + A.T
    Q, _ = np.linalg.qr(rng.uniform(-1, 1, (n, 9)))
    # an orthonormal basis: the Ritz values are the eigenvalues of Q'AQ, nothing is dropped
    for which in ("SA", "LA"):
        theta, C, every = _check_rr(Q, A, 3, which, 9)
        assert np.abs(every - np.linalg.eigvalsh(Q.T @ A @ Q)).max() <= 1e-13 * n
    # a zero column drops out: its row of C is rounding noise (and multiplies zeros)
    S = Q.copy()
    S[:, 4] = 0.0
    theta, C, every = _check_rr(S, A, 3, "SA", 8)
    assert np.abs(C[4]).max() <= 1e-14
    assert np.abs(every - np.linalg.eigvalsh(np.delete(Q, 4, axis=1).T @ A @ np.delete(Q, 4, axis=1))).max() <= 1e-13 * n
    # two equal columns (scaled differently): one direction drops out, the Ritz values are those of the basis without the copy
    S = Q.copy() * rng.uniform(0.5, 2.0, 9)[None, :]
    S[:, 7] = 3.0 * S[:, 2]
    theta, C, every = _check_rr(S, A, 3, "LA", 8)
    assert np.abs(every - np.linalg.eigvalsh(np.delete(Q, 7, axis=1).T @ A @ np.delete(Q, 7, axis=1))).max() <= 1e-12 * n
    # 3k > n: n = 5 rows, 6 columns: at most 5 directions are kept
    S5, A5 = rng.uniform(-1, 1, (5, 6)), np.diag(np.arange(1.0, 6.0))
    theta, C, every = _check_rr(S5, A5, 2, "SA", 5)
    assert np.abs(every - np.arange(1.0, 6.0)).max() <= 1e-12 * 5
    # fewer kept directions than k: what there is, in order
    theta, C, every = _check_rr(np.hstack([Q[:, :2], Q[:, :1]]), A, 3, "SA", 2)
    assert len(theta) == 2
    # the Grams need not be exactly symmetric: they are symmetrised first
    G_A, G_B = Q.T @ A @ Q, Q.T @ Q
    skew = 1e-13 * np.triu(rng.uniform(-1, 1, (9, 9)), 1)
    RR = lc.host().rayleigh_ritz
    t1, t2 = RR(G_A + skew - skew.T, G_B, 3, "SA")[0], RR(G_A, G_B, 3, "SA")[0]
    assert np.array_equal(t1, t2) or np.abs(t1 - t2).max() <= 1e-14 * n


def test_argument_errors_that_need_no_device():
    mod = lc.host()
    assert mod.check_arguments(480, 6, "SA", 1e-8, None) == (6, 4800)
    assert mod.check_arguments(480, 16, "LA", 0.0, 7) == (16, 7)
    assert mod.check_arguments(5, 5, "SA", 1e-8, 0) == (5, 0)
    with pytest.raises(ValueError, match="shift-invert"):
        mod.check_arguments(480, 6, "SM", 1e-8, None)
    for bad in (dict(which="BE"), dict(which="LM"), dict(which="sa"), dict(k=0), dict(k=-1), dict(k=17), dict(n=5, k=6),
                dict(tol=-1.0), dict(tol=float("nan")), dict(maxiter=-1)):
        args = {**dict(n=480, k=6, which="SA", tol=1e-8, maxiter=None), **bad}
        with pytest.raises(ValueError):
            mod.check_arguments(args["n"], args["k"], args["which"], args["tol"], args["maxiter"])
    with pytest.raises(ValueError):
        mod.rayleigh_ritz(np.eye(2), np.eye(2), 1, "LM")
    # the decision order of step 4: non-finite first, then converged, then maxiter, then the Rayleigh-Ritz step
    I2, th = np.eye(2), np.array([1.0])
    assert mod.decide(np.array([np.nan]), I2, I2, th, 1.0, 1, 1, "SA", 1.0, 0)[0] == mod._BREAKDOWN
    assert mod.decide(np.array([0.0]), np.full((2, 2), np.inf), I2, th, 1.0, 1, 1, "SA", 1.0, 0)[0] == mod._BREAKDOWN
    assert mod.decide(np.array([0.0]), I2, I2, th, 1.0, 5, 1, "SA", 1e-8, 0)[0] == mod._CONVERGED
    assert mod.decide(np.array([1.0]), I2, I2, th, 1.0, 5, 1, "SA", 1e-8, 4)[0] == mod._MAXITER
    d, rn, theta, C, anorm = mod.decide(np.array([4.0]), np.diag([3.0, -7.0]), I2, th, 1.0, 4, 1, "SA", 1e-8, 4)
    assert (d, rn.tolist(), theta.tolist(), anorm) == (mod._GO, [2.0], [-7.0], 7.0) and C.shape == (2, 1)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_restatement_converges_on_every_case(mats):
    dense, ev = mats
    worst = np.zeros(4)
    for case, (name, k, which, M) in enumerate(lc.CONVERGENCE):
        A = dense[name]
        vals, X, info = lc.lobpcg(A, k, which, minv=lc.jacobi_weights(A) if M else None)
        fig = lc.figures(A, ev[name], vals, X, info, k, which)
        worst = np.maximum(worst, fig)
        print(f"{name} k {k} {which} {M}: {info['iterations']} iterations, |vals - eigvalsh| {fig[0]:.1e} ||A||, true residual "
              f"{fig[1]:.2f} tol anorm, ||X'X - I|| {fig[2]:.1e}, residual_norms vs true {fig[3]:.1e} anorm")
        assert info["status"] == "converged" and info["iterations"] == lc.ITERATIONS[case]
        assert fig[0] <= 2 * lc.TOL and fig[1] <= 2.0 and fig[2] <= lc.ORTH_TOL and fig[3] <= lc.DRIFT
        assert len(info["history"]) == info["iterations"] and info["history"][-1] == info["residual_norms"].max()
    print(f"worst: values {worst[0]:.1e} ||A||, residual {worst[1]:.2f} tol anorm, orthogonality {worst[2]:.1e}, drift {worst[3]:.1e}")
    assert worst[0] <= 1e-13                                     # far inside the GPU test's 2 tol ||A||


def test_the_documented_eigsh_failure_is_solved_by_the_block(mats):
    """The 16 x 16 grid, k = 4: lambda_11, lambda_12 = lambda_21 (the double value twice), lambda_22, and the mirror set."""
    dense, _ = mats
    for which in ("SA", "LA"):
        vals, _, info = lc.lobpcg(dense["poisson16"], 4, which)
        exact = lc.poisson16_exact(4, which)
        assert info["converged"] and np.abs(vals - exact).max() <= 2 * lc.TOL * 8.0
        assert abs(exact[1] - exact[2]) <= 1e-14 and abs(vals[1] - vals[2]) <= 2 * lc.TOL * 8.0     # the double value, twice


def test_spread_over_summation_orders_and_gram_noise(mats):
    dense, ev = mats
    for name, k, which, M in lc.SPREAD_CASES:
        A = dense[name]
        minv = lc.jacobi_weights(A) if M else None
        base = lc.ITERATIONS[lc.CONVERGENCE.index((name, k, which, M))]
        runs = [(f"order {o}", dict(gram=g)) for o, g in lc.GRAMS.items()]
        runs += [(f"noise {eps:.0e} seed {s}", dict(noise=eps, noise_seed=s)) for eps in (1e-16, 1e-15, 1e-14) for s in (0, 1)]
        counts, figs = [], []
        for label, kw in runs:
            vals, X, info = lc.lobpcg(A, k, which, minv=minv, **kw)
            assert info["status"] == "converged", (name, label)
            counts.append(info["iterations"])
            figs.append(lc.figures(A, ev[name], vals, X, info, k, which))
        figs = np.array(figs)
        print(f"{name} k {k} {which}: iterations {min(counts)} .. {max(counts)} (matmul order: {base}), values <= {figs[:, 0].max():.1e} "
              f"||A||, residual <= {figs[:, 1].max():.2f} tol anorm, orthogonality <= {figs[:, 2].max():.1e}, drift <= "
              f"{figs[:, 3].max():.1e} anorm")
        assert max(counts) <= 1.5 * base + 5 and base <= 1.5 * min(counts) + 5
        assert figs[:, 0].max() <= 1e-12 and figs[:, 1].max() <= 2.0 and figs[:, 2].max() <= lc.ORTH_TOL and figs[:, 3].max() <= lc.DRIFT


def test_first_iterations_spread(mats):
    """theta and anorm after the start and after iterations 1 and 2 under the four Gram orders: the spread that the GPU test's
    VAL_RTOL = 1e-12 anorm stands against (FIRST_CASES: <= 2.6e-15, 400 times less).  The Jacobi case is printed and not used
    there: its [X W] is ill conditioned in the first iterations (W = M .* R is nearly parallel to X while R is large), the Gram
    matrix squares that, and the summation order alone moves theta by 1.5e-10 anorm -- without changing where it converges."""
    dense, _ = mats
    for name, k, which, M in lc.SPREAD_CASES:
        A = dense[name]
        traces = []
        for g in lc.GRAMS.values():
            tr = []
            lc.lobpcg(A, k, which, minv=lc.jacobi_weights(A) if M else None, maxiter=2, gram=g, trace=tr)
            traces.append(tr)
        assert all(len(tr) == 3 for tr in traces)
        spread = max(max(np.abs(tr[s][0] - traces[0][s][0]).max(), abs(tr[s][1] - traces[0][s][1])) / traces[0][s][1]
                     for tr in traces for s in range(3))
        print(f"{name} k {k} {which}: theta and anorm of the first three projections spread by {spread:.1e} anorm")
        assert spread <= (1e-13 if (name, k, which, M) in lc.FIRST_CASES else 1e-8)


def test_restatement_on_the_exact_cases():
    for A in (np.eye(12), np.zeros((12, 12))):
        vals, X, info = lc.lobpcg(A, 3)
        assert (info["status"], info["iterations"]) == ("converged", 1) and np.abs(vals - A[0, 0]).max() <= 1e-15
    d5 = np.diag(np.arange(1.0, 6.0))
    vals, X, info = lc.lobpcg(d5, 5)                             # k = n: the start's projection is the whole problem
    assert info["status"] == "converged" and info["iterations"] <= 2 and np.abs(vals - np.arange(1.0, 6.0)).max() <= 1e-13
    vals, X, info = lc.lobpcg(d5, 2)                             # 3k > n: directions are dropped on the way
    assert info["status"] == "converged" and np.abs(vals - [1.0, 2.0]).max() <= 2 * lc.TOL * 5
    bad = d5.copy()
    bad[2, 2] = np.nan
    vals, X, info = lc.lobpcg(bad, 2)
    assert info["status"] == "breakdown" and np.isnan(vals).all() and not X.any()
    with pytest.raises(ValueError, match="rank deficient"):
        lc.lobpcg(d5, 2, X0=np.ones((5, 2)))
    vals, X, info = lc.lobpcg(np.diag(np.arange(1.0, 61.0)), 4, maxiter=3)
    assert (info["status"], info["iterations"], len(info["history"])) == ("maxiter", 4, 4)
