"""CPU tests of the block eigensolver on a pencil (``hp.lobpcg`` with ``B``): the public names, the header and the binding of
the two new entries, their argument checks (no launch), the host's ``decide_gen`` and ``check_b`` on hand-made inputs, and the
numpy restatement of the whole solve (tests/_lobpcg_gen_cases.py) on every convergence case, checked against
``scipy.linalg.eigh(K, M)`` with the margins of tests/test_gpu_lobpcg_gen.py.  The figures are re-measured and printed here:

  * iterations (held to the suite's cap 1.5 x + 5 around the recorded counts: the long runs move by a few with the summation
    order), the eigenvalue error in units of its bound 2 tol (||A x|| + |theta| ||B x||) / sqrt(lambda_min(B)), the true residual
    in units of tol x the true scale, ||X'BX - I||_max;
  * the diagonal B as weights and as a matrix: the same iteration."""
import os
import re

import numpy as np
import pytest

from tests import _lobpcg_cases as lc
from tests import _lobpcg_gen_cases as gc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_lobpcg_gen_work_bytes", "hpcla_lobpcg_residual_gen_f64"]


@pytest.fixture(scope="module")
def pencils():
    return gc.pencils()


def test_public_names_and_info_fields(hp):
    mod = gc.host()
    assert callable(mod.decide_gen) and callable(mod.check_b)
    info = hp.LobpcgInfo(True, "converged", 1, np.zeros(2))      # the constructions from before the pencil keep working
    assert info.residual_scales.shape == (0,) and info.anorm == 0.0
    import inspect
    params = list(inspect.signature(hp.lobpcg).parameters)
    assert params[-1] == "B" and params[:9] == ["A", "k", "which", "X0", "M", "tol", "maxiter", "seed", "workspace"]
    assert "No generalised problem" not in (hp.lobpcg.__doc__ or "")
    assert list(inspect.signature(hp.LobpcgWorkspace.__init__).parameters)[1:] == ["A", "k", "B"]


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
    # three sums per column and chunk: three times the partials of the standard problem
    for n, k in ((rows, 3), (rows + 1, 16), (16 * rows + 1, 1), (1 << 22, 16)):
        assert lib.hpcla_lobpcg_gen_work_bytes(n, k) == 3 * lib.hpcla_lobpcg_work_bytes(n, k)
    assert lib.hpcla_lobpcg_gen_work_bytes(rows + 1, 16) == 8 * 3 * 16 * 2
    assert lib.hpcla_lobpcg_gen_work_bytes(0, 4) == 8 == lib.hpcla_lobpcg_gen_work_bytes(10, 17)


def test_the_c_entry_refuses_bad_arguments_without_a_gpu(hp):
    """Nulls, negative sizes, short pitches, k outside 1..16, misaligned arrays, bdiag without BW and BW without bdiag: refused
    on the host, nothing is launched."""
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    buf = np.zeros(64)                                           # host memory: only ever looked at as an address
    a16 = buf.ctypes.data + (-buf.ctypes.data) % 16
    P, OFF = a16, a16 + 4
    keys = ("comm", "AX", "ldax", "BX", "ldbx", "theta", "minv", "bdiag", "W", "ldw", "W2", "ldw2", "BW", "ldbw", "n", "k", "sums",
            "work", "stream")
    assert len(keys) == len(hp._capi._SIGNATURES["hpcla_lobpcg_residual_gen_f64"])
    base = dict(comm=None, AX=P, ldax=4, BX=P, ldbx=4, theta=P, minv=None, bdiag=None, W=P, ldw=4, W2=None, ldw2=0, BW=None, ldbw=0,
                n=4, k=4, sums=P, work=P, stream=None)
    res = lambda **kw: lib.hpcla_lobpcg_residual_gen_f64(*[{**base, **kw}[key] for key in keys])
    for bad in (dict(k=0), dict(k=17), dict(n=-1), dict(ldax=3), dict(ldbx=3), dict(ldw=3), dict(W2=P, ldw2=3),
                dict(bdiag=P, BW=P, ldbw=3), dict(sums=None), dict(sums=OFF), dict(AX=None), dict(BX=None), dict(W=None),
                dict(theta=None), dict(work=None), dict(AX=OFF), dict(BX=OFF), dict(W=OFF), dict(W2=OFF, ldw2=4), dict(minv=OFF),
                dict(theta=OFF), dict(work=OFF), dict(bdiag=OFF, BW=P, ldbw=4), dict(bdiag=P, BW=OFF, ldbw=4),
                dict(bdiag=P), dict(BW=P, ldbw=4)):
        assert res(**bad) == INVALID, bad
        assert "lobpcg_residual_gen" in hp._capi.last_error(), bad


# ---- the host's decision ---------------------------------------------------------------------------------------------------------
def _sums(d2, a2, b2):
    out = np.full(48, 7.0)                                       # the entries j >= k are never looked at
    for q, v in enumerate((d2, a2, b2)):
        out[16 * q:16 * q + len(v)] = v
    return out


def test_decide_gen_on_hand_made_inputs():
    mod = gc.host()
    I2, th = np.eye(2), np.array([2.0])
    ok = _sums([0.0], [4.0], [1.0])
    # a non-finite value anywhere that is used: breakdown, before everything else
    for sums, G_A, G_B in ((_sums([np.nan], [4.0], [1.0]), I2, I2), (_sums([0.0], [np.inf], [1.0]), I2, I2),
                           (_sums([0.0], [4.0], [np.nan]), I2, I2), (ok, np.full((2, 2), np.inf), I2),
                           (ok, I2, np.array([[1.0, np.nan], [np.nan, 1.0]]))):
        out = mod.decide_gen(sums, G_A, G_B, th, 1.0, 1, 1, "SA", 1.0, 0)
        assert out[0] == mod._BREAKDOWN and np.isnan(out[1]).all() and np.isnan(out[2]).all()
        assert gc.decide_gen(sums, G_A, G_B, th, 1.0, 1, 1, "SA", 1.0, 0)[0] == "breakdown"
    unused = ok.copy()
    unused[5] = np.nan                                           # an entry j >= k is not looked at
    assert mod.decide_gen(unused, I2, I2, th, 1.0, 1, 1, "SA", 1e-8, 9)[0] == mod._CONVERGED
    # a negative diagonal entry of S'BS: B is not positive definite on that basis column -- even where the rule would stop
    for G_B in (np.diag([1.0, -1e-30]), np.diag([-1.0, 1.0]), -I2):
        assert mod.decide_gen(ok, I2, G_B, th, 1.0, 1, 1, "SA", 1.0, 0)[0] == mod._BREAKDOWN
        assert gc.decide_gen(ok, I2, G_B, th, 1.0, 1, 1, "SA", 1.0, 0)[0] == "breakdown"
    assert mod.decide_gen(ok, I2, np.diag([1.0, 0.0]), th, 1.0, 1, 1, "SA", 1.0, 0)[0] == mod._CONVERGED   # a zero column is no breakdown
    # converged comes before maxiter; the rule is rn <= tol (||A x|| + |theta| ||B x||) = 2^-20 (2 + 2 * 1), met with equality
    # (powers of two: every figure is exact)
    tol = 2.0 ** -20
    d, rn, scale, theta, C, anorm = mod.decide_gen(_sums([2.0 ** -36], [4.0], [1.0]), I2, I2, th, 1.0, 5, 1, "SA", tol, 0)
    assert (d, rn.tolist(), scale.tolist()) == (mod._CONVERGED, [2.0 ** -18], [4.0]) and C is None and theta is th
    assert mod.decide_gen(_sums([2.0 ** -34], [4.0], [1.0]), I2, I2, th, 1.0, 5, 1, "SA", tol, 4)[0] == mod._MAXITER
    assert mod.decide_gen(_sums([2.0 ** -36], [4.0], [1.0]), I2, I2, -th, 1.0, 5, 1, "SA", tol, 4)[0] == mod._CONVERGED   # |theta|
    assert mod.decide_gen(_sums([2.0 ** -34], [4.0], [1.0]), I2, I2, th, 1.0, 4, 1, "SA", tol, 4)[0] == mod._GO
    # otherwise the Rayleigh-Ritz step on (G_A, G_B): the pencil (diag(3, -8), diag(1, 4)) has the values 3 and -2
    d, rn, scale, theta, C, anorm = mod.decide_gen(_sums([4.0], [4.0], [1.0]), np.diag([3.0, -8.0]), np.diag([1.0, 4.0]), th, 1.0, 4, 1,
                                                   "SA", 1e-8, 4)
    assert (d, rn.tolist(), theta.tolist(), anorm) == (mod._GO, [2.0], [-2.0], 3.0) and C.shape == (2, 1)
    assert abs(abs(C[1, 0]) - 0.5) <= 1e-15 and abs(C[0, 0]) <= 1e-15      # B-normalised: c' diag(1, 4) c = 1
    want = gc.decide_gen(_sums([4.0], [4.0], [1.0]), np.diag([3.0, -8.0]), np.diag([1.0, 4.0]), th, 1.0, 4, 1, "SA", 1e-8, 4)
    assert want[0] is None and np.array_equal(want[3], theta) and np.array_equal(want[4], C) and want[5] == anorm
    # the two Gram blocks of the device's product S'[AS | BS]
    G = np.arange(3 * 2 * 6 * 2, dtype=np.float64).reshape(6, 12)
    G_A, G_B = mod.grams_gen(G, 2, 4)
    assert np.array_equal(G_A, G[:4, :4]) and np.array_equal(G_B, G[:4, 6:10])


def test_check_b_argument_rules():
    mod = gc.host()
    h, other = b"rows of A", b"another partition"
    assert mod.check_b(None, 10, h) is None
    assert mod.check_b("sparse", 10, h, (10, 10), h, h) == "sparse"
    assert mod.check_b("vector", 10, h, (10,), h) == "diagonal"
    for bad in (dict(kind="sparse", shape=(10, 12), row_hash=h, col_hash=other),         # not square
                dict(kind="sparse", shape=(12, 12), row_hash=other, col_hash=other),     # another size
                dict(kind="sparse", shape=(10, 10), row_hash=other, col_hash=h),         # rows on another partition
                dict(kind="sparse", shape=(10, 10), row_hash=h, col_hash=other),         # columns on another partition
                dict(kind="sparse", shape=(10, 10), row_hash=h, col_hash=h, same_backend=False),
                dict(kind="vector", shape=(12,), row_hash=other), dict(kind="vector", shape=(10,), row_hash=other),
                dict(kind="vector", shape=(10,), row_hash=h, same_backend=False),
                dict(kind="ndarray"), dict(kind="HPCMatrix"), dict(kind="str")):
        with pytest.raises(ValueError, match="lobpcg: B must be"):
            mod.check_b(bad.pop("kind"), 10, h, **bad)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_restatement_converges_on_every_case(pencils):
    worst = np.zeros(3)
    for case, (name, form, k, which) in enumerate(gc.CONVERGENCE):
        K, M = pencils[name]
        Bd = gc.b_of(M, form)
        want, bmin = gc.reference(K, Bd, k, which)
        runs = [("matrix", Bd)] + ([("weights", gc.lumped(M))] if form == "lumped" else [])
        seen = []
        for label, B in runs:
            vals, X, info = gc.lobpcg_gen(K, B, k, which)
            fig = gc.figures(K, Bd, want, bmin, vals, X)
            worst = np.maximum(worst, fig)
            print(f"{name} {form} ({label}) k {k} {which}: {info['iterations']} iterations (recorded {gc.ITERATIONS[case]}), "
                  f"eigenvalue error {fig[0]:.1e} of its bound, true residual {fig[1]:.2f} tol scale, ||X'BX - I|| {fig[2]:.1e}")
            assert info["status"] == "converged" and np.all(np.diff(vals) >= 0)
            assert info["iterations"] <= 1.5 * gc.ITERATIONS[case] + 5 and gc.ITERATIONS[case] <= 1.5 * info["iterations"] + 5
            assert fig[0] <= 1.0 and fig[1] <= pc.TRUE_RES_FACTOR and fig[2] <= lc.ORTH_TOL
            assert np.all(info["residual_norms"] <= gc.TOL * info["residual_scales"])
            assert len(info["history"]) == info["iterations"] and info["history"][-1] == info["residual_norms"].max()
            seen.append((info["iterations"], vals))
        if len(seen) == 2:                                       # the weights and the diagonal matrix: the same iteration
            assert seen[0][0] == seen[1][0] and np.abs(seen[0][1] - seen[1][1]).max() <= lc.VAL_RTOL * info["anorm"]
    print(f"worst: eigenvalue error {worst[0]:.1e} of its bound, residual {worst[1]:.2f} tol scale, B-orthonormality {worst[2]:.1e}")
    assert worst[0] <= 1e-3                                      # far inside the bound the GPU test uses


def test_the_double_eigenvalues_are_found_twice(pencils):
    """fem2d(16): lambda_12 = lambda_21 lies inside the k = 4 block, and the k = 5 block cuts through lambda_13 = lambda_31."""
    K, M = pencils["fem2d16"]
    import scipy.linalg
    ev = scipy.linalg.eigh(K, M, eigvals_only=True)
    assert abs(ev[1] - ev[2]) <= 1e-10 * ev[-1] and abs(ev[4] - ev[5]) <= 1e-10 * ev[-1] and ev[3] - ev[2] >= 1.0
    vals, _, info = gc.lobpcg_gen(K, M, 4, "SA")
    assert info["converged"] and abs(vals[1] - vals[2]) <= 1e-6 * vals[2] and np.abs(vals - ev[:4]).max() <= 1e-6 * ev[3]


def test_restatement_edge_cases():
    K, M = gc.fem1d(12)
    vals, X, info = gc.lobpcg_gen(K, -np.eye(12), 3)             # B = -I: the start's X'BX has a negative diagonal
    assert info["status"] == "breakdown" and info["iterations"] == 0 and np.isnan(vals).all() and not X.any()
    bad = M.copy()
    bad[5, 5] = np.nan
    vals, X, info = gc.lobpcg_gen(K, bad, 2)
    assert info["status"] == "breakdown" and np.isnan(info["residual_scales"]).all()
    with pytest.raises(ValueError, match="rank deficient"):
        gc.lobpcg_gen(K, M, 2, X0=np.ones((12, 2)))
    vals, X, info = gc.lobpcg_gen(K, M, 2, maxiter=3)
    assert (info["status"], info["iterations"], len(info["history"])) == ("maxiter", 4, 4)
    vals, X, info = gc.lobpcg_gen(K, gc.lumped(M), 12)           # k = n: the start's projection is the whole problem
    import scipy.linalg
    assert info["status"] == "converged" and info["iterations"] <= 2
    assert np.abs(vals - scipy.linalg.eigh(K, np.diag(gc.lumped(M)), eigvals_only=True)).max() <= 1e-12 * vals.max()
    # B = I: the eigenvalues of the standard problem (the stop rules differ, so the counts may)
    A = lc.ddom(257)
    v0, _, i0 = lc.lobpcg(A, 4, "SA")
    v1, _, i1 = gc.lobpcg_gen(A, np.eye(257), 4, "SA")
    assert i0["converged"] and i1["converged"] and np.abs(v0 - v1).max() <= 2 * gc.TOL * i0["anorm"]


def test_the_residual_restatement_matches_its_formula():
    rng = np.random.default_rng(3)
    AX, BX, theta = rng.uniform(-1, 1, (9, 3)), rng.uniform(-1, 1, (9, 3)), rng.uniform(-2, 2, 3)
    minv, bd = rng.uniform(0.5, 2, 9), rng.uniform(0.5, 2, 9)
    W, BW, d = gc.residual_gen(AX, BX, theta, minv, bd)
    for r in range(9):
        for j in range(3):
            t = theta[j] * BX[r, j]
            dd = AX[r, j] - t
            w = minv[r] * dd
            assert (d[r, j], W[r, j], BW[r, j]) == (dd, w, bd[r] * w)
    W, BW, d = gc.residual_gen(AX, BX, theta)
    assert BW is None and np.array_equal(W, d)
    sums = gc.sums_gen(d, AX, BX)
    assert sums.shape == (48,) and not sums[3:16].any() and sums[16] == (AX[:, 0] ** 2).sum() and sums[34] == (BX[:, 2] ** 2).sum()
