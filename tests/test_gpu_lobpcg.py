"""GPU tests of the block eigensolver: the residual and the combine kernel on their own through the C ABI, the first iterations
against the numpy restatement, convergence against the dense spectrum, the case hp.eigsh documents as its failure, the exact
and edge cases, the argument errors and the solve across ranks.  Cases and the restatement: tests/_lobpcg_cases.py.

Margins (none of them taken from the device's results; tests/test_lobpcg_cases.py re-measures the CPU figures and prints them):
  * W of the residual kernel and X', P' of the combine kernel: bit-equal to numpy's separately rounded expressions (the
    library is built with -ffp-contract=off; the combine kernel uses plain multiplies and adds, no MFMA);
  * the residual kernel's sums of squares: 1e-12 of math.fsum relative to the sum of |terms|, the project's margin for its
    reductions; the same bits on a second call;
  * theta and anorm of the first two iterations: VAL_RTOL = 1e-12 of anorm against the restatement (four summation orders on
    the CPU spread by <= 2.6e-15 on these two cases: 400 times less);
  * converged runs: |vals - eigvalsh| <= 2 tol ||A||_2 (the restatement: 4.3e-15 ||A||), true residuals <= 2 tol anorm (hp.gmres's
    factor; the restatement: <= 0.98), ||X'X - I||_max <= 1e-12 (8.3e-15), residual_norms within (1e-12 + DRIFT) anorm of the
    true residuals (DRIFT = 2e-14: iterations x epsilon; measured 4.2e-16), iterations <= 1.5 x the restatement's + 5 (a cap:
    a combine that loses P needs 3 to 8 times as many, summation order and Gram noise moved the count from 16 to at most 23);
    measured on an MI355X: the restatement's count +- 6 everywhere except rand300 k = 5 "SA", 163 against 110 (cap 170): the
    5th to 7th eigenvalues lie within 0.06 and a direction kept just above the Rayleigh-Ritz drop threshold throws the residual
    back once, which other starts show in numpy too (profiles/MEASUREMENTS_lobpcg.md);
  * ranks: vals within 1e-12 anorm of the one-rank result; the ranks' vals and info bit-identical.
Eigenvector signs are not compared."""
import math
import os

import numpy as np
import pytest

from tests import _lobpcg_cases as lc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_lobpcg_worker.py")

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 7, 8, 15, 16)


def _sizes(hp):
    """n = 1 .. 257, one n past the first chunk of partials (two stage-1 workgroups) and one past the first phase of the second
    stage (17 chunks: phase 0 adds two of them), both named from the library's constant."""
    chunk = hp._capi.load().hpcla_lobpcg_chunk_rows(1)
    return (1, 2, 63, 64, 65, 257, chunk + 1, 16 * chunk + 1)


def _matrix(hp, backend, dense):
    rowptr, colidx, vals, n = lc.csr_of(dense)
    return hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, backend)


def _bits_eq(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    return np.array_equal(pc.bits(got), pc.bits(want))


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).cuda()


def _padded(block, pitch, lead=0):
    """The (n, k) block inside an (n, pitch) buffer poisoned with NaN, ``lead`` poisoned doubles in front (an odd ``lead``
    breaks the 16-byte alignment).  Returns (flat device tensor, view of the (n, pitch) rows)."""
    n, k = block.shape
    buf = np.full(lead + n * pitch, np.nan)
    rows = buf[lead:].reshape(n, pitch)
    rows[:, :k] = block
    t = _dev(buf)
    return t, t[lead:].view(n, pitch)


@pytest.fixture(scope="module")
def cases(orc):
    """Every matrix with its dense spectrum and the restatement's results, computed once."""
    dense = lc.dense_matrices(orc)
    out = {"dense": dense, "ev": {name: np.linalg.eigvalsh(A) for name, A in dense.items()}, "ref": {}}
    for name, k, which, M in lc.CONVERGENCE:
        A = dense[name]
        out["ref"][name, k, which, M] = lc.lobpcg(A, k, which, minv=lc.jacobi_weights(A) if M else None)
    return out


# ---- 1. the residual kernel on its own ---------------------------------------------------------------------------------------
def _check_residual(hp, n, k, rng, with_minv, with_copy, pitches, lead=0):
    import torch
    lib = hp._capi.load()
    ldx, ldax, ldw, ldw2 = pitches
    X_h, AX_h = rng.uniform(-1.0, 1.0, (n, k)), rng.uniform(-1.0, 1.0, (n, k))
    theta_h, minv_h = rng.uniform(-2.0, 2.0, k), rng.uniform(0.5, 2.0, n)
    Xf, X = _padded(X_h, ldx, lead)
    AXf, AX = _padded(AX_h, ldax, lead)
    Wf, W = _padded(np.full((n, k), 7.0), ldw, lead)
    W2f, W2 = _padded(np.full((n, k), 7.0), ldw2, lead)
    theta, minv = _dev(theta_h), _dev(minv_h)
    rn2 = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    work = torch.zeros(max(1, lib.hpcla_lobpcg_work_bytes(n, k) // 8), dtype=torch.float64, device="cuda")
    args = (None, X.data_ptr(), ldx, AX.data_ptr(), ldax, theta.data_ptr(), minv.data_ptr() if with_minv else None, W.data_ptr(), ldw,
            W2.data_ptr() if with_copy else None, ldw2 if with_copy else 0, n, k, rn2.data_ptr(), work.data_ptr(), None)
    assert lib.hpcla_lobpcg_residual_f64(*args) == 0
    torch.cuda.synchronize()
    W_want, d = lc.residual(X_h, AX_h, theta_h, minv_h if with_minv else None)
    tag = (n, k, with_minv, with_copy, pitches, lead)
    got = W.cpu().numpy()
    assert _bits_eq(got[:, :k], W_want), tag
    assert np.isnan(got[:, k:]).all() and np.isnan(Wf[:lead].cpu().numpy()).all(), tag        # the padding keeps its poison
    got2 = W2.cpu().numpy()
    assert _bits_eq(got2[:, :k], W_want if with_copy else np.full((n, k), 7.0)) and np.isnan(got2[:, k:]).all(), tag
    assert _bits_eq(X[:, :k], X_h) and _bits_eq(AX[:, :k], AX_h), tag
    sums = rn2.cpu().numpy()
    assert (sums[k:] == 7.0).all(), tag
    worst = 0.0
    for j in range(k):
        terms = (d[:, j] * d[:, j]).tolist()
        worst = max(worst, abs(sums[j] - math.fsum(terms)) / max(math.fsum(terms), 1e-300))
    assert worst <= lc.RED_RTOL, (tag, worst)
    first = rn2.clone()
    assert lib.hpcla_lobpcg_residual_f64(*args) == 0
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int64), rn2.view(torch.int64)), tag                   # the same bits on a second call
    return worst


@pytest.mark.parametrize("k", KS)
def test_residual_kernel_alone(hp, k):
    """Every n of _sizes at this k: tight pitches (16-byte accesses when k is even), wider even pitches with poisoned padding,
    an odd pitch and a base off 16 bytes (both force the 8-byte path), with and without minv, with and without the second
    copy of W on a pitch of its own (k + 1 for an odd k: the SpMM's)."""
    rng = np.random.default_rng(10 + k)
    worst = 0.0
    for n in _sizes(hp):
        even = k + (k & 1)
        for pitches, lead in (((k, k, k, k + (k & 1 if k >= 3 else 0)), 0), ((even + 2, even + 4, 3 * even, even + 2), 0),
                              ((k + 3, k + 2, 2 * k + 1, k + 1), 0), ((even + 2, even + 2, even + 2, even + 2), 1)):
            for with_minv, with_copy in ((False, False), (True, True), (True, False), (False, True)):
                if n > 257 and (with_minv, with_copy) in ((True, False), (False, True)):
                    continue                                     # the large sizes: the two extreme variants
                worst = max(worst, _check_residual(hp, n, k, rng, with_minv, with_copy, pitches, lead))
    print(f"k = {k}: sums of squares within {worst:.1e} of fsum")


# ---- 2. the combine kernel on its own ----------------------------------------------------------------------------------------
def _check_combine(hp, n, k, c_rest, rng, pitch, lead=0, zero_block=None, with_as=True):
    import torch
    lib = hp._capi.load()
    S_h, AS_h = rng.uniform(-1.0, 1.0, (n, 3 * k)), rng.uniform(-1.0, 1.0, (n, 3 * k))
    C_h = rng.uniform(-1.0, 1.0, (k + c_rest, k))
    if zero_block is not None:                                   # a zero row block of C: those columns of S do not count
        C_h[zero_block * k:(zero_block + 1) * k] = 0.0
    Cp = np.full((k + c_rest, 16), np.nan)                       # the doubles behind a row of C are read and ignored
    Cp[:, :k] = C_h
    Sf, S = _padded(S_h, pitch, lead)
    ASf, AS = _padded(AS_h, pitch, lead)
    C = _dev(Cp.reshape(-1))
    assert lib.hpcla_lobpcg_combine_f64(S.data_ptr(), pitch, AS.data_ptr() if with_as else None, pitch, C.data_ptr(), k, c_rest, n,
                                        None) == 0
    torch.cuda.synchronize()
    tag = (n, k, c_rest, pitch, lead, zero_block, with_as)
    for got_t, src, used in ((S, S_h, True), (AS, AS_h, with_as)):
        got = got_t.cpu().numpy()
        assert np.isnan(got[:, 3 * k:]).all(), tag               # the padding keeps its poison
        if not used:
            assert _bits_eq(got[:, :3 * k], src), tag
            continue
        X_want, P_want = lc.combine(src, C_h, k, c_rest)
        assert _bits_eq(got[:, :k], X_want), tag
        assert _bits_eq(got[:, k:2 * k], src[:, k:2 * k]), tag    # the columns of W are unchanged
        assert _bits_eq(got[:, 2 * k:3 * k], P_want if c_rest else src[:, 2 * k:]), tag
    assert np.isnan(Sf[:lead].cpu().numpy()).all()


@pytest.mark.parametrize("k", KS)
def test_combine_kernel_alone(hp, k):
    """Every n of _sizes (one row to 257 tiles of 64 rows) at this k and c_rest in {0, k, 2k}, in place: the tight pitch 3k
    (16-byte accesses when k is even), a wider even pitch, an odd pitch and a base off 16 bytes (8-byte accesses), S alone, and
    C with a zero row block."""
    rng = np.random.default_rng(20 + k)
    for n in _sizes(hp):
        for c_rest in (0, k, 2 * k):
            _check_combine(hp, n, k, c_rest, rng, 3 * k)
            _check_combine(hp, n, k, c_rest, rng, 3 * k + 2 + (k & 1))
            if n <= 257:
                _check_combine(hp, n, k, c_rest, rng, 3 * k + 1 + (k & 1))
                _check_combine(hp, n, k, c_rest, rng, 3 * k + 2 + (k & 1), lead=1)
                _check_combine(hp, n, k, c_rest, rng, 3 * k, with_as=False)
        _check_combine(hp, n, k, 2 * k, rng, 3 * k, zero_block=1)
        _check_combine(hp, n, k, 2 * k, rng, 3 * k, zero_block=0)


# ---- 3. the first two iterations against the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(lc.FIRST_CASES)))
def test_first_iterations_match_the_restatement(hp, cases, gpu_backend_i32, case):
    name, k, which, M = lc.FIRST_CASES[case]
    dense = cases["dense"][name]
    A = _matrix(hp, gpu_backend_i32, dense)
    for maxiter in (0, 1, 2):                                    # theta after the start, after one and after two combines
        want, _, ref = lc.lobpcg(dense, k, which, maxiter=maxiter)
        got, X, info = hp.lobpcg(A, k=k, which=which, maxiter=maxiter)
        assert (info.status, info.iterations) == ("maxiter", maxiter + 1) == (ref["status"], ref["iterations"])
        dv, da = np.abs(got - want).max() / ref["anorm"], abs(info.anorm - ref["anorm"]) / ref["anorm"]
        print(f"{name} k {k} {which} maxiter {maxiter}: theta {dv:.1e}, anorm {da:.1e} (relative to anorm)")
        assert dv <= lc.VAL_RTOL and da <= lc.VAL_RTOL
    hp.clear_plan_cache()


# ---- 4. convergence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(lc.CONVERGENCE)))
def test_convergence_against_the_dense_spectrum(hp, cases, gpu_backend_i32, case):
    name, k, which, M = lc.CONVERGENCE[case]
    dense, ev = cases["dense"][name], cases["ev"][name]
    _, _, ref = cases["ref"][name, k, which, M]
    A = _matrix(hp, gpu_backend_i32, dense)
    got, X, info = hp.lobpcg(A, k=k, which=which, M=M, tol=lc.TOL)
    assert got.dtype == np.float64 and got.shape == (k,) and np.all(np.diff(got) >= 0) and X.shape == (A.shape[0], k)
    Xh = X.gather()
    err, res, orth, est = lc.figures(dense, ev, got, Xh, dict(anorm=info.anorm, residual_norms=info.residual_norms), k, which)
    print(f"{name} k {k} {which} {M}: {info.iterations} iterations (restatement {ref['iterations']}), eigenvalue error {err:.1e} "
          f"||A||, true residual {res:.2f} tol anorm, orthogonality {orth:.1e}, residual_norms vs true {est:.1e} anorm")
    assert info.converged and info.status == "converged" == ref["status"]
    assert err <= 2 * lc.TOL
    assert res <= pc.TRUE_RES_FACTOR
    assert orth <= lc.ORTH_TOL
    assert info.residual_norms.shape == (k,) and np.all(info.residual_norms <= lc.TOL * info.anorm)
    assert est <= 1e-12 + lc.DRIFT
    assert info.iterations <= 1.5 * ref["iterations"] + 5
    assert len(info.history) == info.iterations and info.history[-1] == info.residual_norms.max()
    assert info.anorm <= np.abs(ev).max() * (1 + 1e-12)           # a lower bound of ||A||_2
    hp.clear_plan_cache()


# ---- 5. the case hp.eigsh documents as its failure -------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["SA", "LA"])
def test_the_square_grid_returns_the_double_eigenvalue_twice(hp, cases, gpu_backend_i32, which):
    """The 16 x 16 grid, k = 4: lambda_11, lambda_12, lambda_21, lambda_22 from the closed form 4 - 2cos(i pi/17) - 2cos(j pi/17)
    ("LA": the mirror set).  Single-vector Lanczos returns the double value once and the next distinct value in its place."""
    A = _matrix(hp, gpu_backend_i32, cases["dense"]["poisson16"])
    exact = lc.poisson16_exact(4, which)
    assert abs(exact[1] - exact[2]) <= 1e-14 and min(exact[1] - exact[0], exact[3] - exact[2]) >= 0.03
    got, X, info = hp.lobpcg(A, k=4, which=which)
    norm2 = np.abs(cases["ev"]["poisson16"]).max()
    print(f"{which}: {got} against {exact}: {np.abs(got - exact).max() / norm2:.1e} ||A||")
    assert info.converged and np.abs(got - exact).max() <= 2 * lc.TOL * norm2
    assert abs(got[1] - got[2]) <= 2 * lc.TOL * norm2            # the double value, twice
    hp.clear_plan_cache()


# ---- 6. exact and edge cases -------------------------------------------------------------------------------------------------
def test_exact_cases(hp, gpu_backend_i32):
    """``iterations`` counts the SpMMs after the start, the last one included, so a start that is already exact reads 1: the
    solve stops at its first decision and applies no combine."""
    B = gpu_backend_i32
    for scale in (1.0, 0.0):                                     # A = I and A = 0
        A = hp.HPCSparseMatrix_local(*pc.diag_matrix(np.full(12, scale)), 12, B)
        got, X, info = hp.lobpcg(A, k=3)
        assert (info.status, info.converged, info.iterations, len(info.history)) == ("converged", True, 1, 1)
        assert np.abs(got - scale).max() <= 1e-15 and info.anorm <= scale * (1 + 1e-15)
        assert np.abs(X.gather().T @ X.gather() - np.eye(3)).max() <= lc.ORTH_TOL
    d5 = np.arange(1.0, 6.0)
    A5 = hp.HPCSparseMatrix_local(*pc.diag_matrix(d5), 5, B)
    got, X, info = hp.lobpcg(A5, k=5)                            # k = n: the start's projection is the whole problem
    assert info.converged and info.iterations <= 2 and np.abs(got - d5).max() <= 1e-13
    for which, want in (("SA", [1.0, 2.0]), ("LA", [4.0, 5.0])):  # 3k > n: directions are dropped on the way
        got, X, info = hp.lobpcg(A5, k=2, which=which)
        assert info.converged and np.abs(got - want).max() <= 2 * lc.TOL * 5
        assert np.abs(X.gather().T @ X.gather() - np.eye(2)).max() <= lc.ORTH_TOL
    bad = d5.copy()
    bad[2] = np.nan
    got, X, info = hp.lobpcg(hp.HPCSparseMatrix_local(*pc.diag_matrix(bad), 5, B), k=2)
    assert (info.status, info.converged) == ("breakdown", False) and np.isnan(got).all() and np.isnan(info.residual_norms).all()
    assert got.shape == (2,) and X.shape == (5, 2) and not X.local_values().any()
    A60 = hp.HPCSparseMatrix_local(*pc.diag_matrix(np.arange(1.0, 61.0)), 60, B)
    got, X, info = hp.lobpcg(A60, k=4, maxiter=3)
    assert (info.status, info.converged, info.iterations, len(info.history)) == ("maxiter", False, 4, 4)
    assert got.shape == (4,) and X.shape == (60, 4)
    hp.clear_plan_cache()


def test_x0_and_a_dirty_workspace(hp, cases, gpu_backend_i32):
    dense = cases["dense"]["poisson16"]
    n = dense.shape[0]
    A = _matrix(hp, gpu_backend_i32, dense)
    got, X, info = hp.lobpcg(A, k=4)
    xv = X.local_values().copy()
    X0 = hp.HPCMatrix.from_global(lc.start_block(n, 4, 0), gpu_backend_i32)                # the default start, handed in
    got0, X0r, info0 = hp.lobpcg(A, k=4, X0=X0)
    assert _bits_eq(got0, got) and _bits_eq(X0r.local_values(), xv) and info0.iterations == info.iterations
    X5 = hp.HPCMatrix.from_global(lc.start_block(n, 4, 5), gpu_backend_i32)                # another start: the same values
    got5, _, info5 = hp.lobpcg(A, k=4, X0=X5)
    assert info5.converged and np.abs(got5 - got).max() <= 2 * lc.TOL * info.anorm
    want5, _, ref5 = lc.lobpcg(dense, 4, X0=lc.start_block(n, 4, 5))
    assert info5.iterations <= 1.5 * ref5["iterations"] + 5
    ws = hp.LobpcgWorkspace(A, 4)
    ws.Q.fill_(float("nan"))                                     # dirty in the worst way
    ws.Wp.fill_(float("nan"))
    ws.small.fill_(float("nan"))
    hp.lobpcg(A, k=4, which="LA", maxiter=7, seed=3, workspace=ws)                        # another solve, stopped early
    got3, X3, info3 = hp.lobpcg(A, k=4, workspace=ws)
    assert _bits_eq(got3, got) and _bits_eq(X3.local_values(), xv)
    assert (info3.iterations, info3.history) == (info.iterations, info.history)
    got4, X4, _ = hp.lobpcg(A, k=4, workspace=ws)                # and on its own leftovers
    assert _bits_eq(got4, got) and _bits_eq(X4.local_values(), xv)
    assert X4.A.data_ptr() != ws.Q.data_ptr()                    # the result is not a view of the workspace
    got2, _, info2 = hp.lobpcg(A, k=2, workspace=ws)             # another k: a workspace of its own
    assert info2.converged and np.abs(got2 - got[:2]).max() <= 2 * lc.TOL * info.anorm
    hp.clear_plan_cache()


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------
def test_lobpcg_argument_errors(hp, cases, gpu_backend_i32):
    dense = cases["dense"]["poisson16"]
    n = dense.shape[0]
    B = gpu_backend_i32
    A = _matrix(hp, B, dense)
    with pytest.raises(ValueError, match="shift-invert"):
        hp.lobpcg(A, which="SM")
    for bad in (dict(which="BE"), dict(which="LM"), dict(k=0), dict(k=17), dict(tol=-1.0), dict(maxiter=-1), dict(M="ilu"),
                dict(M=np.ones(n))):
        with pytest.raises(ValueError):
            hp.lobpcg(A, **bad)
    with pytest.raises(ValueError):                                                      # k > n
        hp.lobpcg(hp.HPCSparseMatrix_local(*pc.diag_matrix(np.arange(1.0, 4.0)), 3, B), k=4)
    with pytest.raises(ValueError):
        hp.LobpcgWorkspace(A, 17)
    rowptr, colidx, vals, _ = lc.csr_of(dense)
    with pytest.raises(ValueError):                                                      # a rectangular A
        hp.lobpcg(hp.HPCSparseMatrix_local(rowptr, colidx, vals, n + 7, B))
    with pytest.raises(ValueError):                                                      # X0 with another column count
        hp.lobpcg(A, k=4, X0=hp.HPCMatrix.from_global(np.ones((n, 3)), B))
    with pytest.raises(ValueError):                                                      # X0 on another partition
        hp.lobpcg(A, k=4, X0=hp.HPCMatrix.from_global(np.ones((n + 2, 4)), B))
    with pytest.raises(ValueError):                                                      # X0 that is no HPCMatrix
        hp.lobpcg(A, k=4, X0=np.ones((n, 4)))
    with pytest.raises(ValueError, match="rank deficient"):
        hp.lobpcg(A, k=2, X0=hp.HPCMatrix.from_global(np.ones((n, 2)), B))
    with pytest.raises(ValueError):                                                      # weights on another partition
        hp.lobpcg(A, k=2, M=hp.HPCVector.from_global(np.ones(n + 2), B))
    with pytest.raises(ValueError):                                                      # weights that are not positive
        hp.lobpcg(A, k=2, M=hp.HPCVector.from_global(np.linspace(-1.0, 1.0, n), B))
    with pytest.raises(ValueError):                                                      # Jacobi on a zero diagonal
        hp.lobpcg(hp.HPCSparseMatrix_local(*pc.diag_matrix(np.array([1.0, 0.0, 2.0, 3.0])), 4, B), k=1, M="jacobi")
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    with pytest.raises(TypeError):
        hp.lobpcg(hp.HPCSparseMatrix_local(rowptr, colidx, vals.astype(np.float32), n, b32))
    got, _, info = hp.lobpcg(A, k=2, M=hp.HPCVector.from_global(np.full(n, 0.25), B))      # weights as an HPCVector
    assert info.converged and np.abs(got - lc.poisson16_exact(2, "SA")).max() <= 2 * lc.TOL * 8.0
    hp.clear_plan_cache()


# ---- 8. ranks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_lobpcg_across_ranks(nranks):
    """The ranks share the one GPU (peer-window push transport, like tests/test_gpu_multirank.py); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
