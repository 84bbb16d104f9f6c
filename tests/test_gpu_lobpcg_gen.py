"""GPU tests of the block eigensolver on a pencil (``hp.lobpcg`` with ``B``: ``A x = lambda B x``): the residual kernel of the
pencil on its own through the C ABI, the first iterations against the numpy restatement, convergence against
``scipy.linalg.eigh(K, M)``, the two forms of a diagonal ``B``, ``B = I`` against ``B=None``, the breakdown of a ``B`` that is
not positive definite, a dirty workspace, the argument errors and the solve across ranks.  Cases and the restatement:
tests/_lobpcg_gen_cases.py.

Margins (none of them taken from the device's results; tests/test_lobpcg_gen_cases.py re-measures the CPU figures and prints
them):
  * W, W2 and BW of the residual kernel: bit-equal to numpy's separately rounded expressions (the library is built with
    -ffp-contract=off); its 3k sums: 1e-12 of math.fsum relative to the sum of |terms| (``lc.RED_RTOL``, the project's margin
    for its reductions); the same bits on a second call;
  * theta and anorm of the first iterations: ``lc.VAL_RTOL`` = 1e-12 of anorm against the restatement;
  * converged runs, every right-hand side from dense numpy: |vals_j - lambda_j| <= 2 tol (||A x_j|| + |theta_j| ||B x_j||) /
    sqrt(lambda_min(B)) -- for a B-normalised x, |theta - lambda| <= ||B^{-1/2} r|| <= ||r|| / sqrt(lambda_min(B)), and a
    converged pair has ||r|| <= tol x the scale; factor 2 as elsewhere in the suite; the restatement sits at 2.7e-6 of it --,
    true residuals <= ``pc.TRUE_RES_FACTOR`` = 2 x tol x the true scale (restatement: 0.97), ||X'BX - I||_max <= ``lc.ORTH_TOL``
    = 1e-12 (3.7e-15), iterations <= 1.5 x the restatement's + 5 (the cap and the reasoning of tests/test_gpu_lobpcg.py);
  * ranks: vals within 1e-12 anorm of the one-rank result; the ranks' vals and info bit-identical.
Eigenvector signs are not compared."""
import math
import os

import numpy as np
import pytest

from tests import _lobpcg_cases as lc
from tests import _lobpcg_gen_cases as gc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_lobpcg_gen_worker.py")

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 7, 8, 15, 16)
# every case with a sparse B; the lumped ones with the weights as an HPCVector too
RUNS = [(case, "sparse") for case in range(len(gc.CONVERGENCE))] + [(case, "vector") for case, c in enumerate(gc.CONVERGENCE)
                                                                    if c[1] == "lumped"]


def _sizes(hp):
    """n = 1 .. 257, one n past the first chunk of partials (two stage-1 workgroups) and one past the first phase of the second
    stage (17 chunks: phase 0 adds two of them), both named from the library's constant."""
    chunk = hp._capi.load().hpcla_lobpcg_chunk_rows(1)
    return (1, 2, 63, 64, 65, 257, chunk + 1, 16 * chunk + 1)


def _matrix(hp, backend, dense):
    rowptr, colidx, vals, n = lc.csr_of(dense)
    return hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, backend)


def _diagonal(hp, backend, d):
    return hp.HPCSparseMatrix_local(*pc.diag_matrix(d), len(d), backend)


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
def cases():
    """Every pencil with its dense B, the wanted eigenvalues, lambda_min(B) and the restatement's result, computed once."""
    pencils = gc.pencils()
    out = {"pencils": pencils, "ref": {}}
    for name, form, k, which in gc.CONVERGENCE:
        K, M = pencils[name]
        Bd = gc.b_of(M, form)
        want, bmin = gc.reference(K, Bd, k, which)
        out["ref"][name, form, k, which] = (Bd, want, bmin, gc.lobpcg_gen(K, Bd, k, which)[2])
    return out


def _b_operand(hp, backend, M, form, kind):
    """The device's B of a case: the consistent matrix, or the lumped one as a sparse diagonal matrix or as weights."""
    if form == "consistent":
        return _matrix(hp, backend, M)
    d = gc.lumped(M)
    return _diagonal(hp, backend, d) if kind == "sparse" else hp.HPCVector.from_global(d, backend)


# ---- 1. the residual kernel of the pencil on its own ---------------------------------------------------------------------------
def _check_residual_gen(hp, n, k, rng, with_minv, form, pitches, lead=0):
    """``form``: "none" (W alone), "w2" (the copy on a pitch of its own), "bdiag" (bdiag, BW and the copy)."""
    import torch
    lib = hp._capi.load()
    ldax, ldbx, ldw, ldw2, ldbw = pitches
    AX_h, BX_h = rng.uniform(-1.0, 1.0, (n, k)), rng.uniform(-1.0, 1.0, (n, k))
    theta_h, minv_h, bd_h = rng.uniform(-2.0, 2.0, k), rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    with_copy, with_b = form != "none", form == "bdiag"
    AXf, AX = _padded(AX_h, ldax, lead)
    BXf, BX = _padded(BX_h, ldbx, lead)
    Wf, W = _padded(np.full((n, k), 7.0), ldw, lead)
    W2f, W2 = _padded(np.full((n, k), 7.0), ldw2, lead)
    BWf, BW = _padded(np.full((n, k), 7.0), ldbw, lead)
    theta, minv, bd = _dev(theta_h), _dev(minv_h), _dev(bd_h)
    sums = torch.full((48,), 7.0, dtype=torch.float64, device="cuda")
    work = torch.zeros(max(1, lib.hpcla_lobpcg_gen_work_bytes(n, k) // 8), dtype=torch.float64, device="cuda")
    args = (None, AX.data_ptr(), ldax, BX.data_ptr(), ldbx, theta.data_ptr(), minv.data_ptr() if with_minv else None,
            bd.data_ptr() if with_b else None, W.data_ptr(), ldw, W2.data_ptr() if with_copy else None, ldw2 if with_copy else 0,
            BW.data_ptr() if with_b else None, ldbw if with_b else 0, n, k, sums.data_ptr(), work.data_ptr(), None)
    assert lib.hpcla_lobpcg_residual_gen_f64(*args) == 0, hp._capi.last_error()
    torch.cuda.synchronize()
    W_want, BW_want, d = gc.residual_gen(AX_h, BX_h, theta_h, minv_h if with_minv else None, bd_h if with_b else None)
    untouched = np.full((n, k), 7.0)
    tag = (n, k, with_minv, form, pitches, lead)
    for flat, view, want in ((Wf, W, W_want), (W2f, W2, W_want if with_copy else untouched), (BWf, BW, BW_want if with_b else untouched)):
        got = view.cpu().numpy()
        assert _bits_eq(got[:, :k], want), tag
        assert np.isnan(got[:, k:]).all() and np.isnan(flat[:lead].cpu().numpy()).all(), tag  # the padding keeps its poison
    assert _bits_eq(AX[:, :k], AX_h) and _bits_eq(BX[:, :k], BX_h), tag                        # the inputs are unchanged
    assert np.isnan(AX.cpu().numpy()[:, k:]).all() and np.isnan(BX.cpu().numpy()[:, k:]).all(), tag
    assert _bits_eq(minv, minv_h) and _bits_eq(bd, bd_h) and _bits_eq(theta, theta_h), tag
    got = sums.cpu().numpy()
    worst = 0.0
    for q, block in enumerate((d, AX_h, BX_h)):
        assert (got[16 * q + k:16 * (q + 1)] == 7.0).all(), tag                                # unused sums are untouched
        for j in range(k):
            terms = (block[:, j] * block[:, j]).tolist()
            worst = max(worst, abs(got[16 * q + j] - math.fsum(terms)) / max(math.fsum(terms), 1e-300))
    assert worst <= lc.RED_RTOL, (tag, worst)
    first, first_w = sums.clone(), W.clone()
    assert lib.hpcla_lobpcg_residual_gen_f64(*args) == 0
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int64), sums.view(torch.int64)), tag                   # the same bits on a second call
    assert torch.equal(first_w.view(torch.int64), W.view(torch.int64)), tag
    return worst


@pytest.mark.parametrize("k", KS)
def test_residual_gen_kernel_alone(hp, k):
    """Every n of _sizes at this k: tight pitches (16-byte accesses when k is even), wider even pitches with poisoned padding,
    an odd pitch and a base off 16 bytes (both force the 8-byte path), with and without minv, and the three forms of the
    outputs: W alone, W and its copy, W, its copy and BW = bdiag .* W."""
    rng = np.random.default_rng(30 + k)
    worst = 0.0
    even = k + (k & 1)
    spmm = k + (k & 1 if k >= 3 else 0)                          # the SpMM's pitch of the copy
    for n in _sizes(hp):
        for pitches, lead in (((k, k, k, spmm, k), 0), ((even + 2, even + 4, 3 * even, even + 2, 9 * even), 0),
                              ((k + 3, k + 2, 2 * k + 1, k + 1, k + 5), 0), ((even + 2,) * 5, 1)):
            for with_minv in (False, True):
                for form in ("none", "w2", "bdiag"):
                    if n > 257 and (with_minv, form) not in ((False, "none"), (True, "bdiag")):
                        continue                                 # the large sizes: the two extreme variants
                    worst = max(worst, _check_residual_gen(hp, n, k, rng, with_minv, form, pitches, lead))
    print(f"k = {k}: the 3k sums within {worst:.1e} of fsum")


# ---- 2. the first iterations against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "vector"])
def test_first_iterations_match_the_restatement(hp, cases, gpu_backend_i32, kind):
    name, k, which = gc.FIRST_CASE
    K, M = cases["pencils"][name]
    form = "consistent" if kind == "sparse" else "lumped"
    A, B = _matrix(hp, gpu_backend_i32, K), _b_operand(hp, gpu_backend_i32, M, form, kind)
    B_h = M if kind == "sparse" else gc.lumped(M)
    for maxiter in (0, 1, 2):                                    # theta after the start, after one and after two combines
        want, _, ref = gc.lobpcg_gen(K, B_h, k, which, maxiter=maxiter)
        got, X, info = hp.lobpcg(A, k=k, which=which, maxiter=maxiter, B=B)
        assert (info.status, info.iterations) == ("maxiter", maxiter + 1) == (ref["status"], ref["iterations"])
        dv, da = np.abs(got - want).max() / ref["anorm"], abs(info.anorm - ref["anorm"]) / ref["anorm"]
        print(f"{name} {kind} k {k} {which} maxiter {maxiter}: theta {dv:.1e}, anorm {da:.1e} (relative to anorm)")
        assert dv <= lc.VAL_RTOL and da <= lc.VAL_RTOL
    hp.clear_plan_cache()


# ---- 3. convergence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", range(len(RUNS)))
def test_convergence_against_the_dense_pencil(hp, cases, gpu_backend_i32, run):
    case, kind = RUNS[run]
    name, form, k, which = gc.CONVERGENCE[case]
    K, M = cases["pencils"][name]
    Bd, want, bmin, ref = cases["ref"][name, form, k, which]
    A, B = _matrix(hp, gpu_backend_i32, K), _b_operand(hp, gpu_backend_i32, M, form, kind)
    got, X, info = hp.lobpcg(A, k=k, which=which, tol=gc.TOL, B=B)
    assert got.dtype == np.float64 and got.shape == (k,) and X.shape == (A.shape[0], k)
    err, res, orth = gc.figures(K, Bd, want, bmin, got, X.gather())
    print(f"{name} {form} ({kind}) k {k} {which}: {info.iterations} iterations (restatement {ref['iterations']}), eigenvalue error "
          f"{err:.1e} of its bound, true residual {res:.2f} tol scale, B-orthonormality {orth:.1e}")
    assert info.converged and info.status == "converged" == ref["status"] and np.all(np.diff(got) >= 0)
    assert err <= 1.0
    assert res <= pc.TRUE_RES_FACTOR
    assert orth <= lc.ORTH_TOL
    assert info.residual_norms.shape == (k,) == info.residual_scales.shape
    assert np.all(info.residual_norms <= gc.TOL * info.residual_scales)
    assert len(info.history) == info.iterations and info.history[-1] == info.residual_norms.max()
    assert info.iterations <= 1.5 * ref["iterations"] + 5
    hp.clear_plan_cache()


# ---- 4. the two forms of a diagonal B -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["SA", "LA"])
def test_weights_and_the_diagonal_matrix_agree(hp, cases, gpu_backend_i32, which):
    """BW = b .* W from the residual kernel against BW = B W from the SpMM of the same diagonal: one product each, the same
    rounding, so the two solves walk the same path."""
    K, M = cases["pencils"]["fem2d16"]
    A = _matrix(hp, gpu_backend_i32, K)
    gv, Xv, iv = hp.lobpcg(A, k=4, which=which, B=_b_operand(hp, gpu_backend_i32, M, "lumped", "vector"))
    gs, Xs, is_ = hp.lobpcg(A, k=4, which=which, B=_b_operand(hp, gpu_backend_i32, M, "lumped", "sparse"))
    print(f"{which}: weights {iv.iterations} iterations, matrix {is_.iterations}, vals differ by {np.abs(gv - gs).max() / iv.anorm:.1e} anorm")
    assert iv.converged and is_.converged
    assert np.abs(gv - gs).max() <= lc.VAL_RTOL * iv.anorm
    assert iv.iterations <= 1.5 * is_.iterations + 5 and is_.iterations <= 1.5 * iv.iterations + 5
    hp.clear_plan_cache()


# ---- 5. B = I against B = None ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["SA", "LA"])
def test_identity_b_gives_the_standard_problem(hp, orc, gpu_backend_i32, which):
    """The 5-point matrix on the 16 x 16 grid, k = 4 (the double eigenvalue inside the block).  The stop rules differ, so this
    is no bit comparison: both sets of values lie within tol anorm of the spectrum, hence within 2 tol anorm of each other."""
    name, k, _, _ = lc.SPREAD_CASES[0]
    dense = lc.dense_matrices(orc)[name]
    A = _matrix(hp, gpu_backend_i32, dense)
    g0, _, i0 = hp.lobpcg(A, k=k, which=which)
    g1, X1, i1 = hp.lobpcg(A, k=k, which=which, B=_diagonal(hp, gpu_backend_i32, np.ones(dense.shape[0])))
    assert i0.converged and i1.converged and i0.residual_scales.shape == (0,)
    assert np.abs(g0 - g1).max() <= 2 * lc.TOL * i0.anorm
    assert np.abs(g1 - lc.poisson16_exact(k, which)).max() <= 2 * lc.TOL * 8.0
    Xh = X1.gather()
    assert np.abs(Xh.T @ Xh - np.eye(k)).max() <= lc.ORTH_TOL
    hp.clear_plan_cache()


# ---- 6. breakdown ---------------------------------------------------------------------------------------------------------------
def test_a_negative_definite_b_breaks_down(hp, cases, gpu_backend_i32):
    K, _ = cases["pencils"]["fem2d16"]
    n = K.shape[0]
    A = _matrix(hp, gpu_backend_i32, K)
    got, X, info = hp.lobpcg(A, k=3, B=_diagonal(hp, gpu_backend_i32, -np.ones(n)))
    assert (info.status, info.converged) == ("breakdown", False) and np.isnan(got).all() and np.isnan(info.residual_norms).all()
    assert np.isnan(info.residual_scales).all() and got.shape == (3,) and X.shape == (n, 3) and not X.local_values().any()
    hp.clear_plan_cache()


# ---- 7. workspaces -----------------------------------------------------------------------------------------------------------------
def test_a_dirty_workspace_and_one_of_the_other_shape(hp, cases, gpu_backend_i32):
    K, M = cases["pencils"]["fem2d16"]
    A = _matrix(hp, gpu_backend_i32, K)
    for kind, form in (("sparse", "consistent"), ("vector", "lumped")):
        B = _b_operand(hp, gpu_backend_i32, M, form, kind)
        got, X, info = hp.lobpcg(A, k=4, B=B)
        xv = X.local_values().copy()
        ws = hp.LobpcgWorkspace(A, 4, B)
        assert ws.Q.shape[1] == 9 * 4 and ws.fits(A, 4, B) and not ws.fits(A, 4) and not ws.fits(A, 3, B)
        for t in (ws.Q, ws.Wp, ws.small, ws.up, ws.rwork, ws.gwork):
            t.fill_(float("nan"))                                # dirty in the worst way
        hp.lobpcg(A, k=4, which="LA", maxiter=7, seed=3, workspace=ws, B=B)               # another solve, stopped early
        got2, X2, info2 = hp.lobpcg(A, k=4, workspace=ws, B=B)
        assert _bits_eq(got2, got) and _bits_eq(X2.local_values(), xv)
        assert (info2.iterations, info2.history) == (info.iterations, info.history)
        assert _bits_eq(info2.residual_scales, info.residual_scales)
        assert X2.A.data_ptr() != ws.Q.data_ptr()                # the result is not a view of the workspace
        plain = hp.LobpcgWorkspace(A, 4)                         # a B=None workspace with a B: replaced, not misused
        assert plain.Q.shape[1] == 6 * 4 and plain.fits(A, 4) and not plain.fits(A, 4, B)
        plain.Q.fill_(3.0)
        got3, X3, _ = hp.lobpcg(A, k=4, workspace=plain, B=B)
        assert _bits_eq(got3, got) and _bits_eq(X3.local_values(), xv)
        assert plain.Q.shape[1] == 6 * 4 and bool((plain.Q == 3.0).all())
        got4, _, info4 = hp.lobpcg(A, k=4, workspace=ws)         # and the wide one without a B: replaced too
        assert info4.converged and info4.residual_scales.shape == (0,)
    hp.clear_plan_cache()


# ---- 8. argument errors ------------------------------------------------------------------------------------------------------
def test_b_argument_errors(hp, cases, gpu_backend_i32):
    K, M = cases["pencils"]["fem2d16"]
    n = K.shape[0]
    Bk = gpu_backend_i32
    A = _matrix(hp, Bk, K)
    rowptr, colidx, vals, _ = lc.csr_of(M)
    with pytest.raises(ValueError, match="lobpcg: B must be"):                           # a B on another partition
        hp.lobpcg(A, k=2, B=_diagonal(hp, Bk, np.ones(n + 2)))
    with pytest.raises(ValueError, match="lobpcg: B must be square"):                    # a non-square B
        hp.lobpcg(A, k=2, B=hp.HPCSparseMatrix_local(rowptr, colidx, vals, n + 7, Bk))
    with pytest.raises(ValueError, match="lobpcg: B must be"):                           # weights on another partition
        hp.lobpcg(A, k=2, B=hp.HPCVector.from_global(np.ones(n + 2), Bk))
    with pytest.raises(ValueError, match="lobpcg: B must be"):                           # a vector B with a zero entry
        hp.lobpcg(A, k=2, B=hp.HPCVector.from_global(np.concatenate([[0.0], np.ones(n - 1)]), Bk))
    with pytest.raises(ValueError, match="lobpcg: B must be"):                           # and with a negative one
        hp.lobpcg(A, k=2, B=hp.HPCVector.from_global(np.linspace(-1.0, 1.0, n), Bk))
    for bad in (np.ones(n), np.eye(n), "lumped", hp.HPCMatrix.from_global(np.ones((n, 2)), Bk)):
        with pytest.raises(ValueError, match="lobpcg: B must be"):                       # anything that is neither
            hp.lobpcg(A, k=2, B=bad)
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    with pytest.raises(TypeError):                                                       # a B on a Float32 backend
        hp.lobpcg(A, k=2, B=hp.HPCSparseMatrix_local(rowptr, colidx, vals.astype(np.float32), n, b32))
    with pytest.raises(TypeError):
        hp.lobpcg(A, k=2, B=hp.HPCVector.from_global(np.ones(n, dtype=np.float32), b32))
    with pytest.raises(ValueError, match="rank deficient"):                              # X0 is still checked
        hp.lobpcg(A, k=2, X0=hp.HPCMatrix.from_global(np.ones((n, 2)), Bk), B=_matrix(hp, Bk, M))
    import torch
    off = torch.zeros(n + 1, dtype=torch.float64, device="cuda")[1:]                     # weights 8 bytes off: cloned once
    off.copy_(torch.from_numpy(gc.lumped(M)))
    assert off.data_ptr() % 16 == 8
    aligned = hp.HPCVector.from_global(gc.lumped(M), Bk)
    got, _, info = hp.lobpcg(A, k=2, B=hp.HPCVector(aligned.structural_hash, aligned.partition, off, Bk))
    want, _, _ = hp.lobpcg(A, k=2, B=aligned)
    assert info.converged and _bits_eq(got, want)
    hp.clear_plan_cache()


# ---- 9. ranks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_lobpcg_gen_across_ranks(nranks):
    """The ranks share the one GPU (peer-window push transport, like tests/test_gpu_multirank.py); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
