"""GPU tests of the eigensolver: the rotate kernel and the Lanczos second pass on their own through the C ABI, the first cycle's
projected matrix against the numpy restatement, convergence against the dense spectrum, a dirty workspace, the exact cases, the
argument errors and the solve across ranks.  Cases and the restatement: tests/_eigsh_cases.py.

Margins (none of them taken from the device's results; tests/test_eigsh_cases.py re-measures the CPU figures and prints them):
  * the rotate kernel's outputs, the elements of w, and the small step's T[:, j], beta[j], hn: bit-equal to numpy's separately
    rounded expressions (the library is built with -ffp-contract=off; IEEE sqrt);
  * nn = w.w: 1e-12 of math.fsum relative to the sum of |terms|, the project's margin for its reductions;
  * the first cycle's T and beta: T_RTOL = 1e-12 of max|T|, the project's margin (four summation orders on the CPU spread by
    <= 1.1e-15 of max|T|, 2.9e-15 absolute on this case: about 300 times less; the bound on that spread is 1e-13; at 65 x 63
    they spread by <= 1.4e-15 of max|T|: 700 times less);
  * eigenvalues: VAL_RTOL = 1e-12 of anorm against numpy.linalg.eigvalsh of the dense matrix (the restatement: <= 1.7e-14,
    its spread over the four orders <= 1.3e-14);
  * step counts: within one cycle's m - p steps of the restatement's (identical across the four orders on the CPU);
  * true residuals ||A x_i - vals_i x_i|| <= 2 tol anorm (the restatement: <= 0.99; the factor 2 is hp.gmres's margin);
  * residual_norms[i] within 1e-12 anorm of the true residual of pair i, which is what shows that the estimates are aligned
    with vals: with full reorthogonalisation the two differ by rounding alone (the restatement: <= 3.1e-15 anorm);
  * transpose(X) X within 1e-12 of the identity (the restatement: <= 7.2e-15).
Eigenvector signs are not compared."""
import math
import os

import numpy as np
import pytest

from tests import _eigsh_cases as ec
from tests import _gmres_cases as gc
from tests import _grid_regimes as gr
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_eigsh_worker.py")

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN, INVARIANT = 0, 1, 2, 4
SMALL = ("T", "beta", "h1", "h2", "nn", "hn")


def _matrix(hp, backend, rowptr, colidx, vals, n=None):
    return hp.HPCSparseMatrix_local(rowptr, colidx, vals, len(rowptr) - 1 if n is None else n, backend)


def _bits_eq(t, want):
    got = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.array_equal(pc.bits(got), pc.bits(want))


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).cuda()


@pytest.fixture(scope="module")
def cases(orc):
    """Every convergence case with its dense spectrum and the restatement's results, computed once."""
    mats = ec.matrices(orc)
    out = {"mats": mats, "ev": {name: ec.dense_eigenvalues(*mats[name]) for name in mats}, "ref": {}}
    for name, k, ncv, whiches in ec.CONVERGENCE:
        for which in whiches:
            out["ref"][name, k, ncv, which] = ec.eigsh(*mats[name], k=k, which=which, ncv=ncv)
    return out


# ---- 1. the rotate kernel on its own -------------------------------------------------------------------------------------------
def _rotate(hp, V, ldv, m, p, S, move_last, out, ors, ocs, n):
    P = lambda t: t.data_ptr() if t is not None else None
    assert hp._capi.load().hpcla_eigsh_rotate_f64(P(V), ldv, m, p, P(S), move_last, P(out), ors, ocs, n, None) == 0


def _check_rotate(hp, n, m, p, rng, extra=2):
    """Both forms at one (n, m, p).  The basis has m + 1 + extra columns at an even pitch, the pad of an odd n poisoned with NaN."""
    import torch
    ldv, cols = n + (n & 1), m + 1 + extra
    V_h = rng.uniform(-1.0, 1.0, (cols, n))
    S_h = rng.uniform(-1.0, 1.0, (m, p))
    buf = np.full((cols, ldv), np.nan)
    buf[:, :n] = V_h
    V0, S = _dev(buf.reshape(-1)), _dev(S_h.T.reshape(-1))       # column j of S contiguous
    want = ec.rotate(V_h[:m], S_h)                               # p x n
    for move_last in (0, 1):
        V = V0.clone()
        _rotate(hp, V, ldv, m, p, S, move_last, None, 0, 0, n)
        torch.cuda.synchronize()
        got = V.view(cols, ldv).cpu().numpy()
        assert _bits_eq(got[:p, :n], want), (n, m, p, move_last)
        keep = p
        if move_last:
            assert _bits_eq(got[p, :n], V_h[m]), (n, m, p)
            keep = p + 1
        assert _bits_eq(got[keep:, :n], V_h[keep:]), (n, m, p, move_last)                 # columns beyond keep their bits
        if n & 1:
            assert np.isnan(got[:, n]).all()                                              # the pad stays NaN
    for ors in (p, p + 3):                                       # out of place, row-major: tight and with a larger stride
        V, out = V0.clone(), torch.full((n * ors,), 7.0, dtype=torch.float64, device="cuda")
        _rotate(hp, V, ldv, m, p, S, 0, out, ors, 1, n)
        torch.cuda.synchronize()
        got = out.view(n, ors).cpu().numpy()
        assert _bits_eq(got[:, :p], want.T), (n, m, p, ors)
        assert (got[:, p:] == 7.0).all()
        assert torch.equal(V.view(torch.int64), V0.view(torch.int64))                     # V's bits are left alone


@pytest.mark.parametrize("m,p", [(2, 1), (8, 5), (16, 15), (17, 9), (32, 17), (33, 20), (48, 47), (49, 1), (64, 63)])
def test_rotate_kernel_alone(hp, m, p):
    """(m, p) are the edges of the four register tiles (16 | 17, 32 | 33, 48 | 49, 64); m = 16, 32, 48 and 64 fill their tile and
    take its straight-line path, the others end in a partial chunk of 2, 8, 1, 1 and 1 columns (blocks of 8, 4, 2, 1).  Tiles of
    16 and 32 columns take two rows per lane as double2 and leave an odd last row to a one-row launch, tiles of 48 and 64 one
    row per lane.  256 lanes per workgroup:
    n = 511 is one workgroup of double2 lanes with a tail, 515 the first odd size on two, 2049 and 2051 are several workgroups
    in both forms; n = 1 is the tail alone, n = 2 the body alone."""
    rng = np.random.default_rng(100 * m + p)
    for n in (1, 2, 511, 515, 2049, 2051):
        _check_rotate(hp, n, m, p, rng)


def test_rotate_kernel_at_a_large_size(hp):
    """n = 4 194 307 at (20, 12): 8193 workgroups of double2 lanes and the odd tail; the in-place form with the moved column."""
    import torch
    n, m, p = 4194307, 20, 12
    rng = np.random.default_rng(7)
    ldv = n + 1
    V_h = rng.uniform(-1.0, 1.0, (m + 1, n))
    S_h = rng.uniform(-1.0, 1.0, (m, p))
    buf = np.full((m + 1, ldv), np.nan)
    buf[:, :n] = V_h
    V, S = _dev(buf.reshape(-1)), _dev(S_h.T.reshape(-1))
    _rotate(hp, V, ldv, m, p, S, 1, None, 0, 0, n)
    torch.cuda.synchronize()
    got = V.view(m + 1, ldv).cpu().numpy()
    assert _bits_eq(got[:p, :n], ec.rotate(V_h[:m], S_h)) and _bits_eq(got[p, :n], V_h[m])
    assert _bits_eq(got[p + 1:, :n], V_h[p + 1:]) and np.isnan(got[:, n]).all()


# ---- 2. the Lanczos second pass on its own -------------------------------------------------------------------------------------
class _Alone:
    """Device buffers and the C entry for one (n, c): the basis at an even pitch, the small arrays of ncv = 32."""

    def __init__(self, hp, n, c):
        import torch
        self.torch, self.lib, self.n, self.c, self.m = torch, hp._capi.load(), n, c, 32
        self.ldv = n + (n & 1)
        self.off = [self.lib.hpcla_eigsh_small_offset(self.m, k) for k in range(7)]
        self.work = torch.zeros(self.lib.hpcla_gmres_work_bytes(self.m) // 8, dtype=torch.float64, device="cuda")

    def basis(self, V_h):
        buf = np.full((V_h.shape[0], self.ldv), np.nan)          # the pad (odd n) poisoned: no kernel may read it
        buf[:, :self.n] = V_h
        return _dev(buf.reshape(-1))

    def small(self, **arrays):
        s = np.full(self.off[6], 7.0)
        for name, a in arrays.items():
            k = SMALL.index(name)
            a = np.asarray(a, dtype=np.float64).reshape(-1)
            s[self.off[k]:self.off[k] + a.size] = a
        return _dev(s)

    def view(self, small, name):
        k = SMALL.index(name)
        a = small[self.off[k]:self.off[k + 1]].cpu().numpy()
        return a.reshape(self.m, self.m).copy() if name == "T" else a     # T[j] is column j

    def state(self, done=0, status=RUNNING):
        return self.torch.tensor([done, status, 0, 0], dtype=self.torch.int64, device="cuda")

    def update(self, V, h, w, st, it, small):
        assert self.lib.hpcla_eigsh_update_f64(None, V.data_ptr(), self.ldv, self.c, h.data_ptr(), w.data_ptr(), self.n, it,
                                               self.m, small.data_ptr(), st.data_ptr(), self.work.data_ptr(), None) == 0


@pytest.mark.parametrize("n,c", gr.EIGSH_UPDATE_ALONE)
def test_lanczos_second_pass_alone(hp, n, c):
    """The (n, c) edges of tests/test_gpu_gmres.py: 2049 is the last size on one reduction workgroup with a scalar tail, 2051 the
    first odd size on two; c = 8 | 9 is the edge of the 4-fold unrolled column loop and 17, 31 leave remainders of it.
    614 403 (c = 1 and 9) is odd with 301 partials: eigsh_update_stage2 walks them in two trips of 256 lanes, the last one ragged
    (45 lanes), and gmres_update<true> runs on 301 workgroups; 4 194 307 (c = 9: the basis is (c + 1) n doubles) caps that grid at
    2048 workgroups of five grid-stride trips, eight full trips of the second stage, and is odd.  tests/_grid_regimes.py holds the
    sizes, tests/test_grid_regimes.py checks that they reach every regime."""
    import torch
    K = _Alone(hp, n, c)
    rng = np.random.default_rng(1000 * c + n % 1000)
    j, it = c - 1, 7
    V_h = rng.uniform(-1.0, 1.0, (c + 1, n))
    w_h = rng.uniform(-1.0, 1.0, n)
    h1_h, h2_h = rng.uniform(-1.0, 1.0, c), 1e-3 * rng.uniform(-1.0, 1.0, c)
    pad = lambda a: np.concatenate([a, np.full(K.m - len(a), 7.0)])
    V = K.basis(V_h)

    def run(h1, h2, w0, st):
        small, w = K.small(h1=pad(h1), h2=pad(h2)), _dev(w0)
        K.update(V, small[K.off[3]:K.off[3] + c], w, st, it, small)
        torch.cuda.synchronize()
        return small, w

    # -- running: w, nn, the stored column
    st = K.state()
    small, w = run(h1_h, h2_h, w_h, st)
    w2_h = gc.subtract_columns(w_h, V_h, h2_h)
    assert _bits_eq(w, w2_h) and st.cpu().tolist()[:2] == [0, RUNNING]
    nn = K.view(small, "nn")[0]
    err = abs(nn - math.fsum((w2_h * w2_h).tolist())) / float((w2_h * w2_h).sum())
    print(f"n = {n}, c = {c}: w.w {err:.2e}")
    assert err <= 1e-12
    T_r, beta_r = np.full((K.m, K.m), 7.0), np.full(K.m, 7.0)
    assert ec.small_step(j, h1_h, h2_h, nn, T_r.T, beta_r) == "running"          # T_r[j] is column j
    assert _bits_eq(K.view(small, "T"), T_r) and _bits_eq(K.view(small, "beta"), beta_r)
    assert _bits_eq(K.view(small, "hn"), [math.sqrt(nn)])
    if n & 1:
        assert bool(torch.isnan(V.view(c + 1, K.ldv)[:, n]).all())

    # -- gate I: w = 0 and h2 = 0: the column is stored, beta[j] = hn = 0
    st = K.state()
    small, w = run(h1_h, np.zeros(c), np.zeros(n), st)
    assert st.cpu().tolist()[:2] == [it, INVARIANT] and not w.cpu().numpy().any()
    T_r, beta_r = np.full((K.m, K.m), 7.0), np.full(K.m, 7.0)
    assert ec.small_step(j, h1_h, np.zeros(c), 0.0, T_r.T, beta_r) == "invariant"
    assert _bits_eq(K.view(small, "T"), T_r) and _bits_eq(K.view(small, "beta"), beta_r) and _bits_eq(K.view(small, "hn"), [0.0])

    # -- gate N: a NaN coefficient: nothing of column j is stored
    st = K.state()
    small, w = run(h1_h, np.full(c, np.nan), w_h, st)
    assert st.cpu().tolist()[:2] == [it - 1, BREAKDOWN]
    assert all((K.view(small, name) == 7.0).all() for name in ("T", "beta", "hn"))

    # -- frozen: no byte is written
    for frozen in ([it - 1, BREAKDOWN], [it, INVARIANT], [it, CONVERGED]):
        st = K.state(done=frozen[0], status=frozen[1])
        small = K.small(h1=pad(h1_h), h2=pad(h2_h))
        small0, w, work0 = small.clone(), _dev(w_h), K.work.clone()
        K.update(V, small[K.off[3]:K.off[3] + c], w, st, it, small)
        torch.cuda.synchronize()
        assert _bits_eq(w, w_h) and torch.equal(small.view(torch.int64), small0.view(torch.int64)), frozen
        assert torch.equal(K.work.view(torch.int64), work0.view(torch.int64)) and st.cpu().tolist()[:2] == frozen


# ---- 3. the first cycle's projected matrix against the restatement ------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_first_cycle_matches_the_restatement(hp, cases, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    """24 x 20 at ncv = 20: T and beta of the first cycle within T_RTOL = 1e-12 of max|T| (about 300 times the CPU spread)."""
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    rowptr, colidx, vals = cases["mats"]["plain", (24, 20)]
    n, m = len(rowptr) - 1, 20
    A = _matrix(hp, backend, rowptr, colidx, vals)
    first = {}
    _, _, ref = ec.eigsh(rowptr, colidx, vals, k=4, ncv=m, maxiter=1, first_T=first)
    ws = hp.EigshWorkspace(hp.HPCVector.from_global(np.zeros(n), backend), m)
    _, _, info = hp.eigsh(A, k=4, ncv=m, maxiter=1, workspace=ws)                         # one cycle, then "maxiter"
    assert (info.status, info.iterations, info.restarts) == ("maxiter", m, 0) == (ref["status"], ref["iterations"], ref["restarts"])
    T = ws.small_array("T").cpu().numpy().reshape(m, m).T                                 # T[i, j]
    beta = ws.small_array("beta").cpu().numpy()
    scale = np.abs(first["T"]).max()
    dT = np.abs(np.triu(T) - np.triu(first["T"])).max() / scale
    db = np.abs(beta - first["beta"]).max() / scale
    print(f"{which}: first-cycle T deviation {dT:.2e}, beta {db:.2e} (relative to max|T| = {scale:.3g})")
    assert dT <= ec.T_RTOL and db <= ec.T_RTOL
    assert not np.tril(T, -1).any()                                                       # only the upper triangle is written
    hp.clear_plan_cache()


def test_first_cycle_at_the_large_size(hp, orc, gpu_backend_i32):
    """Plain Poisson at 65 x 63: 4095 rows, odd, so both passes of every Lanczos step run on two stage-1 workgroups and
    eigsh_update_stage2 adds two partials (the other solves of this file stay on one).  ncv = 20, one cycle: T and beta within
    T_RTOL = 1e-12 of max|T|, 700 times the spread of four summation orders on the CPU at this size (T 1.3e-15, beta 1.4e-15;
    tests/test_eigsh_cases.py re-measures both).  No convergence is asserted here."""
    rowptr, colidx, vals = ec.plain_poisson(orc, *ec.LARGE_SIZE)
    n, m = len(rowptr) - 1, 20
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, vals)
    first = {}
    _, _, ref = ec.eigsh(rowptr, colidx, vals, k=4, ncv=m, maxiter=1, first_T=first)
    ws = hp.EigshWorkspace(hp.HPCVector.from_global(np.zeros(n), gpu_backend_i32), m)
    _, _, info = hp.eigsh(A, k=4, ncv=m, maxiter=1, workspace=ws)
    assert (info.status, info.iterations, info.restarts) == ("maxiter", m, 0) == (ref["status"], ref["iterations"], ref["restarts"])
    T = ws.small_array("T").cpu().numpy().reshape(m, m).T
    beta = ws.small_array("beta").cpu().numpy()
    scale = np.abs(first["T"]).max()
    dT = np.abs(np.triu(T) - np.triu(first["T"])).max() / scale
    db = np.abs(beta - first["beta"]).max() / scale
    print(f"{ec.LARGE_SIZE}: first-cycle T deviation {dT:.2e}, beta {db:.2e} (relative to max|T| = {scale:.3g})")
    assert dT <= ec.T_RTOL and db <= ec.T_RTOL
    assert not np.tril(T, -1).any()
    hp.clear_plan_cache()


# ---- 4. convergence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(ec.CONVERGENCE)))
def test_convergence_against_the_dense_spectrum(hp, cases, gpu_backend_i32, case):
    name, k, ncv, whiches = ec.CONVERGENCE[case]
    rowptr, colidx, vals = cases["mats"][name]
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, vals)
    p = k + (ncv - k) // 2
    for which in whiches:
        _, _, ref = cases["ref"][name, k, ncv, which]
        got, X, info = hp.eigsh(A, k=k, which=which, ncv=ncv, tol=ec.TOL)
        assert info.converged and info.status == "converged" == ref["status"]
        assert got.dtype == np.float64 and got.shape == (k,) and np.all(np.diff(got) > 0) and X.shape == (A.shape[0], k)
        err = np.abs(got - ec.reference_values(cases["ev"][name], k, which)).max() / info.anorm
        AX = A @ X
        true = np.array([hp.norm(AX[:, i] - float(got[i]) * X[:, i]) for i in range(k)])
        res = true.max() / (ec.TOL * info.anorm)
        est = np.abs(true - info.residual_norms).max() / info.anorm
        orth = np.abs((hp.transpose(X) @ X).gather() - np.eye(k)).max()
        print(f"{name} k {k} ncv {ncv} {which}: {info.iterations} steps (restatement {ref['iterations']}), {info.restarts} restarts, "
              f"eigenvalue error {err:.1e} anorm, true residual {res:.2f} tol anorm, orthogonality {orth:.1e}, estimate vs true "
              f"residual {est:.1e} anorm")
        assert err <= ec.VAL_RTOL
        assert abs(info.iterations - ref["iterations"]) <= ncv - p
        assert res <= pc.TRUE_RES_FACTOR
        assert orth <= 1e-12
        assert info.residual_norms.shape == (k,) and np.all(info.residual_norms <= ec.TOL * info.anorm)
        assert est <= 1e-12                                      # residual_norms[i] is the estimate of pair i, not of another
        assert len(info.history) == info.restarts + 1 and info.history[-1] == info.residual_norms.max()
        assert info.iterations == ncv + info.restarts * (ncv - p)
    hp.clear_plan_cache()


# ---- 5. return_eigenvectors=False and a dirty workspace ------------------------------------------------------------------------
def test_values_only_and_a_dirty_workspace(hp, cases, gpu_backend_i32):
    rowptr, colidx, vals = cases["mats"]["plain", (24, 20)]
    n = len(rowptr) - 1
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, vals)
    got, X, info = hp.eigsh(A, k=4, which="SA", ncv=20)
    xv = X.local_values().copy()
    got2, X2, info2 = hp.eigsh(A, k=4, which="SA", ncv=20, return_eigenvectors=False)
    assert X2 is None and np.array_equal(pc.bits(got2), pc.bits(got)) and info2.iterations == info.iterations
    ws = hp.EigshWorkspace(hp.HPCVector.from_global(np.zeros(n), gpu_backend_i32), 20)
    hp.eigsh(A, k=2, which="LA", ncv=20, maxiter=30, seed=5, workspace=ws)                # another solve, stopped early
    got3, X3, info3 = hp.eigsh(A, k=4, which="SA", ncv=20, workspace=ws)
    assert np.array_equal(pc.bits(got3), pc.bits(got)) and np.array_equal(pc.bits(X3.local_values()), pc.bits(xv))
    assert (info3.iterations, info3.restarts, info3.history) == (info.iterations, info.restarts, info.history)
    got4, X4, _ = hp.eigsh(A, k=4, which="SA", ncv=20, workspace=ws)                      # and on its own leftovers
    assert np.array_equal(pc.bits(got4), pc.bits(got)) and np.array_equal(pc.bits(X4.local_values()), pc.bits(xv))
    got5, _, _ = hp.eigsh(A, k=4, which="SA", ncv=24, workspace=ws)                       # another ncv: a workspace of its own
    assert np.abs(got5 - got).max() <= 1e-12 * info.anorm
    hp.clear_plan_cache()


# ---- 6. the exact cases ------------------------------------------------------------------------------------------------------
def test_exact_cases(hp, gpu_backend_i32):
    B = gpu_backend_i32
    d = np.arange(1.0, 13.0)
    A = _matrix(hp, B, *pc.diag_matrix(d))
    e3 = np.zeros(12)
    e3[2] = 1.0
    v0 = hp.HPCVector.from_global(e3, B)
    got, X, info = hp.eigsh(A, k=1, v0=v0)                       # A e_3 = 3 e_3: the Krylov space is invariant after one step
    assert (info.status, info.converged, info.iterations, info.restarts) == ("invariant", True, 1, 0)
    assert got.tolist() == [3.0] and X.shape == (12, 1) and np.array_equal(np.abs(X.local_values()[:, 0]), e3)
    assert info.residual_norms.tolist() == [0.0]
    got, X, info = hp.eigsh(A, k=2, v0=v0)                       # one pair found, two wanted
    assert (info.status, info.converged, info.iterations) == ("invariant", False, 1)
    assert got.tolist() == [3.0] and X.shape == (12, 1)
    for which, want in (("LA", [10, 11, 12]), ("SA", [1, 2, 3]), ("LM", [10, 11, 12])):
        got, X, info = hp.eigsh(A, k=3, which=which, ncv=12)     # ncv = n: the whole spectrum after one cycle
        assert (info.status, info.converged, info.iterations, info.restarts) == ("converged", True, 12, 0)
        assert np.abs(got - want).max() <= 1e-12 * 12
    bad = d.copy()
    bad[5] = np.nan
    got, X, info = hp.eigsh(_matrix(hp, B, *pc.diag_matrix(bad)), k=2, ncv=8)
    assert (info.status, info.converged) == ("breakdown", False)
    assert got.shape == (2,) and X.shape == (12, 2) and info.residual_norms.shape == (2,)
    got, X, info = hp.eigsh(_matrix(hp, B, *pc.diag_matrix(np.arange(1.0, 61.0))), k=4, ncv=20, maxiter=5)
    assert (info.status, info.converged, info.iterations, info.restarts) == ("maxiter", False, 20, 0)
    assert len(info.history) == 1 and got.shape == (4,) and X.shape == (60, 4)
    hp.clear_plan_cache()


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------
def test_eigsh_argument_errors(hp, cases, gpu_backend_i32):
    rowptr, colidx, vals = cases["mats"]["plain", (24, 20)]
    n = len(rowptr) - 1
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, vals)
    with pytest.raises(ValueError, match="shift-invert"):
        hp.eigsh(A, which="SM")
    for bad in (dict(which="BE"), dict(k=0), dict(k=6, ncv=6), dict(k=6, ncv=5), dict(ncv=65), dict(tol=-1.0)):
        with pytest.raises(ValueError):
            hp.eigsh(A, **bad)
    with pytest.raises(ValueError):                                                      # ncv > n
        hp.eigsh(_matrix(hp, gpu_backend_i32, *pc.diag_matrix(np.arange(1.0, 13.0))), k=3, ncv=13)
    with pytest.raises(ValueError):
        hp.EigshWorkspace(hp.HPCVector.from_global(np.zeros(n), gpu_backend_i32), 65)
    with pytest.raises(ValueError):                                                      # a rectangular A
        hp.eigsh(_matrix(hp, gpu_backend_i32, rowptr, colidx, vals, n + 7))
    with pytest.raises(ValueError):                                                      # v0 on another partition
        hp.eigsh(A, v0=hp.HPCVector.from_global(np.ones(n + 2), gpu_backend_i32))
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    with pytest.raises(TypeError):
        hp.eigsh(_matrix(hp, b32, rowptr, colidx, vals.astype(np.float32)))
    hp.clear_plan_cache()


# ---- 8. ranks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_eigsh_across_ranks(nranks):
    """The ranks share the one GPU (peer-window push transport, like tests/test_gpu_multirank.py); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
