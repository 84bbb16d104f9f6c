"""GPU tests of the truncated SVD: the second Gram-Schmidt pass of either side on its own through the C ABI, the first cycle's
projected matrix against the numpy restatement, convergence against the dense SVD, a dirty workspace, the exact cases, the
argument errors and the solve across ranks.  Cases and the restatement: tests/_svds_cases.py.

Margins (none of them taken from the device's results; tests/test_svds_cases.py re-measures the CPU figures and prints them):
  * the elements of w, and the small step's B[:, j], alpha, beta[j] and the divisor: bit-equal to numpy's separately rounded
    expressions (the library is built with -ffp-contract=off; IEEE sqrt);
  * aa = u.u and bb = v.v: 1e-12 of math.fsum relative to the sum of |terms|, the project's margin for its reductions;
  * the first cycle's B and beta: T_RTOL = 1e-12 of max|B|, the project's margin (four summation orders on the CPU spread by
    <= 2.2e-15 of max|B| on the 24 x 20 cases, 1.1e-14 absolute: about 450 times less; the bound on that spread is 1e-13; at
    65 x 63 they spread by <= 3.6e-15 of max|B|: 280 times less);
  * singular values: VAL_RTOL = 1e-12 of anorm against numpy.linalg.svd of the dense matrix (the restatement: <= 5.0e-15, its
    spread over the four orders <= 5.7e-15);
  * step counts: within one cycle's m - p steps of the restatement's (identical across the four orders on the CPU);
  * true residuals ||A' u_i - s_i v_i|| <= 2 tol anorm (the restatement: <= 0.95; the factor 2 is hp.gmres's margin);
  * ||A v_i - s_i u_i|| <= 1e-12 anorm: zero up to rounding by construction (the restatement: <= 1.2e-14);
  * residual_norms[i] within 1e-12 anorm of the true residual of triplet i, which is what shows that the estimates are aligned
    with s: with full reorthogonalisation the two differ by rounding alone (the restatement: <= 9.2e-15 anorm);
  * U'U and V'V within 1e-12 of the identity (the restatement: <= 5.8e-15).
Singular vector signs are compared only as the pair (u_i, v_i) through u_i' A v_i > 0."""
import math
import os

import numpy as np
import pytest

from tests import _grid_regimes as gr
from tests import _pcg_cases as pc
from tests import _svds_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_svds_worker.py")

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN, INVARIANT = 0, 1, 2, 4
SMALL = ("B", "beta", "g1", "g2", "h1", "h2", "aa", "bb", "dv")
LEFT, RIGHT = 0, 1


def _matrix(hp, backend, rowptr, colidx, vals, ncols):
    return hp.HPCSparseMatrix_local(rowptr, colidx, vals, ncols, backend)


def _bits_eq(t, want):
    got = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.array_equal(pc.bits(got), pc.bits(np.asarray(want, dtype=np.float64)))


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).cuda()


@pytest.fixture(scope="module")
def cases(orc):
    """Every convergence case with its dense singular values and the restatement's results, computed once."""
    mats = sc.matrices(orc)
    out = {"mats": mats, "sv": {name: sc.dense_singular_values(*mats[name]) for name in mats}, "ref": {}}
    for name, k, ncv in sc.CONVERGENCE:
        out["ref"][name, k, ncv] = sc.svds(*mats[name], k=k, ncv=ncv)
    return out


# ---- 1. the second pass of either side on its own --------------------------------------------------------------------------------
class _Alone:
    """Device buffers and the C entry for one (n, c): the basis at an even pitch, the small arrays of ncv = 32."""

    def __init__(self, hp, n, c):
        import torch
        self.torch, self.lib, self.n, self.c, self.m = torch, hp._capi.load(), n, c, 32
        self.ldw = n + (n & 1)
        self.off = [self.lib.hpcla_svds_small_offset(self.m, k) for k in range(10)]
        self.work = torch.zeros(self.lib.hpcla_gmres_work_bytes(self.m) // 8, dtype=torch.float64, device="cuda")

    def basis(self, W_h):
        buf = np.full((W_h.shape[0], self.ldw), np.nan)          # the pad (odd n) poisoned: no kernel may read it
        buf[:, :self.n] = W_h
        return _dev(buf.reshape(-1))

    def small(self, **arrays):
        s = np.full(self.off[9], 7.0)
        for name, a in arrays.items():
            k = SMALL.index(name)
            a = np.asarray(a, dtype=np.float64).reshape(-1)
            s[self.off[k]:self.off[k] + a.size] = a
        return _dev(s)

    def view(self, small, name):
        k = SMALL.index(name)
        a = small[self.off[k]:self.off[k + 1]].cpu().numpy()
        return a.reshape(self.m, self.m).copy() if name == "B" else a     # B[j] is column j

    def state(self, done=0, status=RUNNING):
        return self.torch.tensor([done, status, 0, 0], dtype=self.torch.int64, device="cuda")

    def update(self, W, side, small, w, st, it):
        k = SMALL.index("g2" if side == LEFT else "h2")          # the second pass's coefficients live in the small buffer
        h = small[self.off[k]:self.off[k] + max(self.c, 1)]
        assert self.lib.hpcla_svds_update_f64(None, W.data_ptr() if W is not None else None, self.ldw, self.c, h.data_ptr(),
                                              w.data_ptr(), self.n, it, self.m, side, small.data_ptr(), st.data_ptr(),
                                              self.work.data_ptr(), None) == 0


def _expected_small(K, side, j, c1, c2, nn):
    """The small arrays after the restated small step, starting from the poison 7.0: (B, beta, dv, status)."""
    B_r, beta_r = np.full((K.m, K.m), 7.0), np.full(K.m, 7.0)
    status, r = sc.small_step(side, j, c1, c2, nn, B_r.T, beta_r)            # B_r[j] is column j
    return B_r, beta_r, (7.0 if r is None else r), status


def _check_update_alone(hp, n, c, side):
    import torch
    K = _Alone(hp, n, c)
    rng = np.random.default_rng(1000 * c + n % 1000 + side)
    j, it = c - side, 7                                          # left: c = j columns; right: c = j + 1
    names = ("g1", "g2", "aa") if side == LEFT else ("h1", "h2", "bb")
    W_h = rng.uniform(-1.0, 1.0, (max(c, 1), n))
    w_h = rng.uniform(-1.0, 1.0, n)
    c1_h, c2_h = rng.uniform(-1.0, 1.0, c), 1e-3 * rng.uniform(-1.0, 1.0, c)
    pad = lambda a: np.concatenate([a, np.full(K.m - len(a), 7.0)])
    W = K.basis(W_h)
    done_z = it - 1 if side == LEFT else it

    def run(c1, c2, w0, st):
        small, w = K.small(**{names[0]: pad(c1), names[1]: pad(c2)}), _dev(w0)
        K.update(W if c else None, side, small, w, st, it)
        torch.cuda.synchronize()
        return small, w

    def untouched(small, c1, c2):                                # the other side's arrays and the coefficients keep their bits
        other = ("h1", "h2", "bb") if side == LEFT else ("g1", "g2", "aa")
        return (all((K.view(small, name) == 7.0).all() for name in other) and _bits_eq(K.view(small, names[0]), pad(c1))
                and _bits_eq(K.view(small, names[1]), pad(c2)))

    # -- running: w, the norm, the stored column or beta, the divisor
    st = K.state()
    small, w = run(c1_h, c2_h, w_h, st)
    w2_h = sc.subtract(w_h, W_h, c2_h)
    assert _bits_eq(w, w2_h) and st.cpu().tolist()[:2] == [0, RUNNING]
    nn = K.view(small, names[2])[0]
    err = abs(nn - math.fsum((w2_h * w2_h).tolist())) / float((w2_h * w2_h).sum())
    print(f"side {side}, n = {n}, c = {c}: w.w {err:.2e}")
    assert err <= 1e-12
    B_r, beta_r, dv_r, status = _expected_small(K, side, j, c1_h, c2_h, nn)
    assert status == "running"
    assert _bits_eq(K.view(small, "B"), B_r) and _bits_eq(K.view(small, "beta"), beta_r) and _bits_eq(K.view(small, "dv"), [dv_r])
    assert untouched(small, c1_h, c2_h)
    if n & 1 and c:
        assert bool(torch.isnan(W.view(max(c, 1), K.ldw)[:, n]).all())

    # -- gates Z and Z': w = 0 and no second correction: the column (left) or beta[j] = 0 (right) is stored, the divisor is 0
    st = K.state()
    small, w = run(c1_h, np.zeros(c), np.zeros(n), st)
    assert st.cpu().tolist()[:2] == [done_z, INVARIANT] and not w.cpu().numpy().any()
    B_r, beta_r, dv_r, status = _expected_small(K, side, j, c1_h, np.zeros(c), 0.0)
    assert status == "invariant" and dv_r == 0.0
    assert _bits_eq(K.view(small, "B"), B_r) and _bits_eq(K.view(small, "beta"), beta_r) and _bits_eq(K.view(small, "dv"), [0.0])

    # -- gates N and N': a NaN in w: nothing of column j is stored
    bad = w_h.copy()
    bad[n // 2] = np.nan
    st = K.state()
    small, w = run(c1_h, c2_h, bad, st)
    assert st.cpu().tolist()[:2] == [it - 1, BREAKDOWN]
    assert all((K.view(small, name) == 7.0).all() for name in ("B", "beta", "dv")) and untouched(small, c1_h, c2_h)

    # -- frozen: no byte is written
    for frozen in ([it - 1, BREAKDOWN], [it, INVARIANT], [it - 1, INVARIANT], [it, CONVERGED]):
        st = K.state(done=frozen[0], status=frozen[1])
        small = K.small(**{names[0]: pad(c1_h), names[1]: pad(c2_h)})
        small0, w, work0 = small.clone(), _dev(w_h), K.work.clone()
        K.update(W if c else None, side, small, w, st, it)
        torch.cuda.synchronize()
        assert _bits_eq(w, w_h) and torch.equal(small.view(torch.int64), small0.view(torch.int64)), frozen
        assert torch.equal(K.work.view(torch.int64), work0.view(torch.int64)) and st.cpu().tolist()[:2] == frozen


@pytest.mark.parametrize("n,c", gr.EIGSH_UPDATE_ALONE)
def test_second_pass_alone_on_both_sides(hp, n, c):
    """The (n, c) edges of the Lanczos second pass (tests/_grid_regimes.py): 2049 is the last size on one reduction workgroup
    with a scalar tail, 2051 the first odd size on two; c = 8 | 9 is the edge of the 4-fold unrolled column loop and 17, 31 leave
    remainders of it; 614 403 has 301 partials (two trips of the second stage, the last one ragged), 4 194 307 caps the grid at
    2048 workgroups.  On the left side c columns are column j = c of B (c <= ncv - 1 = 31), on the right side column j = c - 1.
    The pad of an odd n is NaN and stays NaN (and is never read: w would carry it)."""
    for side in (LEFT, RIGHT):
        _check_update_alone(hp, n, c, side)


@pytest.mark.parametrize("n", [1, 2049, 2051])
def test_left_second_pass_with_an_empty_basis(hp, n):
    """c = 0 on the left side (column 0 of the first cycle): the norm and the small step alone, no basis and no coefficients."""
    _check_update_alone(hp, n, 0, LEFT)


# ---- 2. the first cycle's projected matrix against the restatement ------------------------------------------------------------
def _first_cycle(hp, backend, M, label):
    m = 20
    A = _matrix(hp, backend, *M)
    first = {}
    _, _, _, ref = sc.svds(*M, k=4, ncv=m, maxiter=1, first_B=first)
    ws = hp.SvdsWorkspace(A, m)
    _, _, _, info = hp.svds(A, k=4, ncv=m, maxiter=1, workspace=ws)                       # one cycle, then "maxiter"
    assert (info.status, info.iterations, info.restarts) == ("maxiter", m, 0) == (ref["status"], ref["iterations"], ref["restarts"])
    B = ws.small_array("B").cpu().numpy().reshape(m, m).T                                 # B[i, j]
    beta = ws.small_array("beta").cpu().numpy()
    scale = np.abs(first["B"]).max()
    dB = np.abs(np.triu(B) - np.triu(first["B"])).max() / scale
    db = np.abs(beta - first["beta"]).max() / scale
    print(f"{label}: first-cycle B deviation {dB:.2e}, beta {db:.2e} (relative to max|B| = {scale:.3g})")
    assert dB <= sc.T_RTOL and db <= sc.T_RTOL
    assert not np.tril(B, -1).any()                                                       # the strict lower triangle is never written
    hp.clear_plan_cache()


@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_first_cycle_matches_the_restatement(hp, cases, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    """``tall`` 24 x 20 at ncv = 20: B and beta of the first cycle within T_RTOL = 1e-12 of max|B| (about 450 times the CPU
    spread)."""
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    _first_cycle(hp, gpu_backend_i32 if which == "i32" else gpu_backend_i64, cases["mats"]["tall"], which)


def test_first_cycle_at_the_large_size(hp, orc, gpu_backend_i32):
    """``tall`` at 65 x 63: 8190 x 4095, so the left half's passes run on four stage-1 workgroups and the right half's, over an
    odd length, on two, and svds_update_stage2 adds four and two partials (the other solves of this file stay on one).  B and
    beta within T_RTOL = 1e-12 of max|B|, 280 times the spread of four summation orders on the CPU at this size (3.6e-15;
    tests/test_svds_cases.py re-measures it).  No convergence is asserted here."""
    _first_cycle(hp, gpu_backend_i32, sc.matrix(orc, "tall", sc.LARGE_SIZE), str(sc.LARGE_SIZE))


# ---- 3. convergence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(sc.CONVERGENCE)))
def test_convergence_against_the_dense_svd(hp, cases, gpu_backend_i32, case):
    name, k, ncv = sc.CONVERGENCE[case]
    M = cases["mats"][name]
    A = _matrix(hp, gpu_backend_i32, *M)
    p = k + (ncv - k) // 2
    ref = cases["ref"][name, k, ncv][3]
    U, s, V, info = hp.svds(A, k=k, ncv=ncv, tol=sc.TOL)
    assert info.converged and info.status == "converged" == ref["status"]
    assert s.dtype == np.float64 and s.shape == (k,) and np.all(np.diff(s) < 0)           # descending
    assert U.shape == (A.shape[0], k) and V.shape == (A.shape[1], k)
    f = sc.figures(*M, U.local_values(), s, V.local_values(), info, cases["sv"][name])
    print(f"{name} k {k} ncv {ncv}: {info.iterations} steps (restatement {ref['iterations']}), {info.restarts} restarts, value "
          f"error {f['err']:.1e} anorm, true residual {f['res']:.2f} tol anorm, A v - s u {f['left']:.1e} anorm, orthogonality "
          f"{f['orth']:.1e}, estimate vs true residual {f['est']:.1e} anorm")
    assert f["err"] <= sc.VAL_RTOL
    assert abs(info.iterations - ref["iterations"]) <= ncv - p
    assert info.iterations == ncv + info.restarts * (ncv - p)
    assert f["res"] <= pc.TRUE_RES_FACTOR
    assert f["left"] <= 1e-12
    assert f["est"] <= 1e-12                                     # residual_norms[i] is the estimate of triplet i, not of another
    assert f["orth"] <= 1e-12
    assert f["sign"] > 0                                         # signs as the pair (u_i, v_i)
    assert info.residual_norms.shape == (k,) and np.all(info.residual_norms <= sc.TOL * info.anorm)
    assert len(info.history) == info.restarts + 1 and info.history[-1] == info.residual_norms.max() and info.anorm == s[0]
    hp.clear_plan_cache()


# ---- 4. return_singular_vectors=False and a dirty workspace ---------------------------------------------------------------------
def test_values_only_and_a_dirty_workspace(hp, cases, gpu_backend_i32):
    A = _matrix(hp, gpu_backend_i32, *cases["mats"]["tall"])
    U, s, V, info = hp.svds(A, k=4, ncv=20)
    uv, vv = U.local_values().copy(), V.local_values().copy()
    U2, s2, V2, info2 = hp.svds(A, k=4, ncv=20, return_singular_vectors=False)
    assert U2 is None and V2 is None and np.array_equal(pc.bits(s2), pc.bits(s)) and info2.iterations == info.iterations
    ws = hp.SvdsWorkspace(A, 20)
    assert ws.fits(A, 20) and not ws.fits(A, 24) and not ws.fits(_matrix(hp, gpu_backend_i32, *cases["mats"]["wide"]), 20)
    hp.svds(A, k=2, ncv=20, maxiter=30, seed=5, workspace=ws)                             # another solve, stopped early
    for _ in range(2):                                                                    # ... and then on its own leftovers
        U3, s3, V3, info3 = hp.svds(A, k=4, ncv=20, workspace=ws)
        assert np.array_equal(pc.bits(s3), pc.bits(s)) and np.array_equal(pc.bits(U3.local_values()), pc.bits(uv))
        assert np.array_equal(pc.bits(V3.local_values()), pc.bits(vv))
        assert (info3.iterations, info3.restarts, info3.history) == (info.iterations, info.restarts, info.history)
    _, s5, _, _ = hp.svds(A, k=4, ncv=24, workspace=ws)                                   # another ncv: a workspace of its own
    assert np.abs(s5 - s).max() <= 1e-12 * info.anorm
    hp.clear_plan_cache()


# ---- 5. the exact cases ------------------------------------------------------------------------------------------------------
def test_exact_cases(hp, gpu_backend_i32):
    B = gpu_backend_i32
    d = np.arange(1.0, 13.0)
    A = _matrix(hp, B, *pc.diag_matrix(d), 12)
    e3 = np.zeros(12)
    e3[2] = 1.0
    v0 = hp.HPCVector.from_global(e3, B)
    U, s, V, info = hp.svds(A, k=1, v0=v0)                       # A e_3 = 3 e_3 = A' e_3: gate Z' in the first step
    assert (info.status, info.converged, info.iterations, info.restarts) == ("invariant", True, 1, 0)
    assert s.tolist() == [3.0] and U.shape == V.shape == (12, 1) and info.residual_norms.tolist() == [0.0]
    assert np.array_equal(np.abs(U.local_values()[:, 0]), e3) and np.array_equal(np.abs(V.local_values()[:, 0]), e3)
    U, s, V, info = hp.svds(A, k=2, v0=v0)                       # one triplet found, two wanted
    assert (info.status, info.converged, info.iterations) == ("invariant", False, 1)
    assert s.tolist() == [3.0] and U.shape == V.shape == (12, 1)
    U, s, V, info = hp.svds(A, k=3, ncv=12)                      # ncv = min(M, N): the whole wanted set after one cycle
    assert (info.status, info.converged, info.iterations, info.restarts) == ("converged", True, 12, 0)
    assert np.abs(s - [12, 11, 10]).max() <= 1e-12 * 12
    # a rank-deficient tall matrix and a start with null directions: gate Z (tests/_svds_cases.py works the values out)
    R = _matrix(hp, B, *sc.rank_deficient())
    v0 = hp.HPCVector.from_global(sc.RANK_DEFICIENT_V0, B)
    U, s, V, info = hp.svds(R, k=1, ncv=3, v0=v0)
    assert (info.status, info.converged, info.iterations, info.restarts) == ("invariant", True, 1, 0)
    assert abs(s[0] - 4.0) <= 4e-15 and info.residual_norms.tolist() == [0.0] and U.shape == (6, 1) and V.shape == (4, 1)
    assert np.array_equal(np.abs(U.local_values()[:, 0]), np.eye(6)[0])
    assert np.abs(np.abs(V.local_values()[:, 0]) - np.eye(4)[0]).max() <= 1e-15
    _, s, _, info = hp.svds(R, k=2, ncv=3, v0=v0)
    assert (info.status, info.converged, info.iterations, len(s)) == ("invariant", False, 1, 1)
    U, s, V, info = hp.svds(R, k=1, ncv=3, v0=hp.HPCVector.from_global(np.eye(4)[1], B))   # a start inside the null space
    assert (info.status, info.converged, info.iterations, info.anorm) == ("invariant", False, 0, 0.0)      # gate Z at column 0
    assert s.shape == (0,) and U.shape == (6, 0) and V.shape == (4, 0) and info.residual_norms.shape == (0,)
    bad = d.copy()
    bad[5] = np.nan
    U, s, V, info = hp.svds(_matrix(hp, B, *pc.diag_matrix(bad), 12), k=2, ncv=8)
    assert (info.status, info.converged) == ("breakdown", False) and math.isnan(info.anorm)
    assert s.shape == (2,) and np.isnan(s).all() and info.residual_norms.shape == (2,)
    assert U.shape == V.shape == (12, 2) and not U.local_values().any() and not V.local_values().any()
    U, s, V, info = hp.svds(_matrix(hp, B, *pc.diag_matrix(np.arange(1.0, 61.0)), 60), k=4, ncv=20, maxiter=5)
    assert (info.status, info.converged, info.iterations, info.restarts) == ("maxiter", False, 20, 0)
    assert len(info.history) == 1 and s.shape == (4,) and U.shape == V.shape == (60, 4)
    hp.clear_plan_cache()


def test_a_lazy_transpose_is_the_solve_on_its_materialised_form(hp, cases, gpu_backend_i32):
    """``hp.svds(hp.transpose(W))`` against ``hp.svds(T)``, bit for bit: T's rows and W's rows both have ascending columns, which
    is the order ``transpose(.).materialize()`` stores, so the materialised transpose(W) is T entry for entry and its cached
    transpose W is T's materialised transpose (tests/test_gpu_lsqr.py).  U lives on W's columns, V on W's rows."""
    T = _matrix(hp, gpu_backend_i32, *cases["mats"]["tall"])
    W = _matrix(hp, gpu_backend_i32, *cases["mats"]["wide"])                              # a fresh W: nothing cached on it yet
    U1, s1, V1, info1 = hp.svds(T, k=4, ncv=20)
    U2, s2, V2, info2 = hp.svds(hp.transpose(W), k=4, ncv=20)
    assert U2.shape == (W.shape[1], 4) and V2.shape == (W.shape[0], 4)
    assert np.array_equal(pc.bits(s2), pc.bits(s1)) and (info2.iterations, info2.history) == (info1.iterations, info1.history)
    assert np.array_equal(pc.bits(U2.local_values()), pc.bits(U1.local_values()))
    assert np.array_equal(pc.bits(V2.local_values()), pc.bits(V1.local_values()))
    assert hp.transpose(W).materialize().cached_transpose is W
    hp.clear_plan_cache()


# ---- 6. argument errors ------------------------------------------------------------------------------------------------------
def test_svds_argument_errors(hp, cases, gpu_backend_i32):
    M = cases["mats"]["tall"]
    A = _matrix(hp, gpu_backend_i32, *M)
    with pytest.raises(ValueError, match="harmonic Ritz restarts or shift-invert"):
        hp.svds(A, which="SM")
    for bad in (dict(which="LA"), dict(k=0), dict(k=6, ncv=6), dict(k=6, ncv=5), dict(ncv=65), dict(tol=-1.0)):
        with pytest.raises(ValueError):
            hp.svds(A, **bad)
    with pytest.raises(ValueError):                                                      # ncv > min(M, N)
        hp.svds(_matrix(hp, gpu_backend_i32, *sc.rank_deficient()), k=3, ncv=5)
    with pytest.raises(ValueError):
        hp.SvdsWorkspace(A, 65)
    with pytest.raises(ValueError, match="columns"):                                     # v0 on the row partition of a rectangular A
        hp.svds(A, v0=hp.HPCVector.from_global(np.ones(A.shape[0]), gpu_backend_i32))
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    with pytest.raises(TypeError):
        hp.svds(hp.HPCSparseMatrix_local(M[0], M[1], M[2].astype(np.float32), M[3], b32))
    hp.clear_plan_cache()


# ---- 7. ranks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_svds_across_ranks(nranks):
    """The ranks share the one GPU (peer-window push transport, like tests/test_gpu_multirank.py); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
