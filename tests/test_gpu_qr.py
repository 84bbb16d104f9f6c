"""GPU tests of hp.qr and hp.lstsq (csrc/qr.hip): panel, tree and width edges, R against numpy, rank deficiency, layouts,
determinism, non-finite input, least-squares quality, the argument errors and the factorisation across ranks.  Inputs, limits
and the numpy restatement: tests/_qr_cases.py (tests/test_qr_cases.py runs the restatement against the same limits on the CPU).

Limits (eps = 2^-52; none taken from the device's results):
  * orth = max |Q'Q - I| <= 16 k eps and back = ||QR - X||_2 / ||X||_2 <= 16 k eps: the Householder bound, linear in k and
    independent of kappa.  A numpy TSQR measured 3-7 eps and <= 5 eps; X inv(R) reaches 3.5e-5 at kappa = 1e12 and CholQR
    fails there.  numpy.linalg.qr of the same X is asserted within the same limits.
  * R against the sign-normalised numpy R at kappa = 1e3: 1e-10 relative in the Frobenius norm (perturbation bound about
    kappa k eps = 7e-12; the numpy TSQR measured 4e-16).
  * lstsq: neq <= 16 k eps (numpy TSQR: 0.4 eps at most; numpy.linalg.lstsq asserted too); rnorm within 1e-6 relative of numpy's
    residual (worst measured 3.5e-9 at kappa = 1e10); a consistent system: ||c - c0|| / ||c0|| <= 10 kappa eps and
    rnorm <= 64 eps ||b|| (measured 2.3e-15 / 1.5e-12 and under 1e-15).
The products in the checks are taken on the host in numpy from the gathered Q.  Shapes are written with P and F(k) read from
the library."""
import os

import numpy as np
import pytest

from tests import _qr_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_qr_worker.py")

pytestmark = pytest.mark.gpu


def _consts(hp, k):
    lib = hp._capi.load()
    return lib.hpcla_qr_panel_rows(), lib.hpcla_qr_fan(k)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_np_cache = {}


def _numpy_qr(key, X):
    """numpy.linalg.qr of X, once per input: asserted within the limits, R returned sign-normalised."""
    if key not in _np_cache:
        Qn, Rn = np.linalg.qr(X)
        k = X.shape[1]
        assert qc.orth(Qn) <= qc.limit(k) and qc.back(Qn, Rn, X) <= qc.limit(k), key
        _np_cache[key] = qc.sign_normalised(Rn)
    return _np_cache[key]


def _check(hp, backend, X, key=None, label=""):
    """hp.qr(X) meets the limits, with a well-formed R.  Returns (gathered Q, R)."""
    n, k = X.shape
    if key is not None:
        _numpy_qr(key, X)
    Q, R = hp.qr(hp.HPCMatrix.from_global(X, backend))
    Qg = Q.gather()
    assert Qg.shape == (n, k) and Q.A.is_contiguous() and np.array_equal(Q.row_partition, [0, n])
    o, b = qc.orth(Qg), qc.back(Qg, R, X)
    print(f"{label} n={n} k={k}: orth {o / qc.EPS:.1f} eps, back {b / qc.EPS:.1f} eps, limit {16 * k} eps")
    assert o <= qc.limit(k), (n, k, o)
    assert b <= qc.limit(k), (n, k, b)
    qc.check_r_shape(R, k)
    return Qg, R


# ---- 1. panel and tree edges -------------------------------------------------------------------------------------------------
def _edge_sizes(hp, k):
    P, F = _consts(hp, k)
    if k == 16:
        return (16, 17, P - 1, P, P + 1, 2 * P + 3, P * F, P * F + 1)
    if k == 32:
        return (P * F * F + 1,)
    return (P * F + 1,)


@pytest.mark.parametrize("k", [16, 32, 4])
def test_panel_and_tree_edges(hp, gpu_backend_i32, k):
    sizes = _edge_sizes(hp, k)
    if k == 32:
        assert len(qc.host().tree_levels(sizes[0], k)) == 4          # the leaves and three levels of nodes above them
    for n in sizes:
        X = qc.make(n, k, 1e12, 1)
        _check(hp, gpu_backend_i32, X, key=("edge", n, k), label="edges")


# ---- 2. width edges: every register tile, its first width and its last -------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32])
def test_width_edges(hp, gpu_backend_i32, k):
    P, F = _consts(hp, k)
    n = P * F + 1
    X = qc.make(n, k, 1e6, 2)
    _check(hp, gpu_backend_i32, X, key=("width", n, k), label="widths")


# ---- 3. R against numpy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(65537, 32), (4097, 16)])
def test_r_matches_numpy(hp, gpu_backend_i32, n, k):
    X = qc.make(n, k, 1e3, 3)
    Rn = _numpy_qr(("rnp", n, k), X)
    R = hp.qr(hp.HPCMatrix.from_global(X, gpu_backend_i32), mode="r")
    qc.check_r_shape(R, k)
    rel = np.linalg.norm(R - Rn) / np.linalg.norm(Rn)
    print(f"n={n} k={k}: ||R - R_np||_F / ||R_np||_F = {rel:.1e}")
    assert rel <= 1e-10


# ---- 4. rank deficiency ------------------------------------------------------------------------------------------------------------
def test_rank_deficient_and_zero(hp, gpu_backend_i32):
    X = qc.rank_deficient()
    _, R = _check(hp, gpu_backend_i32, X, key=("rankdef",), label="rank deficient")
    assert R[6, 6] == 0.0
    Z = np.zeros((300, 5))
    Q, R = hp.qr(hp.HPCMatrix.from_global(Z, gpu_backend_i32))
    assert np.all(R == 0.0) and R.shape == (5, 5)
    assert qc.orth(Q.gather()) <= qc.limit(5)


# ---- 5. layouts ----------------------------------------------------------------------------------------------------------------------
def test_layouts_give_the_same_bits(hp, gpu_backend_i32):
    import torch
    P, _ = _consts(hp, 16)
    n, k, part = 2 * P + 3, 16, np.array([0, 2 * P + 3], dtype=np.int64)
    X = qc.make(n, k, 1e6, 5)
    Q0, R0 = hp.qr(hp.HPCMatrix.from_global(X, gpu_backend_i32))
    q0 = Q0.gather()
    assert qc.orth(q0) <= qc.limit(k)

    def block(local):
        return hp.HPCMatrix(part, np.array([0, k], dtype=np.int64), local, gpu_backend_i32)

    wide = torch.full((n, 48), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 8:24] = torch.from_numpy(X).cuda()
    colmajor = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
    odd = torch.full((n, 17), float("nan"), dtype=torch.float64, device="cuda")
    odd[:, :16] = torch.from_numpy(X).cuda()
    for label, local in (("columns 8:24 of pitch 48", wide[:, 8:24]), ("column-major", colmajor), ("pitch 17", odd[:, :16])):
        assert local.shape == (n, k) and not local.is_contiguous(), label
        before = local.clone()
        Q, R = hp.qr(block(local))
        assert np.array_equal(_bits(R), _bits(R0)), label
        assert np.array_equal(_bits(Q.gather()), _bits(q0)), label
        assert torch.equal(local.contiguous().view(torch.int64), before.contiguous().view(torch.int64)), label    # X is not modified
    assert torch.isnan(wide[:, :8]).all() and torch.isnan(wide[:, 24:]).all() and torch.isnan(odd[:, 16]).all()


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------------
def test_determinism_mode_r_and_x_unchanged(hp, gpu_backend_i32):
    P, F = _consts(hp, 16)
    n, k = P * F + 1, 16
    X = qc.make(n, k, 1e12, 6)
    Xh = hp.HPCMatrix.from_global(X, gpu_backend_i32)
    Q1, R1 = hp.qr(Xh)
    Q2, R2 = hp.qr(Xh)
    assert np.array_equal(_bits(R1), _bits(R2)) and np.array_equal(_bits(Q1.gather()), _bits(Q2.gather()))
    assert Q1.A.data_ptr() != Q2.A.data_ptr() != Xh.A.data_ptr()
    Rr = hp.qr(Xh, mode="r")
    assert np.array_equal(_bits(Rr), _bits(R1))
    assert np.array_equal(_bits(Xh.gather()), _bits(X))


# ---- 7. non-finite input ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_input_propagates_and_leaves_no_state(hp, gpu_backend_i32, bad):
    P, F = _consts(hp, 16)
    n, k = P * F + 1, 16
    X = qc.make(n, k, 1e12, 1)
    Xb = X.copy()
    Xb[P + 1, 3] = bad
    Q, R = hp.qr(hp.HPCMatrix.from_global(Xb, gpu_backend_i32))
    assert np.isnan(R).any() and Q.gather().shape == (n, k)
    _check(hp, gpu_backend_i32, X, key=("edge", n, k), label="after non-finite")


# ---- 8. lstsq quality ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,kappa", [(4097, 16, 1e6), (65537, 31, 1e3), (300, 7, 1e10), (257, 1, 1.0)])
def test_lstsq_quality(hp, gpu_backend_i32, n, k, kappa):
    X = qc.make(n, k, kappa, 7)
    b = np.random.default_rng(9).standard_normal(n)
    cn = np.linalg.lstsq(X, b, rcond=None)[0]
    assert qc.neq(X, b, cn) <= qc.limit(k)
    Xh = hp.HPCMatrix.from_global(X, gpu_backend_i32)
    c, rnorm = hp.lstsq(Xh, hp.HPCVector.from_global(b, gpu_backend_i32))
    assert isinstance(c, hp.HPCVector) and np.array_equal(c.partition, Xh.col_partition) and isinstance(rnorm, float)
    cg = c.gather()
    want = np.linalg.norm(b - X @ cn)
    print(f"n={n} k={k} kappa={kappa:g}: neq {qc.neq(X, b, cg) / qc.EPS:.2f} eps (limit {16 * k}), rnorm off {abs(rnorm - want) / want:.1e}")
    assert qc.neq(X, b, cg) <= qc.limit(k)
    assert abs(rnorm - want) <= 1e-6 * want
    assert np.array_equal(_bits(Xh.gather()), _bits(X))


# ---- 9. consistent systems -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", [1e3, 1e6])
def test_lstsq_consistent_system(hp, gpu_backend_i32, kappa):
    n, k = 4097, 16
    X = qc.make(n, k, kappa, 8)
    c0 = np.random.default_rng(10).standard_normal(k)
    b = X @ c0
    c, rnorm = hp.lstsq(hp.HPCMatrix.from_global(X, gpu_backend_i32), hp.HPCVector.from_global(b, gpu_backend_i32))
    err = np.linalg.norm(c.gather() - c0) / np.linalg.norm(c0)
    print(f"kappa={kappa:g}: ||c - c0|| / ||c0|| = {err:.1e} (limit {10 * kappa * qc.EPS:.1e}), rnorm / ||b|| = {rnorm / np.linalg.norm(b):.1e}")
    assert err <= 10 * kappa * qc.EPS
    assert rnorm <= 64 * qc.EPS * np.linalg.norm(b)


# ---- 10. several right-hand sides ---------------------------------------------------------------------------------------------------
def test_lstsq_several_right_hand_sides(hp, gpu_backend_i32):
    n, k, m = 2049, 29, 3
    X = qc.make(n, k, 1e3, 12)
    Bm = np.random.default_rng(13).standard_normal((n, m))
    Xh = hp.HPCMatrix.from_global(X, gpu_backend_i32)
    C, rnorms = hp.lstsq(Xh, hp.HPCMatrix.from_global(Bm, gpu_backend_i32))
    assert isinstance(C, hp.HPCMatrix) and np.array_equal(C.row_partition, Xh.col_partition)
    Cg = C.gather()
    assert Cg.shape == (k, m) and rnorms.shape == (m,)
    for j in range(m):
        c, rn = hp.lstsq(Xh, hp.HPCVector.from_global(Bm[:, j], gpu_backend_i32))
        assert np.linalg.norm(Cg[:, j] - c.gather()) <= 1e-12 * np.linalg.norm(c.gather()), j
        assert abs(rnorms[j] - rn) <= 1e-12 * rn, j


# ---- 11. argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors(hp, gpu_backend_i32):
    B = gpu_backend_i32
    rng = np.random.default_rng(0)
    X = hp.HPCMatrix.from_global(rng.standard_normal((100, 4)), B)
    b = hp.HPCVector.from_global(rng.standard_normal(100), B)
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    X32 = hp.HPCMatrix.from_global(rng.standard_normal((100, 4)).astype(np.float32), b32)
    with pytest.raises(TypeError):
        hp.qr(X32)
    with pytest.raises(TypeError):
        hp.lstsq(X32, hp.HPCVector.from_global(np.ones(100, dtype=np.float32), b32))
    with pytest.raises(ValueError, match="1..32"):
        hp.qr(hp.HPCMatrix.from_global(rng.standard_normal((100, 33)), B))
    with pytest.raises(ValueError, match="1..32"):
        hp.qr(hp.HPCMatrix.from_global(np.zeros((100, 0)), B))
    with pytest.raises(ValueError, match="k \\+ m <= 32"):                               # k + m = 33
        hp.lstsq(hp.HPCMatrix.from_global(rng.standard_normal((100, 30)), B),
                 hp.HPCMatrix.from_global(rng.standard_normal((100, 3)), B))
    with pytest.raises(ValueError, match="k \\+ m <= 32"):
        hp.lstsq(hp.HPCMatrix.from_global(rng.standard_normal((100, 32)), B), b)
    with pytest.raises(ValueError, match="n >= k"):
        hp.qr(hp.HPCMatrix.from_global(rng.standard_normal((7, 8)), B))
    with pytest.raises(ValueError, match="mode"):
        hp.qr(X, mode="complete")
    with pytest.raises(ValueError, match="Incompatible backends"):                      # mixed backends: b lives on the host
        hp.lstsq(X, hp.to_backend(b, hp.cpu_version(B)))
    with pytest.raises(TypeError):                                                      # a Float32 right-hand side
        hp.lstsq(X, hp.HPCVector.from_global(np.ones(100, dtype=np.float32), b32))
    with pytest.raises(ValueError, match="dimension mismatch"):
        hp.lstsq(X, hp.HPCVector.from_global(np.ones(99), B))


# ---- 12. lstsq on a rank-deficient matrix ------------------------------------------------------------------------------------------
def test_lstsq_rank_deficient_raises(hp, gpu_backend_i32):
    X = hp.HPCMatrix.from_global(qc.rank_deficient(), gpu_backend_i32)
    with pytest.raises(ValueError, match="lstsq: X is rank deficient"):
        hp.lstsq(X, hp.HPCVector.from_global(np.ones(1000), gpu_backend_i32))


# ---- ranks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_qr_across_ranks(nranks):
    """The ranks share the one GPU (as tests/test_gpu_lobpcg.py::test_lobpcg_across_ranks); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
