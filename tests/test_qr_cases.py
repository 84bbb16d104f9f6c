"""CPU tests of hp.qr / hp.lstsq: the argument rules and the tree shape (plain Python in linearalgebrampi.jl_amd/qr.py, no
device), and the numpy restatement of the tree (tests/_qr_cases.py) against the limits the GPU tests use -- this pins the
generator and the limits where a CPU can run them.  Each limit is also asserted for numpy.linalg.qr / lstsq on the same input."""
import numpy as np
import pytest

from tests import _qr_cases as qc


def test_argument_rules_need_no_device():
    mod = qc.host()
    assert mod.check_arguments(100, 1) == 1 and mod.check_arguments(32, 32) == 32 and mod.check_arguments(40, 16, "r") == 16
    assert mod.check_arguments(100, 29, "r", 3, what="lstsq") == 29
    for n, k in ((100, 0), (100, 33), (100, -1)):
        with pytest.raises(ValueError, match="1..32"):
            mod.check_arguments(n, k)
    with pytest.raises(ValueError, match="k \\+ m <= 32"):
        mod.check_arguments(100, 30, "r", 3, what="lstsq")            # k + m = 33
    with pytest.raises(ValueError, match="n >= k"):
        mod.check_arguments(15, 16)
    with pytest.raises(ValueError, match="mode"):
        mod.check_arguments(100, 4, "complete")
    # the rank test of lstsq reads the diagonal of R: zero counts as deficient
    R = np.triu(np.ones((4, 4)))
    C, rn = mod.solve_augmented(R, 3)
    assert C.shape == (3, 1) and np.allclose(R[:3, :3] @ C[:, 0], R[:3, 3]) and rn[0] == 1.0
    for bad in (0.0, 3 * qc.EPS):
        Rb = R.copy()
        Rb[1, 1] = bad
        with pytest.raises(ValueError, match="rank deficient"):
            mod.solve_augmented(Rb, 3)
    Rn = R.copy()
    Rn[0, 2] = np.nan                                                  # non-finite: no exception, the NaN propagates
    assert np.isnan(mod.solve_augmented(Rn, 3)[0]).any()


def test_tree_shape():
    mod = qc.host()
    P = mod.PANEL_ROWS
    assert P == 256 and [mod.fan(k) for k in (1, 4, 5, 8, 9, 16, 17, 32)] == [64, 64, 32, 32, 16, 16, 8, 8]
    for k in (1, 4, 8, 16, 17, 32):
        F = mod.fan(k)
        want = {0: [], 1: [1], P: [1], P + 1: [2, 1], P * F: [F, 1], P * F + 1: [F + 1, 2, 1], P * F * F + 1: [F * F + 1, F + 1, 2, 1]}
        for n_loc, levels in want.items():
            assert mod.tree_levels(n_loc, k) == levels, (k, n_loc)
            assert mod.tree_shape(n_loc, k, 1) == (levels, 0, [])
    for nranks in range(2, 9):
        for k in (1, 16, 32):
            local, rows, stack = mod.tree_shape(1000, k, nranks)
            assert rows == nranks * k and local == [4, 1]
            assert stack == ([1] if rows <= P else [-(-rows // P), 1])      # 8 ranks x 32: 256 rows, still one panel
    assert mod.tree_shape(0, 16, 3) == ([], 48, [1])
    with pytest.raises(ValueError):
        mod.fan(33)


def _np_within(X):
    Qn, Rn = np.linalg.qr(X)
    k = X.shape[1]
    assert qc.orth(Qn) <= qc.limit(k) and qc.back(Qn, Rn, X) <= qc.limit(k)
    return qc.sign_normalised(Rn)


@pytest.mark.parametrize("n,k,kappa", [(16, 16, 1e12), (17, 16, 1e12), (257, 16, 1e12), (515, 16, 1e12), (4097, 16, 1e12),
                                         (16385, 32, 1e12), (16385, 4, 1e12), (8193, 5, 1e6), (2049, 31, 1e6), (300, 1, 1e6)])
def test_restatement_meets_the_qr_limits(n, k, kappa):
    X = qc.make(n, k, kappa, 1)
    Rn = _np_within(X)
    Q, R = qc.tsqr(X)
    o, b = qc.orth(Q), qc.back(Q, R, X)
    print(f"n={n} k={k} kappa={kappa:g}: orth {o / qc.EPS:.1f} eps, back {b / qc.EPS:.1f} eps, limit {16 * k} eps")
    assert o <= qc.limit(k) and b <= qc.limit(k)
    qc.check_r_shape(R, k)
    if kappa <= 1e6:
        assert np.linalg.norm(R - Rn) <= 1e-8 * np.linalg.norm(Rn)


def test_restatement_rank_deficient_zero_and_ranks():
    X = qc.rank_deficient()
    _np_within(X)
    Q, R = qc.tsqr(X)
    assert qc.orth(Q) <= qc.limit(8) and qc.back(Q, R, X) <= qc.limit(8) and R[6, 6] == 0.0
    Q, R = qc.tsqr(np.zeros((300, 5)))
    assert np.all(R == 0.0) and qc.orth(Q) <= qc.limit(5)
    k, big = 16, 256 * 16 + 1
    for part in ([0, big, big + 5], [0, big, big + 5, big + 5], [0, 5, 5, 5 + big]):
        X = qc.make(part[-1], k, 1e12, 3)
        _np_within(X)
        Q, R = qc.tsqr(X, partition=part)
        assert qc.orth(Q) <= qc.limit(k) and qc.back(Q, R, X) <= qc.limit(k), part
        qc.check_r_shape(R, k)


@pytest.mark.parametrize("n,k,kappa", [(4097, 16, 1e6), (65537, 31, 1e3), (300, 7, 1e10), (257, 1, 1.0)])
def test_restatement_meets_the_lstsq_limits(n, k, kappa):
    X = qc.make(n, k, kappa, 7)
    b = np.random.default_rng(9).standard_normal(n)
    cn = np.linalg.lstsq(X, b, rcond=None)[0]
    assert qc.neq(X, b, cn) <= qc.limit(k)
    C, rn = qc.lstsq_augmented(X, b)
    want = np.linalg.norm(b - X @ cn)
    print(f"n={n} k={k}: neq {qc.neq(X, b, C[:, 0]) / qc.EPS:.2f} eps, rnorm off by {abs(rn[0] - want) / want:.1e}")
    assert qc.neq(X, b, C[:, 0]) <= qc.limit(k)
    assert abs(rn[0] - want) <= 1e-6 * want
    with pytest.raises(ValueError, match="rank deficient"):
        qc.lstsq_augmented(qc.rank_deficient(), np.ones(1000))
