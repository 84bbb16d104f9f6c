"""Inputs, limits and a numpy restatement of the tall-skinny Householder QR (hp.qr, hp.lstsq).  No device.

Inputs: ``X = U diag(s) V'`` with ``U`` (n x k) and ``V`` (k x k) the orthonormal factors of seeded ``default_rng`` normal
matrices and ``s = logspace(0, -log10(kappa), k)``.

Limits (``eps = 2^-52``), the Householder bound -- linear in k, independent of kappa:
    orth = max |Q'Q - I|             <= 16 k eps
    back = ||Q R - X||_2 / ||X||_2   <= 16 k eps
    neq  = ||X'(b - X c)||_2 / (||X||_2 (||b||_2 + ||X||_2 ||c||_2))  <= 16 k eps       (least squares)
A numpy TSQR with 64-row leaves and a binary tree measured 3-7 eps for orth and <= 5 eps for back at n <= 65537, k in 1..32,
kappa in 1..1e12; numpy.linalg.qr gives 3-6 eps.  The methods the limits exclude: at kappa = 1e12 ``X inv(R)`` reaches 3.5e-5
and CholQR fails; eight decades or more above the limit.  Every test that uses a limit also asserts numpy.linalg.qr (or
lstsq) of the same input within it, so a change of the generator cannot hide a failure.

The restatement (:func:`tsqr`) is the tree of csrc/qr.hip in numpy: panels of P rows, nodes of F(k) triangles, the rank stack,
``tau = 0`` for a column whose sum of squares below the diagonal is exactly zero, ``D = sign(diag R)`` folded into Q, Q by
applying the reflectors in reverse to ``[top; 0]``.  Its sums are numpy's, not the kernel's: it agrees with the device to
rounding, and it pins the generator and the limits where a CPU can run them.
"""
import sys

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def make(n, k, kappa, seed):
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, k)))
    V, _ = np.linalg.qr(rng.standard_normal((k, k)))
    s = np.logspace(0, -np.log10(kappa), k)
    return (U * s) @ V.T


def rank_deficient(seed=11):
    """Test 4's matrix: n = 1000, k = 8, kappa = 10, column 5 a copy of column 2, column 6 zero."""
    X = make(1000, 8, 10.0, seed)
    X[:, 5] = X[:, 2]
    X[:, 6] = 0.0
    return X


def limit(k):
    return 16 * k * EPS


def orth(Q):
    return float(np.abs(Q.T @ Q - np.eye(Q.shape[1])).max())


def back(Q, R, X):
    nx = np.linalg.norm(X, 2)
    return float(np.linalg.norm(Q @ R - X, 2) / nx) if nx else float(np.linalg.norm(Q @ R - X, 2))


def neq(X, b, c):
    nx = np.linalg.norm(X, 2)
    return float(np.linalg.norm(X.T @ (b - X @ c)) / (nx * (np.linalg.norm(b) + nx * np.linalg.norm(c))))


def sign_normalised(R):
    """numpy.linalg.qr's R with a non-negative diagonal."""
    d = np.where(np.diag(R) < 0, -1.0, 1.0)
    return d[:, None] * R


def check_r_shape(R, k):
    """R is (k, k), exact zeros below the diagonal, a non-negative diagonal."""
    assert R.shape == (k, k) and R.dtype == np.float64
    assert np.all(R[np.tril_indices(k, -1)] == 0.0), "entries below the diagonal"
    assert np.all(np.diag(R) >= 0.0), np.diag(R)


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------
def panel_factor(A):
    """Householder QR of one zero-padded panel, unblocked (dlarfg / dlarf).  Returns (V with R on and above the diagonal, tau)."""
    A = np.array(A, dtype=np.float64)
    rows, k = A.shape
    tau = np.zeros(k)
    for j in range(min(k, rows)):
        sigma = float(np.sum(A[j + 1:, j] ** 2))
        if sigma == 0.0:
            continue                                  # tau = 0: the identity; a_jj stays
        ajj = A[j, j]
        alpha = -np.copysign(np.sqrt(ajj * ajj + sigma), ajj)
        tau[j] = (alpha - ajj) / alpha
        v = np.concatenate([[1.0], A[j + 1:, j] / (ajj - alpha)])
        w = v @ A[j:, j + 1:]
        A[j:, j + 1:] -= np.outer(v, tau[j] * w)
        A[j, j] = alpha
        A[j + 1:, j] = v[1:]
    return A, tau


def panel_apply(V, tau, top):
    """H_1 .. H_k [top; 0] for the panel's stored reflectors."""
    rows, k = V.shape
    Qp = np.zeros((max(rows, k), k))
    Qp[:k] = top
    Vp = np.zeros((max(rows, k), k))
    Vp[:rows] = V
    for j in range(k - 1, -1, -1):
        if tau[j] == 0.0:
            continue
        v = np.concatenate([[1.0], Vp[j + 1:, j]])
        w = v @ Qp[j:]
        Qp[j:] -= np.outer(v, tau[j] * w)
    return Qp[:rows]


def _tree_factor(M, k, P, F):
    """Bottom up over the rows of M.  Returns (levels, root): a level is (matrix of reflectors, rows per panel, taus)."""
    levels, cur, rpp = [], np.array(M, dtype=np.float64), P
    while True:
        rows = cur.shape[0]
        npan = -(-rows // rpp)
        V, taus, tris = np.zeros_like(cur), [], np.zeros((npan * k, k))
        for p in range(npan):
            blk = cur[p * rpp:(p + 1) * rpp]
            padded = np.zeros((max(blk.shape[0], k), k))
            padded[:blk.shape[0]] = blk
            Vp, tau = panel_factor(padded)
            V[p * rpp:p * rpp + blk.shape[0]] = Vp[:blk.shape[0]]
            tris[p * k:(p + 1) * k] = np.triu(Vp[:k])
            taus.append(tau)
        levels.append((V, rpp, taus))
        if npan == 1:
            return levels, tris
        cur, rpp = tris, F * k


def _tree_apply(levels, top, k):
    tops = top
    for V, rpp, taus in reversed(levels):
        out = np.zeros_like(V)
        for p, tau in enumerate(taus):
            blk = V[p * rpp:(p + 1) * rpp]
            out[p * rpp:p * rpp + blk.shape[0]] = panel_apply(blk, tau, tops[p * k:(p + 1) * k])
        tops = out
    return tops


def tsqr(X, P=256, F=None, partition=None):
    """(Q, R) of X by the tree of csrc/qr.hip; ``partition``: row offsets of the ranks (None: one rank)."""
    X = np.asarray(X, dtype=np.float64)
    n, k = X.shape
    if F is None:
        F = P // (4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else 32)
    partition = [0, n] if partition is None else list(partition)
    nranks = len(partition) - 1
    trees, roots = [], []
    for r in range(nranks):
        rows = X[partition[r]:partition[r + 1]]
        if rows.shape[0] == 0:
            trees.append(None)
            roots.append(np.zeros((k, k)))
            continue
        levels, root = _tree_factor(rows, k, P, F)
        trees.append(levels)
        roots.append(root)
    if nranks > 1:
        stack_levels, root = _tree_factor(np.vstack(roots), k, P, F)
    else:
        root = roots[0]
    d = np.where(np.diag(root) < 0, -1.0, 1.0)
    R = np.triu(d[:, None] * root)
    tops = np.diag(d)
    if nranks > 1:
        tops = _tree_apply(stack_levels, tops, k)
    Q = [(_tree_apply(trees[r], tops[r * k:(r + 1) * k], k) if trees[r] is not None else np.zeros((0, k)))
         for r in range(nranks)]
    return np.vstack(Q), R


def host():
    """The package's host part (linearalgebrampi.jl_amd/qr.py): importable without a device."""
    import hpcla_amd as hp
    return sys.modules[hp.qr.__module__]


def lstsq_augmented(X, B, **kw):
    """(C, rnorms) through the R of the augmented block, as hp.lstsq does."""
    B = B.reshape(len(B), -1)
    _, R = tsqr(np.hstack([X, B]), **kw)
    return host().solve_augmented(R, X.shape[1])
