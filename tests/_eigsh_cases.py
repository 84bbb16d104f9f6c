"""Shared cases of the eigensolver (``hp.eigsh``) and a numpy restatement of its loop.

The restatement is plain arrays; it follows the device loop's gate order and rounding order literally (csrc/solvers.hip,
``eigsh_steps_impl``; the kernels in csrc/vecops.hip and csrc/eigsh.hip): the start is a division by ``sqrt(v0.v0)``, the running
subtractions of the two Gram-Schmidt passes run over the basis columns in ascending order, ``T[i, j] = h1[i] + h2[i]``,
``beta[j] = sqrt(nn)``, gates N and I are tested where the device tests them, the host's cycle end (the assembly of T, ``eigh``,
the selection, the estimates, the stop rules, the choice of p) is stated again here and not imported from the package, and the
restart forms each new column as ``acc = V_0 S[0, j];  acc = acc + V_i S[i, j]`` with i ascending (``rotate``).  It is an
independent statement of the algorithm, not of the device's summation order: ``dot`` can be swapped (``_bicgstab_cases.DOTS``:
four summation orders) to measure how far the order alone moves T, the eigenvalues and the step counts, which is where the
margins of tests/test_gpu_eigsh.py come from (tests/test_eigsh_cases.py re-measures and prints them).

Cases (v0 = numpy.random.default_rng(seed).uniform(-1, 1, n), seed 0 unless said)
  plain Poisson          the oracle's 5-point ``poisson2d_rows(nx, ny)`` at 24 x 20 (n = 480) and 33 x 31 (n = 1023: an odd
                         length, so the basis pitch is n + 1 and the kernels' scalar tails run).  NOT 16 x 16: a square grid has
                         ``lambda_ij = lambda_ji``, and single-vector Lanczos returns a multiple eigenvalue once.
  saddle                 ``_minres_cases.saddle`` on 24 x 20: 960 rows, half the eigenvalues negative.
  scaled Poisson         ``_pcg_cases.scaled_poisson`` at 33 x 31, ``"LA"`` only (its ``"SA"`` needs 1254 steps).
  exact                  diag(1..12) with v0 = e_3 (invariant after one step) and with the default start at ncv = 12 (one cycle).

Figures of this restatement, tol = 1e-10 (steps, cycles):
  plain 24 x 20, k 4, ncv 20    LA 148 (17), SA 156 (18)          eigenvalue error <= 1.7e-14 anorm and true residual <= 0.99 tol anorm over all cases
  plain 24 x 20, k 1, ncv 8     LA 184 (45)
  plain 33 x 31, k 6, ncv 32    LA 214 (15)
  saddle 24 x 20, k 4, ncv 20   236 - 284 over four seeds and the three ``which``
  scaled 33 x 31, k 4, ncv 24   LA 84 (7)
identical under all four summation orders; the first cycle's T and beta spread by <= 1.1e-15 of max|T| (2.9e-15 absolute on the
plain cases, max|T| = 4.3; 6.2e-15 on the saddle, 5.5; 2.6e-13 on the scaled case, 274), the eigenvalues by <= 1.3e-14 anorm.
"""
import math

import numpy as np

from tests import _bicgstab_cases as bc
from tests import _minres_cases as mc
from tests import _pcg_cases as pc

DOTS = bc.DOTS
TOL = 1e-10
T_RTOL = 1e-12             # first-cycle T and beta against the restatement, relative to max|T|: the project's margin
VAL_RTOL = 1e-12           # eigenvalues against numpy.linalg.eigvalsh of the dense matrix, relative to anorm
SPREAD = 1e-13             # bound on the CPU spread of T and of the eigenvalues over the four summation orders
RANK_CASE = ("plain", (24, 20), 4, 20)
LARGE_SIZE = pc.LARGE_SIZE  # 65 x 63, first cycle at ncv = 20: T_RTOL is 700 times the CPU spread of T and beta there (1.4e-15)


def plain_poisson(orc, nx, ny):
    """(rowptr, colidx, vals) of the oracle's 5-point matrix, global 0-based CSR (int64 indices)."""
    n = nx * ny
    rows = orc.poisson2d_rows(nx, ny, 0, n)
    return rows.rowptr.astype(np.int64), rows.colidx.astype(np.int64), rows.vals.copy()


def matrices(orc):
    """{name: (rowptr, colidx, vals)}: every matrix the convergence tests use."""
    return {("plain", (24, 20)): plain_poisson(orc, 24, 20), ("plain", (33, 31)): plain_poisson(orc, 33, 31),
            ("saddle", (24, 20)): mc.saddle(orc, 24, 20)[:3], ("scaled", (33, 31)): pc.scaled_poisson(orc, 33, 31)[:3]}


# (matrix, k, ncv, the ``which`` it runs)
CONVERGENCE = [(("plain", (24, 20)), 4, 20, ("LA", "SA", "LM")), (("plain", (24, 20)), 1, 8, ("LA", "SA", "LM")),
               (("plain", (33, 31)), 6, 32, ("LA", "SA", "LM")), (("saddle", (24, 20)), 4, 20, ("LA", "SA", "LM")),
               (("scaled", (33, 31)), 4, 24, ("LA",))]


def dense_eigenvalues(rowptr, colidx, vals):
    return np.linalg.eigvalsh(bc.dense_of(rowptr, colidx, vals))


def reference_values(ev, k, which):
    """The k wanted eigenvalues of the dense spectrum ``ev`` (ascending), ascending."""
    if which == "LA":
        return ev[-k:]
    if which == "SA":
        return ev[:k]
    return np.sort(ev[np.argsort(-np.abs(ev), kind="stable")[:k]])


def start_vector(n, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def rotate(V, S):
    """Rows of the result: acc = V_0 S[0, j];  acc = acc + V_i S[i, j], i ascending (V: columns as rows of a 2-D array)."""
    m, p = S.shape
    out = np.empty((p, V.shape[1]))
    for j in range(p):
        acc = V[0] * S[0, j]
        for i in range(1, m):
            acc = acc + V[i] * S[i, j]
        out[j] = acc
    return out


def order(theta, which):
    """Indices, the most wanted first; ties to the larger value, then to the lower index."""
    keys = {"LA": [(-t, i) for i, t in enumerate(theta)], "SA": [(t, i) for i, t in enumerate(theta)],
            "LM": [(-abs(t), -t, i) for i, t in enumerate(theta)]}[which]
    return np.array([key[-1] for key in sorted(keys)], dtype=np.int64)


def small_step(j, h1, h2, nn, T, beta):
    """The Lanczos small step of column j on T (T[i, j]) and beta, updated in place.  Returns "breakdown" (gate N, nothing
    stored), "invariant" (gate I, column stored) or "running"."""
    if nn != nn:
        return "breakdown"
    for i in range(j + 1):
        T[i, j] = h1[i] + h2[i]
    beta[j] = math.sqrt(nn)
    return "invariant" if nn == 0.0 else "running"


def cycle(A, V, T, beta, p, m, dot):
    """Columns p .. m-1 on V ((m + 1) x n rows), T and beta in place.  Returns (status, columns finished)."""
    for j in range(p, m):
        c = j + 1
        w = A(V[j])
        h1 = np.array([dot(V[i], w) for i in range(c)])
        for i in range(c):
            w = w - h1[i] * V[i]
        h2 = np.array([dot(V[i], w) for i in range(c)])
        for i in range(c):
            w = w - h2[i] * V[i]
        nn = dot(w, w)
        status = small_step(j, h1, h2, nn, T, beta)
        if status == "breakdown":
            return status, j
        if status == "invariant":
            return status, c
        V[c] = w / beta[j]
    return "running", m


def symmetric_T(T, theta_kept, p, c):
    out = np.zeros((c, c))
    for i in range(min(p, c)):
        out[i, i] = theta_kept[i]
    for j in range(p, c):
        out[:j + 1, j] = T[:j + 1, j]
    return np.triu(out) + np.triu(out, 1).T


def eigsh(rowptr, colidx, vals, k=6, which="LA", ncv=None, tol=TOL, maxiter=None, v0=None, seed=0, dot=bc._dot_np,
          first_T=None):
    """The solver's loop on the host.  Returns (vals, X (n x k), dict(status, converged, iterations, restarts, residual_norms,
    history, anorm)).  ``first_T``: a dict that receives the first cycle's T (m x m, upper triangle) and beta."""
    n = len(rowptr) - 1
    m = min(n, 64, max(2 * k + 1, 20)) if ncv is None else ncv
    maxiter = 10 * n if maxiter is None else maxiter
    A = lambda u: pc.matvec(rowptr, colidx, vals, u)
    v0 = start_vector(n, seed) if v0 is None else np.asarray(v0, dtype=np.float64)
    V = np.zeros((m + 1, n))
    V[0] = v0 / math.sqrt(dot(v0, v0))
    T, beta = np.zeros((m, m)), np.zeros(m)
    p, iterations, restarts, theta_kept, history = 0, 0, 0, np.zeros(0), []
    while True:
        T[:], beta[:] = 0.0, 0.0
        status, c = cycle(A, V, T, beta, p, m, dot)
        if first_T is not None and not first_T:
            first_T.update(T=T.copy(), beta=beta.copy())
        iterations += c - p
        if status == "breakdown" or c == 0:
            return np.full(k, np.nan), np.zeros((n, k)), dict(status="breakdown", converged=False, iterations=iterations,
                                                              restarts=restarts, residual_norms=np.full(k, np.nan),
                                                              history=history, anorm=math.nan)
        theta, S = np.linalg.eigh(symmetric_T(T, theta_kept, p, c))
        wanted = order(theta, which)[:k]
        wanted = np.array(sorted(wanted, key=lambda i: (theta[i], i)), dtype=np.int64)
        rho = np.abs(beta[c - 1] * S[c - 1, wanted])
        anorm = float(np.max(np.abs(theta)))
        history.append(float(rho.max()))
        if status == "invariant":
            done = ("invariant", c >= k)
        elif np.all(rho <= tol * anorm):
            done = ("converged", True)
        elif iterations >= maxiter:
            done = ("maxiter", False)
        else:
            p = k + (m - k) // 2
            keep = order(theta, which)[:p]
            theta_kept = theta[keep].copy()
            last = V[m].copy()
            V[:p] = rotate(V[:m], S[:, keep])
            V[p] = last
            restarts += 1
            continue
        X = rotate(V[:c], S[:, wanted]).T
        return theta[wanted].copy(), X, dict(status=done[0], converged=done[1], iterations=iterations, restarts=restarts,
                                             residual_norms=rho, history=history, anorm=anorm)
