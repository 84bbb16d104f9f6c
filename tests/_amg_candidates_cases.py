"""Shared cases of ``hp.amg(A, B=...)``, the near-nullspace candidates of the tentative prolongator, and a numpy / scipy
restatement of what they change, on top of tests/_amg_cases.py (``ac``) and tests/_amg_nonsym_cases.py (``nc``), written from
the method's description, not from the kernels.

With ``B`` (n x k, 1 <= k <= 8) a level differs from ``ac``'s / ``nc``'s in these steps:
  unknowns    k per aggregate, the coarse unknown k agg + c; the aggregation runs on the rows of A as before
  stall       k n_aggregates >= 0.8 n, decided after the fit (a level that stalls has had its aggregates checked too)
  fit         per aggregate, its members in ascending row order, B[members, :] = Q R (m x k times k x k).  Column j:
              v = B[members, j]; n0 = sqrt(sum v_m^2); twice: h_c = sum_m q_c[m] v[m] for every c < j, all taken before any
              update, then v = v - h_c q_c for c ascending; R_cj = the first pass's h_c plus the second's; nr = sqrt(sum v_m^2);
              R_jj = nr, q_j = v / nr.  Every sum over the members is sequential in ascending member order from +0.0
              (``seqsum``: a cumulative sum, not ``@``), products and sums separately rounded.  !(nr > 1e-10 n0) drops the
              column: q_j = 0, row j of R = 0, and the column takes no part in later ones (h = +0.0).  Q fills the rows of the
              dense n x k ``Tv``, R the rows k a .. k a + k - 1 of the next level's candidates, +0.0 below the diagonal.
              In a hierarchy a dropped column is an error.
  T           k stored entries per row: columns k agg(i) .. k agg(i) + k - 1, values Tv[i, :], exact zeros stored
  P           p_e = (col // k == agg(i) ? Tv[i, col - k agg(i)] : 0) - s_i (A T)_e on the pattern of A T
  R           Pt (symmetric); else r_cj = (agg(j) == c // k ? Tv[j, c - k agg(j)] : 0) - (Tt A)_cj s_j on the pattern of Tt A
Everything else (weights, strength, independent set, join, Galerkin products, last level, cycle) is ``ac``'s / ``nc``'s.

Cases: ``scaled(nx, ny)``: D G D with G the 5-point grid and d = 10^U(-1, 1), near-nullspace 1 ./ d; ``elasticity(nx, ny)``: Q1
plane-strain elasticity on unit squares, left edge clamped, near-nullspace the three rigid-body modes; ``scaled_nonsym``: the
convection-diffusion stencil of ``nc`` scaled the same way; the 7-point 16^3 grid with [1, x, y]; the star with the constant.
"""
import numpy as np
import scipy.sparse as sp

from tests import _amg_cases as ac
from tests import _amg_nonsym_cases as nc

SEED_SCALING = 20261021
DROP = 1e-10
MAX_K = 8
SMALL = 8                      # coarse_size of the hierarchy tests: every case aggregates at least once
COUNT_FACTOR = 0.5             # with the right candidates CG takes at most this share of the default hierarchy's count
SOLVES = {"scaled64x64": "cg", "elas32x32": "cg", "cdscaled33x31": "gmres"}


# ---- matrices -------------------------------------------------------------------------------------------------------------------
def scaling(n):
    return 10.0 ** np.random.default_rng(SEED_SCALING).uniform(-1.0, 1.0, n)


def _scale(G, d):
    A = (sp.diags(d) @ G @ sp.diags(d)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def scaled(nx, ny):
    """(D G D, d): G = ac.grid2d(nx, ny)."""
    d = scaling(nx * ny)
    return _scale(ac.grid2d(nx, ny), d), d


def scaled_nonsym(nx, ny):
    d = scaling(nx * ny)
    return _scale(nc.convection_diffusion(nx, ny), d), d


def _q1_plane_strain(E=1.0, nu=0.3):
    """The 8 x 8 stiffness of the unit square, nodes (0,0), (1,0), (1,1), (0,1), unknowns 2 node + component, 2 x 2 Gauss."""
    D = E / ((1 + nu) * (1 - 2 * nu)) * np.array([[1 - nu, nu, 0.0], [nu, 1 - nu, 0.0], [0.0, 0.0, (1 - 2 * nu) / 2]])
    g = 0.5 / np.sqrt(3.0)
    K = np.zeros((8, 8))
    for x in (0.5 - g, 0.5 + g):
        for y in (0.5 - g, 0.5 + g):
            dx = np.array([-(1 - y), 1 - y, y, -y])
            dy = np.array([-(1 - x), -x, x, 1 - x])
            Bm = np.zeros((3, 8))
            Bm[0, 0::2] = dx
            Bm[1, 1::2] = dy
            Bm[2, 0::2] = dy
            Bm[2, 1::2] = dx
            K += 0.25 * Bm.T @ D @ Bm
    return K


def elasticity(nx, ny):
    """(A, modes): nx x ny unit Q1 elements under plane strain (E = 1, nu = 0.3), unknowns 2 node + component with
    node = j (nx + 1) + i, the nodes with i = 0 eliminated; modes: (1, 0), (0, 1), (-y, x) on the free unknowns."""
    K = _q1_plane_strain()
    nodes = (nx + 1) * (ny + 1)
    rows, cols, vals = [], [], []
    for j in range(ny):
        for i in range(nx):
            nd = [j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i]
            dof = np.array([2 * n + c for n in nd for c in (0, 1)])
            rows.append(np.repeat(dof, 8))
            cols.append(np.tile(dof, 8))
            vals.append(K.ravel())
    full = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * nodes, 2 * nodes))
    node = np.arange(nodes)
    x, y = (node % (nx + 1)).astype(np.float64), (node // (nx + 1)).astype(np.float64)
    free = np.flatnonzero(np.repeat(node % (nx + 1) != 0, 2))
    A = full[free][:, free].tocsr()
    A.sum_duplicates()
    A.sort_indices()
    modes = np.zeros((2 * nodes, 3))
    modes[0::2, 0] = 1.0
    modes[1::2, 1] = 1.0
    modes[0::2, 2] = -y
    modes[1::2, 2] = x
    return A, np.ascontiguousarray(modes[free])


def grid_xy(n=16):
    """[1, x, y] on the n^3 grid of ``ac.grid3d`` (x fastest)."""
    g = np.arange(n ** 3)
    return np.ascontiguousarray(np.stack([np.ones(n ** 3), (g % n).astype(np.float64), ((g // n) % n).astype(np.float64)], axis=1))


def path_candidates(n=257):
    """[1, x, x^2] on the path: independent on three rows, not on the two of the path's last aggregate."""
    x = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.stack([np.ones(n), x, x * x], axis=1))


def hierarchy_cases():
    """name -> (A, B, symmetric)."""
    out = {}
    for nx, ny in ((33, 31), (16, 16)):
        A, d = scaled(nx, ny)
        out[f"scaled{nx}x{ny}"] = (A, (1.0 / d).reshape(-1, 1), True)
    A, modes = elasticity(16, 16)
    out["elas16x16"] = (A, modes, True)
    out["elas16x16-translations"] = (A, np.ascontiguousarray(modes[:, :2]), True)
    out["grid16x16x16-1xy"] = (ac.grid3d(16), grid_xy(16), True)
    out["star300"] = (ac.star(300), np.ones((301, 1)), True)
    C = nc.convection_diffusion(33, 31)
    out["cd33x31"] = (C, np.ones((C.shape[0], 1)), False)
    A, d = scaled_nonsym(33, 31)
    out["cdscaled33x31"] = (A, (1.0 / d).reshape(-1, 1), False)
    for A, _, _ in out.values():
        A.sum_duplicates()
        A.sort_indices()
    return out


def solve_cases():
    """name -> (A, B, symmetric): the systems of ``SOLVES``."""
    A, d = scaled(64, 64)
    E, modes = elasticity(32, 32)
    C, dc = scaled_nonsym(33, 31)
    return {"scaled64x64": (A, (1.0 / d).reshape(-1, 1), True), "elas32x32": (E, modes, True),
            "cdscaled33x31": (C, (1.0 / dc).reshape(-1, 1), False)}


# ---- the fit --------------------------------------------------------------------------------------------------------------------
def seqsum(x):
    """The sum of x taken one term at a time in order, from +0.0."""
    return float(np.cumsum(np.concatenate([[0.0], np.asarray(x, dtype=np.float64)]))[-1])


def fit_block(Bm):
    """(Q, R, dropped columns) of one aggregate's m x k block."""
    Bm = np.asarray(Bm, dtype=np.float64)
    m, k = Bm.shape
    Q, R, dropped = np.zeros((m, k)), np.zeros((k, k)), []
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):
            v = Bm[:, j].copy()
            n0 = np.sqrt(seqsum(v * v))
            live = [c for c in range(j) if c not in dropped]
            total = np.zeros(k)
            for _ in range(2):
                h = {c: seqsum(Q[:, c] * v) for c in live}
                for c in live:
                    v = v - h[c] * Q[:, c]
                    total[c] = total[c] + h[c]
            R[:j, j] = total[:j]
            nr = np.sqrt(seqsum(v * v))
            if not (nr > DROP * n0):
                dropped.append(j)
                R[j, :] = 0.0
                continue
            R[j, j] = nr
            Q[:, j] = v / nr
    for j in dropped:                                           # the whole row, the later columns' too
        R[j, :] = 0.0
    return Q, R, dropped


def members_of(agg, n_agg):
    """(pointer, members): the rows of every aggregate in ascending order."""
    agg = np.asarray(agg, dtype=np.int64)
    order = np.argsort(agg, kind="stable").astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=n_agg))]).astype(np.int64)
    return ptr, order


def fit(B, ptr, members):
    """(Tv, Bc, reports): Tv n x k, Bc (k n_agg) x k, reports the (aggregate, column) pairs that were dropped, ascending."""
    B = np.asarray(B, dtype=np.float64)
    n, k = B.shape
    n_agg = len(ptr) - 1
    Tv, Bc, reports = np.zeros((n, k)), np.zeros((n_agg * k, k)), []
    for a in range(n_agg):
        rows = members[ptr[a]:ptr[a + 1]]
        Q, R, dropped = fit_block(B[rows])
        Tv[rows] = Q
        Bc[k * a:k * a + k] = R
        reports += [(a, j) for j in dropped]
    return Tv, Bc, reports


def fit_word(reports):
    """The error word of the fit: -1, or 8 a + j of the smallest reporting aggregate and its first dropped column."""
    return min(8 * a + j for a, j in reports) if reports else -1


# ---- setup ----------------------------------------------------------------------------------------------------------------------
def tentative(agg, Tv, n_agg):
    n, k = Tv.shape
    cols = (k * agg[:, None] + np.arange(k)[None, :]).reshape(-1)
    return sp.csr_matrix((Tv.reshape(-1).copy(), cols, k * np.arange(n + 1)), shape=(n, k * n_agg))


def prolongator_values(AT, agg, Tv, s):
    """p_e on a pattern with the columns of A T."""
    k = Tv.shape[1]
    row = np.repeat(np.arange(AT.shape[0]), np.diff(AT.indptr))
    c = AT.indices.astype(np.int64) - k * agg[row]
    own = (c >= 0) & (c < k)
    return np.where(own, Tv[row, np.clip(c, 0, k - 1)], 0.0) - s[row] * AT.data


def restrictor_values(TA, agg, Tv, s, row_offset=0):
    """r_cj on a pattern with the rows of Tt A (coarse unknowns from ``row_offset``) and the level's rows as columns."""
    k = Tv.shape[1]
    c = row_offset + np.repeat(np.arange(TA.shape[0]), np.diff(TA.indptr))
    j = TA.indices.astype(np.int64)
    return np.where(agg[j] == c // k, Tv[j, c % k], 0.0) - TA.data * s[j]


def setup(A, B, theta=0.0, max_levels=12, coarse_size=128, coarse_sweeps=4, symmetric=True):
    """The hierarchy in one block: levels as ``ac.setup``'s with ``B`` (the level's candidates) and, where the level has a P,
    ``Tv``, ``T`` and ``Bc``; ``R`` and ``Pt`` both hold the restriction, so ``ac.cycle`` runs on them.  A dropped column raises
    ValueError."""
    A = A.tocsr()
    B = np.asarray(B, dtype=np.float64)
    B = B.reshape(-1, 1) if B.ndim == 1 else B
    k = B.shape[1]
    assert 1 <= k <= MAX_K and B.shape[0] == A.shape[0]
    levels = []
    while True:
        n = A.shape[0]
        partition = [0, n]
        s, w, rho = ac.weights(A)
        lvl = dict(A=A, s=s, w=w, rho=rho, n=n, partition=partition, B=B)
        levels.append(lvl)
        last = n <= coarse_size or len(levels) >= max_levels
        if not last:
            agg, counts, roots, rounds, graph = (ac if symmetric else nc).aggregate(A, partition, theta)
            lvl.update(agg=agg, counts=counts, roots=roots, rounds=rounds, graph=graph)
            n_agg = int(counts.sum())
            ptr, members = members_of(agg, n_agg)
            Tv, Bc, reports = fit(B, ptr, members)              # before the stall rule: every aggregation made is checked
            if reports:
                a, j = divmod(fit_word(reports), 8)
                raise ValueError(f"the aggregate of row {int(members[ptr[a]])} (level of {n} rows) has "
                                 f"{int(ptr[a + 1] - ptr[a])} members and cannot carry candidate column {j}")
            last = k * n_agg >= ac.STALL * n
        if last:
            if n <= coarse_size:
                D = A.toarray()
                lvl["inv"] = np.linalg.inv((D + D.T) / 2 if symmetric else D)
            else:
                lvl["sweeps"] = coarse_sweeps
            return levels
        T = tentative(agg, Tv, n_agg)
        AT = ac.structural_product(A, T)
        P = sp.csr_matrix((prolongator_values(AT, agg, Tv, s), AT.indices.copy(), AT.indptr.copy()), shape=AT.shape)
        if symmetric:
            R = P.T.tocsr()
            R.sort_indices()
        else:
            Tt = T.T.tocsr()
            Tt.sort_indices()
            TA = ac.structural_product(Tt, A)
            R = sp.csr_matrix((restrictor_values(TA, agg, Tv, s), TA.indices.copy(), TA.indptr.copy()), shape=TA.shape)
        lvl.update(P=P, Pt=R, R=R, Tv=Tv, T=T, Bc=Bc, ptr=ptr, members=members)
        A = ac.structural_product(R, ac.structural_product(A, P))
        B = Bc


def default_setup(A, symmetric=True, **kw):
    return ac.setup(A, **kw) if symmetric else nc.setup(A, **kw)


def solve(kind, A, b, levels, **kw):
    """(x, iterations, converged) of CG or GMRES(30) with the cycle of ``levels``, as ``ac.pcg_amg`` / ``nc.gmres_amg``."""
    if kind == "cg":
        x, its, status, _ = ac.pcg_amg(A, b, levels, **kw)
        return x, its, status == "converged"
    out = nc.gmres_amg(A, b, levels, **kw)
    return out[0], out[1], out[2] == "converged"


# ---- hand-made inputs of the fit entry alone -------------------------------------------------------------------------------------
def fit_sizes(k):
    return sorted({1, max(k - 1, 1), k, k + 1, 7, 8, 9, 64, 65, 301})


def fit_case(k, n_agg, seed, bad=(), short=True):
    """(B, ptr, members, n): ``n_agg`` aggregates whose sizes cycle through ``fit_sizes(k)`` from the large end (those of at
    least k members only unless ``short``), over rows dealt out by a permutation (members ascending within an aggregate; a few
    rows belong to none).  ``bad``: (aggregate, kind) pairs, kind in "repeat" (column k - 1 = column 0), "zero" (column 0 = 0),
    "nan" (one NaN in column k - 1)."""
    rng = np.random.default_rng(seed)
    sizes = [m for m in fit_sizes(k)[::-1] if short or m >= k]
    size = np.array([sizes[a % len(sizes)] for a in range(n_agg)], dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    n = int(ptr[-1]) + 5
    rows = rng.permutation(n)[:int(ptr[-1])]
    members = np.concatenate([np.sort(rows[ptr[a]:ptr[a + 1]]) for a in range(n_agg)]).astype(np.int64)
    B = rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-3, 3, size=(1, k))
    for a, kind in bad:
        r = members[ptr[a]:ptr[a + 1]]
        if kind == "repeat":
            B[r, k - 1] = B[r, 0]
        elif kind == "zero":
            B[r, 0] = 0.0
        elif kind == "nan":
            B[r[len(r) // 2], k - 1] = np.nan
    return np.ascontiguousarray(B), ptr, members, n


# ---- the argument rules ---------------------------------------------------------------------------------------------------------
GOOD_B = (np.float64, (10, 3), [0, 5, 10])                      # next to ac.GOOD_ARGUMENTS: (element type, shape, row partition)
BAD_B = [((np.float64, (10, 9), [0, 5, 10]), ValueError), ((np.float64, (10, 0), [0, 5, 10]), ValueError),
         ((np.float64, (12, 3), [0, 6, 12]), ValueError), ((np.float64, (10, 3), [0, 4, 10]), ValueError),
         ((np.float32, (10, 3), [0, 5, 10]), TypeError)]
