"""Shared cases of the smoothed-aggregation multigrid preconditioner (``hp.amg``) and a numpy / scipy restatement of its setup,
its cycle and of ``hp.cg`` with ``M = hp.amg(A)``, written from the method's description, not from the kernels.

Everything works on one global scipy CSR matrix and a row ``partition`` (a list of boundaries): the rank-local form of the
method is the same arithmetic with the strength graph cut at the block boundaries, so aggregates never cross a block, while
the weights, ``A T``, ``P`` and ``Pt A P`` use whole rows.  One block is the serial method.

Level setup, on the current level's A:
  weight      rho = max_i sum_j |a_ij| / a_ii, w = 4 / (3 rho), s = w ./ diag(A)
  strength    (i, j) kept when j != i, j in i's block, a_ij != 0 and |a_ij| >= theta sqrt(a_ii a_jj)
  roots       a distance-2 maximal independent set: key_i = (h(g_i) << 31) | local row; rounds of two neighbour maxima over
              k (the key of an undecided row, 2^62 for a root, -1 for a row that is out); an undecided row whose second maximum
              is its own key becomes a root, one whose second maximum is a root's goes out
  join        a non-root takes the neighbouring root with the largest key; a row still free takes the aggregate of the
              aggregated neighbour with the largest key; ids by the scan of the root flags, block after block
  stall       n_c >= 0.8 n: the level is the last one
  P           T - diag(s) (A T) on the pattern of A T;  A_c = Pt (A P), patterns structural (a sum that cancels stays stored)
  last level  n <= coarse_size: the inverse of (A + A') / 2; else ``coarse_sweeps`` damped Jacobi sweeps from zero

Cases (``cases()``): 5-point grids 16x16, 32x32, 64x64 and 37x53, the 7-point grid 16^3, the anisotropic 40x40 grid (couplings
1 and 0.01), a diagonal matrix, n = 1 and n = 2, path graphs of 255, 256 and 257 rows, a star whose hub has 300 neighbours, and
a seeded random symmetric diagonally dominant matrix of 600 rows.

For the tests that call the kernels' C entries on their own (tests/test_gpu_precond_kernels.py): ``split_block`` gives one block
of a partition in the rank-local split form the entries read, ghosts included; ``weights_stored_order`` the weights with the row
sum in the order the method defines; ``mis2_states`` the independent set round by round on a block's own graph;
``compressed_columns`` a column space that is not in ascending order; ``chain_levels`` / ``chain_coverage`` the levels those
tests walk and the edges they hold.
"""
import math

import numpy as np
import scipy.sparse as sp

BLOCKS = [1, 2, 3, 8]
ROOT = 1 << 62
MASK31 = (1 << 31) - 1
STALL = 0.8
MAX_ROUNDS = 64
GRIDS = ["grid16x16", "grid32x32", "grid64x64", "grid37x53", "grid16x16x16"]
BOUND_GRIDS = ["grid32x32", "grid64x64", "grid37x53", "grid16x16x16"]      # 16x16 sits at 0.27 and is left out of the bound
JACOBI_FACTOR = 0.3
JACOBI_FACTOR_128 = 0.1
ANISO_FACTOR = 0.5
SEED_RHS = 20261020


# ---- matrices -------------------------------------------------------------------------------------------------------------------
def grid2d(nx, ny, cx=1.0, cy=1.0):
    """5-point stencil, x fastest: couplings -cx along x and -cy along y, diagonal 2 cx + 2 cy."""
    tx = sp.diags([-cx, 2 * cx, -cx], [-1, 0, 1], shape=(nx, nx))
    ty = sp.diags([-cy, 2 * cy, -cy], [-1, 0, 1], shape=(ny, ny))
    return (sp.kron(sp.identity(ny), tx) + sp.kron(ty, sp.identity(nx))).tocsr()


def grid3d(n):
    t = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    i = sp.identity(n)
    return (sp.kron(sp.kron(i, i), t) + sp.kron(sp.kron(i, t), i) + sp.kron(sp.kron(t, i), i)).tocsr()


def path(n):
    return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n)).tocsr() if n > 1 else sp.csr_matrix(np.array([[2.0]]))


def star(leaves=300):
    n = leaves + 1
    rows = np.concatenate([np.zeros(leaves, dtype=np.int64), np.arange(1, n), np.arange(n)])
    cols = np.concatenate([np.arange(1, n), np.zeros(leaves, dtype=np.int64), np.arange(n)])
    vals = np.concatenate([-np.ones(2 * leaves), np.concatenate([[leaves + 1.0], 2.0 * np.ones(leaves)])])
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def random_sdd(n=600, per_row=4, seed=7):
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n), per_row)
    j = rng.integers(0, n, size=n * per_row)
    keep = i != j
    v = -rng.uniform(0.1, 1.0, size=n * per_row)
    L = sp.csr_matrix((v[keep], (i[keep], j[keep])), shape=(n, n))
    L = L + L.T
    d = np.asarray(abs(L).sum(axis=1)).ravel() + 0.05
    return (L + sp.diags(d)).tocsr()


def diagonal(n=37):
    return sp.diags(1.0 + np.arange(n) / n).tocsr()


def cases():
    """name -> scipy CSR with sorted indices."""
    out = {"grid16x16": grid2d(16, 16), "grid32x32": grid2d(32, 32), "grid64x64": grid2d(64, 64), "grid37x53": grid2d(37, 53),
           "grid16x16x16": grid3d(16), "aniso40x40": grid2d(40, 40, 1.0, 0.01), "diagonal": diagonal(),
           "one": path(1), "two": path(2), "path255": path(255), "path256": path(256), "path257": path(257),
           "star300": star(300), "random600": random_sdd()}
    for A in out.values():
        A.sum_duplicates()
        A.sort_indices()
    return out


def rhs(n, seed=SEED_RHS):
    return np.random.default_rng(seed).standard_normal(n)


def equal_blocks(n, k):
    return [(n * j) // k for j in range(k + 1)]


# ---- setup ----------------------------------------------------------------------------------------------------------------------
def hash31(g):
    """h(g) of the description for an array of global rows: 31 bits."""
    x = (np.asarray(g, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(32)
    x = x * np.uint64(0xD6E8FEB86659FD93)
    x ^= x >> np.uint64(32)
    return (x >> np.uint64(33)).astype(np.int64)


def keys_of(partition):
    n = int(partition[-1])
    g = np.arange(n, dtype=np.int64)
    block = np.searchsorted(np.asarray(partition), g, side="right") - 1
    local = g - np.asarray(partition, dtype=np.int64)[block]
    return (hash31(g) << 31) | local, block


def weights(A):
    d = A.diagonal()
    rho = float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / d))
    w = 4.0 / (3.0 * rho)
    return w / d, w, rho


def strength(A, partition, theta):
    """The strength graph as CSR (indptr, indices) with global columns, cut at the block boundaries."""
    A = A.tocsr()
    n = A.shape[0]
    d = A.diagonal()
    _, block = keys_of(partition)
    row = np.repeat(np.arange(n), np.diff(A.indptr))
    col = A.indices
    keep = (row != col) & (block[row] == block[col]) & (A.data != 0) & (np.abs(A.data) >= theta * np.sqrt(d[row] * d[col]))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=n))]).astype(np.int64)
    return indptr, col[keep].astype(np.int64)


def neighbour_max(indptr, indices, v):
    """max(v_i, max over the neighbours j of v_j)."""
    out = v.copy()
    rows = np.flatnonzero(np.diff(indptr) > 0)
    if len(rows):
        out[rows] = np.maximum(v[rows], np.maximum.reduceat(v[indices], indptr[rows]))
    return out


def mis2(indptr, indices, key):
    """(state, rounds): state is 2^62 for a root and -1 for every other row."""
    k = key.copy()
    rounds = 0
    while np.any((k >= 0) & (k < ROOT)):
        if rounds == MAX_ROUNDS:
            raise RuntimeError("mis2: no end after 64 rounds")
        m2 = neighbour_max(indptr, indices, neighbour_max(indptr, indices, k))
        und = (k >= 0) & (k < ROOT)
        k = np.where(und & (m2 == key), ROOT, np.where(und & (m2 >= ROOT), -1, k))
        rounds += 1
    return k, rounds


def _best_neighbour(indptr, indices, score):
    """Per row the neighbour with the largest score >= 0 (-1 where none): scores are distinct keys, or -1."""
    n = len(indptr) - 1
    best = np.full(n, -1, dtype=np.int64)
    rows = np.flatnonzero(np.diff(indptr) > 0)
    if len(rows):
        s = score[indices]
        top = np.maximum.reduceat(s, indptr[rows])
        row = np.repeat(np.arange(n), np.diff(indptr))
        top_of_row = np.full(n, -2, dtype=np.int64)
        top_of_row[rows] = top
        hit = (s == top_of_row[row]) & (s >= 0)
        best[row[hit]] = indices[hit]
    return best


def aggregate(A, partition, theta):
    """(agg, counts, roots, rounds, (indptr, indices)): the global aggregate id of every row, the aggregates per block, the
    root flags, the rounds the independent set took, the strength graph."""
    indptr, indices = strength(A, partition, theta)
    key, block = keys_of(partition)
    n = len(key)
    state, rounds = mis2(indptr, indices, key)
    root = state == ROOT
    owner = np.where(root, np.arange(n), -1)
    near = _best_neighbour(indptr, indices, np.where(root, key, -1))
    owner = np.where((owner < 0) & (near >= 0), near, owner)
    far = _best_neighbour(indptr, indices, np.where(owner >= 0, key, -1))
    owner2 = np.where(owner < 0, owner[np.maximum(far, 0)], owner)
    assert np.all(owner2 >= 0)
    ids = np.cumsum(root) - 1                                   # the scan of the root flags, in row order
    agg = ids[owner2]
    counts = np.bincount(block[root], minlength=len(partition) - 1)
    return agg.astype(np.int64), counts.astype(np.int64), root, rounds, (indptr, indices)


def structural_product(A, B):
    """A @ B with every structural entry stored, cancelled sums as explicit zeros; sorted indices."""
    A, B = A.tocsr(), B.tocsr()
    ones = lambda M: sp.csr_matrix((np.ones(len(M.data)), M.indices, M.indptr), shape=M.shape)
    pat = (ones(A) @ ones(B)).tocsr()
    pat.sort_indices()
    C = (A @ B).tocsr()
    C.sort_indices()
    ncol = max(B.shape[1], 1)
    kp = np.repeat(np.arange(pat.shape[0]), np.diff(pat.indptr)) * ncol + pat.indices
    kc = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr)) * ncol + C.indices
    vals = np.zeros(len(kp))
    vals[np.searchsorted(kp, kc)] = C.data
    return sp.csr_matrix((vals, pat.indices.copy(), pat.indptr.copy()), shape=pat.shape)


def prolongator(A, agg, nc, s):
    n = A.shape[0]
    T = sp.csr_matrix((np.ones(n), agg, np.arange(n + 1)), shape=(n, nc))
    AT = structural_product(A, T)
    row = np.repeat(np.arange(n), np.diff(AT.indptr))
    vals = (AT.indices == agg[row]).astype(np.float64) - s[row] * AT.data
    return sp.csr_matrix((vals, AT.indices.copy(), AT.indptr.copy()), shape=(n, nc))


def setup(A, partition=None, theta=0.0, max_levels=12, coarse_size=128, coarse_sweeps=4):
    """The hierarchy: a list of levels (dicts: A, s, w, rho, n, partition, and on all but the last agg, counts, roots, rounds,
    P, Pt), the last one with ``inv`` (dense) or ``sweeps``."""
    A = A.tocsr()
    partition = [0, A.shape[0]] if partition is None else [int(v) for v in partition]
    levels = []
    while True:
        n = A.shape[0]
        s, w, rho = weights(A)
        lvl = dict(A=A, s=s, w=w, rho=rho, n=n, partition=partition)
        levels.append(lvl)
        last = n <= coarse_size or len(levels) >= max_levels
        if not last:
            agg, counts, roots, rounds, graph = aggregate(A, partition, theta)
            lvl.update(agg=agg, counts=counts, roots=roots, rounds=rounds, graph=graph)
            nc = int(counts.sum())
            last = nc >= STALL * n
        if last:
            if n <= coarse_size:
                D = A.toarray()
                lvl["inv"] = np.linalg.inv((D + D.T) / 2)
            else:
                lvl["sweeps"] = coarse_sweeps
            return levels
        P = prolongator(A, agg, nc, s)
        Pt = P.T.tocsr()
        Pt.sort_indices()
        lvl.update(P=P, Pt=Pt)
        A = structural_product(Pt, structural_product(A, P))
        partition = [0] + np.cumsum(counts).tolist()


def operator_complexity(levels):
    return sum(l["A"].nnz for l in levels) / levels[0]["A"].nnz


def cycle(levels, b, k=0):
    lvl = levels[k]
    A, s = lvl["A"], lvl["s"]
    if k == len(levels) - 1:
        if "inv" in lvl:
            return lvl["inv"] @ b
        x = s * b
        for _ in range(lvl["sweeps"] - 1):
            x = x + s * (b - A @ x)
        return x
    x = s * b
    r = b - A @ x
    xc = cycle(levels, lvl["Pt"] @ r, k + 1)
    x = x + lvl["P"] @ xc
    return x + s * (b - A @ x)


def pcg_m(A, b, prec, rtol=1e-8, atol=0.0, maxiter=None, x0=None):
    """``_pcg_cases.pcg`` with z = prec(r) and r.z as one dot, in the device loop's gate order: (x, iterations, status,
    residual_norms)."""
    n = len(b)
    maxiter = 10 * n if maxiter is None else maxiter
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    r = b.copy() if x0 is None else b - A @ x
    z = prec(r)
    p = z.copy()
    rr, rz, bb = float(r @ r), float(r @ z), float(b @ b)
    if bb == 0.0:
        return np.zeros(n), 0, "converged", [0.0]
    thr = max(rtol * math.sqrt(bb), atol) ** 2
    hist = [math.sqrt(rr)]
    if rr <= thr:
        return x, 0, "converged", hist
    for j in range(1, maxiter + 1):
        Ap = A @ p
        pAp = float(p @ Ap)
        if not (pAp > 0):
            return x, j - 1, "breakdown", hist
        a = rz / pAp
        r = r - a * Ap
        rr = float(r @ r)
        hist.append(math.sqrt(rr))
        converged = rr <= thr
        z = prec(r)
        rz_new = float(r @ z)
        beta = rz_new / rz
        x = x + a * p
        p = z + beta * p
        rz = rz_new
        if converged:
            return x, j, "converged", hist
    return x, maxiter, "maxiter", hist


def pcg_amg(A, b, levels, **kw):
    return pcg_m(A, b, lambda r: cycle(levels, r), **kw)


def pcg_jacobi(A, b, **kw):
    dinv = 1.0 / A.diagonal()
    return pcg_m(A, b, lambda r: dinv * r, **kw)


# ---- one block at a time: the inputs and stages of the kernels' C entries ----------------------------------------------------
def split_block(A, partition, j, base=0, Ti=np.int32):
    """The rank-local split form of block j's rows: (rowptr, colval_split, vals, n_own, ghosts).  An owned column c becomes
    c - lo, a ghost n_own + its position among the block's sorted distinct ghosts (``ghosts``: their global ids); entries stay
    in stored (global ascending) order, so ghosts below lo come before the owned columns.  ``base`` is added to both index
    arrays, which have type ``Ti``."""
    A = A.tocsr()
    lo, hi = int(partition[j]), int(partition[j + 1])
    a, b = int(A.indptr[lo]), int(A.indptr[hi])
    cols = A.indices[a:b].astype(np.int64)
    own = (cols >= lo) & (cols < hi)
    ghosts = np.unique(cols[~own])
    split = np.where(own, cols - lo, (hi - lo) + np.searchsorted(ghosts, cols))
    rowptr = A.indptr[lo:hi + 1].astype(np.int64) - a
    return (rowptr + base).astype(Ti), (split + base).astype(Ti), A.data[a:b].copy(), hi - lo, ghosts


def weights_stored_order(A):
    """(d, sum_j |a_ij| / d) with the row sum added one entry at a time in stored order (``weights`` adds pairwise); d = 0
    where no diagonal is stored."""
    A = A.tocsr()
    n = A.shape[0]
    d = A.diagonal()
    start, length = A.indptr[:-1].astype(np.int64), np.diff(A.indptr)
    absval = np.abs(A.data)
    total = np.zeros(n)
    for k in range(int(length.max()) if n else 0):              # the k-th stored entry of every row that has one
        rows = np.flatnonzero(length > k)
        total[rows] = total[rows] + absval[start[rows] + k]
    with np.errstate(divide="ignore", invalid="ignore"):
        return d, total / d


def mis2_states(indptr, indices, key):
    """The state array after each round of ``mis2`` on one graph and its keys (a block's own: local columns, the block's keys);
    the last one has no undecided row."""
    k = key.copy()
    while np.any((k >= 0) & (k < ROOT)):
        m2 = neighbour_max(indptr, indices, neighbour_max(indptr, indices, k))
        und = (k >= 0) & (k < ROOT)
        k = np.where(und & (m2 == key), ROOT, np.where(und & (m2 >= ROOT), -1, k))
        yield k.copy()


def compressed_columns(rows_indices, rng):
    """(colval_local, col_indices): a block's global columns as local ids into ``col_indices``, which lists the distinct columns
    in a shuffled order, not an ascending one: col_indices[colval_local] gives the columns back."""
    distinct = np.unique(np.asarray(rows_indices, dtype=np.int64))
    order = rng.permutation(len(distinct))
    col_indices = distinct[order]
    where = np.empty(len(distinct), dtype=np.int64)
    where[order] = np.arange(len(distinct))
    return where[np.searchsorted(distinct, rows_indices)], col_indices


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


CHAIN_COARSE = 8               # coarse_size at which every case but n = 1, 2 aggregates at least once


def theta_of(name):
    return 0.25 if name.startswith("aniso") else 0.0


def aggregate_product(lvl):
    """A T of a level that aggregated (T: one 1.0 per row at its aggregate), every structural entry stored."""
    n, nc = lvl["n"], int(lvl["counts"].sum())
    T = sp.csr_matrix((np.ones(n), lvl["agg"], np.arange(n + 1)), shape=(n, nc))
    return structural_product(lvl["A"], T)


def chain_levels(matrices, names=None):
    """(name, blocks) -> the levels that aggregate of ``setup`` at coarse_size = CHAIN_COARSE over ``equal_blocks``, theta 0.25
    on the anisotropic grid and 0 elsewhere: what the tests of the kernels' C entries walk block by block."""
    out = {}
    for name in (matrices if names is None else names):
        A = matrices[name]
        for k in BLOCKS:
            levels = setup(A, equal_blocks(A.shape[0], k), theta_of(name), coarse_size=CHAIN_COARSE)
            out[name, k] = [lvl for lvl in levels if "agg" in lvl]
    return out


def chain_coverage(levels_by_case):
    """What those levels hold: their number, the blocks (chains), the blocks of one row, the stored zeros, the levels with a row
    that has no strong neighbour, the most ghost entries of a level and the longest row of A T."""
    out = dict(levels=0, chains=0, one_row_blocks=0, stored_zeros=0, isolated=0, ghost_entries=0, longest_row=0)
    for levels in levels_by_case.values():
        for lvl in levels:
            A, part = lvl["A"], np.asarray(lvl["partition"])
            sizes = np.diff(part)
            out["levels"] += 1
            out["chains"] += int(np.sum(sizes > 0))
            out["one_row_blocks"] += int(np.sum(sizes == 1))
            out["stored_zeros"] += int(np.sum(A.data == 0))
            out["isolated"] += int(np.any(np.diff(lvl["graph"][0]) == 0))
            _, block = keys_of(lvl["partition"])
            row = np.repeat(np.arange(lvl["n"]), np.diff(A.indptr))
            out["ghost_entries"] = max(out["ghost_entries"], int(np.sum(block[row] != block[A.indices])))
            out["longest_row"] = max(out["longest_row"], int(np.diff(aggregate_product(lvl).indptr).max()))
    return out


# ---- the argument rules, restated ---------------------------------------------------------------------------------------------
BAD_ARGUMENTS = [                                               # (keyword overrides, exception)
    (dict(T=np.float32), TypeError),
    (dict(shape=(10, 12)), ValueError),
    (dict(col_partition=[0, 4, 10]), ValueError),
    (dict(theta=-0.1), ValueError), (dict(theta=1.0), ValueError), (dict(theta=float("nan")), ValueError),
    (dict(max_levels=0), ValueError),
    (dict(coarse_size=0), ValueError), (dict(coarse_size=1025), ValueError),
    (dict(coarse_sweeps=0), ValueError),
]
GOOD_ARGUMENTS = dict(T=np.float64, shape=(10, 10), row_partition=[0, 5, 10], col_partition=[0, 5, 10], theta=0.0, max_levels=12,
                      coarse_size=128, coarse_sweeps=4)
