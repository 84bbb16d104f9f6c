"""Shared cases of the nonsymmetric mode of ``hp.amg`` (``symmetric=False``) and a numpy / scipy restatement of what it changes,
on top of tests/_amg_cases.py (``ac``), written from the method's description, not from the kernels.

A level differs from the symmetric method's in three places:
  strength    the graph is E u E^T, E the graph of ``ac.strength`` (stored, same block, a_ij != 0, j != i, |a_ij| >= theta
              sqrt(a_ii a_jj)): rows as sorted sets of distinct neighbours.  The maxima of the independent set and of the join
              run over distinct keys, so the order and the multiplicity of a row's entries do not matter.
  R           Tt (I - A S): r_cj = [agg(j) == c] - (Tt A)_cj s_j on the structural pattern of Tt A; A_c = R (A P)
  last level  the inverse of the coarse matrix itself
The weights, the independent set, the join, the numbering, P, the stall rule and the cycle (with R for Pt) are ``ac``'s.
GMRES and BiCGStab are ``_ilu_cases.gmres_op`` / ``bicgstab_op`` with K = the cycle.

Cases: the unscaled 5-point convection-diffusion stencil (diagonal 4; west, east, south, north -1.5, -0.5, -1.3, -0.7: the
values of tests/_bicgstab_cases.py without its scaling) at 16x16, 24x20, 33x31 and 65x63; the purely upwind 33x31 stencil
(diagonal 4, west and south -2, the zero east / north couplings not stored: a structurally nonsymmetric pattern); and for the
graph kernels alone ``graph_cases()``: n = 1, n = 2 with one directed edge, a directed path of 600 rows, an in-star and an
out-star of 300 leaves, ``_ilu_cases.asymmetric_pattern()``, directed paths of 255, 256, 257 and 1025 rows (scan.h's chunk is 1024),
a matrix with stored explicit zeros, and one whose couplings are strong one way only (-1 against -0.01 at theta = 0.25).
"""
import numpy as np
import scipy.sparse as sp

from tests import _amg_cases as ac
from tests import _bicgstab_cases as bc
from tests import _ilu_cases as ic

SIZES = [(16, 16), (24, 20), (33, 31)]
LARGE_SIZE = (65, 63)
UPWIND_SIZE = (33, 31)
COARSE_SIZES = [128, 8]        # the default: three levels at 33x31; 8: four
JACOBI_FACTOR = 0.3            # the cycle's GMRES(30) count against Jacobi's, both restated (the issue's condition)
HEAD = 9                       # history entries compared, as tests/_gmres_cases.py
HEAD_BICGSTAB = 4              # as tests/_ilu_cases.py
COUNT_SLACK = 2                # iterations, as tests/test_gpu_pcg.py allows
BLOCKS = ac.BLOCKS


# ---- matrices -------------------------------------------------------------------------------------------------------------------
def stencil(nx, ny, west, east, south, north, diagonal=4.0):
    """x fastest; a coupling that is 0.0 is not stored."""
    def line(n, lo, hi):
        d, o = [np.zeros(n)], [0]
        if lo != 0.0:
            d.append(np.full(n - 1, lo)); o.append(-1)
        if hi != 0.0:
            d.append(np.full(n - 1, hi)); o.append(1)
        return sp.diags(d, o, shape=(n, n))
    A = sp.kron(sp.identity(ny), line(nx, west, east)) + sp.kron(line(ny, south, north), sp.identity(nx)) \
        + diagonal * sp.identity(nx * ny)
    A = A.tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def convection_diffusion(nx, ny):
    return stencil(nx, ny, bc.WEST, bc.EAST, bc.SOUTH, bc.NORTH)


def upwind(nx, ny):
    return stencil(nx, ny, -2.0, 0.0, -2.0, 0.0)


def csr_of(rowptr, cols, vals):
    n = len(rowptr) - 1
    A = sp.csr_matrix((np.asarray(vals, dtype=np.float64), np.asarray(cols), np.asarray(rowptr)), shape=(n, n))
    A.sort_indices()
    return A


def from_edges(n, edges, value=-1.0, diagonal=None):
    """Directed edges (i, j) as entries a_ij = value next to a diagonal that dominates; explicit zeros stay stored."""
    i = np.array([e[0] for e in edges], dtype=np.int64).reshape(-1)
    j = np.array([e[1] for e in edges], dtype=np.int64).reshape(-1)
    v = np.broadcast_to(np.asarray(value, dtype=np.float64), i.shape)
    d = 1.0 + np.bincount(i, weights=np.abs(v), minlength=n) if diagonal is None else np.full(n, float(diagonal))
    rows, cols, vals = np.concatenate([i, np.arange(n)]), np.concatenate([j, np.arange(n)]), np.concatenate([v, d])
    order = np.lexsort((cols, rows))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return csr_of(rowptr, cols[order], vals[order])


def directed_path(n):
    return from_edges(n, [(i, i + 1) for i in range(n - 1)])


def in_star(leaves=300):
    return from_edges(leaves + 1, [(i, 0) for i in range(1, leaves + 1)])


def out_star(leaves=300):
    return from_edges(leaves + 1, [(0, i) for i in range(1, leaves + 1)])


def stored_zeros(n=97):
    """A ring of directed edges i -> i + 1 with weight -1 and stored explicit zeros at (i, i + 3) and (i + 5, i)."""
    e1 = [(i, (i + 1) % n) for i in range(n)]
    e0 = [(i, (i + 3) % n) for i in range(n)] + [((i + 5) % n, i) for i in range(0, n, 2)]
    return from_edges(n, e1 + e0, value=np.concatenate([-np.ones(len(e1)), np.zeros(len(e0))]))


def one_way(n=64):
    """a_{i, i+1} = -1 and a_{i+1, i} = -0.01 on a unit diagonal: at theta = 0.25 only the upper coupling is strong."""
    e = [(i, i + 1) for i in range(n - 1)] + [(i + 1, i) for i in range(n - 1)]
    return from_edges(n, e, value=np.concatenate([-np.ones(n - 1), -0.01 * np.ones(n - 1)]), diagonal=1.0)


ONE_WAY_THETA = 0.25


def graph_cases():
    """name -> (scipy CSR, theta)."""
    out = {"one": (ac.path(1), 0.0), "two_directed": (from_edges(2, [(0, 1)]), 0.0), "dpath600": (directed_path(600), 0.0),
           "instar300": (in_star(), 0.0), "outstar300": (out_star(), 0.0), "asym120": (csr_of(*ic.asymmetric_pattern()), 0.0),
           "upwind33x31": (upwind(*UPWIND_SIZE), 0.0), "dpath255": (directed_path(255), 0.0),
           "dpath256": (directed_path(256), 0.0), "dpath257": (directed_path(257), 0.0), "dpath1025": (directed_path(1025), 0.0),
           "zeros97": (stored_zeros(), 0.0), "oneway64": (one_way(), ONE_WAY_THETA)}
    return out


def hierarchy_cases():
    out = {f"cd{nx}x{ny}": convection_diffusion(nx, ny) for nx, ny in SIZES}
    out["upwind33x31"] = upwind(*UPWIND_SIZE)
    return out


def solve_cases():
    out = hierarchy_cases()
    out["cd65x63"] = convection_diffusion(*LARGE_SIZE)
    return out


def csr_arrays(A):
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.copy()


# ---- setup ----------------------------------------------------------------------------------------------------------------------
def symmetrised(indptr, indices):
    """E u E^T of a graph in CSR with global columns: CSR with each row's distinct neighbours ascending."""
    n = len(indptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    pairs = np.unique(np.stack([np.concatenate([row, indices]), np.concatenate([indices, row])], axis=1), axis=0) \
        if len(indices) else np.zeros((0, 2), dtype=np.int64)
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(pairs[:, 0], minlength=n))]).astype(np.int64)
    return out_ptr, pairs[:, 1].astype(np.int64)


def strength(A, partition, theta):
    return symmetrised(*ac.strength(A, partition, theta))


def aggregate(A, partition, theta):
    """``ac.aggregate`` on the symmetrised graph: (agg, counts, roots, rounds, (indptr, indices))."""
    indptr, indices = strength(A, partition, theta)
    key, block = ac.keys_of(partition)
    n = len(key)
    state, rounds = ac.mis2(indptr, indices, key)
    root = state == ac.ROOT
    owner = np.where(root, np.arange(n), -1)
    near = ac._best_neighbour(indptr, indices, np.where(root, key, -1))
    owner = np.where((owner < 0) & (near >= 0), near, owner)
    far = ac._best_neighbour(indptr, indices, np.where(owner >= 0, key, -1))
    owner2 = np.where(owner < 0, owner[np.maximum(far, 0)], owner)
    assert np.all(owner2 >= 0), "a row was left without an aggregate"
    ids = np.cumsum(root) - 1
    counts = np.bincount(block[root], minlength=len(partition) - 1)
    return ids[owner2].astype(np.int64), counts.astype(np.int64), root, rounds, (indptr, indices)


def restrictor(A, agg, nc, s):
    n = A.shape[0]
    Tt = sp.csr_matrix((np.ones(n), agg, np.arange(n + 1)), shape=(n, nc)).T.tocsr()
    Tt.sort_indices()
    TA = ac.structural_product(Tt, A)
    row = np.repeat(np.arange(nc), np.diff(TA.indptr))
    vals = (agg[TA.indices] == row).astype(np.float64) - TA.data * s[TA.indices]
    return sp.csr_matrix((vals, TA.indices.copy(), TA.indptr.copy()), shape=(nc, n))


def setup(A, partition=None, theta=0.0, max_levels=12, coarse_size=128, coarse_sweeps=4):
    """``ac.setup`` for ``symmetric=False``: levels as there, with ``R`` where ``ac``'s have ``Pt`` and ``Pt = R`` as well, so
    ``ac.cycle`` runs on them unchanged."""
    A = A.tocsr()
    partition = [0, A.shape[0]] if partition is None else [int(v) for v in partition]
    levels = []
    while True:
        n = A.shape[0]
        s, w, rho = ac.weights(A)
        lvl = dict(A=A, s=s, w=w, rho=rho, n=n, partition=partition)
        levels.append(lvl)
        last = n <= coarse_size or len(levels) >= max_levels
        if not last:
            agg, counts, roots, rounds, graph = aggregate(A, partition, theta)
            lvl.update(agg=agg, counts=counts, roots=roots, rounds=rounds, graph=graph)
            nc = int(counts.sum())
            last = nc >= ac.STALL * n
        if last:
            if n <= coarse_size:
                lvl["inv"] = np.linalg.inv(A.toarray())
            else:
                lvl["sweeps"] = coarse_sweeps
            return levels
        if not np.all(A.diagonal() > 0):
            raise ValueError("a diagonal that is not positive")
        P = ac.prolongator(A, agg, nc, s)
        R = restrictor(A, agg, nc, s)
        lvl.update(P=P, R=R, Pt=R)
        A = ac.structural_product(R, ac.structural_product(A, P))
        partition = [0] + np.cumsum(counts).tolist()


def cycle(levels, b):
    return ac.cycle(levels, b)


def gmres_amg(A, b, levels, **kw):
    return ic.gmres_op(*csr_arrays(A), b, lambda r: ac.cycle(levels, r), **kw)


def bicgstab_amg(A, b, levels, **kw):
    return ic.bicgstab_op(*csr_arrays(A), b, lambda r: ac.cycle(levels, r), **kw)


def gmres_jacobi(A, b, **kw):
    dinv = 1.0 / A.diagonal()
    return ic.gmres_op(*csr_arrays(A), b, lambda r: dinv * r, **kw)


# ---- the argument rules ---------------------------------------------------------------------------------------------------------
BAD_SYMMETRIC = [0, 1, None, "no", 1.0]
