"""The reverse Cuthill-McKee ordering of hp.rcm restated in numpy, twice, and the graphs the tests walk.

``rcm_sequential`` is the textbook queue: pop ``v``, append its unvisited neighbours sorted by ``(degree, index)``.
``rcm_levels`` is the form the device runs (csrc/rcm.hip): per level, ``parent[u]`` = the smallest number among the level
vertices that list ``u``, new vertices numbered in ascending ``(parent << 32) | rank``; given the two caps of the library it
also replays which levels the one-workgroup kernel walks and which go device-wide.  tests/test_rcm_cases.py holds the two
against each other and against scipy's bandwidth; tests/test_gpu_rcm.py holds the device against them.

Both work on a graph ``(indptr, indices)`` without self-loops and without repeated neighbours; a vertex's degree is the length
of its list, so on a directed graph (a nonsymmetric pattern walked as it is) it is the out-degree.  Every case matrix is the
named graph under a fixed random relabelling, with a diagonal that makes it positive definite where it is symmetric."""
import functools

import numpy as np
import scipy.sparse as sp

FRONTIER_CAP = 4096          # hpcla_rcm_frontier_cap(), asserted by the device tests
CANDIDATE_CAP = 8192         # hpcla_rcm_candidate_cap()
UNVISITED = 2 ** 31 - 1


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def block_graph(A, lo=0, hi=None, symmetric=True):
    """(indptr, indices) of rows and columns lo .. hi - 1 of the scipy matrix ``A`` without the diagonal (stored entries count,
    whatever their value); ``symmetric=False``: of E u E^T.  Ascending neighbours, none repeated."""
    hi = A.shape[0] if hi is None else hi
    B = sp.csr_matrix(A)[lo:hi, lo:hi].tocoo()
    keep = B.row != B.col
    G = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int8), (B.row[keep], B.col[keep])), shape=(hi - lo, hi - lo))
    if not symmetric:
        G = sp.csr_matrix(G + G.T)
    G.sum_duplicates()
    G.sort_indices()
    return G.indptr.astype(np.int64), G.indices.astype(np.int64)


def by_degree_of(indptr):
    deg = np.diff(indptr)
    order = np.lexsort((np.arange(len(deg)), deg))           # (deg, index) ascending
    rank = np.empty(len(deg), dtype=np.int64)
    rank[order] = np.arange(len(deg))
    return deg, order, rank


def rcm_sequential(indptr, indices):
    """The queue algorithm; returns p (local, p[new] = old)."""
    n = len(indptr) - 1
    deg, by_degree, _ = by_degree_of(indptr)
    visited = np.zeros(n, dtype=bool)
    order = [int(v) for v in by_degree if deg[v] == 0]
    visited[order] = True
    for s in by_degree:
        if visited[s]:
            continue
        visited[s] = True
        queue = [int(s)]
        head = 0
        while head < len(queue):
            v = queue[head]
            head += 1
            nb = [int(u) for u in indices[indptr[v]:indptr[v + 1]] if not visited[u]]
            nb.sort(key=lambda u: (deg[u], u))
            for u in nb:
                visited[u] = True
            queue.extend(nb)
        order.extend(queue)
    return np.array(order[::-1], dtype=np.int64)


def _neighbours_of(indptr, indices, front):
    """(the concatenated neighbour lists of ``front``, the position in ``front`` of each entry's owner)."""
    lens = indptr[front + 1] - indptr[front]
    total = int(lens.sum())
    owner = np.repeat(np.arange(len(front)), lens)
    starts = np.repeat(indptr[front] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return indices[starts + np.arange(total)], owner


def rcm_levels(indptr, indices, frontier_cap=FRONTIER_CAP, candidate_cap=CANDIDATE_CAP):
    """The level form; returns (p, facts) with facts = components, levels, narrow_launches, wide_levels as hp.rcm counts them."""
    n = len(indptr) - 1
    deg, by_degree, rank = by_degree_of(indptr)
    parent = np.full(n, UNVISITED, dtype=np.int64)
    order = np.empty(n, dtype=np.int64)
    z = int((deg == 0).sum())
    order[:z] = by_degree[:z]
    parent[by_degree[:z]] = np.arange(z)
    cnt = cursor = z
    components, levels, narrow, wide = z, 0, 1 if n else 0, 0
    while cnt < n:                                          # a start is always found by the one-workgroup kernel
        while parent[by_degree[cursor]] != UNVISITED:
            cursor += 1
        s = by_degree[cursor]
        parent[s] = cnt
        order[cnt] = s
        lo, cnt = cnt, cnt + 1
        hi = cnt
        components += 1
        levels += 1
        in_narrow = True
        while True:
            front = order[lo:hi]
            nbrs, owner = _neighbours_of(indptr, indices, front)
            if in_narrow and (len(front) > frontier_cap or len(nbrs) > candidate_cap):
                in_narrow = False                            # the kernel leaves the level untouched
            if not in_narrow:
                wide += 1
            fresh = parent[nbrs] == UNVISITED
            new, nums = nbrs[fresh], lo + owner[fresh]
            if len(new) == 0:
                if not in_narrow:
                    narrow += 1                              # the host hands the next start back to the kernel
                break
            np.minimum.at(parent, new, nums)
            cand = np.unique(new)
            keys = np.sort((parent[cand] << 32) | rank[cand])
            cand = by_degree[keys & 0xffffffff]
            order[cnt:cnt + len(cand)] = cand
            lo, hi = hi, cnt + len(cand)
            cnt = hi
            levels += 1
            if not in_narrow and len(cand) <= frontier_cap and len(cand) * len(indices) <= candidate_cap * n:
                in_narrow = True
                narrow += 1
    facts = dict(components=components, levels=levels, narrow_launches=narrow, wide_levels=wide)
    return order[::-1].copy(), facts


def bandwidth_of_graph(indptr, indices, p=None):
    """max |i - j| over the graph's entries, in old numbers or -- p given -- in new ones."""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    if not len(rows):
        return 0
    if p is None:
        return int(np.abs(rows - indices).max())
    inv = np.empty(n, dtype=np.int64)
    inv[p] = np.arange(n)
    return int(np.abs(inv[rows] - inv[indices]).max())


def bandwidth_of_matrix(A):
    C = sp.coo_matrix(A)
    return int(np.abs(C.row - C.col).max()) if C.nnz else 0


def is_permutation(p, n):
    return len(p) == n and np.array_equal(np.sort(p), np.arange(n))


# ---- the graphs --------------------------------------------------------------------------------------------------------------
def _from_edges(n, i, j, seed, symmetric=True):
    """The matrix of the graph with edges (i, j) (both ways when ``symmetric``) under a fixed random relabelling: -1 off the
    diagonal, the row's entry count + 1 on it (symmetric: positive definite)."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    q = np.random.default_rng(seed).permutation(n)
    i, j = q[i], q[j]
    if symmetric:
        i, j = np.concatenate([i, j]), np.concatenate([j, i])
    off = i != j
    G = sp.csr_matrix((np.ones(int(off.sum())), (i[off], j[off])), shape=(n, n))
    G.sum_duplicates()
    G.data[:] = -1.0
    A = sp.csr_matrix(G + sp.diags(np.diff(G.indptr) + 1.0))
    A.sort_indices()
    return A


def _grid_edges(nx, ny, offset=0):
    idx = np.arange(nx * ny).reshape(ny, nx) + offset
    return (np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]), np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()]))


def _path(n, seed):
    return _from_edges(n, np.arange(n - 1), np.arange(1, n), seed)


def _grid(nx, ny, seed):
    return _from_edges(nx * ny, *_grid_edges(nx, ny), seed)


def _delaunay(npts, seed):
    from scipy.spatial import Delaunay
    tri = Delaunay(np.random.default_rng(seed).random((npts, 2))).simplices
    return _from_edges(npts, np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]]), np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]]), seed + 1)


def _random(n, density, seed, symmetric=True):
    rng = np.random.default_rng(seed)
    m = int(round(density * n * n))
    return _from_edges(n, rng.integers(0, n, m), rng.integers(0, n, m), seed + 1, symmetric)


def _components(seed):
    """Two grids (17 x 9 and 12 x 12) and 7 vertices without a neighbour: 9 components."""
    a, b = _grid_edges(17, 9), _grid_edges(12, 12, offset=153)
    return _from_edges(153 + 144 + 7, np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), seed)


def _star(leaves, seed):
    return _from_edges(leaves + 1, np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1), seed)


def _tree(second_level, seed, children=64):
    """A tail (the only vertex of degree 1, so the walk starts there), a root, ``children`` children and ``second_level``
    grandchildren dealt to the children in turn.  Consecutive grandchildren are joined (a last odd one to its predecessor), so
    none has degree 1; those edges stay inside the level.  Levels: 1, 1, children, second_level."""
    g = np.arange(second_level)
    first = 2 + children
    mates = np.arange(0, second_level - 1, 2)
    i = np.concatenate([[1], np.zeros(children, dtype=np.int64), 2 + g % children, first + mates,
                        [first + second_level - 2] if second_level % 2 else []]).astype(np.int64)
    j = np.concatenate([[0], 2 + np.arange(children), first + g, first + mates + 1,
                        [first + second_level - 1] if second_level % 2 else []]).astype(np.int64)
    return _from_edges(first + second_level, i, j, seed)


def _degree_sum(over, seed, children=64):
    """A tail (the only vertex of degree 1), a root, 64 children that all list the same pool of 127 grandchildren: the
    children's degrees sum to CANDIDATE_CAP exactly while only the pool is claimed.  ``over``: one more vertex joined to two
    children, which puts the sum 2 over the cap."""
    pool = CANDIDATE_CAP // children - 1                     # every child lists the root and the pool
    c = 2 + np.arange(children)
    first = 2 + children
    i = np.concatenate([[1], np.zeros(children, dtype=np.int64), np.repeat(c, pool), c[:2] if over else []]).astype(np.int64)
    j = np.concatenate([[0], c, np.tile(first + np.arange(pool), children), [first + pool] * 2 if over else []]).astype(np.int64)
    return _from_edges(first + pool + (1 if over else 0), i, j, seed)


_BUILDERS = {
    "path1": lambda: _path(1, 1),
    "path2": lambda: _path(2, 2),
    "path300": lambda: _path(300, 3),
    "grid33x31": lambda: _grid(33, 31, 4),
    "grid64x64": lambda: _grid(64, 64, 5),
    "grid200x20": lambda: _grid(200, 20, 6),
    "delaunay2000": lambda: _delaunay(2000, 7),
    "delaunay8000": lambda: _delaunay(8000, 9),
    "random1500": lambda: _random(1500, 0.002, 11),
    "components9": lambda: _components(13),
    "pairs500": lambda: _from_edges(1000, 2 * np.arange(500), 2 * np.arange(500) + 1, 14),
    "nonsymmetric": lambda: _random(900, 0.004, 15, symmetric=False),
    "star_cap": lambda: _star(CANDIDATE_CAP, 17),
    "star_cap_plus1": lambda: _star(CANDIDATE_CAP + 1, 18),
    "tree_frontier_cap": lambda: _tree(FRONTIER_CAP, 19),
    "tree_frontier_cap_plus1": lambda: _tree(FRONTIER_CAP + 1, 20),
    "degree_sum_cap": lambda: _degree_sum(0, 21),
    "degree_sum_cap_plus1": lambda: _degree_sum(1, 22),
    "random20000": lambda: _random(20000, 4.0 / 20000, 23),  # 4 n edges: about 8 neighbours each
    "grid256x256": lambda: _grid(256, 256, 25),
}
CASES = list(_BUILDERS)
SYMMETRIC_CASES = [c for c in CASES if c != "nonsymmetric"]
# scipy's reverse_cuthill_mckee is held against on these (the issue's list): grids, meshes, the random pattern, the components
SCIPY_CASES = ["grid33x31", "grid64x64", "grid200x20", "delaunay2000", "delaunay8000", "random1500", "components9"]


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The case's scipy CSR matrix (float64, ascending columns, a full diagonal); built once."""
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name, symmetric=True, lo=0, hi=None):
    """(p, facts, (indptr, indices)) of the level form on the block lo .. hi - 1 of the case; computed once and shared."""
    g = block_graph(matrix(name), lo, hi, symmetric)
    p, facts = rcm_levels(*g)
    facts = dict(facts, bandwidth_before=bandwidth_of_graph(*g), bandwidth_after=bandwidth_of_graph(*g, p))
    p.setflags(write=False)
    return p, facts, g
