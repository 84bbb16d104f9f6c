"""The reverse Cuthill-McKee ordering of hp.rcm restated in numpy, twice, and the graphs the tests walk.

``rcm_sequential`` is the textbook queue: pop ``v``, append its unvisited neighbours sorted by ``(degree, index)``.
``rcm_levels`` is the form the device runs (csrc/rcm.hip): per level, ``parent[u]`` = the smallest number among the level
vertices that list ``u``, new vertices numbered in ascending ``(parent << 32) | rank``; given the two caps of the library it
also replays which levels the one-workgroup kernel walks and which go device-wide.  tests/test_rcm_cases.py holds the two
against each other and against scipy's bandwidth; tests/test_gpu_rcm.py holds the device against them.

Below them each kernel of csrc/rcm.hip is restated on its own (``graph_of_block``, ``degrees_of``, ``init_of``, ``expand_of``,
``keys_of``, ``number_of``), and ``rcm_trace`` replays the walk launch by launch -- the state every launch is entered with, the
record the one-workgroup kernel must leave, the candidates of every device-wide level -- for tests/test_gpu_rcm_kernels.py,
which calls every C entry alone.  These accept lists with repeated neighbours (E u E^T as the device builds it).

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


# ---- the kernels one by one (csrc/rcm.hip; tests/test_gpu_rcm_kernels.py holds each C entry against these) ---------------------------
DONE, WIDE = 0, 1            # the status word of the one-workgroup kernel's record
FREE = -7                    # what rcm_trace keeps in the places of ``order`` that no launch has written yet


def split_block(A, lo, hi, base, Ti, shuffle_seed=None):
    """What a rank holds of rows lo .. hi - 1 of the scipy matrix ``A``: (rowptr, colval, col_indices) with ``colval`` a
    position in ``col_indices``, the sorted global ids of the columns the rows store.  ``base`` is added to all three;
    ``shuffle_seed``: every row's entries in a random stored order."""
    R = sp.csr_matrix(A)[lo:hi]
    R.sort_indices()
    rowptr, gcols = R.indptr.astype(np.int64), R.indices.astype(np.int64)
    col_indices = np.unique(gcols)
    colval = np.searchsorted(col_indices, gcols)
    if shuffle_seed is not None:
        rows = np.repeat(np.arange(hi - lo), np.diff(rowptr))
        colval = colval[np.lexsort((np.random.default_rng(shuffle_seed).random(len(colval)), rows))]
    return (rowptr + base).astype(Ti), (colval + base).astype(Ti), col_indices + base


def graph_of_block(rowptr, colval, col_indices, nrows, row_start, base):
    """(g_rowptr, g_cols) as hpcla_rcm_graph_count / _fill define them: an entry is kept when its global column names another
    row of the block; kept entries stay in stored order, a repeated column as often as it is stored."""
    rowptr = np.asarray(rowptr, dtype=np.int64)[:nrows + 1] - base
    colval, col_indices = np.asarray(colval, dtype=np.int64), np.asarray(col_indices, dtype=np.int64)
    rows = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(rowptr))
    c = col_indices[colval[rowptr[0]:rowptr[nrows]] - base] - base - row_start if nrows else np.zeros(0, dtype=np.int64)
    keep = (c >= 0) & (c < nrows) & (c != rows)
    g_rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=nrows))]).astype(np.int64)
    return g_rowptr, c[keep]


def doubled_graph(indptr, indices):
    """E u E^T as hpcla_amg_symmetrise_count / _fill leave it: every row's out-list, then its in-list (here by ascending
    source; the device's order within the in-list is that of its atomics).  An edge stored both ways is listed twice."""
    n = len(indptr) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    rows, cols = np.concatenate([src, indices]), np.concatenate([indices, src])
    keep = np.lexsort((np.arange(len(rows)), rows))          # stable by row: out-list first
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64), cols[keep]


def degrees_of(g_rowptr, g_cols, distinct):
    """deg[i] = the entries of row i, or -- distinct -- those that no earlier entry of the row repeats."""
    n = len(g_rowptr) - 1
    if not distinct:
        return np.diff(g_rowptr).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(g_rowptr))
    pairs = np.unique(rows * max(n, 1) + np.asarray(g_cols, dtype=np.int64)[:len(rows)])
    return np.bincount(pairs // max(n, 1), minlength=n).astype(np.int64)


def init_of(deg, by_degree):
    """(rank, parent, order[:z], z) after hpcla_rcm_init: rank inverts by_degree, the z vertices without a neighbour hold the
    numbers 0 .. z - 1 in index order, everything else is unvisited."""
    n = len(deg)
    by_degree = np.asarray(by_degree, dtype=np.int64)
    rank = np.empty(n, dtype=np.int64)
    rank[by_degree] = np.arange(n)
    z = int((np.asarray(deg) == 0).sum())
    parent = np.full(n, UNVISITED, dtype=np.int64)
    parent[by_degree[:z]] = np.arange(z)
    return rank, parent, by_degree[:z].copy(), z


def _expand_into(g_rowptr, g_cols, parent, order, lo, hi):
    """One level on ``parent`` in place: every listed vertex takes the minimum with its lister's number (a vertex numbered
    earlier holds less and keeps it); returns the vertices that were unvisited, ascending.  Repeats change nothing."""
    nbrs, owner = _neighbours_of(g_rowptr, g_cols, order[lo:hi])
    claimed = np.unique(nbrs[parent[nbrs] == UNVISITED])
    np.minimum.at(parent, nbrs, lo + owner)
    return claimed


def expand_of(g_rowptr, g_cols, parent, order, lo, hi):
    """(parent after hpcla_rcm_expand of the level order[lo .. hi), the SET of vertices it claims, ascending)."""
    parent = np.array(parent, dtype=np.int64)
    claimed = _expand_into(np.asarray(g_rowptr, dtype=np.int64), np.asarray(g_cols, dtype=np.int64), parent,
                           np.asarray(order, dtype=np.int64), lo, hi)
    return parent, claimed


def keys_of(cand, parent, rank):
    cand = np.asarray(cand, dtype=np.int64)
    return (np.asarray(parent, dtype=np.int64)[cand] << 32) | np.asarray(rank, dtype=np.int64)[cand]


def number_of(sorted_keys, by_degree):
    return np.asarray(by_degree, dtype=np.int64)[np.asarray(sorted_keys, dtype=np.int64) & 0xffffffff]


def rcm_trace(indptr, indices, frontier_cap=FRONTIER_CAP, candidate_cap=CANDIDATE_CAP):
    """The walk of hp.rcm launch by launch, as linearalgebrampi.jl_amd/rcm.py routes it; the graph may repeat neighbours (degrees
    are the distinct ones, row lengths the stored ones).  Yields dicts, all arrays copies:
      kind "narrow"  one launch of the one-workgroup kernel.  Entered with ``first`` (then lo = hi = cursor = z) or with
                     ``lo, hi, cursor``, and with ``parent`` and ``order``; leaves ``record`` = (lo, hi, cursor, status, levels,
                     starts), ``parent_after`` and ``order_after``.  ``cursor`` is the last found start's position in by_degree
                     plus 1; a launch that finds no start leaves the cursor it was given.  ``marks``: (lo, hi, cursor, levels
                     done, starts done in this launch) whenever a level is about to be expanded or a component has ended.
      kind "wide"    one device-wide level ``lo, hi`` on ``parent`` and ``order``: ``cand`` (the set claimed, ascending),
                     ``parent_after``, ``order_after`` (order[hi : hi + len(cand)] numbered).
    Every dict also has ``deg, by_degree, rank, z``.  Places of ``order`` not yet written hold FREE."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n = len(indptr) - 1
    deg = degrees_of(indptr, indices, True)
    by_degree = np.lexsort((np.arange(n), deg))
    rank, parent, head, z = init_of(deg, by_degree)
    lens = np.diff(indptr)
    order = np.full(n, FREE, dtype=np.int64)
    order[:z] = head
    common = dict(deg=deg, by_degree=by_degree, rank=rank, z=z)
    lo = hi = cursor = z
    first = True
    while n:
        entry = dict(common, kind="narrow", first=first, lo=lo, hi=hi, cursor=cursor, parent=parent.copy(), order=order.copy())
        levels = starts = 0
        marks = []
        while True:
            if hi == lo:                                    # a component ended (or none has begun): the next start
                marks.append((lo, hi, cursor, levels, starts))
                if hi >= n:
                    status = DONE
                    break
                cursor += int(np.flatnonzero(parent[by_degree[cursor:]] == UNVISITED)[0]) + 1
                s = by_degree[cursor - 1]
                parent[s] = hi
                order[hi] = s
                lo, hi = hi, hi + 1
                starts += 1
                levels += 1
            if hi - lo > frontier_cap or int(lens[order[lo:hi]].sum()) > candidate_cap:
                status = WIDE                               # the level is left whole
                break
            marks.append((lo, hi, cursor, levels, starts))
            claimed = _expand_into(indptr, indices, parent, order, lo, hi)
            if len(claimed) == 0:
                lo = hi
                continue
            order[hi:hi + len(claimed)] = number_of(np.sort(keys_of(claimed, parent, rank)), by_degree)
            lo, hi = hi, hi + len(claimed)
            levels += 1
        yield dict(entry, record=(lo, hi, cursor, status, levels, starts), marks=marks, parent_after=parent.copy(),
                   order_after=order.copy())
        first = False
        if status == DONE:
            return
        while True:                                         # one level per pass, as long as the frontier is wide
            state = dict(common, kind="wide", lo=lo, hi=hi, parent=parent.copy(), order=order.copy())
            claimed = _expand_into(indptr, indices, parent, order, lo, hi)
            ncand = len(claimed)
            order[hi:hi + ncand] = number_of(np.sort(keys_of(claimed, parent, rank)), by_degree)
            yield dict(state, cand=claimed, parent_after=parent.copy(), order_after=order.copy())
            if ncand == 0:
                lo = hi
                break
            lo, hi = hi, hi + ncand
            if ncand <= frontier_cap and ncand * len(indices) <= candidate_cap * n:
                break


def trace_facts(trace, n):
    """components, levels, narrow_launches, wide_levels summed from a trace as hp.rcm sums them."""
    narrow = [t for t in trace if t["kind"] == "narrow"]
    wide = [t for t in trace if t["kind"] == "wide"]
    z = trace[0]["z"] if trace else 0
    return dict(components=z + sum(t["record"][5] for t in narrow),
                levels=sum(t["record"][4] for t in narrow) + sum(1 for t in wide if len(t["cand"])),
                narrow_launches=len(narrow), wide_levels=len(wide))


def state_at(final, lo, hi):
    """(parent, order) of a walk that has numbered order[: hi) and no more, from its last launch's ``final``: a vertex's parent
    is final once it is numbered, every other vertex is unvisited."""
    order = final["order_after"].copy()
    parent = np.full(len(order), UNVISITED, dtype=np.int64)
    parent[order[:hi]] = final["parent_after"][order[:hi]]
    order[hi:] = FREE
    return parent, order


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


def _tree(second_level, seed, children=64, more=None):
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
    return _from_edges(first + second_level, i, j, seed) if more is None else more(first + second_level, first, i, j)


def _tree_then_narrow(seed):
    """``_tree(FRONTIER_CAP + 1)`` with three small levels behind the wide one: 10 vertices that two grandchildren each list (so
    the smaller number must win), then 5 that two of those each list, joined in a ring (no vertex but the tail has degree 1).
    The wide level claims 10 vertices, which fit both caps: the one-workgroup kernel is resumed with a frontier of 10 that an
    earlier launch numbered, and walks the level behind it."""
    def more(n, first, i, j):
        a, b = n + np.arange(10), n + 10 + np.arange(5)
        i2 = np.concatenate([i, first + 7 * np.arange(10), first + 2000 + 3 * np.arange(10), a[:5], a[5:], b])
        j2 = np.concatenate([j, a, a, b, b, np.roll(b, 1)])
        return _from_edges(n + 15, i2, j2, seed)
    return _tree(FRONTIER_CAP + 1, seed, more=more)


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


def _path_and_clique(length, seed, clique=6):
    """A path of ``length`` vertices and a clique of 6: the path's vertices (degrees 1 and 2) fill by_degree[: length], the
    clique (degree 5) by_degree[length : length + 6].  The walk starts at a path end, by_degree[0], and leaves the cursor at 1,
    so the scan for the second start passes length - 1 numbered vertices before it meets the clique."""
    c = length + np.arange(clique)
    a, b = np.triu_indices(clique, 1)
    return _from_edges(length + clique, np.concatenate([np.arange(length - 1), c[a]]), np.concatenate([np.arange(1, length), c[b]]), seed)


def _directed_wide(n, edges, both, seed):
    """``edges`` random directed edges, the first ``both`` of them stored the other way as well: in E u E^T as the device builds
    it those neighbours are listed twice, and the doubled lists are long enough for every lane of a group to meet a repeat."""
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, n, edges), rng.integers(0, n, edges)
    return _from_edges(n, np.concatenate([i, j[:both]]), np.concatenate([j, i[:both]]), seed + 1, symmetric=False)


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
    "star_chunk_wrap": lambda: _star(1024 * 256 + 1, 27),    # the centre's row: 1025 chunks of the wide expand, one more than grid.y
    "path1024_k6": lambda: _path_and_clique(1024, 29),       # the second start: the last lane of the scan's first sweep,
    "path1025_k6": lambda: _path_and_clique(1025, 31),       # the first lane of its second,
    "path3000_k6": lambda: _path_and_clique(3000, 33),       # its third sweep
    "nonsymmetric_wide": lambda: _directed_wide(20000, 80000, 40000, 35),
    "tree_then_narrow": lambda: _tree_then_narrow(37),       # a wide level, then the one-workgroup kernel resumed on 10 vertices
}
CASES = list(_BUILDERS)
NONSYMMETRIC_CASES = ["nonsymmetric", "nonsymmetric_wide"]
SYMMETRIC_CASES = [c for c in CASES if c not in NONSYMMETRIC_CASES]
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


@functools.lru_cache(maxsize=None)
def traced(name, doubled=False):
    """(the list rcm_trace yields, (indptr, indices)) of the case's graph -- ``doubled``: of E u E^T with its repeats, as the
    device walks a nonsymmetric pattern; computed once and shared, so nobody writes into it."""
    g = block_graph(matrix(name))
    if doubled:
        g = doubled_graph(*g)
    trace = list(rcm_trace(*g))
    for t in trace:
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return trace, g
