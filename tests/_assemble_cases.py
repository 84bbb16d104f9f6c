"""Case generators and the numpy restatement of COO assembly (linearalgebrampi.jl_amd/assemble.py, csrc/assemble.hip), with
the order of the additions explicit.

The restatement: a STABLE argsort of the keys ``(row - row_lo) * ncols + col`` lists every output entry's contributions in
ascending position of the value list.  Sums are formed in rounds: round r adds the r-th contribution of every list that has
one, so each list is summed strictly left to right, started from its first value and not from 0.0.  The chunk rule: a list
longer than ``CH`` is cut into consecutive chunks of ``CH`` contributions; each chunk is summed by rounds, then the chunks'
partial sums are summed by rounds, in chunk order.  A list without contributions (the vector form) gives +0.0.

tests/test_assemble_cases.py holds this file against scipy; tests/test_gpu_assemble.py holds the kernels against this file,
bit for bit."""
import numpy as np

CH = 512                      # hpcla_assemble_chunk(): asserted against the library by the GPU tests
RUN = 1024                    # hpcla_assemble_run(): output entries per workgroup
PASS = 2048                   # hpcla_assemble_pass(): contributions per LDS pass
SCAN_CHUNK = 1024             # hpcla_submatrix_scan_chunk()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _sum_lists(v, start, length):
    """out[k] = v[start[k]] + v[start[k] + 1] + ... left to right over length[k] values, by rounds; +0.0 for length 0."""
    out = np.zeros(len(start), dtype=np.float64)
    if len(start) == 0:
        return out
    has = length > 0
    out[has] = v[start[has]]
    with np.errstate(invalid="ignore"):                             # Inf + (-Inf) is a case, not a mistake
        for r in range(1, int(length.max())):
            idx = np.flatnonzero(length > r)
            out[idx] = out[idx] + v[start[idx] + r]
    return out


def sum_segments(v_sorted, seg_ptr, ch=CH):
    """The sums of the lists v_sorted[seg_ptr[k]:seg_ptr[k + 1]] in the library's order (chunks of ``ch``)."""
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    nseg = len(seg_ptr) - 1
    length = np.diff(seg_ptr)
    nch = (length + ch - 1) // ch                                   # 0 for an empty list
    first = np.cumsum(nch) - nch
    seg_of = np.repeat(np.arange(nseg, dtype=np.int64), nch)
    c = np.arange(int(nch.sum()), dtype=np.int64) - first[seg_of]
    cstart = seg_ptr[seg_of] + c * ch
    clen = np.minimum(cstart + ch, seg_ptr[seg_of + 1]) - cstart
    partial = _sum_lists(np.asarray(v_sorted, dtype=np.float64), cstart, clen)
    return _sum_lists(partial, first, nch)


def inverted_index(keys):
    """(perm, seg_ptr, ukeys): the stable order of the keys, the cuts where the sorted key changes, the distinct keys."""
    keys = np.asarray(keys, dtype=np.int64)
    perm = np.argsort(keys, kind="stable")
    sk = keys[perm]
    head = np.ones(len(sk), dtype=bool)
    head[1:] = sk[1:] != sk[:-1]
    seg_ptr = np.concatenate([np.flatnonzero(head), [len(sk)]]).astype(np.int64)
    return perm, seg_ptr, sk[head]


def assemble_ref(rows, cols, vals, shape, row_lo=0, row_hi=None, ch=CH):
    """The CSR (rowptr, global cols, vals) of the rows [row_lo, row_hi) assembled from a value list whose triplets all lie in
    those rows."""
    m, n = shape
    row_hi = m if row_hi is None else row_hi
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    perm, seg_ptr, uk = inverted_index((rows - row_lo) * n + cols)
    out = sum_segments(np.asarray(vals, dtype=np.float64)[perm], seg_ptr, ch)
    rowptr = np.searchsorted(uk // n, np.arange(row_hi - row_lo + 1), side="left").astype(np.int64)
    return rowptr, uk % n, out


def assemble_vector_ref(idx, vals, n, lo=0, hi=None, ch=CH):
    hi = n if hi is None else hi
    keys = np.asarray(idx, dtype=np.int64) - lo
    perm = np.argsort(keys, kind="stable")
    seg_ptr = np.searchsorted(keys[perm], np.arange(hi - lo + 1), side="left")
    return sum_segments(np.asarray(vals, dtype=np.float64)[perm], seg_ptr, ch)


# -- generators -------------------------------------------------------------------------------------------------------
def values_for(n, seed, kind="random"):
    rng = np.random.default_rng(seed)
    if kind == "integer":
        return rng.integers(-40, 41, n).astype(np.float64)
    if kind == "dyadic":
        return rng.integers(-2048, 2049, n).astype(np.float64) / 64.0
    return rng.standard_normal(n) * np.exp(rng.uniform(-6.0, 6.0, n))


def planted_lengths(lengths, shape, seed, shuffle=True):
    """Triplets in which entry k (distinct positions, drawn at random) has ``lengths[k]`` contributions."""
    rng = np.random.default_rng(seed)
    m, n = shape
    cells = rng.choice(m * n, size=len(lengths), replace=False)
    keys = np.repeat(cells, lengths)
    if shuffle:
        keys = keys[rng.permutation(len(keys))]
    return (keys // n).astype(np.int64), (keys % n).astype(np.int64)


def edge_lengths():
    """1, 2, the wave and workgroup edges, the chunk edges, one of 5 000, planted among short ones."""
    special = [1, 2, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 1, 5000]
    rng = np.random.default_rng(11)
    out = []
    for L in special:
        out += list(rng.integers(1, 4, 7)) + [L]
    return np.array(out + [1, 3, 2], dtype=np.int64)


def random_coo(n_in, shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, shape[0], n_in).astype(np.int64), rng.integers(0, shape[1], n_in).astype(np.int64)


# -- the P1 fixture ---------------------------------------------------------------------------------------------------
P1_ELEMENT = np.array([[1.0, -0.5, -0.5], [-0.5, 0.5, 0.0], [-0.5, 0.0, 0.5]])    # right angle at the first vertex; dyadic


def p1_triangles(nx, ny):
    """Right isosceles triangles of an nx x ny grid of nodes (node (i, j) -> i + nx * j), two per cell, the right angle
    first.  int64 [2 (nx - 1)(ny - 1), 3], in natural element order."""
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i + nx * j).T.ravel()
    b, c, d = a + 1, a + nx, a + nx + 1
    tri = np.empty((2 * len(a), 3), dtype=np.int64)
    tri[0::2] = np.stack([a, b, c], axis=1)
    tri[1::2] = np.stack([d, c, b], axis=1)
    return tri


def p1_triplets(nx, ny, coeff=None, identity=True):
    """Element contributions (9 per triangle, element by element) of -div(k grad u) with k constant per element (``coeff``,
    default 1), then one unit triplet per diagonal."""
    tri = p1_triangles(nx, ny)
    k = np.ones(len(tri)) if coeff is None else np.asarray(coeff, dtype=np.float64)
    rows = np.repeat(tri, 3, axis=1).ravel()
    cols = np.tile(tri, (1, 3)).ravel()
    vals = (k[:, None] * P1_ELEMENT.ravel()[None, :]).ravel()
    if identity:
        d = np.arange(nx * ny, dtype=np.int64)
        rows, cols, vals = np.concatenate([rows, d]), np.concatenate([cols, d]), np.concatenate([vals, np.ones(nx * ny)])
    return rows.astype(np.int64), cols.astype(np.int64), vals


def p1_expected(nx, ny):
    """The same operator written down edge by edge, without elements: an axis-parallel edge weighs half the number of
    triangles that contain it (1 inside, 1/2 on the boundary), a cell's diagonal b-c is stored with weight 0, the diagonal
    entry is the sum of a node's edge weights plus one.  Inside the grid a row is the 5-point stencil -1 -1 5 -1 -1."""
    import scipy.sparse as sp
    N = nx * ny
    r, c, v = [], [], []

    def edge(p, q, w):
        r.extend([p, q, p, q]); c.extend([q, p, p, q]); v.extend([-w, -w, w, w])
    for j in range(ny):
        for i in range(nx):
            p = i + nx * j
            if i + 1 < nx:
                edge(p, p + 1, 0.5 * ((j > 0) + (j + 1 < ny)))
            if j + 1 < ny:
                edge(p, p + nx, 0.5 * ((i > 0) + (i + 1 < nx)))
            if i + 1 < nx and j + 1 < ny:
                edge(p + 1, p + nx, 0.0)
    d = np.arange(N)
    A = sp.coo_matrix((np.concatenate([v, np.ones(N)]), (np.concatenate([r, d]), np.concatenate([c, d]))), shape=(N, N)).tocsr()
    A.sort_indices()
    return A


def element_partition_triplets(nx, ny, nranks, rank, coeff=None):
    """The P1 triplets of the elements with index in rank's contiguous share of the element list (rank 0 also adds the
    identity): rows on the seam between two shares belong to one rank and receive from the other."""
    tri = p1_triangles(nx, ny)
    ne = len(tri)
    lo, hi = (ne * rank) // nranks, (ne * (rank + 1)) // nranks
    k = np.ones(ne) if coeff is None else np.asarray(coeff, dtype=np.float64)
    t = tri[lo:hi]
    rows = np.repeat(t, 3, axis=1).ravel()
    cols = np.tile(t, (1, 3)).ravel()
    vals = (k[lo:hi, None] * P1_ELEMENT.ravel()[None, :]).ravel()
    if rank == 0:
        d = np.arange(nx * ny, dtype=np.int64)
        rows, cols, vals = np.concatenate([rows, d]), np.concatenate([cols, d]), np.concatenate([vals, np.ones(nx * ny)])
    return rows.astype(np.int64), cols.astype(np.int64), vals


def rank_value_list(all_triplets, part, rank):
    """The value list of ``rank`` in the stated order: its own triplets in input order (those of its rows), then the ones
    received, in ascending sender rank, each in the sender's order.  ``all_triplets[r]`` = rank r's (rows, cols, vals).
    Returns (rows, cols, vals) of the list."""
    lo, hi = int(part[rank]), int(part[rank + 1])
    R, C, V = [], [], []
    for r in [rank] + [q for q in range(len(all_triplets)) if q != rank]:
        rows, cols, vals = all_triplets[r]
        keep = (rows >= lo) & (rows < hi)
        R.append(rows[keep]); C.append(cols[keep]); V.append(vals[keep])
    return np.concatenate(R), np.concatenate(C), np.concatenate(V)
