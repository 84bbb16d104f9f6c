"""rcm(): the reverse Cuthill-McKee ordering of a square ``A``, computed on the device; bandwidth(): max |i - j| of a matrix.

``p, info = hp.rcm(A)`` returns this rank's own global rows in their new order (``p[new] = old``, a device int64 tensor), ready
for ``hp.select(A, p, p)``, ``hp.take(b, p)`` and ``hp.put_(x, p, y)``.  Only the structure of ``A`` is read; ``A`` is neither
changed nor hashed, and any element type and both index types are accepted.

The graph is the rank's owned block with the diagonal dropped (entries whose column the rank owns), so the ordering is
rank-local, as ``hp.ilu0`` and ``hp.fsai`` are: every rank permutes its own row range, nothing is communicated and the result
keeps ``A``'s partition.  ``symmetric=True`` is the caller's promise that the pattern is symmetric; the rows are walked as they
are, and a broken promise gives the ordering of the directed graph (still a permutation, its quality not promised).
``symmetric=False`` walks ``E u E^T``, built with the multigrid setup's symmetrise kernels.

The ordering, exactly (tests/_rcm_cases.py restates it in numpy, in the sequential queue form and in this level form):
  1. ``deg[v]`` = the number of neighbours of ``v``; ``by_degree`` = the vertices sorted by ``(deg, index)`` (one stable sort),
     ``rank[v]`` = the position of ``v`` in it;
  2. the vertices without a neighbour take the numbers ``0 .. z - 1`` in index order;
  3. while unnumbered vertices remain, the first unnumbered vertex of ``by_degree`` starts a component and takes the next number
     (there is no pseudo-peripheral search);
  4. level by level, every unnumbered neighbour ``u`` of a level vertex gets ``parent[u]``, the smallest number among the level
     vertices that list it, and the new vertices are numbered in ascending ``(parent[u] << 32) | rank[u]`` -- the order in which
     a queue would append them, each vertex's unvisited neighbours sorted by ``(deg, index)``;
  5. the numbering is reversed: ``p[i] = order[n - 1 - i] + row_start``.

Levels are walked by one of two paths that give the same numbers (csrc/rcm.hip): a single workgroup walks level after level in
one launch while the frontier has at most ``hpcla_rcm_frontier_cap()`` vertices and its degrees sum to at most
``hpcla_rcm_candidate_cap()`` (one read-back of a small record per launch); a level beyond either cap takes three launches over
the whole device, the library-wide ``torch.sort`` of its keys and one 8-byte read-back, and the walk returns to the single
workgroup once a new frontier fits the first cap and, at the graph's mean degree, would fit the second.

Limits: at most 2^31 - 2 rows and fewer than 2^31 graph entries per rank.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi
from .backends import comm_allgather, comm_rank, require_device
from .indexing import _col_indices_dev
from .sparse import HPCSparseMatrix
from .vectors import current_stream_ptr, dptr

_INT32_MAX = 2 ** 31 - 1
_DONE, _WIDE = 0, 1


def _torch():
    import torch
    return torch


@dataclass
class RCMInfo:
    """``components``: connected components of the graph walked (a vertex without a neighbour is one); ``levels``: the BFS levels
    walked over all components with an edge (a start is a level); ``bandwidth_before`` / ``bandwidth_after``: the maximum of
    ``|i - j|`` over the owned block's stored entries in old and in new numbers; ``narrow_launches``: launches of the
    one-workgroup kernel; ``wide_levels``: level expansions that took the device-wide path."""
    components: int = 0
    levels: int = 0
    bandwidth_before: int = 0
    bandwidth_after: int = 0
    narrow_launches: int = 0
    wide_levels: int = 0


def check_arguments(shape, row_partition, col_partition) -> None:
    """The argument rules, on host values only; they hold on every rank alike."""
    if int(shape[0]) != int(shape[1]):
        raise ValueError(f"rcm: the matrix must be square, got {shape[0]} x {shape[1]}")
    if not np.array_equal(np.asarray(row_partition), np.asarray(col_partition)):
        raise ValueError("rcm: A's rows and columns must be partitioned alike")
    rows = np.diff(np.asarray(row_partition, dtype=np.int64))
    if len(rows) and int(rows.max()) >= _INT32_MAX:
        raise ValueError(f"rcm: rank {int(np.argmax(rows))} holds {int(rows.max())} rows; at most 2^31 - 2 per rank")


def _check_entries(nnz: int) -> None:
    if nnz > _INT32_MAX:
        raise ValueError(f"rcm: the owned block's graph has {nnz} entries; at most 2^31 - 1 per rank")


def _structure(A: HPCSparseMatrix):
    rank = comm_rank(A.backend.comm)
    row_start = int(A.row_partition[rank])
    sfx = "i64" if A.Ti == np.dtype(np.int64) else "i32"
    return sfx, row_start, (dptr(A.rowptr_target), dptr(A.colval_target()), dptr(_col_indices_dev(A)), int(A.nrows_local), row_start, 0)


def _graph(A: HPCSparseMatrix, symmetric: bool):
    """(g_rowptr, g_cols, deg, longest row, entries) of the owned block without its diagonal, or of E u E^T."""
    torch = _torch()
    lib = _capi.load()
    dev = A.backend.torch_device
    n = int(A.nrows_local)
    s = current_stream_ptr()
    sfx, _, structure = _structure(A)
    i64 = lambda k: torch.empty(max(k, 1), dtype=torch.int64, device=dev)
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    work = i64(lib.hpcla_rcm_work_bytes(n) // 8)
    g_rowptr = i64(n + 1)
    _capi.call(f"hpcla_rcm_graph_count_{sfx}", *structure, dptr(g_rowptr), dptr(info), dptr(work), s)
    nnz = int(info.item())
    _check_entries(nnz)
    g_cols = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    _capi.call(f"hpcla_rcm_graph_fill_{sfx}", *structure, dptr(g_rowptr), dptr(g_cols), s)
    if not symmetric:                                        # E u E^T: out-lists then in-lists; an edge stored both ways twice
        indeg, u_rowptr = i64(n), i64(n + 1)
        _capi.call("hpcla_amg_symmetrise_count", dptr(g_rowptr), dptr(g_cols), n, dptr(indeg), dptr(u_rowptr), dptr(info), dptr(work), s)
        nnz = int(info.item())
        _check_entries(nnz)
        u_cols = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        _capi.call("hpcla_amg_symmetrise_fill", dptr(g_rowptr), dptr(g_cols), n, dptr(u_rowptr), dptr(indeg), dptr(u_cols), s)
        g_rowptr, g_cols = u_rowptr, u_cols
    deg = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _capi.call("hpcla_rcm_degrees", dptr(g_rowptr), dptr(g_cols), n, 0 if symmetric else 1, dptr(deg), s)
    longest = int((g_rowptr[1:n + 1] - g_rowptr[:n]).max().item()) if n else 0
    return g_rowptr, g_cols, deg[:n], longest, nnz


def _rcm(A: HPCSparseMatrix, symmetric: bool = True, timings: Optional[dict] = None):
    """``rcm`` proper.  ``timings`` (a dict) receives host seconds of the graph, the narrow launches and the wide levels, each
    taken between the read-backs that end them."""
    if not isinstance(A, HPCSparseMatrix):
        raise TypeError("rcm: an HPCSparseMatrix is required")
    check_arguments(A.shape, A.row_partition, A.col_partition)
    require_device(A.backend, "rcm")
    torch = _torch()
    lib = _capi.load()
    dev = A.backend.torch_device
    n = int(A.nrows_local)
    info = RCMInfo()
    p = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return p, info
    s = current_stream_ptr()
    row_start = int(A.row_partition[comm_rank(A.backend.comm)])
    t0 = time.perf_counter()
    g_rowptr, g_cols, deg, longest, nnz = _graph(A, bool(symmetric))
    by_degree = torch.sort(deg, stable=True).indices.to(torch.int32)        # plumbing: (deg, index) ascending
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)
    rank, parent, order, inv = i32(), i32(), i32(), i32()
    words = torch.zeros(16, dtype=torch.int64, device=dev)                  # z | count | before, after | the record
    z_dev, count, bands, record = words[0:1], words[1:2], words[2:4], words[8:14]
    _capi.call("hpcla_rcm_init", dptr(deg), dptr(by_degree), n, dptr(rank), dptr(parent), dptr(order), dptr(z_dev), s)
    frontier_cap, candidate_cap = int(lib.hpcla_rcm_frontier_cap()), int(lib.hpcla_rcm_candidate_cap())
    graph = (dptr(g_rowptr), dptr(g_cols))
    cand = keys = None
    first = dptr(z_dev)
    lo = hi = cursor = 0
    starts = 0
    t_narrow = t_wide = 0.0
    if timings is not None:
        torch.cuda.synchronize()
    t1 = time.perf_counter()
    while True:
        _capi.call("hpcla_rcm_narrow", *graph, dptr(by_degree), dptr(rank), n, lo, hi, cursor, first, dptr(parent), dptr(order),
                   dptr(record), s)
        first = None
        lo, hi, cursor, status, levels, began = (int(v) for v in record.tolist())
        info.narrow_launches += 1
        info.levels += levels
        starts += began
        t2 = time.perf_counter()
        t_narrow += t2 - t1
        t1 = t2
        if status == _DONE:
            break
        if status != _WIDE:
            raise RuntimeError("rcm: the walk found no unnumbered vertex although some remain")
        if cand is None:
            cand, keys = i32(), torch.empty(n, dtype=torch.int64, device=dev)
        while True:                                                          # one level per pass, as long as the frontier is wide
            _capi.call("hpcla_rcm_expand", *graph, n, dptr(order), lo, hi, longest, dptr(parent), dptr(cand), dptr(count), s)
            ncand = int(count.item())
            info.wide_levels += 1
            if ncand == 0:                                                   # the component is complete
                lo = hi
                break
            _capi.call("hpcla_rcm_keys", dptr(cand), ncand, n, dptr(parent), dptr(rank), dptr(keys), s)
            ordered = torch.sort(keys[:ncand]).values                        # distinct keys: no stability needed
            _capi.call("hpcla_rcm_number", dptr(ordered), ncand, n, dptr(by_degree), hi, dptr(order), s)
            info.levels += 1
            lo, hi = hi, hi + ncand
            # back to the one-workgroup kernel when the new frontier fits and, at the graph's mean degree, its degree sum
            # would: a guess that costs a bounced launch or a wide level when wrong, never an output element
            if ncand <= frontier_cap and ncand * nnz <= candidate_cap * n:
                break
        t2 = time.perf_counter()
        t_wide += t2 - t1
        t1 = t2
    _capi.call("hpcla_rcm_finish", dptr(order), n, row_start, dptr(p), dptr(inv), s)
    _capi.call("hpcla_rcm_graph_bandwidth", *graph, n, None, dptr(bands[0:1]), s)
    _capi.call("hpcla_rcm_graph_bandwidth", *graph, n, dptr(inv), dptr(bands[1:2]), s)
    z, _, before, after = (int(v) for v in words[0:4].tolist())
    info.components = starts + z
    info.bandwidth_before, info.bandwidth_after = before, after
    if timings is not None:
        timings.update(graph=t1 - t0 - t_narrow - t_wide, narrow=t_narrow, wide=t_wide, finish=time.perf_counter() - t1)
    return p, info


def rcm(A: HPCSparseMatrix, symmetric: bool = True):
    """``p, info = rcm(A)``: the reverse Cuthill-McKee ordering of this rank's owned block of the square ``A`` (see the module
    docstring for the exact rule).  ``p``: a device int64 tensor, ``p[new] = old`` in global 0-based rows, this rank's own;
    ``info``: an ``RCMInfo``.  Raises ValueError, on every rank alike, for a non-square ``A``, for row and column partitions
    that differ and for a rank with more than 2^31 - 2 rows; a rank whose graph exceeds 2^31 - 1 entries raises it alone
    (nothing here is collective, so no rank waits for it)."""
    return _rcm(A, symmetric)


def bandwidth(A: HPCSparseMatrix) -> int:
    """The maximum of ``|i - j|`` over all stored entries of ``A`` in global numbers (0 for an empty matrix), reduced to a
    maximum over the ranks: collective."""
    if not isinstance(A, HPCSparseMatrix):
        raise TypeError("bandwidth: an HPCSparseMatrix is required")
    require_device(A.backend, "bandwidth")
    torch = _torch()
    out = torch.zeros(1, dtype=torch.int64, device=A.backend.torch_device)
    sfx, _, structure = _structure(A)
    _capi.call(f"hpcla_bandwidth_{sfx}", *structure, dptr(out), current_stream_ptr())
    return int(comm_allgather(A.backend.comm, np.array([int(out.item())], dtype=np.int64)).max())
