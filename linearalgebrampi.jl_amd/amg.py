"""amg(): the smoothed-aggregation algebraic multigrid preconditioner: of a symmetric positive definite ``A`` for ``hp.cg``, and
with ``symmetric=False`` of a nonsymmetric ``A`` with a positive diagonal for ``hp.gmres`` and ``hp.bicgstab``.

Level setup (csrc/amg.hip for what the library's products do not cover), repeated on the current level's ``A``:
  weight      rho = max_i sum_j |a_ij| / a_ii over whole rows (a max across ranks), w = 4 / (3 rho), s = w ./ diag(A)
  strength    (i, j) kept when j != i, j owned by this rank, a_ij != 0 and |a_ij| >= theta sqrt(a_ii a_jj): device CSR
  roots       a distance-2 maximal independent set over keyed rows, three launches a round, the host reads the rows left
  join        non-roots take the neighbouring root (then the neighbour's) with the largest key; ids by a scan of the root flags,
              plus the rank's offset: aggregates never cross ranks and a level's setup exchanges nothing but sizes
  stall       the level is the last one when the aggregates number >= 0.8 n
  P           T (one 1.0 per row at its aggregate), A T by ``spgemm``, p_ij = [j == agg(i)] - s_i (A T)_ij,
              Pt = transpose(P), A_c = Pt (A P) (the rows of Pt split into runs where the product is over spgemm's bound)
  last level  n <= coarse_size: the inverse of the symmetrised matrix, formed once on the host, an HPCMatrix applied by the
              dense mat-vec; else ``coarse_sweeps`` damped Jacobi sweeps from zero

The cycle is a symmetric V(1,1): x = s .* b, r = b - A x, x += P cycle(R r), x += s .* (b - A x) with R = Pt; ``M`` is positive
definite.  Its SpMVs are the ordinary ones on ordinary plans; x = s .* b and x += s .* (b - t) are fused kernels of csrc/amg.hip.

``symmetric=False`` changes three steps of a level and nothing else (rho bounds the spectral radius of D^-1 A for any A with a
positive diagonal, so the weights and the smoother stay):
  strength    the graph becomes E u E^T (E: the graph above), built on the device from E's own CSR: the independent set and the
              join assume an undirected graph (on a directed one rows that do not see each other all become roots: on an
              out-star every leaf, two edges from every other leaf, so the set is not independent and aggregates degenerate).  The
              threshold is symmetric in i and j, so this is max(|a_ij|, |a_ji|) >= theta sqrt(a_ii a_jj) with an entry that is
              not stored counting as 0.  Ghost columns stay out both ways.
  R           the Petrov-Galerkin restriction Tt (I - A S), S = diag(s): Tt A by ``spgemm`` (its rows split like those of Pt
              below where the product is over the bound), r_cj = [agg(j) == c] - (Tt A)_cj s_j; A_c = R (A P).  ``Pt`` is not
              formed.  On a symmetric A the first level's R has the bits of Pt.
  last level  the inverse of the coarse matrix itself.
The cycle is then a fixed linear operator that is not symmetric: right-preconditioned GMRES and BiCGStab take it, ``cg`` refuses it.

Limits: Float64; ``cg`` for ``A`` symmetric positive definite, ``gmres`` / ``bicgstab`` for either mode; a positive stored diagonal
on every level (a strongly convective or non-M-matrix ``A`` can give a coarse diagonal that is not: the setup raises), rows and
columns partitioned alike, one rank (the aggregation is rank-local and runs on several; the products and transposes of the
setup move values between ranks through RCCL only, so the hierarchy across ranks waits for a transport that ranks sharing a GPU
have too).

``B=`` (an HPCVector, or an HPCMatrix of k <= 8 columns, on A's rows) gives the near-nullspace candidates the tentative prolongator
is fitted to: ``1 ./ d`` for a scaled scalar problem ``D A D``, the rigid-body modes for elasticity.  Without it T is the
constant's, one 1.0 per row, and every launch is the one it was.  With it a level changes in these steps and no other:
  unknowns    k per aggregate, the coarse unknown k agg + c; ``coarse_partition`` is k times the aggregates'; the aggregation
              itself runs on the rows of A as before (on unknowns: it is not node-blocked)
  stall       k n_aggregates >= 0.8 n, decided after the fit: every aggregation made is checked for dropped columns, also the
              one of a level that then stalls (few members per aggregate is what makes a level stall and a column drop)
  members     the rows of every aggregate in ascending order: a stable sort of the aggregate ids, the pointer from a bincount
  fit         per aggregate B[members, :] = Q R (csrc/amg.hip: hpcla_amg_fit_f64, whose arithmetic is part of the method): Q
              fills the dense n x k ``Tv``, R the rows k a .. k a + k - 1 of the next level's candidates.  A column that is
              dropped (an aggregate with fewer members than candidates, candidates that are dependent on it, a zero column, a
              NaN) is an error: ValueError on every rank, naming the first member's global row
  T           k stored entries per row, columns k agg(i) .. k agg(i) + k - 1, values Tv[i, :], exact zeros stored
  P, R        T - diag(s) (A T) and, with ``symmetric=False``, Tt - (Tt A) diag(s), on the patterns of A T and Tt A
The candidates are not smoothed, and ``hp.spgemm``'s bound on the candidate products of an output row is reached k times sooner
(the split into runs and its NotImplementedError apply unchanged).
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from . import _capi
from .sparse import HPCSparseMatrix, HPCSparseMatrix_local_device, get_vector_plan, mul_
from .vectors import HPCVector, current_stream_ptr, dptr, f64_only, rd16, wr16

STALL = 0.8
MAX_ROUNDS = 64
MAX_COARSE_SIZE = 1024


def _torch():
    import torch
    return torch


MAX_CANDIDATES = 8             # AMG_G of csrc/amg.hip: the lanes of the group that fits an aggregate


def check_arguments(T, shape, row_partition, col_partition, theta=0.0, max_levels=12, coarse_size=128, coarse_sweeps=4,
                    symmetric=True, B=None) -> None:
    """The argument rules, on host values only: ``T`` the element type, ``shape`` and the partitions A's; ``B`` None or the
    candidates' (element type, global shape (rows, k), row partition)."""
    if not isinstance(symmetric, (bool, np.bool_)):
        raise TypeError(f"amg: symmetric must be a bool, got {symmetric!r}")
    if np.dtype(T) != np.dtype(np.float64):
        raise TypeError("amg: offered for Float64 backends only")
    if int(shape[0]) != int(shape[1]):
        raise ValueError(f"amg: the matrix must be square, got {shape[0]} x {shape[1]}")
    if not np.array_equal(np.asarray(row_partition), np.asarray(col_partition)):
        raise ValueError("amg: A's rows and columns must be partitioned alike")
    if not (0.0 <= float(theta) < 1.0):
        raise ValueError(f"amg: theta must lie in [0, 1), got {theta}")
    if int(max_levels) < 1:
        raise ValueError("amg: max_levels must be at least 1")
    if not (1 <= int(coarse_size) <= MAX_COARSE_SIZE):
        raise ValueError(f"amg: coarse_size must lie in 1..{MAX_COARSE_SIZE}")
    if int(coarse_sweeps) < 1:
        raise ValueError("amg: coarse_sweeps must be at least 1")
    if B is not None:
        TB, shape_B, partition_B = B
        if np.dtype(TB) != np.dtype(np.float64):
            raise TypeError("amg: the candidates B must be Float64")
        if not (1 <= int(shape_B[1]) <= MAX_CANDIDATES):
            raise ValueError(f"amg: B must have 1..{MAX_CANDIDATES} columns, got {shape_B[1]}")
        if int(shape_B[0]) != int(shape[0]):
            raise ValueError(f"amg: B has {shape_B[0]} rows, A has {shape[0]}")
        if not np.array_equal(np.asarray(partition_B), np.asarray(row_partition)):
            raise ValueError("amg: B must be partitioned like the rows of A")


class AMGLevel:
    """One level: ``A``, the smoother ``s`` (an HPCVector) with its weight ``w`` and ``rho``, ``n`` (global rows), and on every
    level but the last ``P``, ``R`` (the restriction: ``Pt`` itself in the symmetric mode; in the other ``Pt`` stays None),
    ``aggregates`` (global ids of the local rows, a device tensor), ``n_roots`` (this rank's), ``coarse_partition``, and the
    runs the two products were split into (``galerkin``; ``restriction_split`` for ``Tt A``, nonsymmetric mode only).  A level
    that stalled keeps its aggregation.  The last level has ``inverse`` (an HPCMatrix: this rank's rows of the dense inverse)
    or ``sweeps``.  Built with ``B=``: ``candidates`` (this level's n_local x k block, a row-major device tensor) and, where
    the level has a P, ``Tv`` (n_local x k: row i holds the k values of row i of T) and ``T``; None otherwise."""

    def __init__(self, A: HPCSparseMatrix):
        self.A = A
        self.n = int(A.shape[0])
        self.candidates = self.Tv = self.T = None
        self.s = self.w = self.rho = None
        self.P = self.Pt = self.R = self.aggregates = self.coarse_partition = self.inverse = None
        self.n_roots = self.rounds = self.sweeps = self.galerkin = self.restriction_split = None


class AMGWorkspace:
    """The vectors of a cycle: per level x, b (the coarse ones), t (where the level multiplies by its A) and r / e (where it has a
    P).  One per user of a hierarchy: a ``PCGWorkspace`` holds its own next to its solve vectors (two solves with one hierarchy
    do not share any), a ``GMRESWorkspace`` and a ``BiCGStabWorkspace`` likewise; ``AMG.apply`` uses the hierarchy's unless it is
    given one."""

    def __init__(self, levels: List[AMGLevel]):
        mk = lambda lvl: HPCVector.zeros(lvl.A.row_partition, lvl.A.backend)
        self.x = [mk(l) for l in levels]
        self.b = [None] + [mk(l) for l in levels[1:]]
        self.t = [mk(l) if l.inverse is None else None for l in levels]
        self.r = [mk(l) if l.P is not None else None for l in levels]


class AMG:
    """The hierarchy.  ``levels``: AMGLevel objects, fine to coarse; ``operator_complexity``: the stored entries of every
    level's A over those of the first (global counts); ``symmetric``: the mode it was built in; ``candidates_per_aggregate``:
    the columns of ``B`` (None without)."""

    def __init__(self, levels: List[AMGLevel], operator_complexity: float, symmetric: bool = True,
                 candidates_per_aggregate: Optional[int] = None):
        self.levels = levels
        self.operator_complexity = float(operator_complexity)
        self.symmetric = bool(symmetric)
        self.candidates_per_aggregate = candidates_per_aggregate
        self._work: Optional[AMGWorkspace] = None

    def workspace(self) -> AMGWorkspace:
        """The vectors ``apply`` works in: calls of ``apply`` on one hierarchy must follow each other on one stream."""
        if self._work is None:
            self._work = AMGWorkspace(self.levels)
        return self._work

    def apply(self, r: HPCVector, out: Optional[HPCVector] = None, workspace: Optional[AMGWorkspace] = None) -> HPCVector:
        """``out = M r``: one V(1,1) cycle from zero; r on A's row partition.  ``workspace``: the level vectors to work in (the
        solvers pass their own); the hierarchy's by default."""
        ws = self.workspace() if workspace is None else workspace
        if r.structural_hash != ws.x[0].structural_hash:
            raise ValueError("amg: r must be partitioned like the rows of A")
        out = r.similar() if out is None else out
        rv, (xv, land) = rd16(r.v), wr16(out.v)              # the smoother kernels read and write 16 bytes at a time
        wrap = lambda v, t: v if t is v.v else HPCVector(v.structural_hash, v.partition, t, v.backend)
        self._cycle(0, wrap(r, rv), wrap(out, xv), ws)
        land()
        return out

    def _cycle(self, k: int, b: HPCVector, x: HPCVector, ws: AMGWorkspace) -> None:
        lvl = self.levels[k]
        n, s = b.local_length, current_stream_ptr()
        if lvl.inverse is not None:
            from .dense import dense_matvec
            dense_matvec(lvl.inverse, b, y=x)
            return
        t = ws.t[k]
        _capi.call("hpcla_amg_presmooth_f64", dptr(lvl.s.v), dptr(b.v), dptr(x.v), n, s)                 # x = s .* b
        if lvl.P is None:
            for _ in range(lvl.sweeps - 1):
                mul_(t, lvl.A, x)
                _capi.call("hpcla_amg_postsmooth_f64", dptr(lvl.s.v), dptr(b.v), dptr(t.v), dptr(x.v), n, s)
            return
        r = ws.r[k]
        mul_(t, lvl.A, x)                                                                                  # t = A x
        _capi.call("hpcla_axpby_f64", 1.0, dptr(b.v), -1.0, dptr(t.v), dptr(r.v), n, s)                    # r = b - t
        mul_(ws.b[k + 1], lvl.R, r)                                                                        # bc = R r
        self._cycle(k + 1, ws.b[k + 1], ws.x[k + 1], ws)
        mul_(r, lvl.P, ws.x[k + 1])                                                                        # e = P xc
        _capi.call("hpcla_axpy_f64", 1.0, None, None, dptr(r.v), dptr(x.v), n, s)                          # x += e
        mul_(t, lvl.A, x)                                                                                  # t = A x
        _capi.call("hpcla_amg_postsmooth_f64", dptr(lvl.s.v), dptr(b.v), dptr(t.v), dptr(x.v), n, s)      # x += s .* (b - t)


def _raise_together(backend, local_row: int, row_start: int, message) -> None:
    """``local_row`` < 0: this rank has nothing to report.  Every rank raises ValueError for the smallest global row."""
    from .backends import comm_allgather
    mine = -1 if local_row < 0 else row_start + local_row
    every = comm_allgather(backend.comm, np.array([mine], dtype=np.int64))
    bad = every[every >= 0]
    if len(bad):
        raise ValueError(message(int(bad.min())))


def _weights(lvl: AMGLevel, plan, sfx: str, row_start: int):
    """diag(A) on the device, s = w ./ diag(A); raises on every rank for a diagonal that is not positive."""
    from .partition import compute_partition_hash
    from .vectors import maximum
    torch = _torch()
    A = lvl.A
    backend, dev, n = A.backend, A.backend.torch_device, A.nrows_local
    diag = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
    ratio = torch.zeros(n, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    s = current_stream_ptr()
    _capi.call(f"hpcla_amg_weights_f64_{sfx}", dptr(plan.rowptr_of(A)), dptr(plan.colval_split), dptr(A.nzval), n, plan.n_own, 0,
               dptr(diag), dptr(ratio), dptr(info), s)
    _raise_together(backend, int(info.item()), row_start,
                    lambda row: f"amg: the diagonal of row {row} is not positive (level of {lvl.n} rows)")
    h = compute_partition_hash(A.row_partition)
    lvl.rho = maximum(HPCVector(h, A.row_partition, ratio, backend))
    lvl.w = 4.0 / (3.0 * lvl.rho)
    sv = torch.zeros(n, dtype=torch.float64, device=dev)
    _capi.call("hpcla_amg_smoother_f64", lvl.w, dptr(diag), dptr(sv), n, s)
    lvl.s = HPCVector(h, A.row_partition, sv, backend)
    return diag


def _aggregate(lvl: AMGLevel, plan, sfx: str, diag, theta: float, row_start: int, symmetric: bool = True) -> None:
    """Strength graph (E u E^T unless ``symmetric``), roots, join, numbering: fills lvl.aggregates, lvl.n_roots, lvl.rounds,
    lvl.coarse_partition."""
    from .backends import comm_allgather, comm_rank
    torch = _torch()
    lib = _capi.load()
    A = lvl.A
    backend, dev, n = A.backend, A.backend.torch_device, A.nrows_local
    s = current_stream_ptr()
    i64 = lambda k, fill=0: torch.full((max(k, 1),), fill, dtype=torch.int64, device=dev)
    work = i64(lib.hpcla_amg_work_bytes(n) // 8)
    info = i64(2)
    s_rowptr = i64(n + 1)
    structure = (dptr(plan.rowptr_of(A)), dptr(plan.colval_split), dptr(A.nzval), dptr(diag), n, plan.n_own, 0, float(theta))
    _capi.call(f"hpcla_amg_strength_count_f64_{sfx}", *structure, dptr(s_rowptr), dptr(info), dptr(work), s)
    s_cols = torch.empty(max(int(info[0].item()), 1), dtype=torch.int32, device=dev)      # the size the graph is allocated by
    _capi.call(f"hpcla_amg_strength_fill_f64_{sfx}", *structure, dptr(s_rowptr), dptr(s_cols), s)
    if not symmetric:                                        # E u E^T: in-degrees, the combined row pointer, out-lists then in-lists
        indeg, u_rowptr = i64(n), i64(n + 1)
        _capi.call("hpcla_amg_symmetrise_count", dptr(s_rowptr), dptr(s_cols), n, dptr(indeg), dptr(u_rowptr), dptr(info), dptr(work), s)
        u_cols = torch.empty(max(int(info[0].item()), 1), dtype=torch.int32, device=dev)
        _capi.call("hpcla_amg_symmetrise_fill", dptr(s_rowptr), dptr(s_cols), n, dptr(u_rowptr), dptr(indeg), dptr(u_cols), s)
        s_rowptr, s_cols = u_rowptr, u_cols

    key, m1, m2, state, state_next = (i64(n) for _ in range(5))
    counts = i64(lib.hpcla_amg_round_blocks(n))
    _capi.call("hpcla_amg_mis_init", n, row_start, dptr(key), dptr(state), s)
    rounds = 0
    while True:                                              # a rank's set is its own: no rank waits for another here
        if rounds == MAX_ROUNDS:
            raise RuntimeError("amg: the independent set did not finish in 64 rounds")
        _capi.call("hpcla_amg_mis_round", dptr(s_rowptr), dptr(s_cols), n, dptr(key), dptr(state), dptr(m1), dptr(m2),
                   dptr(state_next), dptr(counts), s)
        state, state_next = state_next, state
        rounds += 1
        if n == 0 or int(counts.sum().item()) == 0:          # the one read-back of a round
            break
    owner_a = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    owner_b = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    rootid = i64(n)
    _capi.call("hpcla_amg_join", dptr(s_rowptr), dptr(s_cols), n, dptr(key), dptr(state), dptr(owner_a), dptr(owner_b), dptr(rootid),
               dptr(info), dptr(work), s)
    lost, n_roots = (int(v) for v in info.cpu().tolist())
    if lost != -1:
        raise RuntimeError(f"amg: local row {lost} was left without an aggregate")
    every = comm_allgather(backend.comm, np.array([n_roots], dtype=np.int64))
    lvl.coarse_partition = np.concatenate([[0], np.cumsum(every)]).astype(np.int64)
    lvl.n_roots, lvl.rounds = n_roots, rounds
    agg = torch.empty(n, dtype=torch.int64, device=dev)
    _capi.call("hpcla_amg_aggregate_ids", dptr(owner_b), dptr(rootid), n, int(lvl.coarse_partition[comm_rank(backend.comm)]),
               dptr(agg), s)
    lvl.aggregates = agg


def _restrictor(lvl: AMGLevel, T: HPCSparseMatrix, lo: int, k: Optional[int] = None) -> HPCSparseMatrix:
    """R = Tt (I - A S) on the pattern of Tt A (one rank: every column of Tt A is a local row of the level).  ``k``: the
    candidates per aggregate of a level with ``Tv``; ``lo`` is then the rank's first coarse unknown."""
    from .indexing import _col_indices_dev
    from .transpose import transpose
    A = lvl.A
    Tt = transpose(T).materialize()
    TA, lvl.restriction_split = _split_product(Tt, A, 1, lvl, "restriction")
    vals = _torch().zeros_like(TA.nzval)
    sfx = "i64" if TA.Ti == np.dtype(np.int64) else "i32"
    pattern = (dptr(TA.rowptr_target), dptr(TA.colval_target()), dptr(_col_indices_dev(TA)), dptr(TA.nzval), dptr(lvl.aggregates),
               dptr(lvl.s.v))
    if k is None:
        _capi.call(f"hpcla_amg_restrictor_f64_{sfx}", *pattern, TA.nrows_local, A.nrows_local, lo, 0, dptr(vals),
                   current_stream_ptr())
    else:
        _capi.call(f"hpcla_amg_restrictor_b_f64_{sfx}", *pattern, dptr(lvl.Tv), k, TA.nrows_local, A.nrows_local, lo, 0, dptr(vals),
                   current_stream_ptr())
    return TA._with_values(vals)


def _fit(lvl: AMGLevel, k: int, first_aggregate: int, row_start: int):
    """The members of every aggregate (ascending local rows), ``lvl.Tv`` and the next level's candidates from
    ``lvl.candidates``; raises on every rank for a dropped column."""
    torch = _torch()
    A = lvl.A
    backend, dev, n = A.backend, A.backend.torch_device, A.nrows_local
    n_agg = lvl.n_roots
    local = lvl.aggregates - first_aggregate
    members = torch.sort(local, stable=True).indices
    mptr = torch.zeros(n_agg + 1, dtype=torch.int64, device=dev)
    mptr[1:] = torch.cumsum(torch.bincount(local, minlength=n_agg)[:n_agg], 0)
    lvl.Tv = torch.zeros((n, k), dtype=torch.float64, device=dev)
    coarse = torch.zeros((n_agg * k, k), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    _capi.call("hpcla_amg_fit_f64", dptr(lvl.candidates), n, k, dptr(mptr), dptr(members), n, n_agg, dptr(lvl.Tv), dptr(coarse),
               dptr(info), current_stream_ptr())
    word = int(info.item())
    first, size, column = -1, 0, 0
    if word >= 0:                                            # 8 a + j: the smallest aggregate that dropped a column, its first
        a, column = word >> 3, word & 7
        e0, e1 = (int(v) for v in mptr[a:a + 2].cpu().tolist())
        first, size = int(members[e0].item()), e1 - e0
    _raise_together(backend, first, row_start,
                    lambda row: f"amg: the aggregate of row {row} (level of {lvl.n} rows) has {size} members and cannot carry "
                                f"candidate column {column} of B's {k}: too few members, or candidates that are dependent, zero "
                                "or not finite on it")
    return coarse


def _prolongator(lvl: AMGLevel, symmetric: bool = True, k: Optional[int] = None) -> HPCSparseMatrix:
    """P on the pattern of A T, and R (Pt, or the Petrov-Galerkin restriction); returns the next level's A.  ``k``: the
    candidates per aggregate of a level that ``_fit`` has run on (``lvl.Tv``; ``lvl.coarse_partition`` counts unknowns)."""
    from .backends import comm_rank
    from .indexing import _col_indices_dev
    from .matmat import spgemm
    from .transpose import transpose
    torch = _torch()
    A = lvl.A
    backend, dev, n = A.backend, A.backend.torch_device, A.nrows_local
    part = lvl.coarse_partition
    nc = int(part[-1])
    lo = int(part[comm_rank(backend.comm)])
    sfx = lambda M: "i64" if M.Ti == np.dtype(np.int64) else "i32"
    if k is None:
        window = (lo, lo + lvl.n_roots - 1) if lvl.n_roots > 0 else (0, 0)
        T = HPCSparseMatrix_local_device(torch.arange(n + 1, dtype=torch.int64, device=dev), lvl.aggregates,
                                         torch.ones(n, dtype=torch.float64, device=dev), nc, backend, col_partition=part,
                                         col_window=window)
        AT = spgemm(A, T)
        vals = torch.empty_like(AT.nzval)
        _capi.call(f"hpcla_amg_prolongator_f64_{sfx(AT)}", dptr(AT.rowptr_target), dptr(AT.colval_target()),
                   dptr(_col_indices_dev(AT)), dptr(AT.nzval), dptr(lvl.aggregates), dptr(lvl.s.v), n, 0, dptr(vals),
                   current_stream_ptr())
    else:
        window = (lo, lo + k * lvl.n_roots - 1) if lvl.n_roots > 0 else (0, 0)
        cols = (lvl.aggregates * k).unsqueeze(1) + torch.arange(k, dtype=torch.int64, device=dev)
        T = lvl.T = HPCSparseMatrix_local_device(torch.arange(n + 1, dtype=torch.int64, device=dev) * k, cols.reshape(-1),
                                                 lvl.Tv.reshape(-1), nc, backend, col_partition=part, col_window=window)
        AT = spgemm(A, T)
        vals = torch.empty_like(AT.nzval)
        _capi.call(f"hpcla_amg_prolongator_b_f64_{sfx(AT)}", dptr(AT.rowptr_target), dptr(AT.colval_target()),
                   dptr(_col_indices_dev(AT)), dptr(AT.nzval), dptr(lvl.aggregates), dptr(lvl.s.v), dptr(lvl.Tv), k, n, 0,
                   dptr(vals), current_stream_ptr())
    lvl.P = AT._with_values(vals)
    if symmetric:
        lvl.R = lvl.Pt = transpose(lvl.P).materialize()
    else:
        lvl.R = _restrictor(lvl, T, lo, k)
    return galerkin(lvl, A)


FORCE_SPLIT = 0                # tests set it to split the rows of Pt below on matrices that do not need it
MAX_SPLIT = 32


def _split_rows(Pt: HPCSparseMatrix, q: int) -> List[HPCSparseMatrix]:
    """Pt as a sum of q matrices of its shape: part j keeps, of every row, the j-th of q runs of its stored entries (order kept).
    Index arithmetic on the device; the parts are assembled like any device-built matrix."""
    from .indexing import _col_indices_dev
    torch = _torch()
    dev, n = Pt.backend.torch_device, Pt.nrows_local
    rowptr = Pt.rowptr_target.to(torch.int64)
    counts = rowptr[1:] - rowptr[:-1]
    row_of = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), counts)
    pos = torch.arange(Pt.nnz, dtype=torch.int64, device=dev) - rowptr[row_of]
    part_of = (pos * q) // counts[row_of]
    cols = _col_indices_dev(Pt)[Pt.colval_target().to(torch.int64)]
    parts = []
    for j in range(q):
        keep = part_of == j
        if not bool(keep.any()):
            continue
        rp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(torch.bincount(row_of[keep], minlength=n), 0)
        parts.append(HPCSparseMatrix_local_device(rp, cols[keep].contiguous(), Pt.nzval[keep].contiguous(), int(Pt.shape[1]),
                                                  Pt.backend, col_partition=Pt.col_partition))
    return parts


def galerkin(lvl: AMGLevel, A: HPCSparseMatrix) -> HPCSparseMatrix:
    """``Pt (A P)``.  ``hp.spgemm`` bounds the candidate products of an output row (the lengths of the rows of ``A P`` that a row
    of ``Pt`` names, summed); the aggregates of a 3-D stencil's coarse levels are over it.  There the rows of ``Pt`` are split
    into q runs of their entries, ``Pt = Pt_1 + ... + Pt_q``, and the coarse matrix is ``Pt_1 (A P) + ... + Pt_q (A P)``: the
    same pattern, the same products, the sums of an entry associated run by run, so the last bits can differ from the unsplit
    product's.  q doubles until every part fits; ``lvl.galerkin`` records it (1: not split).  With ``symmetric=False`` the left
    factor is ``lvl.R``, and ``Tt A`` inside it is formed the same way (``lvl.restriction_split``)."""
    from .matmat import spgemm
    AP = spgemm(A, lvl.P)
    Ac, lvl.galerkin = _split_product(lvl.R, AP, max(int(FORCE_SPLIT), 1), lvl, "coarse matrix")
    return Ac


def _split_product(L: HPCSparseMatrix, B: HPCSparseMatrix, q: int, lvl: AMGLevel, what: str):
    """``(L B, q)``: the product with the rows of L in q runs, q doubling from the given one while a part is over the bound."""
    from .addition import sparse_add
    from .matmat import spgemm
    while True:
        try:
            if q == 1:
                C = spgemm(L, B)
            else:
                parts = _split_rows(L, q)
                C = spgemm(parts[0], B)
                for part in parts[1:]:
                    C = sparse_add(C, spgemm(part, B))
            return C, q
        except NotImplementedError as exc:
            if "candidate entries" not in str(exc) or 2 * q > MAX_SPLIT:
                raise NotImplementedError(f"amg: the {what} of the level of {lvl.n} rows cannot be formed: {exc}") from None
            q *= 2


def _dense_inverse(lvl: AMGLevel, symmetric: bool = True) -> None:
    """The last level's rows on the host; the inverse of the symmetrised matrix (of the matrix itself unless ``symmetric``),
    applied by the dense mat-vec."""
    from .dense import HPCMatrix
    torch = _torch()
    A = lvl.A
    n = lvl.n
    D = np.zeros((n, n))
    if A.nnz:
        rowptr = A.rowptr.astype(np.int64)
        cols = A.col_indices[A.colval.astype(np.int64)]
        D[np.repeat(np.arange(n), np.diff(rowptr)), cols] = A.nzval.cpu().numpy()
    inv = np.linalg.inv((D + D.T) / 2 if symmetric else D)
    mine = torch.from_numpy(np.ascontiguousarray(inv)).to(A.backend.torch_device)
    lvl.inverse = HPCMatrix(A.row_partition, A.row_partition, mine, A.backend)


def aggregate_level(A: HPCSparseMatrix, theta: float = 0.0, symmetric: bool = True) -> AMGLevel:
    """The rank-local part of a level's setup alone, for tests: the weights and the aggregation of ``A`` as an AMGLevel (``s``,
    ``w``, ``rho``, ``aggregates``, ``n_roots``, ``rounds``, ``coarse_partition``; no P).  It exchanges nothing but sizes, the
    maximum of rho and the error word, in either mode (``symmetric=False``: the graph E u E^T, ghost columns out both ways),
    so unlike ``amg`` it runs on several ranks.  Raises like ``amg``."""
    from .backends import comm_rank
    f64_only(A.backend, "amg")
    check_arguments(A.backend.T, A.shape, A.row_partition, A.col_partition, theta, symmetric=symmetric)
    lvl = AMGLevel(A)
    plan = get_vector_plan(A, HPCVector.zeros(A.col_partition, A.backend))
    sfx = "i64" if plan.is_i64 else "i32"
    row_start = int(A.row_partition[comm_rank(A.backend.comm)])
    _aggregate(lvl, plan, sfx, _weights(lvl, plan, sfx, row_start), theta, row_start, bool(symmetric))
    return lvl


def _candidate_block(B):
    """(local block as a 2-D device tensor, row partition) of an HPCVector (one column) or an HPCMatrix."""
    from .dense import HPCMatrix
    if isinstance(B, HPCVector):
        return B.v.reshape(-1, 1), B.partition
    if isinstance(B, HPCMatrix):
        return B.A, B.row_partition
    raise TypeError(f"amg: B must be an HPCVector or an HPCMatrix, got {type(B).__name__}")


def amg(A: HPCSparseMatrix, theta: float = 0.0, max_levels: int = 12, coarse_size: int = 128, coarse_sweeps: int = 4,
        symmetric: bool = True, B=None) -> AMG:
    """Build the smoothed-aggregation multigrid preconditioner of a symmetric positive definite ``A`` for
    ``hp.cg(A, b, M=hp.amg(A))``, or with ``symmetric=False`` that of a nonsymmetric ``A`` with a positive diagonal for
    ``hp.gmres`` and ``hp.bicgstab`` (which take a hierarchy of either mode; ``hp.cg`` refuses one built with ``symmetric=False``).

    ``theta``: the strength threshold in [0, 1) (0 keeps every stored coupling; 0.25 suits anisotropic problems).  Setup stops
    at ``n <= coarse_size`` (1..1024; solved densely), at ``max_levels``, or when a level's aggregates number >= 0.8 n; a last
    level above ``coarse_size`` gets ``coarse_sweeps`` damped Jacobi sweeps.  Raises ValueError, with the global row, for a
    diagonal that is not positive (a NaN counts), and NotImplementedError for a communicator of more than one rank and for a
    level whose coarse matrix is over ``hp.spgemm``'s bound in both orders of the product.

    ``symmetric=False`` (a bool) aggregates on the symmetrised strength graph E u E^T, restricts with the Petrov-Galerkin
    ``R = Tt (I - A S)`` in place of ``Pt`` (``AMGLevel.R``; ``Pt`` stays None) and inverts the last level's matrix as it is.  A
    strongly convective or non-M-matrix ``A`` can give a coarse diagonal that is not positive, which raises as above.

    ``B``: the near-nullspace candidates, an HPCVector or an HPCMatrix of k = 1..8 columns on A's row partition, Float64, in
    either mode.  Without it the tentative prolongator is the constant vector's, and a two-sided scaling ``D A D`` takes most
    of the gain away: pass ``B = 1 ./ d`` there, and the rigid-body modes for elasticity.  Every aggregate then carries k coarse
    unknowns (``AMG.candidates_per_aggregate``; the stall rule counts k per aggregate), and one that cannot (fewer members than
    candidates, candidates dependent, zero or not finite on it) raises ValueError with the global row of its first member.
    rho is not invariant under a rough scaling, so with the right ``B`` a scaled problem converges at a rate independent of
    the grid but not at the unscaled problem's (README)."""
    from .backends import comm_allgather, comm_rank, comm_size
    f64_only(A.backend, "amg")
    block = None if B is None else _candidate_block(B)
    check_arguments(A.backend.T, A.shape, A.row_partition, A.col_partition, theta, max_levels, coarse_size, coarse_sweeps, symmetric,
                    None if B is None else (B.backend.T, (int(block[1][-1]), int(block[0].shape[1])), block[1]))
    symmetric = bool(symmetric)
    backend = A.backend
    k = None if B is None else int(block[0].shape[1])
    candidates = None if B is None else block[0].contiguous()   # a block that is not row-major is packed here, once
    if B is not None and int(candidates.shape[0]) != A.nrows_local:
        raise ValueError(f"amg: B holds {candidates.shape[0]} local rows, A {A.nrows_local}")
    if comm_size(backend.comm) > 1:                              # the same on every rank
        raise NotImplementedError("amg: one rank only in this version.  Across ranks the setup's products and transposes move "
                                  "their values through RCCL, which ranks that share one GPU do not have, so the hierarchy and "
                                  "the solve across ranks cannot be tested yet; the aggregation itself is rank-local")
    rank = comm_rank(backend.comm)
    levels: List[AMGLevel] = []
    nnz = []
    while True:
        lvl = AMGLevel(A)
        lvl.candidates = candidates
        levels.append(lvl)
        nnz.append(int(comm_allgather(backend.comm, np.array([A.nnz], dtype=np.int64)).sum()))
        plan = get_vector_plan(A, HPCVector.zeros(A.col_partition, backend))
        sfx = "i64" if plan.is_i64 else "i32"
        row_start = int(A.row_partition[rank])
        diag = _weights(lvl, plan, sfx, row_start)
        last = lvl.n <= coarse_size or len(levels) >= max_levels
        if not last:
            _aggregate(lvl, plan, sfx, diag, theta, row_start, symmetric)
            if k is not None:                                    # k unknowns per aggregate; the fit comes before the stall
                lvl.coarse_partition = lvl.coarse_partition * k  # rule, so every aggregation made is checked for dropped columns
                candidates = _fit(lvl, k, int(lvl.coarse_partition[rank]) // k, row_start)
            last = int(lvl.coarse_partition[-1]) >= STALL * lvl.n
        if last:
            if lvl.n <= coarse_size:
                _dense_inverse(lvl, symmetric)
            else:
                lvl.sweeps = int(coarse_sweeps)
            return AMG(levels, sum(nnz) / max(nnz[0], 1), symmetric, k)
        A = _prolongator(lvl, symmetric, k)
