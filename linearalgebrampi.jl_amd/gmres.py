"""Restarted GMRES(m) for a square, not necessarily symmetric ``A`` (``hp.gmres``), next to ``hp.cg`` and ``hp.bicgstab``.

The residual-minimising fallback: its residual never rises and it has no breakdown on a solvable system (``hp.bicgstab``
reports one on ``[[0, 1], [-1, 0]]``, which GMRES solves in two steps).  A caller of the reference's operators would compose
it from ``A*p`` (src/sparse.jl:2096-2128), ``dot`` (src/vectors.jl:798-812) and broadcast updates (src/vectors.jl:1203-1226):
with twice-applied classical Gram-Schmidt the step that orthogonalises against ``c`` basis columns is ``2c`` dots, ``2c`` axpys
and ``2c + 1`` host read-backs.  Here it is one SpMV and the fused HIP steps of csrc/vecops.hip (``gmres_dots``: all ``c`` sums
with one read of the basis; ``gmres_update``: the whole running subtraction in one pass), whose scalars, Givens rotations,
stop rule and breakdown test stay on the device; the host enqueues ``check_every`` inner steps per library call
(``hpcla_gmres_iterations_f64_*``, csrc/solvers.hip) and reads 16 bytes of state per chunk, exactly as the other two solvers do.

Right-preconditioned, ``K`` = identity, ``dinv .*`` or the operator of ``hp.ilu0`` / ``hp.amg`` (ilu.py, amg.py; ``_gmres_operator`` enqueues the same
steps with ``dinv == NULL`` one by one and applies ``K`` between them); gate order and rounding order (tests/_gmres_cases.py restates them):

    start / restart   w = b - A x (w = b when x is zero);  rr = w.w
                      gate R  rr <= thr: converged at a restart, hist[k] = rr
                      beta = sqrt(rr);  g = (beta, 0, ...);  V_0 = w / beta;  z = K V_0
    step k            column j = (k - 1) mod m, c = j + 1 basis columns so far
                      w = A z;  h1 = V^T w;  w = w - V h1;  h2 = V^T w;  w = w - V h2;  nn = w.w
                      col = h1 + h2, sqrt(nn);  the stored rotations;  d = sqrt(col[j]^2 + col[j+1]^2)
                      gate D  !(d > 0): breakdown at k - 1
                      c_j, s_j, R[:, j], g[j], g[j+1];  hist[k] = g[j+1]^2
                      gate C  hist[k] <= thr: converged at k
                      V_{j+1} = w / col[c];  z = K V_{j+1}          (while c < m)
    cycle end         y = R^-1 g;  x = x + K (V y);  then the restart above
"""
from __future__ import annotations

from typing import Optional, Tuple

from . import _capi
from .krylov import (CGInfo, _AMGOperator, _bicgstab_dinv, _ilu_operator, _PairHistory, _residual_norms, _run_chunks,
                     _solver_arguments, _stop_rule_or_done)
from .sparse import get_vector_plan, mul_
from .vectors import HPCVector, current_stream_ptr, dptr, norm, rd16_vector

_STATUS = {0: "maxiter", 1: "converged", 2: "breakdown", 3: "converged"}     # 3: converged at a restart
_SMALL = ("R", "c", "s", "g", "h1", "h2", "col", "y", "nn", "hn")
MAX_RESTART = 64


def _torch():
    import torch
    return torch


def _check_restart(restart) -> int:
    restart = int(restart)
    if not 1 <= restart <= MAX_RESTART:
        raise ValueError(f"gmres: restart must be in 1..{MAX_RESTART}, got {restart}")
    return restart


class GMRESWorkspace(_PairHistory):
    """What a ``gmres`` solve allocates: ``restart + 1`` basis columns at a pitch rounded up to an even number of doubles (every
    column is then 16-byte aligned even when the local length is odd), w, z (once a preconditioner is used), x, the small
    arrays (R, the rotations c and s, g, h1, h2, y and scratch, in one buffer), the history (pairs, like the other solvers';
    the second entry of a pair is not used; it grows by doubling between chunks), and the scratch of the gated kernels whose
    last 32 bytes are the solve's device state (done_iter, status, thr).  Reusable: every solve resets all of it."""

    def __init__(self, b: HPCVector, restart: int = 30, hist_iters: int = 254):
        torch = _torch()
        lib = _capi.load()
        dev = b.v.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.restart = _check_restart(restart)
        self.x = HPCVector.zeros(b.partition, b.backend)
        self.w = b.similar()
        self.z: Optional[HPCVector] = None
        self.ldv = b.local_length + (b.local_length & 1)
        self.V = torch.zeros((self.restart + 1) * self.ldv, **f64)
        self.small = torch.zeros(lib.hpcla_gmres_small_offset(self.restart, len(_SMALL)), **f64)
        self.hist = torch.zeros(2 * (int(hist_iters) + 2), **f64)
        self.tmp = torch.ones(1, **f64)                                # |b|^2 for a given x0
        self.work = torch.zeros(lib.hpcla_gmres_work_bytes(self.restart) // 8, **f64)
        self.state = self.work[-4:].view(torch.int64)                  # done_iter, status, thr (a double), reserved

    def fits(self, b: HPCVector, restart: int) -> bool:
        return self.restart == restart and self.x.structural_hash == b.structural_hash and self.x.v.device == b.v.device

    def with_preconditioner(self) -> None:
        if self.z is None:
            self.z = self.x.similar()

    def with_operator(self) -> None:
        """z, and what ``x = x + K (V y)`` needs when K is an operator (``hp.ilu0``): u = V y, ku = K u, the constant 1."""
        self.with_preconditioner()
        if getattr(self, "u", None) is None:
            self.u, self.ku = self.x.similar(), self.x.similar()
            self.one = _torch().ones(1, dtype=self.V.dtype, device=self.V.device)

    def small_array(self, name: str):
        """A view of one of the small arrays (R, c, s, g, h1, h2, col, y, nn, hn)."""
        lib = _capi.load()
        k = _SMALL.index(name)
        return self.small[lib.hpcla_gmres_small_offset(self.restart, k):lib.hpcla_gmres_small_offset(self.restart, k + 1)]


def _open_columns(status: int, iterations: int, maxiter: int, m: int) -> int:
    """Basis columns of the cycle that is still open when the chunk loop ends: what the finish call has to apply."""
    if status == 1:                                              # gate C at k
        return iterations - m * ((iterations - 1) // m)
    if status == 2:                                              # gate D with done_iter = iterations
        return iterations % m
    if status == 0:                                              # maxiter while still running
        return maxiter % m
    return 0                                                     # gate R: x is already updated


def _gmres_operator(A, b: HPCVector, x0, rtol: float, atol: float, m: int, maxiter: int, op, check_every: int,
                    ws: GMRESWorkspace) -> Tuple[HPCVector, CGInfo]:
    """``gmres`` with ``K = op.apply`` (the ILU0 of ilu.py, or the multigrid cycle of amg.py): the order of
    hpcla_gmres_iterations_*, enqueued from here through the exported gated entries with dinv == NULL; each ``dinv .*`` is
    ``op.apply``.  The application is not gated: behind the deciding step its input is frozen and it rewrites z and its own
    scratch with what they held (the cycle is a fixed sequence of launches on the basis column, the hierarchy and level vectors
    that nothing else writes: the same input gives the same bits in every one of them).  The ILU0 reads the basis column through
    its raw pointer; the cycle reads it as an HPCVector over the column's storage (the pitch keeps it 16-byte aligned).
    ``x = x + K (V y)`` goes
    through a scratch vector: u = 0, the gated update adds V y into u, ku = K u, and a gated update of one column adds
    1 * ku into x -- behind a stop u stays zero and nothing is added."""
    ws.with_operator()
    n, ldv, comm = ws.x.local_length, ws.ldv, A.backend.rccl
    state, small, work = dptr(ws.state), dptr(ws.small), dptr(ws.work)
    hn, y, h1, h2 = (dptr(ws.small_array(k)) for k in ("hn", "y", "h1", "h2"))
    one = dptr(ws.one)
    column = lambda c: ws.V.data_ptr() + 8 * c * ldv

    def apply_to_column(c):
        if not n:
            return
        if isinstance(op, _AMGOperator):
            op.apply(HPCVector(ws.x.structural_hash, ws.x.partition, ws.V[c * ldv:c * ldv + n], ws.x.backend), out=ws.z)
        else:
            op._enqueue(column(c), dptr(ws.z.v))

    def start_cycle(k):                                          # the residual (w holds A x, or 0), gate R, V_0, z = K V_0
        s = current_stream_ptr()
        _capi.call("hpcla_gmres_residual_f64", comm, dptr(b.v), dptr(ws.w.v), n, k, m, small, dptr(ws.hist[2 * k:]), state, work, s)
        _capi.call("hpcla_gmres_next_f64", dptr(ws.w.v), hn, None, column(0), None, n, state, s)
        apply_to_column(0)

    def add_cycle(ncols, gate):                                  # x = x + K (V y) over ncols columns
        s = current_stream_ptr()
        ws.u.v.zero_()
        _capi.call("hpcla_gmres_xupdate_f64", dptr(ws.V), ldv, ncols, y, None, dptr(ws.u.v), n, gate, s)
        op.apply(ws.u, out=ws.ku)
        _capi.call("hpcla_gmres_xupdate_f64", dptr(ws.ku.v), ldv, 1, one, None, dptr(ws.x.v), n, gate, s)

    ws.hist.zero_()
    ws.small.zero_()
    ws.work.zero_()                                              # done_iter = 0, status = running, thr = 0
    ws.V.zero_()
    if x0 is None:                                               # w = b - 0, not b - A 0
        ws.x.v.zero_()
        ws.w.v.zero_()
    else:
        b._same_partition(x0)
        ws.x.v.copy_(x0.v)
        norm(b, 2, out=ws.tmp[0:1])
        mul_(ws.w, A, ws.x)
    start_cycle(0)
    done = _stop_rule_or_done(ws, b, x0 is not None, rtol, atol, maxiter)
    if done is not None:
        return ws.x, done

    def enqueue(first, count):
        for k in range(first, first + count):
            s = current_stream_ptr()
            c = (k - 1) % m + 1
            mul_(ws.w, A, ws.z)
            _capi.call("hpcla_gmres_dots_f64", comm, dptr(ws.V), ldv, c, dptr(ws.w.v), n, state, h1, work, s)
            _capi.call("hpcla_gmres_update_f64", comm, dptr(ws.V), ldv, c, h1, dptr(ws.w.v), n, k, m, None, None, state, work, s)
            _capi.call("hpcla_gmres_dots_f64", comm, dptr(ws.V), ldv, c, dptr(ws.w.v), n, state, h2, work, s)
            _capi.call("hpcla_gmres_update_f64", comm, dptr(ws.V), ldv, c, h2, dptr(ws.w.v), n, k, m, small, dptr(ws.hist[2 * k:]),
                       state, work, s)
            if c < m:
                _capi.call("hpcla_gmres_next_f64", dptr(ws.w.v), hn, None, column(c), None, n, state, s)
                apply_to_column(c)
                continue
            _capi.call("hpcla_gmres_solve_f64", c, m, small, state, s)
            add_cycle(c, state)
            mul_(ws.w, A, ws.x)
            start_cycle(k)

    iterations, status = _run_chunks(ws, A.backend, maxiter, check_every, enqueue)
    open_columns = _open_columns(status, iterations, maxiter, m)
    if open_columns:
        _capi.call("hpcla_gmres_solve_f64", open_columns, m, small, None, current_stream_ptr())
        add_cycle(open_columns, None)
    h = _residual_norms(ws, b.backend, iterations)
    return ws.x, CGInfo(status in (1, 3), iterations, _STATUS[status], h)


def gmres(A, b: HPCVector, x0: Optional[HPCVector] = None, rtol: float = 1e-8, atol: float = 0.0, restart: int = 30,
          maxiter: Optional[int] = None, M=None, check_every: int = 8,
          workspace: Optional[GMRESWorkspace] = None) -> Tuple[HPCVector, CGInfo]:
    """Solve ``A x = b`` for a square ``A`` (symmetry is not needed) by right-preconditioned restarted GMRES(``restart``).

    Stops at the first inner step with ``||r_k|| <= max(rtol * ||b||, atol)`` (the rule of ``hp.cg`` and ``hp.bicgstab``; also
    tested on the true residual at every restart), after ``maxiter`` inner steps (default ``10 n``), or on a breakdown (a
    new Hessenberg column that is zero or NaN: ``A`` is singular on the Krylov space).  ``restart`` is the cycle length, 1..64;
    a cycle keeps ``restart + 1`` basis vectors.  ``M``: ``None``, ``"jacobi"`` (``1 ./ diag(A)``, formed on the device; no
    diagonal entry may be zero), an HPCVector holding the inverse diagonal to apply, or the ``ILU0`` object of ``hp.ilu0(A)``
    (its triangular sweeps, enqueued from here between the gated steps), or the ``AMG`` object of ``hp.amg`` (one V-cycle per
    step, enqueued the same way in level vectors that belong to the workspace; ``hp.amg(A, symmetric=False)`` for a nonsymmetric
    ``A``, and a symmetric hierarchy is a valid fixed operator too).  ``x0`` defaults to zero.  Returns
    ``(x, CGInfo)``; x is the workspace's vector.  ``iterations`` counts inner steps: one SpMV each, plus one per restart.
    ``residual_norms[k]`` is the Givens estimate ``|g_{j+1}|`` of ``||r_k||`` after step k -- with the preconditioner on the
    right that is the norm of the true residual ``b - A x_k`` -- and entry 0 is the true ``||b - A x0||``; it never rises.

    The breakdown test is an exact-zero / NaN test, as everywhere in this package: a matrix that is singular only up to
    rounding stagnates instead and ends as ``"maxiter"``, as does a ``restart`` too short for the problem.

    Every test runs on the device.  The host enqueues ``check_every`` steps in one library call and then reads the 16-byte
    state (the only synchronisation); steps enqueued behind the one that decided are no-ops, so the answer does not depend
    on ``check_every``.  The cycle that is open when the solve ends is applied to x by one more call."""
    maxiter, check_every = _solver_arguments("gmres", A, rtol, atol, maxiter, check_every)
    m = _check_restart(restart)
    if int(b.partition[-1]) != int(A.shape[0]):
        raise ValueError("gmres: b must be partitioned like the rows of A")
    b = rd16_vector(b)                                           # every cycle's residual kernel reads b 16 bytes at a time
    ws = workspace if workspace is not None and workspace.fits(b, m) else GMRESWorkspace(b, m)
    plan = get_vector_plan(A, ws.x)
    if plan.result_partition_hash != ws.x.structural_hash:
        raise ValueError("gmres: b must be partitioned like the rows of A")
    op = _ilu_operator(A, M, "gmres", ws)
    if op is not None:
        return _gmres_operator(A, b, x0, rtol, atol, m, maxiter, op, check_every, ws)
    dinv = _bicgstab_dinv(A, b, M, "gmres")
    if dinv is not None:
        ws.with_preconditioner()
    n, stream = ws.x.local_length, current_stream_ptr()
    sfx = "i64" if plan.is_i64 else "i32"
    blk = plan.matrix_block(A)
    spmv = (blk[0], A.backend.rccl, *blk[1:])
    dv, zv = (dptr(dinv.v), dptr(ws.z.v)) if dinv is not None else (None, None)

    def solve():                                                 # the history may have grown since the last call
        return (dv, dptr(b.v), dptr(ws.x.v), dptr(ws.V), ws.ldv, dptr(ws.w.v), zv, dptr(ws.small), dptr(ws.hist), dptr(ws.work), m)

    # -- setup: w = b - A x0, hist[0] = w.w, g = (beta, 0, ...), V_0 = w / beta, z = dinv V_0, the state -------------------
    ws.hist.zero_()
    ws.small.zero_()
    ws.work.zero_()                                              # done_iter = 0, status = running, thr = 0
    ws.V.zero_()
    if x0 is None:                                               # w = b - 0, not b - A 0
        ws.x.v.zero_()
        ws.w.v.zero_()
        _capi.call("hpcla_gmres_residual_f64", A.backend.rccl, dptr(b.v), dptr(ws.w.v), n, 0, m, dptr(ws.small), dptr(ws.hist),
                   dptr(ws.state), dptr(ws.work), stream)
        _capi.call("hpcla_gmres_next_f64", dptr(ws.w.v), dptr(ws.small_array("hn")), dv, dptr(ws.V), zv, n, dptr(ws.state), stream)
    else:
        b._same_partition(x0)
        ws.x.v.copy_(x0.v)
        norm(b, 2, out=ws.tmp[0:1])
        _capi.call(f"hpcla_gmres_restart_f64_{sfx}", *spmv, *solve(), 0, stream)
    done = _stop_rule_or_done(ws, b, x0 is not None, rtol, atol, maxiter)
    if done is not None:
        return ws.x, done

    # -- chunks of check_every steps; one 16-byte read-back each -----------------------------------------------------------
    def enqueue(first, count):
        _capi.call(f"hpcla_gmres_iterations_f64_{sfx}", *spmv, *solve(), first, count, current_stream_ptr())

    iterations, status = _run_chunks(ws, A.backend, maxiter, check_every, enqueue)
    _capi.call("hpcla_gmres_finish_f64", dptr(ws.V), ws.ldv, _open_columns(status, iterations, maxiter, m), m, dptr(ws.small), dv,
               dptr(ws.x.v), n, current_stream_ptr())
    h = _residual_norms(ws, b.backend, iterations)
    return ws.x, CGInfo(status in (1, 3), iterations, _STATUS[status], h)
