"""Conjugate-gradient harness for BASELINE config 4 (3-D Poisson, 100 iterations).

The reference has no Krylov solver; a caller composes one from ``A*p``
(src/sparse.jl:2096-2128), ``dot`` (src/vectors.jl:798-812) and broadcast updates
(src/vectors.jl:1203-1226).  This harness does exactly that with the DeviceROCm operators, keeping
every scalar on the device: alpha = rr/pAp and beta = rr_new/rr are consumed by the update kernels
as (numerator, denominator) device pointers, so an iteration never synchronises the host.

Forms, identical arithmetic per element (only the reduction trees differ):

* ``fused=False``  one library call per reference operator: SpMV, dot, axpy, axpy, norm, xpay
  (8 kernel launches, SpMV + 96 B/row of vector traffic -- the "textbook unfused" count of SURVEY 8d);
* ``fused=True``   SpMV with the p.Ap partials in its epilogue, one kernel for r -= a Ap / sum r^2, one for
  x += a p / p = r + b p (the x update is deferred to where p is read anyway): SpMV + 64 B/row.
  ``native_loop=True`` (default) hands ALL iterations to the library in one call
  (``hpcla_cg_iterations_f64_*``: the same three launches per iteration, same arguments, same bits), so
  the host language is not in the loop at all; ``native_loop=False`` issues the three calls per iteration
  from Python.

The solve is split into ``cg_setup`` (x = 0, r = p = b, sum r0^2 -- allocation lives in a reusable
``CGWorkspace``) and ``cg_iterate`` (exactly k iterations, enqueue only), so a benchmark can time the
iterations and nothing else; ``cg_fixed_iterations`` is the two together plus the history read-back.

``cg`` is the solver built from the same launches: a stop rule, an optional preconditioner (a diagonal, or the factorised
sparse approximate inverse of fsai.py: two more SpMVs and one reduction per iteration, ``hpcla_pcg_fsai_iterations_f64_*``) and
a breakdown check, all decided on the device (the gated kernels of csrc/vecops.hip, chained by ``hpcla_pcg_iterations_f64_*`` in
csrc/solvers.hip); the host reads 16 bytes of state once per ``check_every`` iterations, and the iterations enqueued behind the
deciding one are no-ops.  What ``cg`` shares with the other chunked solvers (``CGInfo``, the chunk loop) is in krylov.py.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import numpy as np

from . import _capi
from .fsai import FSAI
from .krylov import _STATUS, CGInfo, _PairHistory, _residual_norms, _run_chunks, _solver_arguments, _stop_rule_or_done
from .sparse import get_vector_plan, mul_, mul_dot_
from .vectors import HPCVector, _Scratch, cg_direction_, cg_residual_, current_stream_ptr, dot, dptr, norm, rd16_vector


def _torch():
    import torch
    return torch


def _cg_iteration(A, x, r, p, Ap, rr_cur, rr_nxt, pAp, fused: bool) -> None:
    if fused:
        mul_dot_(Ap, A, p, pAp)                                 # Ap = A*p, pAp = p.Ap
        cg_residual_(r, Ap, 1.0, rr_cur, pAp, rr_nxt)           # r -= a Ap; rr_new        (a = rr/pAp)
        cg_direction_(x, p, r, 1.0, rr_cur, pAp, 1.0, rr_nxt, rr_cur)   # x += a p; p = r + (rr_new/rr) p
        return
    mul_(Ap, A, p)                                              # Ap = A*p
    dot(p, Ap, out=pAp)                                         # pAp
    x.axpy_(1.0, p, num=rr_cur, den=pAp)                        # x += (rr/pAp) p
    r.axpy_(-1.0, Ap, num=rr_cur, den=pAp)                      # r -= (rr/pAp) Ap
    norm(r, 2, out=rr_nxt)                                      # rr_new = sum(r^2)
    p.xpay_(r, 1.0, num=rr_nxt, den=rr_cur)                     # p = r + (rr_new/rr) p


class CGWorkspace:
    """Everything a solve allocates: x, r, p, Ap (partitioned like b), the history array (sum r_k^2 lives in
    hist[k] -- it IS the rr storage of the iteration, so recording costs no copies), pAp.  Reusable across
    solves of the same size; ``cg_fixed_iterations`` makes one when none is given."""

    def __init__(self, b: HPCVector, max_iters: int):
        torch = _torch()
        dev = b.v.device
        self.x = HPCVector.zeros(b.partition, b.backend)
        self.r = b.similar()
        self.p = b.similar()
        self.Ap = b.similar()
        self.max_iters = int(max_iters)
        self.hist = torch.zeros(self.max_iters + 2, dtype=torch.float64, device=dev)
        self.pAp = torch.zeros(1, dtype=torch.float64, device=dev)
        self.done = 0                  # iterations since the last cg_setup

    def fits(self, b: HPCVector, iters: int) -> bool:
        return self.max_iters >= iters and self.x.structural_hash == b.structural_hash and self.x.v.device == b.v.device


def cg_setup(A, b: HPCVector, ws: CGWorkspace, fused: bool = True):
    """x0 = 0, r0 = p0 = b, hist[0] = sum r0^2; builds / looks up the plan.  Returns the state ``cg_iterate``
    continues from.  Not an iteration: benchmarks keep it outside the timed region."""
    from .vectors import f64_only
    f64_only(A.backend, "the CG building blocks")
    plan = get_vector_plan(A, ws.p)
    fused = bool(fused and plan.result_partition_hash == ws.p.structural_hash)
    ws.x.v.zero_()
    ws.r.v.copy_(b.v)
    ws.p.v.copy_(b.v)
    ws.hist.zero_()
    norm(ws.r, 2, out=ws.hist[0:1])            # out form leaves sum(r^2) on the device (8 B/elt)
    ws.done = 0
    if fused:                                  # the SpMV+dot scratch hangs off the plan
        plan.dot_work(A)
    return plan, fused


def cg_iterate(A, ws: CGWorkspace, plan, fused: bool, iters: int, native_loop: bool = True) -> None:
    """Exactly ``iters`` more iterations, enqueued on the current stream (no allocation, no host sync)."""
    first = ws.done
    if first + iters > ws.max_iters:
        raise ValueError("cg_iterate: workspace history too short")
    hist = ws.hist
    if fused and native_loop and A._packed_for(plan) is None:
        sfx = "i64" if plan.is_i64 else "i32"
        work, _ = _Scratch.get(ws.r.v.device)
        blk = plan.matrix_block(A, narrow=False)
        _capi.call(f"hpcla_cg_iterations_f64_{sfx}", blk[0], A.backend.rccl, *blk[1:],
                   dptr(ws.x.v), dptr(ws.r.v), dptr(ws.p.v), dptr(ws.Ap.v), dptr(hist[first:]), dptr(ws.pAp),
                   dptr(plan.dot_work(A)), dptr(work), int(iters), current_stream_ptr())
    else:
        for k in range(first, first + iters):
            _cg_iteration(A, ws.x, ws.r, ws.p, ws.Ap, hist[k:k + 1], hist[k + 1:k + 2], ws.pAp, fused)
    ws.done = first + iters


def cg_fixed_iterations(A, b: HPCVector, iters: int, record_history: bool = True,
                        fused: bool = True, graph: bool = False, native_loop: bool = True,
                        workspace: Optional[CGWorkspace] = None) -> Tuple[HPCVector, List[float]]:
    """Textbook CG from x0 = 0, exactly ``iters`` iterations, no convergence exit.
    Returns (x, [||r_0||, ..., ||r_iters||]) (history read back once at the end; ``record_history=False``
    skips the read-back and returns []).

    ``graph=True`` captures one PAIR of iterations (their scalars ping-pong through two fixed slots and return
    to the start after two) into a HIP graph and replays it: every library entry point only enqueues work on
    the stream it is given (no allocation, no host sync) and the exchange epoch lives in device memory, so
    whole distributed iterations are capturable.  Same kernels, same arguments, hence the same bits as the
    eager loop.  It pays off where an iteration is shorter than the host time to issue its launches (small
    systems); profiles/MEASUREMENTS_r03.md has the measurement for large ones, where eager stays the default."""
    if A.backend.T == np.dtype(np.float32):
        return _cg_composed_f32(A, b, iters, record_history)
    torch = _torch()
    ws = workspace if workspace is not None and workspace.fits(b, iters) else CGWorkspace(b, iters)
    plan, fused = cg_setup(A, b, ws, fused)
    if not graph or iters < 4:
        cg_iterate(A, ws, plan, fused, iters, native_loop)
    else:
        _cg_graph_replay(A, ws, plan, fused, iters)
    h = ws.hist[:iters + 1].sqrt().cpu().tolist() if record_history else []
    if h and h[-1] != h[-1]:                   # NaN: breakdown, or the poison of an expired exchange wait -- ask
        from .sparse import check_exchange_health
        check_exchange_health(b.backend)
    return ws.x, h


def _cg_composed_f32(A, b: HPCVector, iters: int, record_history: bool):
    """The same iteration on a Float32 backend, composed from the Float32 operators the way a caller of the reference composes
    it (`A*p`, `dot`, the vector updates; there is no reference solver): mul!, dot (formed in double, rounded to
    Float32), u + a*v.  Not fused, one host read-back per scalar -- the fused entries (hpcla_cg_iterations_*) are Float64's."""
    from .sparse import mul_
    from .vectors import dot
    x = HPCVector.zeros(b.partition, b.backend)
    r, p = b.copy(), b.copy()
    Ap = b.similar()
    rr = dot(r, r)
    hist = [math.sqrt(rr)]
    for _ in range(iters):
        mul_(Ap, A, p)
        pAp = dot(p, Ap)
        alpha = float(np.float32(rr) / np.float32(pAp))
        x = x._axpby(1.0, p, alpha)
        r = r._axpby(1.0, Ap, -alpha)
        rr_new = dot(r, r)
        beta = float(np.float32(rr_new) / np.float32(rr))
        p = r._axpby(1.0, p, beta)
        rr = rr_new
        hist.append(math.sqrt(rr))
    if hist[-1] != hist[-1]:
        from .sparse import check_exchange_health
        check_exchange_health(b.backend)
    return x, (hist if record_history else [])


class CGGraphPair:
    """One PAIR of iterations captured into a HIP graph (state must have run >= 2 eager iterations: they size
    the scratch buffers and probe the plan).  ``replay(n)`` continues the solve by 2n iterations."""

    def __init__(self, A, ws: CGWorkspace, plan, fused: bool, native_loop: bool = False):
        torch = _torch()
        dev = ws.hist.device
        self.ws = ws
        self.rr = torch.zeros(2, dtype=torch.float64, device=dev)
        self.pair_hist = torch.zeros(2, dtype=torch.float64, device=dev)
        rr = self.rr
        self.graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(self.graph):                           # capture only: nothing executes here
            _cg_iteration(A, ws.x, ws.r, ws.p, ws.Ap, rr[0:1], rr[1:2], ws.pAp, fused)
            self.pair_hist[0:1].copy_(rr[1:2])
            _cg_iteration(A, ws.x, ws.r, ws.p, ws.Ap, rr[1:2], rr[0:1], ws.pAp, fused)
            self.pair_hist[1:2].copy_(rr[0:1])

    def replay(self, n_pairs: int, record_history: bool = True) -> None:
        ws = self.ws
        self.rr[0:1].copy_(ws.hist[ws.done:ws.done + 1])
        for _ in range(n_pairs):
            self.graph.replay()
            if record_history:
                ws.hist[ws.done + 1:ws.done + 3].copy_(self.pair_hist)
            ws.done += 2
        if not record_history:
            ws.hist[ws.done:ws.done + 1].copy_(self.rr[0:1])


def _cg_graph_replay(A, ws: CGWorkspace, plan, fused: bool, iters: int) -> None:
    cg_iterate(A, ws, plan, fused, 2, native_loop=False)             # eager: allocations, plan probes
    g = CGGraphPair(A, ws, plan, fused)
    g.replay((iters - 2) // 2)
    if ws.done < iters:
        cg_iterate(A, ws, plan, fused, iters - ws.done, native_loop=False)


# ---- the converging solver ---------------------------------------------------------------------------------------------
class PCGWorkspace(_PairHistory):
    """What a ``cg`` solve allocates: x, r, p, Ap, the history of (sum r_j^2, sum r_j.(dinv r_j)) pairs (it IS the scalar
    storage of the iterations; it grows by doubling between chunks), pAp, and the scratch of the gated kernels whose last
    32 bytes are the solve's device state (done_iter, status, thr).  Reusable: every solve resets all of it.  ``u`` and ``z``
    (u = G r, z = Gt u) exist once a solve with ``M=<FSAI>`` has used the workspace, ``z`` and ``amg`` (the cycle's level vectors)
    once one with ``M=<AMG>`` has.  ``enqueue_ms``: set it to a list and every chunk appends the host's time in its enqueueing
    (milliseconds, the chunk's read-back outside); benchmarks/bench_amg.py reads it."""

    def __init__(self, b: HPCVector, hist_iters: int = 254):
        torch = _torch()
        dev = b.v.device
        self.x = HPCVector.zeros(b.partition, b.backend)
        self.r = b.similar()
        self.p = b.similar()
        self.Ap = b.similar()
        self.hist = torch.zeros(2 * (int(hist_iters) + 2), dtype=torch.float64, device=dev)
        self.pAp = torch.zeros(1, dtype=torch.float64, device=dev)
        self.tmp = torch.ones(2, dtype=torch.float64, device=dev)      # [0]: |b|^2 for a given x0; [1]: the constant 1
        self.work = torch.zeros(_capi.load().hpcla_pcg_work_bytes() // 8, dtype=torch.float64, device=dev)
        self.state = self.work[-4:].view(torch.int64)                  # done_iter, status, thr (a double), reserved
        self.u = self.z = self.amg = self._amg_of = None

    def fsai_vectors(self) -> None:
        if self.u is None:
            self.u = self.r.similar()
        if self.z is None:
            self.z = self.r.similar()

    def amg_vectors(self, mg) -> None:
        """z, and this workspace's own level vectors for the hierarchy ``mg``: allocated once, kept for later solves with it."""
        from .amg import AMGWorkspace
        if self.z is None:
            self.z = self.r.similar()
        if self.amg is None or self._amg_of is not mg:
            self.amg, self._amg_of = AMGWorkspace(mg.levels), mg

    def fits(self, b: HPCVector) -> bool:
        return self.x.structural_hash == b.structural_hash and self.x.v.device == b.v.device


def _cg_amg(A, M):
    """M when it is the hierarchy of ``hp.amg`` (amg.py is looked at only for an M that is nothing else), checked against A."""
    if M is None or isinstance(M, (str, HPCVector)):
        return None
    from .amg import AMG
    if not isinstance(M, AMG):
        return None
    top = M.levels[0].A
    if not np.array_equal(top.row_partition, A.row_partition) or top.shape != A.shape:
        raise ValueError("cg: the AMG preconditioner was built for a matrix of another shape or partition")
    if not M.symmetric:
        raise ValueError("cg: the AMG preconditioner was built with symmetric=False: its cycle is not a symmetric operator "
                         "(it is for hp.gmres and hp.bicgstab)")
    return M


def _cg_dinv(A, b: HPCVector, M) -> Optional[HPCVector]:
    if M is None:
        return None
    if isinstance(M, str):
        if M != "jacobi":
            raise ValueError(f"cg: unknown preconditioner {M!r} (None, 'jacobi' or an HPCVector of 1 ./ diagonal)")
        from .indexing import diag
        from .vectors import minimum
        if not (minimum(diag(A)) > 0):
            raise ValueError("cg: M='jacobi' needs a positive diagonal (minimum(diag(A)) > 0)")
        return diag(A, reciprocal=True)
    if not isinstance(M, HPCVector):
        raise ValueError("cg: M must be None, 'jacobi', an HPCVector on A's row partition, an FSAI (hp.fsai(A)) or an AMG "
                         "(hp.amg(A))")
    b._same_partition(M)
    return rd16_vector(M)                                        # the step kernels read it 16 bytes at a time


def cg(A, b: HPCVector, x0: Optional[HPCVector] = None, rtol: float = 1e-8, atol: float = 0.0,
       maxiter: Optional[int] = None, M=None, check_every: int = 8,
       workspace: Optional[PCGWorkspace] = None) -> Tuple[HPCVector, CGInfo]:
    """Solve ``A x = b`` for a symmetric positive definite ``A`` by (preconditioned) conjugate gradients.

    Stops at the first iteration with ``||r_k|| <= max(rtol * ||b||, atol)`` (scipy's rule; r_k is the recurrence residual),
    after ``maxiter`` iterations (default ``10 n``), or on a breakdown (``p.Ap <= 0`` or NaN: A is not positive definite
    along p).  ``M``: ``None``, ``"jacobi"`` (``1 ./ diag(A)``, formed on the device; the diagonal must be positive), an
    HPCVector holding the inverse diagonal to apply, or the ``FSAI`` object of ``hp.fsai(A)`` (``z = Gt (G r)``: two more SpMVs
    per iteration, ``r.M r`` formed as ``sum (G r)^2``), or the ``AMG`` object of ``hp.amg(A)`` (``z`` = one multigrid V-cycle on
    ``r``, enqueued from here between the gated steps; a hierarchy built with ``symmetric=False`` is refused with ValueError:
    its cycle is not symmetric).  ``x0`` defaults to zero.  Returns ``(x, CGInfo)``; x is the workspace's
    vector.

    The stop test and the breakdown test run on the device.  The host enqueues ``check_every`` iterations in one library
    call and then reads the 16-byte state (the only synchronisation); iterations enqueued behind the one that decided are
    no-ops, so the answer does not depend on ``check_every``.  With ``M=None`` the iterations produce the bits of
    ``cg_fixed_iterations``."""
    maxiter, check_every = _solver_arguments("cg", A, rtol, atol, maxiter, check_every)
    ws = workspace if workspace is not None and workspace.fits(b) else PCGWorkspace(b)
    plan = get_vector_plan(A, ws.p)
    if plan.result_partition_hash != ws.p.structural_hash:
        raise ValueError("cg: b must be partitioned like the rows of A")
    op = M if isinstance(M, FSAI) else None
    mg = _cg_amg(A, M) if op is None else None
    dinv = None if op is not None or mg is not None else _cg_dinv(A, b, M)
    if mg is not None:
        ws.amg_vectors(mg)
    if op is not None:
        if not np.array_equal(op.G.row_partition, A.row_partition) or op.G.shape != A.shape:
            raise ValueError("cg: the FSAI preconditioner was built for a matrix of another shape or partition")
        ws.fsai_vectors()
        plan_g, plan_t = get_vector_plan(op.G, ws.r), get_vector_plan(op.Gt, ws.u)
        if not (plan.is_i64 == plan_g.is_i64 == plan_t.is_i64):
            raise NotImplementedError("cg: the plans of A and of the FSAI factors use different index widths")
    dot_work = plan.dot_work(A)

    # -- setup: r0 = b - A x0, p0 = dinv r0, pair 0, the state ----------------------------------------------------------
    ws.hist.zero_()
    ws.work.zero_()                                              # done_iter = 0, status = running, thr = 0
    ws.tmp.fill_(1.0)
    ws.r.v.copy_(b.v)
    if x0 is None:
        ws.x.v.zero_()
    else:
        b._same_partition(x0)
        ws.x.v.copy_(x0.v)
        mul_(ws.Ap, A, ws.x)
        ws.r.axpy_(-1.0, ws.Ap)
        norm(b, 2, out=ws.tmp[0:1])
    norm(ws.r, 2, out=ws.hist[0:1])
    one = ws.tmp[1:2]
    if op is not None:                                           # u = G r, z = Gt u, p = z, pair 0's second slot = sum u^2
        mul_(ws.u, op.G, ws.r)
        mul_(ws.z, op.Gt, ws.u)
        ws.p.v.copy_(ws.z.v)
        norm(ws.u, 2, out=ws.hist[1:2])
    elif mg is not None:                                         # z = M r (one cycle), p = z, pair 0's second slot = r.z
        mg._cycle(0, ws.r, ws.z, ws.amg)
        ws.p.v.copy_(ws.z.v)
        dot(ws.r, ws.z, out=ws.hist[1:2])
    elif dinv is None:
        ws.p.v.copy_(ws.r.v)
        ws.hist[1:2].copy_(ws.hist[0:1])
    else:                                                        # p = dinv r + 1 * 0 through the direction kernel (x += 1 * 0)
        ws.p.v.zero_()
        _capi.call("hpcla_pcg_direction_f64", dptr(one), dptr(one), dptr(one), dptr(one), dptr(ws.r.v), dptr(dinv.v),
                   dptr(ws.x.v), dptr(ws.p.v), ws.x.local_length, 1, dptr(ws.state), current_stream_ptr())
        dot(ws.r, ws.p, out=ws.hist[1:2])
    done = _stop_rule_or_done(ws, b, x0 is not None, rtol, atol, maxiter)
    if done is not None:
        return ws.x, done

    # -- chunks of check_every iterations; one 16-byte read-back each ---------------------------------------------------------
    sfx = "i64" if plan.is_i64 else "i32"
    blk = plan.matrix_block(A)

    def enqueue_diagonal(first, count):
        _capi.call(f"hpcla_pcg_iterations_f64_{sfx}", blk[0], A.backend.rccl, *blk[1:],
                   dptr(dinv.v) if dinv is not None else None, dptr(ws.x.v), dptr(ws.r.v), dptr(ws.p.v), dptr(ws.Ap.v),
                   dptr(ws.hist), dptr(ws.pAp), dptr(dot_work), dptr(ws.work), first, count, current_stream_ptr())

    def enqueue_fsai(first, count):
        _capi.call(f"hpcla_pcg_fsai_iterations_f64_{sfx}", A.backend.rccl, *blocks, dptr(ws.x.v), dptr(ws.r.v), dptr(ws.p.v),
                   dptr(ws.Ap.v), dptr(ws.u.v), dptr(ws.z.v), dptr(ws.hist), dptr(ws.pAp), dptr(dot_work), dptr(ws.work),
                   first, count, current_stream_ptr())

    def enqueue_amg(first, count):
        """The order of hpcla_pcg_fsai_iterations_*, enqueued from here through the exported gated entries: Ap and pAp, the
        residual step (dinv == NULL), the cycle on r into z (not gated: behind the deciding iteration r is frozen and the cycle
        rewrites its own vectors with what they held), r.z into the pair's second slot, the direction step with z for r."""
        n, s, comm = ws.x.local_length, current_stream_ptr(), A.backend.rccl
        for j in range(first, first + count):
            prev, cur = ws.hist[2 * j - 1:2 * j], ws.hist[2 * j:2 * j + 2]
            mul_dot_(ws.Ap, A, ws.p, ws.pAp)
            _capi.call("hpcla_pcg_residual_f64", comm, dptr(prev), dptr(ws.pAp), dptr(ws.Ap.v), None, dptr(ws.r.v), n, j,
                       dptr(ws.state), dptr(cur), dptr(ws.work), s)
            mg._cycle(0, ws.r, ws.z, ws.amg)
            dot(ws.r, ws.z, out=cur[1:2])
            _capi.call("hpcla_pcg_direction_f64", dptr(prev), dptr(ws.pAp), dptr(cur[1:2]), dptr(prev), dptr(ws.z.v), None,
                       dptr(ws.x.v), dptr(ws.p.v), n, j, dptr(ws.state), s)

    if op is not None:
        blocks = blk + plan_g.matrix_block(op.G) + plan_t.matrix_block(op.Gt)
    enqueue = enqueue_fsai if op is not None else (enqueue_amg if mg is not None else enqueue_diagonal)
    iterations, status = _run_chunks(ws, A.backend, maxiter, check_every, enqueue)
    h = _residual_norms(ws, b.backend, iterations)
    return ws.x, CGInfo(status == 1, iterations, _STATUS[status], h)
