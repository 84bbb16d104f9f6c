"""BiCGStab for a square, not necessarily symmetric ``A`` (``hp.bicgstab``), next to ``hp.cg``.

The reference solves a general ``A \\ b`` through MUMPS on the host; a caller of its operators would compose a Krylov method
from ``A*p`` (src/sparse.jl:2096-2128), ``dot`` (src/vectors.jl:798-812) and broadcast updates (src/vectors.jl:1203-1226): five
host read-backs and about 13 launches per BiCGStab iteration.  Here an iteration is two SpMVs and five gated HIP steps
(csrc/vecops.hip, chained by ``hpcla_bicgstab_iterations_f64_*`` in csrc/solvers.hip) whose scalars, stop rule and breakdown tests stay on the device; the
host enqueues ``check_every`` iterations per library call and reads 16 bytes of state per chunk, exactly as ``hp.cg`` does.

Right-preconditioned, ``K`` = identity, ``dinv .*`` or the operator of ``hp.ilu0`` / ``hp.amg`` (ilu.py, amg.py; the same steps with ``dinv == NULL``,
enqueued one by one from here with ``K`` applied between them); gate order and rounding order (tests/_bicgstab_cases.py restates them):

    setup  x = x0 or 0;  r = b - A x;  rhat = r;  p = r;  rho = rhat.r;  hist[0] = r.r;  thr = max(rtol |b|, atol)^2
    j      ph = K p;  v = A ph;  rv = rhat.v                      gate A  !(rho != 0 and rv != 0): breakdown at j - 1
           a = rho / rv;  s = r - a v;  sh = K s;  t = A sh
           ts, tt, ss = t.s, t.t, s.s                             gate S  ss <= thr: x += a ph, converged at j (half step)
                                                                  gate T  !(tt > 0): breakdown at j - 1
           w = ts / tt;  x = (x + a ph) + w sh;  r = s - w t
           rho', rr = rhat.r, r.r                                 gate B  rr <= thr: converged at j
                                                                  gate O  ts == 0: breakdown at j
           b = (rho' / rho) (a / w);  p = r + b (p - w v);  rho = rho'
"""
from __future__ import annotations

from typing import Optional, Tuple

from . import _capi
from .krylov import (CGInfo, _bicgstab_dinv, _ilu_operator, _PairHistory, _residual_norms, _run_chunks, _solver_arguments,
                     _stop_rule_or_done)
from .sparse import get_vector_plan, mul_
from .vectors import HPCVector, current_stream_ptr, dptr, norm

_STATUS = {0: "maxiter", 1: "converged", 2: "breakdown", 3: "converged"}     # 3: converged at the half step


def _torch():
    import torch
    return torch


class BiCGStabWorkspace(_PairHistory):
    """What a ``bicgstab`` solve allocates: x, r, rhat, p, v, s, t (and ph, sh once a preconditioner is used), the history of
    (sum r_j^2, rhat.r_j) pairs (it IS the scalar storage of the iterations; it grows by doubling between chunks), the four
    scalars (rv, ts, tt, ss), and the scratch of the gated kernels whose last 32 bytes are the solve's device state
    (done_iter, status, thr).  Reusable: every solve resets all of it."""

    def __init__(self, b: HPCVector, hist_iters: int = 254):
        torch = _torch()
        dev = b.v.device
        self.x = HPCVector.zeros(b.partition, b.backend)
        self.r, self.rhat, self.p = b.similar(), b.similar(), b.similar()
        self.v, self.s, self.t = b.similar(), b.similar(), b.similar()
        self.ph: Optional[HPCVector] = None
        self.sh: Optional[HPCVector] = None
        self.hist = torch.zeros(2 * (int(hist_iters) + 2), dtype=torch.float64, device=dev)
        self.scal = torch.zeros(4, dtype=torch.float64, device=dev)
        self.tmp = torch.ones(3, dtype=torch.float64, device=dev)      # [0]: |b|^2 for a given x0; [1], [2]: the constant 1
        self.work = torch.zeros(_capi.load().hpcla_bicgstab_work_bytes() // 8, dtype=torch.float64, device=dev)
        self.state = self.work[-4:].view(torch.int64)                  # done_iter, status, thr (a double), reserved

    def fits(self, b: HPCVector) -> bool:
        return self.x.structural_hash == b.structural_hash and self.x.v.device == b.v.device

    def with_preconditioner(self) -> None:
        if self.ph is None:
            self.ph, self.sh = self.x.similar(), self.x.similar()


def bicgstab(A, b: HPCVector, x0: Optional[HPCVector] = None, rtol: float = 1e-8, atol: float = 0.0,
             maxiter: Optional[int] = None, M=None, check_every: int = 8,
             workspace: Optional[BiCGStabWorkspace] = None) -> Tuple[HPCVector, CGInfo]:
    """Solve ``A x = b`` for a square ``A`` (symmetry is not needed) by right-preconditioned BiCGStab.

    Stops at the first iteration with ``||r_k|| <= max(rtol * ||b||, atol)`` (``hp.cg``'s rule; also tested on the half-step
    residual ``s_k``), after ``maxiter`` iterations (default ``10 n``), or on a breakdown (``rhat.v``, ``rho``, ``t.t`` or
    ``t.s`` zero or NaN).  ``M``: ``None``, ``"jacobi"`` (``1 ./ diag(A)``, formed on the device; no diagonal entry may be
    zero), an HPCVector holding the inverse diagonal to apply, or the ``ILU0`` object of ``hp.ilu0(A)`` (``ph = M p``,
    ``sh = M s``: its triangular sweeps, enqueued from here between the gated steps), or the ``AMG`` object of ``hp.amg`` (one V-cycle
    each, enqueued the same way in level vectors that belong to the workspace; ``hp.amg(A, symmetric=False)`` for a nonsymmetric
    ``A``, and a symmetric hierarchy is a valid fixed operator too).  ``x0`` defaults to zero.  Returns
    ``(x, CGInfo)``; x is the workspace's vector, ``residual_norms[j]`` is ``||r_j||`` (``||s_j||`` for a half-step stop) of the
    recurrence.

    Every test runs on the device.  The host enqueues ``check_every`` iterations in one library call and then reads the
    16-byte state (the only synchronisation); iterations enqueued behind the one that decided are no-ops, so the answer does
    not depend on ``check_every``."""
    maxiter, check_every = _solver_arguments("bicgstab", A, rtol, atol, maxiter, check_every)
    ws = workspace if workspace is not None and workspace.fits(b) else BiCGStabWorkspace(b)
    plan = get_vector_plan(A, ws.p)
    if plan.result_partition_hash != ws.p.structural_hash:
        raise ValueError("bicgstab: b must be partitioned like the rows of A")
    op = _ilu_operator(A, M, "bicgstab", ws)
    dinv = None if op is not None else _bicgstab_dinv(A, b, M)

    # -- setup: r0 = b - A x0, rhat = p0 = r0, ph0 = dinv p0, pair 0, the state ------------------------------------------
    ws.hist.zero_()
    ws.scal.zero_()
    ws.work.zero_()                                              # done_iter = 0, status = running, thr = 0
    ws.tmp.fill_(1.0)
    ws.r.v.copy_(b.v)
    if x0 is None:
        ws.x.v.zero_()
    else:
        b._same_partition(x0)
        ws.x.v.copy_(x0.v)
        mul_(ws.v, A, ws.x)
        ws.r.axpy_(-1.0, ws.v)
        norm(b, 2, out=ws.tmp[0:1])
    ws.rhat.v.copy_(ws.r.v)
    norm(ws.r, 2, out=ws.hist[0:1])
    ws.hist[1:2].copy_(ws.hist[0:1])                             # rho_0 = rhat.r = r.r
    one = ws.tmp[1:2]
    if op is not None:                                           # p = r, ph = M p
        ws.with_preconditioner()
        ws.p.v.copy_(ws.r.v)
        op.apply(ws.p, out=ws.ph)
    elif dinv is None:
        ws.p.v.copy_(ws.r.v)
    else:                                                        # p = r + 1 * (0 - 1 * 0), ph = dinv p through the step-7 kernel
        ws.with_preconditioner()
        ws.p.v.zero_()
        ws.v.v.zero_()
        _capi.call("hpcla_bicg_p_f64", dptr(one), dptr(one), dptr(one), dptr(ws.tmp[1:3]), dptr(ws.r.v), dptr(ws.v.v), dptr(dinv.v),
                   dptr(ws.p.v), dptr(ws.ph.v), ws.x.local_length, 1, dptr(ws.state), current_stream_ptr())
    done = _stop_rule_or_done(ws, b, x0 is not None, rtol, atol, maxiter)
    if done is not None:
        return ws.x, done

    # -- chunks of check_every iterations; one 16-byte read-back each -------------------------------------------------------
    sfx = "i64" if plan.is_i64 else "i32"
    blk = plan.matrix_block(A)
    pre = (dptr(ws.ph.v), dptr(ws.sh.v)) if dinv is not None else (None, None)

    def enqueue(first, count):
        _capi.call(f"hpcla_bicgstab_iterations_f64_{sfx}", blk[0], A.backend.rccl, *blk[1:],
                   dptr(dinv.v) if dinv is not None else None, dptr(ws.x.v), dptr(ws.r.v), dptr(ws.rhat.v), dptr(ws.p.v),
                   pre[0], dptr(ws.v.v), dptr(ws.s.v), pre[1], dptr(ws.t.v), dptr(ws.hist), dptr(ws.scal), dptr(ws.work),
                   first, count, current_stream_ptr())

    def enqueue_operator(first, count):
        """The order of hpcla_bicgstab_iterations_*, enqueued from here through the exported gated entries with dinv == NULL;
        each ``dinv .*`` is ``op.apply`` (not gated: behind the deciding iteration s and p are frozen and the sweeps rewrite
        sh, ph and their own scratch with what they held)."""
        n, s, comm = ws.x.local_length, current_stream_ptr(), A.backend.rccl
        rv, triple = dptr(ws.scal), dptr(ws.scal[1:])
        state = dptr(ws.state)
        for j in range(first, first + count):
            rho, cur = dptr(ws.hist[2 * j - 1:]), dptr(ws.hist[2 * j:])
            mul_(ws.v, A, ws.ph)
            _capi.call("hpcla_bicg_dot_f64", comm, dptr(ws.rhat.v), dptr(ws.v.v), n, j, rho, state, rv, dptr(ws.work), s)
            _capi.call("hpcla_bicg_s_f64", rho, rv, dptr(ws.r.v), dptr(ws.v.v), None, dptr(ws.s.v), None, n, j, state, s)
            op.apply(ws.s, out=ws.sh)
            mul_(ws.t, A, ws.sh)
            _capi.call("hpcla_bicg_tts_f64", comm, dptr(ws.t.v), dptr(ws.s.v), n, j, state, triple, dptr(ws.work), s)
            _capi.call("hpcla_bicg_xr_f64", comm, rho, rv, triple, dptr(ws.ph.v), dptr(ws.sh.v), dptr(ws.s.v), dptr(ws.t.v),
                       dptr(ws.rhat.v), dptr(ws.x.v), dptr(ws.r.v), n, j, state, cur, dptr(ws.work), s)
            _capi.call("hpcla_bicg_p_f64", dptr(ws.hist[2 * j + 1:]), rho, rv, triple, dptr(ws.r.v), dptr(ws.v.v), None,
                       dptr(ws.p.v), None, n, j, state, s)
            op.apply(ws.p, out=ws.ph)

    iterations, status = _run_chunks(ws, A.backend, maxiter, check_every, enqueue_operator if op is not None else enqueue)
    h = _residual_norms(ws, b.backend, iterations)
    return ws.x, CGInfo(status in (1, 3), iterations, _STATUS[status], h)
