"""MINRES for a symmetric, possibly indefinite ``A`` (``hp.minres``), next to ``hp.cg``.

Saddle-point and KKT blocks, shifted operators ``A - sigma I``, negative definite operators: what ``ldlt(A) \\ b`` serves in the
reference (src/mumps_factorization.jl:247-259, MUMPS on the host).  ``hp.cg`` breaks down on them in its first or second
iteration (``p.Ap <= 0``); ``hp.gmres`` solves them but ignores the symmetry.  A caller of the reference composes MINRES from
``A*v`` (src/sparse.jl:2096-2128), ``dot`` (src/vectors.jl:798-812) and broadcast updates (src/vectors.jl:1203-1226): about ten
launches and three host read-backs per iteration.  Here an iteration is the SpMV with the partials of ``y . A y`` in its
epilogue and two gated HIP steps (csrc/vecops.hip, chained by ``hpcla_minres_iterations_f64_*`` in csrc/solvers.hip) whose scalars, stop rule and history stay
on the device; the host enqueues ``check_every`` iterations per library call and reads 16 bytes of state per chunk, exactly as
``hp.cg`` does.

Paige and Saunders' Lanczos recurrence with NO vector normalised in memory: r1 and r2 are kept unnormalised next to their
M-norms oldb and beta, y = M r2 is the SpMV's operand (r2 itself without M), v = y / beta is never stored.  Two buffers each of
r, w (and y with M) rotate by pointer inside the library's loop.  Gate order and rounding order (tests/_minres_cases.py restates
them):

    setup  x = x0 or 0;  r2 = b - A x;  y = M r2;  beta = sqrt(r2.y);  phibar = beta;  cs = -1;  sn = dbar = epsln = 0;  w1 = w2 = 0
    j      t = A y;  yt = y.t;  alfa = yt / (beta beta)
           rn = (t / beta - (alfa / beta) r2) - (beta / oldb) r1   (j = 1: no r1 term);  yn = M rn;  bb = rn.yn
           gate N  !(bb >= 0), or bb or alfa not finite: breakdown at j - 1
           beta' = sqrt(bb);  oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta'
           dbar = (-cs) beta';  gamma = sqrt(gbar gbar + beta' beta');  gate G  !(gamma > 0): breakdown at j - 1
           cs = gbar / gamma;  sn = beta' / gamma;  phi = cs phibar;  phibar = sn phibar;  hist j = phibar phibar
           gate C  hist j <= thr: converged at j;  oldb = beta;  beta = beta'
           w = ((y / oldb - oldeps w1) - delta w2) / gamma;  x = x + phi w;  (r1, r2, y, w1, w2) = (r2, rn, yn, w2, w)
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

from . import _capi
from .krylov import _STATUS, CGInfo, _PairHistory, _residual_norms, _run_chunks, _solver_arguments
from .partition import compute_partition_hash
from .sparse import get_vector_plan, mul_
from .vectors import HPCVector, current_stream_ptr, dot, dptr, maximum, minimum, norm, rd16_vector

# slots of the scalar buffer (include/hpcla_rocm.h); _B2 is its reserved slot, used by the setup only (b.M b for a given x0)
_BETA, _BB, _CS, _PHIBAR, _B2, _SCALARS = 0, 3, 5, 14, 15, 16


def _torch():
    import torch
    return torch


class MinresWorkspace(_PairHistory):
    """What a ``minres`` solve allocates: x, two buffers each of r and w, t (all partitioned like b; two more for y once a
    solve has a preconditioner), the history of (phibar_j^2, beta_{j+1}^2) pairs (it grows by doubling between chunks), the
    scalar slots, and the scratch of the gated kernels whose last 32 bytes are the solve's device state (done_iter, status,
    thr).  Reusable: every solve resets all of it."""

    def __init__(self, b: HPCVector, hist_iters: int = 254):
        torch = _torch()
        dev = b.v.device
        self.x = HPCVector.zeros(b.partition, b.backend)
        self.r = (b.similar(), b.similar())
        self.w = (b.similar(), b.similar())
        self.t = b.similar()
        self.y = None
        self.hist = torch.zeros(2 * (int(hist_iters) + 2), dtype=torch.float64, device=dev)
        self.scal = torch.zeros(_SCALARS, dtype=torch.float64, device=dev)
        self.work = torch.zeros(_capi.load().hpcla_minres_work_bytes() // 8, dtype=torch.float64, device=dev)
        self.state = self.work[-4:].view(torch.int64)                  # done_iter, status, thr (a double), reserved

    def fits(self, b: HPCVector) -> bool:
        return self.x.structural_hash == b.structural_hash and self.x.v.device == b.v.device


def _minres_dinv(A, b: HPCVector, M) -> Optional[HPCVector]:
    if M is None:
        return None
    if isinstance(M, str):
        if M != "jacobi":
            raise ValueError(f"minres: unknown preconditioner {M!r} (None, 'jacobi' or an HPCVector of positive weights)")
        from .indexing import diag
        d = diag(A)
        mag = HPCVector(d.structural_hash, d.partition, d.v.abs(), d.backend)
        if not (minimum(mag) > 0 and math.isfinite(maximum(mag))):
            raise ValueError("minres: M='jacobi' needs a diagonal without zero or non-finite entries (it applies 1 ./ abs(diag(A)))")
        mag.v = 1.0 / mag.v
        return mag
    if not isinstance(M, HPCVector):
        raise ValueError("minres: M must be None, 'jacobi' or an HPCVector on A's row partition")
    b._same_partition(M)
    M = rd16_vector(M)                                           # the check below and the step kernels read it 16 bytes at a time
    if not (minimum(M) > 0):
        raise ValueError("minres: M must be positive definite (minimum(M) > 0)")
    return M


def minres(A, b: HPCVector, x0: Optional[HPCVector] = None, rtol: float = 1e-8, atol: float = 0.0,
           maxiter: Optional[int] = None, M=None, check_every: int = 8,
           workspace: Optional[MinresWorkspace] = None) -> Tuple[HPCVector, CGInfo]:
    """Solve ``A x = b`` for a symmetric ``A``, definite or not, by (preconditioned) MINRES.  The caller asserts the symmetry;
    it is not checked.  The residual norm of the recurrence never rises.

    ``M`` must be positive definite and diagonal: ``None``, ``"jacobi"`` (``1 ./ abs(diag(A))``: a saddle-point matrix has
    diagonal entries of both signs; a zero or non-finite entry raises ``ValueError``) or an HPCVector of positive inverse
    diagonal weights on A's row partition.  ``x0`` defaults to zero.

    Stops at the first iteration with ``phibar_j <= max(rtol * sqrt(b . M b), atol)``, where ``phibar_j`` is the recurrence's
    residual norm; after ``maxiter`` iterations (default ``10 n``); or on a breakdown (a non-finite scalar or a Lanczos norm that
    is not a real number: x keeps its last value).  Without ``M`` this is ``hp.cg``'s rule, ``||r_j||_2 <= max(rtol ||b||_2,
    atol)``; with ``M`` both norms are the M norm ``sqrt(r . M r)``, as in scipy and MATLAB.  A singular inconsistent system is
    out of scope (it ends as "maxiter" or "breakdown"): ``hp.lsqr`` is the solver for it.  Returns ``(x, CGInfo)``; x is the
    workspace's vector and ``residual_norms`` holds ``|phibar_0| .. |phibar_iterations|``.

    The stop test and the breakdown tests run on the device.  The host enqueues ``check_every`` iterations in one library
    call and then reads the 16-byte state (the only synchronisation); iterations enqueued behind the one that decided are
    no-ops, so the answer does not depend on ``check_every``."""
    maxiter, check_every = _solver_arguments("minres", A, rtol, atol, maxiter, check_every)
    torch = _torch()
    if b.structural_hash != compute_partition_hash(A.row_partition):
        raise ValueError("minres: b must be partitioned like the rows of A")
    ws = workspace if workspace is not None and workspace.fits(b) else MinresWorkspace(b)
    plan = get_vector_plan(A, ws.r[0])
    if plan.result_partition_hash != ws.x.structural_hash:
        raise ValueError("minres: the columns of A must be partitioned like its rows")
    dinv = _minres_dinv(A, b, M)
    if dinv is not None and ws.y is None:
        ws.y = (b.similar(), b.similar())
    dot_work = plan.dot_work(A)
    comm, n_loc = A.backend.rccl, ws.x.local_length
    P = lambda v: dptr(v.v) if v is not None else None

    # -- setup: t = b - A x0, then r2 = t, y = dinv .* r2, bb = r2.y through the residual kernel; one read-back -----------
    ws.hist.zero_()
    ws.scal.zero_()
    ws.work.zero_()                                              # done_iter = 0, status = running, thr = 0
    ws.w[0].v.zero_()
    ws.w[1].v.zero_()
    ws.t.v.copy_(b.v)
    if x0 is None:
        ws.x.v.zero_()
    else:
        b._same_partition(x0)
        ws.x.v.copy_(x0.v)
        mul_(ws.r[1], A, ws.x)
        ws.t.axpy_(-1.0, ws.r[1])
        if dinv is None:
            norm(b, 2, out=ws.scal[_B2:_B2 + 1])
        else:
            dot(b, HPCVector(b.structural_hash, b.partition, dinv.v * b.v, b.backend), out=ws.scal[_B2:_B2 + 1])
    ws.r[1].v.zero_()                                            # r0 = t / 1 - (0 / 1) * 0: beta = 1, yt = 0, r2 = 0
    ws.scal[_BETA:_BETA + 1].fill_(1.0)
    _capi.call("hpcla_minres_r_f64", comm, dptr(ws.scal), dptr(ws.t.v), dptr(ws.r[1].v), P(dinv), dptr(ws.r[0].v),
               P(ws.y[0]) if dinv is not None else None, n_loc, 1, dptr(ws.state), None, dptr(ws.work), current_stream_ptr())
    first = ws.scal.cpu().tolist()
    rr0 = first[_BB]
    bb = first[_B2] if x0 is not None else rr0
    if bb == 0.0:                                                # b = 0: x = 0
        ws.x.v.zero_()
        return ws.x, CGInfo(True, 0, "converged", [0.0])
    thr = max(rtol * math.sqrt(bb), atol) ** 2 if bb >= 0 else math.nan
    if rr0 <= thr or maxiter == 0:
        if rr0 != rr0:
            from .sparse import check_exchange_health
            check_exchange_health(b.backend)
        return ws.x, CGInfo(rr0 <= thr, 0, "converged" if rr0 <= thr else "maxiter", [math.sqrt(rr0) if rr0 >= 0 else math.nan])
    beta1 = math.sqrt(rr0) if rr0 >= 0 else math.nan             # a NaN start ends at gate N of iteration 1
    init = [0.0] * _SCALARS
    init[_BETA], init[_PHIBAR], init[_CS] = beta1, beta1, -1.0
    ws.scal.copy_(torch.tensor(init, dtype=torch.float64))
    ws.hist[0:1].fill_(rr0)
    ws.work[-2:-1].fill_(thr)

    # -- chunks of check_every iterations; one 16-byte read-back each ---------------------------------------------------------
    sfx = "i64" if plan.is_i64 else "i32"
    blk = plan.matrix_block(A)
    ys = ws.y if dinv is not None else (None, None)

    def enqueue(first_iter, count):
        _capi.call(f"hpcla_minres_iterations_f64_{sfx}", blk[0], comm, *blk[1:], P(dinv), dptr(ws.x.v),
                   dptr(ws.r[0].v), dptr(ws.r[1].v), P(ys[0]), P(ys[1]), dptr(ws.w[0].v), dptr(ws.w[1].v), dptr(ws.t.v),
                   dptr(ws.hist), dptr(ws.scal), dptr(dot_work), dptr(ws.work), first_iter, count, current_stream_ptr())

    iterations, status = _run_chunks(ws, A.backend, maxiter, check_every, enqueue)
    h = _residual_norms(ws, b.backend, iterations)
    if status == 2:                                              # maybe the poison of an expired exchange wait -- ask
        from .sparse import check_exchange_health
        check_exchange_health(b.backend)
    return ws.x, CGInfo(status == 1, iterations, _STATUS[status], h)
