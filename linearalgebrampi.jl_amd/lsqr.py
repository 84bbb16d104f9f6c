"""LSQR for a rectangular ``A`` (``hp.lsqr``): least squares, minimum norm and the damped form, next to ``hp.cg``.

``min ||A x - b||`` for an over-determined system, the minimum-norm solution of an under-determined one, and the damped
(Tikhonov) form ``min ||A x - b||^2 + damp^2 ||x||^2`` -- what ``A \\ b`` means in Julia for a non-square ``A``.  The reference
has no such path (its ``A \\ b`` goes through MUMPS and needs a square matrix); a caller composes LSQR from ``A*v``
(src/sparse.jl:2096-2128), ``transpose(A)*u`` (src/sparse.jl:2136-2142), ``norm`` (src/vectors.jl:758-780) and broadcast
updates (src/vectors.jl:1203-1226): two SpMVs, about ten launches and four host read-backs per iteration.  Here an iteration
is the two SpMVs -- on ``A``'s plan and on the plan of the materialised, cached ``transpose(A)`` -- and three gated HIP steps
(csrc/vecops.hip, chained by ``hpcla_lsqr_iterations_f64_*`` in csrc/solvers.hip) whose scalars, stop rules and history stay on the device; the host
enqueues ``check_every`` iterations per library call and reads 16 bytes of state per chunk, exactly as ``hp.cg`` does.

Paige and Saunders' Golub-Kahan recurrences with NO vector normalised in memory: uh and vh are kept unnormalised next to their
norms beta and alpha, and the scalings ride in the passes that read the vectors anyway.  Every norm refers to the system
Abar = [A; damp I], bbar = [b; 0].  Gate order and rounding order (tests/_lsqr_cases.py restates them):

    setup  x = x0 or 0;  uh = b - A x;  uu = uh.uh;  beta = sqrt(uu);  tv = At uh;  vh = tv / beta;  vv = vh.vh
           alpha = sqrt(vv);  w = vh / alpha;  phibar = beta;  rhobar = alpha;  hist 0 = (uu, vv uu)
    j      tu = A vh;  uh = tu / alpha - (alpha / beta) uh;  uu = uh.uh;  beta' = sqrt(uu);  tv = At uh
           gate U  uu == 0: vh is left alone, alpha' = 0;  else vh = tv / beta' - (beta' / alpha) vh;  alpha' = sqrt(vh.vh)
           the scalar step (anorm2, the two rotations, t1, t2, rn2, arn);  hist j = (rn2, arn^2)
           gates  rn2 or arn not finite: breakdown at j - 1;  rn2 <= thr: converged at j
                  arn^2 <= ntol^2 anorm2 rn2: least squares at j
           x += t1 w;  w = vh / alpha' - t2 w          (x only in the iteration that stopped)
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

from . import _capi
from .krylov import _PairHistory, _run_chunks
from .partition import compute_partition_hash
from .sparse import get_vector_plan, mul_
from .transpose import TransposedHPCSparseMatrix
from .vectors import HPCVector, current_stream_ptr, dptr, f64_only, norm

_STATUS = {0: "maxiter", 1: "converged", 2: "breakdown", 3: "least_squares"}
# slots of the scalar buffer (include/hpcla_rocm.h); _BB is one of its reserved slots, used by the setup only
_ALPHA, _BETA, _UU, _VV, _PHIBAR, _RHOBAR, _ANORM2, _DAMP, _BB, _SCALARS = 0, 1, 2, 3, 4, 5, 7, 17, 18, 24


def _torch():
    import torch
    return torch


@dataclass
class LSQRInfo:
    """What ``lsqr`` reports: ``iterations`` is the iteration the device stopped on (``maxiter`` when it did not stop);
    ``residual_norms`` holds ||rbar_0|| ... ||rbar_iterations|| and ``normal_residual_norms`` ||Abar' rbar_0|| ..., both the
    recurrences' estimates for Abar = [A; damp I]; ``anorm`` is the running Frobenius estimate of Abar the second stop rule
    used.  ``converged`` is true for the statuses "converged" and "least_squares"."""
    converged: bool
    iterations: int
    status: str
    residual_norms: List[float]
    normal_residual_norms: List[float]
    anorm: float


class LSQRWorkspace(_PairHistory):
    """What an ``lsqr`` solve allocates: x, vh, w, tv on A's columns, uh, tu on A's rows, the history of (||rbar_j||^2,
    ||Abar' rbar_j||^2) pairs (it grows by doubling between chunks), the scalar slots, and the scratch of the gated kernels
    whose last 32 bytes are the solve's device state (done_iter, status, thr, ntol^2).  Reusable: every solve resets all of it."""

    def __init__(self, A, b: HPCVector, hist_iters: int = 254):
        torch = _torch()
        if isinstance(A, TransposedHPCSparseMatrix):
            A = A.materialize()
        dev = b.v.device
        self.x = HPCVector.zeros(A.col_partition, b.backend)
        self.vh, self.w, self.tv = self.x.similar(), self.x.similar(), self.x.similar()
        self.uh, self.tu = b.similar(), b.similar()
        self.hist = torch.zeros(2 * (int(hist_iters) + 2), dtype=torch.float64, device=dev)
        self.scal = torch.zeros(_SCALARS, dtype=torch.float64, device=dev)
        self.work = torch.zeros(_capi.load().hpcla_lsqr_work_bytes() // 8, dtype=torch.float64, device=dev)
        self.state = self.work[-4:].view(torch.int64)                  # done_iter, status, thr and ntol^2 (doubles)

    def fits(self, A, b: HPCVector) -> bool:
        if isinstance(A, TransposedHPCSparseMatrix):
            cols = A.parent.row_partition
        else:
            cols = A.col_partition
        return (self.x.structural_hash == compute_partition_hash(cols) and self.uh.structural_hash == b.structural_hash
                and self.x.v.device == b.v.device)


def lsqr(A, b: HPCVector, x0: Optional[HPCVector] = None, damp: float = 0.0, rtol: float = 1e-8, atol: float = 0.0,
         ntol: float = 1e-8, maxiter: Optional[int] = None, check_every: int = 8,
         workspace: Optional[LSQRWorkspace] = None) -> Tuple[HPCVector, LSQRInfo]:
    """Solve ``min ||A x - b||^2 + damp^2 ||x||^2`` for an ``A`` of any shape m x n (an HPCSparseMatrix, or a lazy
    ``transpose(B)``, which is materialised and then has ``B`` as its transpose) by LSQR.  From ``x0 = 0`` a consistent
    under-determined system gets its minimum-norm solution.  ``b`` lives on A's row partition; the returned ``x`` is the
    workspace's vector, on A's column partition.

    With Abar = [A; damp I] and rbar = [b; 0] - Abar x the solve stops at the first iteration with, in this order,
    ``||rbar|| <= max(rtol ||b||, atol)`` ("converged": ``hp.cg``'s rule, what a consistent system ends on), or
    ``||Abar' rbar|| <= ntol anorm ||rbar||`` ("least_squares": the normal equations' residual is small against the running
    Frobenius estimate ``anorm`` of Abar, scipy's second rule; what an inconsistent or damped system ends on); on a
    non-finite norm ("breakdown": x keeps its last finite value); or after ``maxiter`` iterations (default ``10 n``).  Both
    norms are the recurrences' estimates.  ``x0`` cannot be combined with ``damp != 0``: the damped correction problem is a
    different problem.  Returns ``(x, LSQRInfo)``.

    Every test runs on the device.  The host enqueues ``check_every`` iterations in one library call and then reads the
    16-byte state (the only synchronisation); iterations enqueued behind the one that decided are no-ops, so the answer does
    not depend on ``check_every``."""
    backend = A.parent.backend if isinstance(A, TransposedHPCSparseMatrix) else A.backend
    f64_only(backend, "lsqr")
    check_every = int(check_every)
    if check_every < 1:
        raise ValueError("lsqr: check_every must be at least 1")
    if not (rtol >= 0 and atol >= 0 and ntol >= 0):
        raise ValueError("lsqr: rtol, atol and ntol must be non-negative")
    if not (damp >= 0):
        raise ValueError("lsqr: damp must be non-negative")
    if x0 is not None and damp != 0:
        raise ValueError("lsqr: x0 cannot be combined with damp != 0 (the damped correction problem is a different problem)")
    if maxiter is not None and int(maxiter) < 0:
        raise ValueError("lsqr: maxiter must be non-negative")
    if isinstance(A, TransposedHPCSparseMatrix):
        A = A.materialize()
    maxiter = 10 * int(A.shape[1]) if maxiter is None else int(maxiter)
    if b.structural_hash != compute_partition_hash(A.row_partition):
        raise ValueError("lsqr: b must be partitioned like the rows of A")
    if x0 is not None and x0.structural_hash != compute_partition_hash(A.col_partition):
        raise ValueError("lsqr: x0 must be partitioned like the columns of A")
    At = TransposedHPCSparseMatrix(A).materialize()
    ws = workspace if workspace is not None and workspace.fits(A, b) else LSQRWorkspace(A, b)
    plan, plan_t = get_vector_plan(A, ws.vh), get_vector_plan(At, ws.uh)
    if plan.is_i64 != plan_t.is_i64:
        raise NotImplementedError("lsqr: the plans of A and of its transpose use different index widths (one of them was "
                                  "narrowed to Int32, the other could not be: a dimension or the nonzero count is near 2^31)")
    comm, s = backend.rccl, current_stream_ptr()
    m_loc, n_loc = ws.uh.local_length, ws.x.local_length

    # -- setup: uh = b - A x0, vh = At uh / beta, their norms; one read-back; then the scalars, pair 0, the state, w ----------
    ws.hist.zero_()
    ws.scal.zero_()
    ws.work.zero_()                                              # done_iter = 0, status = running, thr = ntol^2 = 0
    ws.vh.v.zero_()
    ws.w.v.zero_()
    ws.uh.v.copy_(b.v)
    if x0 is None:
        ws.x.v.zero_()
    else:
        ws.x.v.copy_(x0.v)
        mul_(ws.tu, A, ws.x)
        ws.uh.axpy_(-1.0, ws.tu)
        norm(b, 2, out=ws.scal[_BB:_BB + 1])
    norm(ws.uh, 2, out=ws.scal[_UU:_UU + 1])
    mul_(ws.tv, At, ws.uh)
    ws.scal[_ALPHA:_ALPHA + 1].fill_(1.0)                        # vh = tv / beta - (beta / 1) * 0 through the step-4 kernel
    _capi.call("hpcla_lsqr_v_f64", comm, dptr(ws.scal), dptr(ws.tv.v), dptr(ws.vh.v), n_loc, 1, dptr(ws.state), None,
               dptr(ws.work), s)
    first = ws.scal.cpu().tolist()
    uu, vv = first[_UU], first[_VV]
    bb = first[_BB] if x0 is not None else uu
    if bb == 0.0:                                                # b = 0: x = 0
        ws.x.v.zero_()
        return ws.x, LSQRInfo(True, 0, "converged", [0.0], [0.0], 0.0)
    thr = max(rtol * math.sqrt(bb), atol) ** 2
    h0 = [math.sqrt(uu) if uu >= 0 else math.nan]
    n0 = [math.sqrt(vv * uu) if vv * uu >= 0 else math.nan]
    early = None
    if uu <= thr:
        early = "converged"
    elif not math.isfinite(vv):
        early = "breakdown"
    elif vv == 0.0:
        early = "least_squares"                                  # b is orthogonal to range(A): x stays
    elif maxiter == 0:
        early = "maxiter"
    if early is not None:
        if uu != uu or vv != vv:
            from .sparse import check_exchange_health
            check_exchange_health(backend)
        return ws.x, LSQRInfo(early in ("converged", "least_squares"), 0, early, h0, n0, 0.0)
    alpha, beta = math.sqrt(vv), math.sqrt(uu)
    torch = _torch()
    init = [0.0] * _SCALARS
    init[_ALPHA], init[_BETA], init[_PHIBAR], init[_RHOBAR], init[_DAMP] = alpha, beta, beta, alpha, float(damp)
    ws.scal.copy_(torch.tensor(init, dtype=torch.float64))
    ws.hist[0:2].copy_(torch.tensor([uu, vv * uu], dtype=torch.float64))
    ws.work[-2:].copy_(torch.tensor([thr, float(ntol) * float(ntol)], dtype=torch.float64))
    _capi.call("hpcla_lsqr_xw_f64", dptr(ws.scal), dptr(ws.vh.v), dptr(ws.x.v), dptr(ws.w.v), n_loc, 1, dptr(ws.state), s)   # w = vh / alpha

    # -- chunks of check_every iterations; one 16-byte read-back each -------------------------------------------------------
    sfx = "i64" if plan.is_i64 else "i32"
    blocks = plan.matrix_block(A) + plan_t.matrix_block(At)

    def enqueue(first_iter, count):
        _capi.call(f"hpcla_lsqr_iterations_f64_{sfx}", comm, *blocks, dptr(ws.x.v), dptr(ws.uh.v), dptr(ws.vh.v), dptr(ws.w.v),
                   dptr(ws.tu.v), dptr(ws.tv.v), dptr(ws.hist), dptr(ws.scal), dptr(ws.work), first_iter, count,
                   current_stream_ptr())

    iterations, status = _run_chunks(ws, backend, maxiter, check_every, enqueue)
    pairs = ws.hist[0:2 * (iterations + 1)].sqrt().cpu().tolist()
    anorm2 = float(ws.scal[_ANORM2].item())
    if pairs[-2] != pairs[-2] or status == 2:                    # NaN: maybe the poison of an expired exchange wait -- ask
        from .sparse import check_exchange_health
        check_exchange_health(backend)
    return ws.x, LSQRInfo(status in (1, 3), iterations, _STATUS[status], pairs[0::2], pairs[1::2],
                          math.sqrt(anorm2) if anorm2 >= 0 else math.nan)
