"""What the chunked Krylov solvers share (``hp.cg``, ``hp.bicgstab``, ``hp.gmres``, ``hp.minres``, ``hp.lsqr``).

Each of them enqueues ``check_every`` iterations per library call (the host-side loops of csrc/solvers.hip) and reads 16 bytes
of device state per chunk.  Here: the result record, the history of pairs that is the iterations' scalar storage, the argument
rules, the setup's stop rule, the chunk loop with its read-back, and the resolution of a preconditioner ``M`` that
``hp.bicgstab`` and ``hp.gmres`` have in common (an inverse diagonal, or the operator of ``hp.ilu0`` / ``hp.amg``).  ``hp.cg`` and
``hp.minres`` keep diagonal rules of their own (cg.py, minres.py): they ask different things of the diagonal.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .vectors import HPCVector, norm, rd16_vector


def _torch():
    import torch
    return torch


_STATUS = {0: "maxiter", 1: "converged", 2: "breakdown"}


@dataclass
class CGInfo:
    """What ``cg`` reports: ``iterations`` is the iteration the device stopped on (``maxiter`` when it did not stop),
    ``residual_norms`` holds ||r_0|| ... ||r_iterations|| of the recurrence residual."""
    converged: bool
    iterations: int
    status: str
    residual_norms: List[float]


class _PairHistory:
    """The history of a chunked solve (``cg``, ``bicgstab``): pairs of doubles, pair j written by iteration j; it IS the
    scalar storage of the iterations and grows by doubling between chunks."""

    def hist_capacity(self) -> int:
        return self.hist.numel() // 2 - 1                              # the last iteration whose pair fits

    def grow_hist(self, upto: int) -> None:
        torch = _torch()
        cap = self.hist.numel() // 2
        while cap - 1 < upto:
            cap *= 2
        new = torch.zeros(2 * cap, dtype=torch.float64, device=self.hist.device)
        new[:self.hist.numel()].copy_(self.hist)
        self.hist = new


def _solver_arguments(name: str, A, rtol: float, atol: float, maxiter: Optional[int], check_every: int) -> Tuple[int, int]:
    """The argument rules ``cg`` and ``bicgstab`` share.  Returns (maxiter, check_every)."""
    from .vectors import f64_only
    f64_only(A.backend, name)
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"{name}: the matrix must be square, got {A.shape[0]} x {A.shape[1]}")
    check_every = int(check_every)
    if check_every < 1:
        raise ValueError(f"{name}: check_every must be at least 1")
    if not (rtol >= 0 and atol >= 0):
        raise ValueError(f"{name}: rtol and atol must be non-negative")
    maxiter = 10 * int(A.shape[0]) if maxiter is None else int(maxiter)
    if maxiter < 0:
        raise ValueError(f"{name}: maxiter must be non-negative")
    return maxiter, check_every


def _stop_rule_or_done(ws, b, have_x0: bool, rtol: float, atol: float, maxiter: int) -> Optional["CGInfo"]:
    """After the setup (hist[0] = sum r_0^2, tmp[0] = |b|^2 when x0 was given): the setup's one read-back.  Returns the result
    of a solve that needs no iteration (b = 0, r_0 within the stop rule, maxiter = 0), else writes thr into the state."""
    rr0 = float(ws.hist[0].item())
    bb = float(ws.tmp[0].item()) if have_x0 else rr0
    if bb == 0.0:                                                # b = 0: x = 0
        ws.x.v.zero_()
        return CGInfo(True, 0, "converged", [0.0])
    thr = max(rtol * math.sqrt(bb), atol) ** 2
    if rr0 <= thr or maxiter == 0:
        if rr0 != rr0:
            from .sparse import check_exchange_health
            check_exchange_health(b.backend)
        return CGInfo(rr0 <= thr, 0, "converged" if rr0 <= thr else "maxiter", [math.sqrt(rr0)])
    ws.work[-2:-1].fill_(thr)
    return None


def _run_chunks(ws, backend, maxiter: int, check_every: int, enqueue) -> Tuple[int, int]:
    """Chunks of ``check_every`` iterations, ``enqueue(first_iter, count)`` each, one 16-byte read-back of the state per chunk.
    Returns (iterations, status); a status other than 0 is the device's, 0 means ``maxiter`` iterations ran."""
    from .backends import comm_allgather, comm_size
    multi = comm_size(backend.comm) > 1
    j, done_iter, status = 1, 0, 0
    while j <= maxiter:
        k = min(check_every, maxiter - j + 1)
        if j + k - 1 > ws.hist_capacity():
            ws.grow_hist(min(maxiter, 2 * (j + k)))
        clock = getattr(ws, "enqueue_ms", None)                  # a list: the host's time in each chunk's enqueueing is appended
        t0 = time.perf_counter() if clock is not None else 0.0
        enqueue(j, int(k))
        if clock is not None:
            clock.append((time.perf_counter() - t0) * 1e3)
        j += k
        done_iter, status = (int(v) for v in ws.state[:2].cpu().tolist())
        if multi:                                                # no rank leaves the loop alone, whatever produced its scalars
            every = comm_allgather(backend.comm, np.array([done_iter, status], dtype=np.int64)).reshape(-1, 2)
            stopped = every[every[:, 1] != 0]
            if len(stopped):
                done_iter, status = int(stopped[:, 0].min()), int(stopped[0, 1])
        if status != 0:
            break
    return (done_iter if status != 0 else maxiter), status


def _residual_norms(ws, backend, iterations: int) -> List[float]:
    """sqrt of the first entries of pairs 0 .. iterations, read back once."""
    h = ws.hist[0:2 * (iterations + 1):2].sqrt().cpu().tolist()
    if h[-1] != h[-1]:                         # NaN: the poison of an expired exchange wait -- ask
        from .sparse import check_exchange_health
        check_exchange_health(backend)
    return h


# ---- the preconditioner M of the nonsymmetric solvers (bicgstab, gmres) ----------------------------------------------------
def _bicgstab_dinv(A, b: HPCVector, M, name: str = "bicgstab") -> Optional[HPCVector]:
    if M is None:
        return None
    if isinstance(M, str):
        if M != "jacobi":
            raise ValueError(f"{name}: unknown preconditioner {M!r} (None, 'jacobi' or an HPCVector of 1 ./ diagonal)")
        from .indexing import diag
        dinv = diag(A, reciprocal=True)
        # minimum(abs(diag(A))) > 0  <=>  maximum(abs(1 ./ diag(A))) is finite (a missing or zero entry gives Inf)
        if not math.isfinite(norm(dinv, math.inf)):
            raise ValueError(f"{name}: M='jacobi' needs a diagonal without zeros (minimum(abs(diag(A))) > 0)")
        return dinv
    if not isinstance(M, HPCVector):
        raise ValueError(f"{name}: M must be None, 'jacobi', an HPCVector on A's row partition, an ILU0 (hp.ilu0(A)) or an AMG "
                         f"(hp.amg(A, symmetric=False))")
    b._same_partition(M)
    return rd16_vector(M)                                        # the step kernels read it 16 bytes at a time


class _AMGOperator:
    """The hierarchy of ``hp.amg`` (either mode) as the operator of one solver workspace: ``apply`` is one cycle in level vectors
    that belong to that workspace (allocated once, kept for later solves with the same hierarchy), so two solves with one
    hierarchy share none."""

    def __init__(self, mg, ws):
        from .amg import AMGWorkspace
        if getattr(ws, "amg", None) is None or ws._amg_of is not mg:
            ws.amg, ws._amg_of = AMGWorkspace(mg.levels), mg
        self.mg, self.work = mg, ws.amg

    def apply(self, r: HPCVector, out: HPCVector) -> HPCVector:
        return self.mg.apply(r, out=out, workspace=self.work)


def _ilu_operator(A, M, name: str, ws=None):
    """M when it is the operator of ``hp.ilu0``, or the hierarchy of ``hp.amg`` wrapped for the workspace ``ws`` (ilu.py and
    amg.py are looked at only for an M that is nothing else), checked against A."""
    if M is None or isinstance(M, (str, HPCVector)):
        return None
    from .amg import AMG
    if isinstance(M, AMG):
        top = M.levels[0].A
        if not np.array_equal(top.row_partition, A.row_partition) or top.shape != A.shape:
            raise ValueError(f"{name}: the AMG preconditioner was built for a matrix of another shape or partition")
        return _AMGOperator(M, ws)
    from .ilu import ILU0
    if not isinstance(M, ILU0):
        return None
    if not np.array_equal(M.row_partition, A.row_partition) or M.shape != tuple(int(v) for v in A.shape):
        raise ValueError(f"{name}: the ILU0 preconditioner was built for a matrix of another shape or partition")
    return M
