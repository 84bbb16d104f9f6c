"""GPU tests of the BiCGStab solver: the gated step kernels on their own through the C ABI, ``hp.bicgstab`` against the numpy
restatement, independence of the chunk, the freeze behind the deciding iteration, breakdowns, convergence on the
convection-diffusion cases and the solve across ranks.  Cases and the restatement: tests/_bicgstab_cases.py.

Margins (none of them taken from the device's results; tests/test_bicgstab_cases.py re-measures the CPU figures and prints them):
  * elements of s, sh, x, r, p, ph: bit-equal to numpy's separately rounded expressions (the library is built with
    -ffp-contract=off);
  * the six sums: 1e-12 of math.fsum relative to the sum of |terms| -- the terms of a dot are signed, so relative to the sum
    itself would test cancellation and not the kernel; n <= 4.2e6 terms in a two-stage tree of doubles, worst case
    n * 2^-53 = 4.7e-10, observed growth ~ sqrt(log n) ulps; 1e-12 is the project's margin for its reductions;
  * histories: HIST_RTOL = 1e-12 on the first HEAD = 5 entries: four summation orders on the CPU spread by <= 6.5e-14 there
    (15 times less) and by 3e-12 at entry 13 -- BiCGStab amplifies rounding much faster than CG, so only the head is compared;
    at 65 x 63 they spread by <= 3.3e-14 over the same head (30 times less);
  * iteration counts with Jacobi: +-2 of the restatement's (33 / 40 / 59, identical across those orders; 108-111 / 133-141 /
    174-182 without), and 2 * jacobi <= none (>= 1.47 times that in every order);
  * true residual: <= 2 rtol (0.17-0.97 rtol across those orders).
"""
import math
import os

import numpy as np
import pytest

from tests import _bicgstab_cases as bc
from tests import _grid_regimes as gr
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_bicgstab_worker.py")

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN, HALF = 0, 1, 2, 3


def _matrix(hp, backend, rowptr, colidx, vals, n):
    return hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, backend)


@pytest.fixture(scope="module")
def cases(orc):
    """The three convection-diffusion cases with the restatement's results, computed once."""
    out = {}
    for nx, ny in bc.SIZES:
        rowptr, colidx, vals, b = bc.convection_diffusion(orc, nx, ny)
        d = pc.host_diag(rowptr, colidx, vals)
        ref = {"jacobi": bc.bicgstab(rowptr, colidx, vals, b, dinv=1.0 / d, rtol=1e-8),
               "none": bc.bicgstab(rowptr, colidx, vals, b, rtol=1e-8)}
        out[(nx, ny)] = dict(rowptr=rowptr, colidx=colidx, vals=vals, b=b, d=d, ref=ref)
    return out


# ---- 1. the kernels on their own ----------------------------------------------------------------------------------------
def _sum_err(got, terms):
    return abs(got - math.fsum(terms.tolist())) / float(np.abs(terms).sum())


@pytest.mark.parametrize("n", gr.BICGSTAB_ALONE)
def test_gated_kernels_alone(hp, n):
    """The reductions (bicg_dot, bicg_tts, bicg_xr) use the grid of the existing stage-1 reductions, ceil(floor(n / 2) / 1024)
    capped at 2048: 2049 is the last size on one workgroup with a scalar tail, 2051 the first odd size on two,
    4 194 307 = 2 * 256 * 4 * 2048 + 3 caps the grid and is odd.  The elementwise kernels (bicg_s, bicg_p) use
    ceil(floor(n / 2) / 256) capped at 4096: 511 is the last odd size on one workgroup, 515 the first on two, and the largest
    size makes every thread stride twice.  614 403 is odd with 301 partials: the gated second stages walk them in two trips of
    256 lanes, the last one ragged (45 lanes), and the elementwise kernels have 1201 workgroups.  tests/_grid_regimes.py holds
    the sizes and tests/test_grid_regimes.py checks that they reach every regime of both grids."""
    import torch
    lib = hp._capi.load()
    rng = np.random.default_rng(n)
    host = {k: rng.uniform(-1.0, 1.0, n) for k in ("r", "v", "t", "x", "p", "rhat")}
    host["dinv"] = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)          # a diagonal need not be positive here
    rho, rv, ts, tt, rho_new, j = 0.7310585786300049, -1.9, 0.6, 1.7, -0.37, 5
    a, w = rho / rv, ts / tt
    beta = (rho_new / rho) * (a / w)
    f64 = dict(dtype=torch.float64, device="cuda")
    scal = torch.tensor([rho, rv, ts, tt, 0.0, rho_new, 0.0, float("nan")], **f64)   # [4], [6]: zeros, [7]: NaN
    RHO, RV, TRIPLE, RHO_NEW = scal[0:1], scal[1:2], scal[2:5], scal[5:6]
    work = torch.zeros(lib.hpcla_bicgstab_work_bytes() // 8, **f64)
    up = lambda k: torch.from_numpy(host[k]).cuda()
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    P = lambda t: t.data_ptr() if t is not None else None
    bits_eq = lambda t, want: np.array_equal(pc.bits(t.cpu().numpy()), pc.bits(want))
    same = lambda t, u: torch.equal(t.view(torch.int64), u.view(torch.int64))
    fresh_state = lambda thr=0.0: torch.tensor([0, RUNNING, np.float64(thr).view(np.int64), 0], dtype=torch.int64, device="cuda")
    read = lambda st: st.cpu().tolist()[:2]
    rhat, v, t, dinv = up("rhat"), up("v"), up("t"), up("dinv")
    ones = torch.ones(n, **f64)

    def k_dot(v_, st, out, rho_=RHO):
        assert lib.hpcla_bicg_dot_f64(None, P(rhat), P(v_), n, j, P(rho_), P(st), P(out), P(work), None) == 0

    def k_s(r_, d_, s_, sh_, st, rv_=RV):
        assert lib.hpcla_bicg_s_f64(P(RHO), P(rv_), P(r_), P(v), P(d_), P(s_), P(sh_), n, j, P(st), None) == 0

    def k_tts(t_, s_, st, out):
        assert lib.hpcla_bicg_tts_f64(None, P(t_), P(s_), n, j, P(st), P(out), P(work), None) == 0

    def k_xr(ph_, sh_, s_, x_, r_, st, pair, triple=TRIPLE):
        assert lib.hpcla_bicg_xr_f64(None, P(RHO), P(RV), P(triple), P(ph_), P(sh_), P(s_), P(t), P(rhat), P(x_), P(r_), n, j,
                                     P(st), P(pair), P(work), None) == 0

    def k_p(r_, d_, p_, ph_, st):
        assert lib.hpcla_bicg_p_f64(P(RHO_NEW), P(RHO), P(RV), P(TRIPLE), P(r_), P(v), P(d_), P(p_), P(ph_), n, j, P(st),
                                    None) == 0

    # -- with dinv, running: every step from hand-set scalars
    st = fresh_state()
    s_h = host["r"] - a * host["v"]
    sh_h = host["dinv"] * s_h
    ph_h = host["dinv"] * host["p"]
    x_h = (host["x"] + a * ph_h) + w * sh_h
    r_h = s_h - w * host["t"]
    p_h = r_h + beta * (host["p"] - w * host["v"])
    rv_out, triple_out, pair = torch.zeros(1, **f64), torch.zeros(3, **f64), torch.tensor([3.0, 4.0], **f64)
    s, sh = torch.full((n,), 7.0, **f64), torch.full((n,), 7.0, **f64)
    ph, x, r, p = dev(ph_h), up("x"), up("r"), up("p")
    k_dot(v, st, rv_out)
    k_s(r, dinv, s, sh, st)
    k_tts(t, s, st, triple_out)
    k_xr(ph, sh, s, x, r, st, pair)
    k_p(r, dinv, p, ph, st)
    torch.cuda.synchronize()
    assert bits_eq(s, s_h) and bits_eq(sh, sh_h)
    assert bits_eq(x, x_h) and bits_eq(r, r_h)
    assert bits_eq(p, p_h) and bits_eq(ph, host["dinv"] * p_h)
    errs = {"rhat.v": _sum_err(rv_out.item(), host["rhat"] * host["v"]),
            "t.s": _sum_err(triple_out[0].item(), host["t"] * s_h), "t.t": _sum_err(triple_out[1].item(), host["t"] * host["t"]),
            "s.s": _sum_err(triple_out[2].item(), s_h * s_h),
            "r.r": _sum_err(pair[0].item(), r_h * r_h), "rhat.r": _sum_err(pair[1].item(), host["rhat"] * r_h)}
    print(f"n = {n}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert all(e <= 1e-12 for e in errs.values()), errs
    assert st.cpu().tolist()[:2] == [0, RUNNING]                                        # thr = 0 < every sum of squares

    # -- dinv = NULL and dinv = 1: the same bits
    runs = []
    for d_ in (None, ones):
        pre = d_ is not None
        s1, x1, r1, p1 = torch.full((n,), 7.0, **f64), up("x"), up("r"), up("p")
        sh1 = torch.full((n,), 7.0, **f64) if pre else None
        ph1 = up("p") if pre else None                                                  # 1 .* p
        pair1, tr1 = torch.zeros(2, **f64), torch.zeros(3, **f64)
        k_s(r1, d_, s1, sh1, st)
        k_tts(t, s1, st, tr1)
        k_xr(ph1 if pre else p1, sh1, s1, x1, r1, st, pair1)
        k_p(r1, d_, p1, ph1, st)
        torch.cuda.synchronize()
        if pre:
            assert same(sh1, s1) and same(ph1, p1)
        runs.append((s1, x1, r1, p1, pair1, tr1))
    for got, want in zip(runs[0], runs[1]):
        assert same(got, want)
    assert bits_eq(runs[0][1], (host["x"] + a * host["p"]) + w * s_h) and bits_eq(runs[0][3], p_h)

    # -- frozen: no kernel writes a byte (converged, broken down, or a half step of another iteration)
    for frozen in ([j - 1, CONVERGED], [j, CONVERGED], [j - 1, BREAKDOWN], [j - 1, HALF], [j + 1, HALF]):
        stf = torch.tensor(frozen + [0, 0], dtype=torch.int64, device="cuda")
        outs = [torch.full((k,), 7.0, **f64) for k in (1, 3, 2)]
        vecs = [torch.full((n,), 7.0, **f64) for _ in range(6)]                          # s, sh, x, r, p, ph
        k_dot(v, stf, outs[0])
        k_s(up("r"), dinv, vecs[0], vecs[1], stf)
        k_tts(t, up("r"), stf, outs[1])
        k_xr(up("p"), up("r"), up("r"), vecs[2], vecs[3], stf, outs[2])
        k_p(up("r"), dinv, vecs[4], vecs[5], stf)
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs + vecs), frozen
        assert stf.cpu().tolist() == frozen + [0, 0]

    # -- the half-step form: status 3 at this iteration updates x only, and its gate stores ss as the pair's first entry
    half_triple = torch.tensor([ts, tt, 0.25], **f64)
    for sh_ in (None, sh):
        sth = torch.tensor([j, HALF, 0, 0], dtype=torch.int64, device="cuda")
        x2, r2, pair2 = up("x"), torch.full((n,), 7.0, **f64), torch.tensor([3.0, 4.0], **f64)
        k_xr(ph, sh_, s, x2, r2, sth, pair2, triple=half_triple)
        torch.cuda.synchronize()
        assert bits_eq(x2, host["x"] + a * (host["dinv"] * p_h)) and bool((r2 == 7.0).all())   # ph now holds dinv .* p_new
        assert pair2.cpu().tolist() == [0.25, 4.0] and sth.cpu().tolist() == [j, HALF, 0, 0]

    # -- gate A: rho = 0, rho = NaN, rhat.v = 0 -> breakdown at j - 1; bicg_s under gate A's predicate writes nothing
    zeros = torch.zeros(n, **f64)
    for v_, rho_ in ((v, scal[4:5]), (v, scal[7:8]), (zeros, RHO)):
        sta = fresh_state()
        k_dot(v_, sta, rv_out, rho_)
        torch.cuda.synchronize()
        assert read(sta) == [j - 1, BREAKDOWN]
    sta = fresh_state()
    s3 = torch.full((n,), 7.0, **f64)
    k_s(up("r"), None, s3, None, sta, rv_=scal[4:5])                                    # rv = 0, state still running
    torch.cuda.synchronize()
    assert bool((s3 == 7.0).all()) and read(sta) == [0, RUNNING]
    # -- gate S: ss <= thr -> status 3 at j;  gate T: t = 0 -> breakdown at j - 1
    sts = fresh_state(4.0 * n)                                                          # |s| < 2 elementwise: ss < 4 n
    k_tts(t, s, sts, triple_out)
    torch.cuda.synchronize()
    assert read(sts) == [j, HALF] and 0.0 < triple_out[2].item() <= 4.0 * n
    stt = fresh_state()
    pair3 = torch.tensor([3.0, 4.0], **f64)
    k_tts(zeros, s, stt, triple_out)
    torch.cuda.synchronize()
    assert read(stt) == [j - 1, BREAKDOWN] and triple_out[1].item() == 0.0
    # -- gate B: rr <= thr -> converged at j;  gate O: ts = 0 -> breakdown at j with x and r updated
    stb = fresh_state(16.0 * n)                                                         # |r| < 1 + |w| < 2 elementwise
    k_xr(ph, sh, s, up("x"), up("r"), stb, pair3)
    torch.cuda.synchronize()
    assert read(stb) == [j, CONVERGED]
    sto = fresh_state()
    x4, r4 = up("x"), torch.full((n,), 7.0, **f64)
    k_xr(ph, sh, s, x4, r4, sto, pair3, triple=torch.tensor([0.0, tt, 0.0], **f64))
    torch.cuda.synchronize()
    assert read(sto) == [j, BREAKDOWN]
    assert bits_eq(r4, s_h - 0.0 * host["t"]) and bits_eq(x4, (host["x"] + a * (host["dinv"] * p_h)) + 0.0 * sh_h)


# ---- 2. the head of the history against the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_history_head_matches_the_restatement(hp, cases, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    """First HEAD = 5 entries within HIST_RTOL = 1e-12: 15 times the spread of four summation orders on the CPU (6.5e-14,
    tests/test_bicgstab_cases.py prints it)."""
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    c = cases[(24, 20)]
    n = len(c["b"])
    A = _matrix(hp, backend, c["rowptr"], c["colidx"], c["vals"], n)
    b = hp.HPCVector.from_global(c["b"], backend)
    for name, M, dinv in (("jacobi", "jacobi", 1.0 / c["d"]), ("none", None, None)):
        _, its_ref, status_ref, h_ref = bc.bicgstab(c["rowptr"], c["colidx"], c["vals"], c["b"], dinv=dinv, rtol=0.0, atol=0.0,
                                                    maxiter=8)
        assert (its_ref, status_ref, len(h_ref)) == (8, "maxiter", 9)
        x, info = hp.bicgstab(A, b, rtol=0.0, atol=0.0, maxiter=8, M=M, check_every=8)
        assert (info.iterations, info.status, info.converged) == (8, "maxiter", False)
        assert len(info.residual_norms) == 9
        head = max(abs(g - w_) / w_ for g, w_ in zip(info.residual_norms[:bc.HEAD], h_ref[:bc.HEAD]))
        print(f"{which} {name}: head deviation {head:.2e}")
        assert head <= bc.HIST_RTOL, (name, head)
    hp.clear_plan_cache()


def test_history_head_at_the_large_size(hp, orc, gpu_backend_i32):
    """65 x 63: 4095 rows, odd, so every reduction of the step runs on two stage-1 workgroups and the gated second stages add
    two partials (the other solves of this file stay on one).  The first HEAD = 5 entries within HIST_RTOL = 1e-12: 30 times the
    spread of four summation orders on the CPU at this size (3.3e-14 with Jacobi, 4.7e-15 without;
    tests/test_bicgstab_cases.py re-measures both).  No convergence or count is asserted here."""
    rowptr, colidx, vals, bg = bc.convection_diffusion(orc, *bc.LARGE_SIZE)
    n = len(bg)
    d = pc.host_diag(rowptr, colidx, vals)
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, vals, n)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    for name, M, dinv in (("jacobi", "jacobi", 1.0 / d), ("none", None, None)):
        _, its_ref, status_ref, h_ref = bc.bicgstab(rowptr, colidx, vals, bg, dinv=dinv, rtol=0.0, atol=0.0, maxiter=bc.HEAD)
        assert (its_ref, status_ref, len(h_ref)) == (bc.HEAD, "maxiter", bc.HEAD + 1)
        x, info = hp.bicgstab(A, b, rtol=0.0, atol=0.0, maxiter=bc.HEAD, M=M)
        assert (info.iterations, info.status, info.converged) == (bc.HEAD, "maxiter", False)
        assert len(info.residual_norms) == bc.HEAD + 1
        head = max(abs(g - w_) / w_ for g, w_ in zip(info.residual_norms[:bc.HEAD], h_ref[:bc.HEAD]))
        print(f"{bc.LARGE_SIZE} {name}: head deviation {head:.2e}")
        assert head <= bc.HIST_RTOL, (name, head)
    hp.clear_plan_cache()


# ---- 3. the chunk -----------------------------------------------------------------------------------------------------------
def test_answer_does_not_depend_on_the_chunk(hp, cases, gpu_backend_i32):
    c = cases[(24, 20)]
    A = _matrix(hp, gpu_backend_i32, c["rowptr"], c["colidx"], c["vals"], len(c["b"]))
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    runs = []
    for chunk in (1, 3, 8, 64):
        x, info = hp.bicgstab(A, b, M="jacobi", rtol=1e-8, check_every=chunk)
        assert info.converged
        runs.append((info.iterations, pc.bits(x.local_values()).copy(), pc.bits(info.residual_norms).copy()))
    for its, xb, hb in runs[1:]:
        assert its == runs[0][0] and np.array_equal(xb, runs[0][1]) and np.array_equal(hb, runs[0][2])


# ---- 4. the freeze ----------------------------------------------------------------------------------------------------------
def test_freeze_on_a_diagonal_system_and_a_dirty_workspace(hp, orc, gpu_backend_i32):
    rowptr, colidx, d, bg = pc.diagonal_case(orc)
    n = len(bg)
    _, its_ref, status_ref, _ = bc.bicgstab(rowptr, colidx, d, bg, dinv=1.0 / d, rtol=1e-8, maxiter=50)
    assert (its_ref, status_ref) == (1, "converged")
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, d, n)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    ws = hp.BiCGStabWorkspace(b)
    x, info = hp.bicgstab(A, b, M="jacobi", rtol=1e-8, check_every=8, maxiter=50, workspace=ws)
    assert x is ws.x
    assert (info.converged, info.iterations, info.status, len(info.residual_norms)) == (True, 1, "converged", 2)
    xv = x.local_values()
    assert np.all(np.isfinite(xv)) and np.all(np.abs(xv - bg / d) <= 4 * np.spacing(np.abs(bg / d)))
    # a second solve on the now dirty workspace, and one on a workspace dirtied by a different solve: a fresh one's bits
    x2, info2 = hp.bicgstab(A, b, M="jacobi", rtol=1e-8, check_every=8, maxiter=50, workspace=ws)
    assert info2 == info and np.array_equal(pc.bits(x2.local_values()), pc.bits(xv))
    hp.bicgstab(A, b, M=None, rtol=0.0, maxiter=3, workspace=ws)
    x3, info3 = hp.bicgstab(A, b, M="jacobi", rtol=1e-8, check_every=8, maxiter=50, workspace=ws)
    assert info3 == info and np.array_equal(pc.bits(x3.local_values()), pc.bits(xv))


def test_freeze_on_the_identity(hp, orc, gpu_backend_i32):
    bg = orc.fill_uniform(0, 5, pc.SEED_RHS)
    A = _matrix(hp, gpu_backend_i32, *pc.diag_matrix(np.ones(5)), 5)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    x, info = hp.bicgstab(A, b, M=None, rtol=0.0, atol=0.0)                            # thr = 0, s_1 = 0 exactly; carried on: 0 / 0
    assert (info.converged, info.iterations, info.status) == (True, 1, "converged")
    assert info.residual_norms[1] == 0.0 and np.array_equal(pc.bits(x.local_values()), pc.bits(bg))
    # b = 0: x = 0 without an iteration
    x, info = hp.bicgstab(A, hp.HPCVector.from_global(np.zeros(5), gpu_backend_i32))
    assert (info.converged, info.iterations, info.status, info.residual_norms) == (True, 0, "converged", [0.0])
    assert not x.local_values().any()


def test_half_step_stop_reports_the_norm_of_s(hp, orc, gpu_backend_i32):
    """A half-step stop with ss > 0 (tests/_bicgstab_cases.py): the whole history within HALF_HIST_RTOL = 1e-11 of the
    restatement's (45 times the CPU spread of four summation orders) and the last entry within the stop rule."""
    rowptr, colidx, vals, bg = bc.convection_diffusion(orc, *bc.HALF_SIZE)
    d = pc.host_diag(rowptr, colidx, vals)
    _, its_ref, status_ref, h_ref = bc.bicgstab(rowptr, colidx, vals, bg, dinv=1.0 / d, rtol=bc.HALF_RTOL)
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, vals, len(bg))
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    x, info = hp.bicgstab(A, b, M="jacobi", rtol=bc.HALF_RTOL)
    assert (info.converged, info.iterations, info.status) == (True, its_ref, "converged") and its_ref == bc.HALF_ITERATIONS
    assert len(info.residual_norms) == len(h_ref)
    dev = max(abs(g - w_) / w_ for g, w_ in zip(info.residual_norms, h_ref))
    print(f"half-step case: history deviation {dev:.2e}, last entry / |b| = {info.residual_norms[-1] / hp.norm(b):.4f}")
    assert dev <= bc.HALF_HIST_RTOL
    assert 0.0 < info.residual_norms[-1] <= bc.HALF_RTOL * hp.norm(b)
    # x took the half step only: b - A x is s_8 up to the gap between true and recurrence residual, which the convergence
    # tests allow to be rtol |b| at rtol = 1e-8
    assert abs(hp.norm(b - A @ x) - info.residual_norms[-1]) <= 1e-8 * hp.norm(b)
    hp.clear_plan_cache()


# ---- 5. breakdown and -I ------------------------------------------------------------------------------------------------------
def test_breakdown_and_minus_identity(hp, orc, gpu_backend_i32):
    for mat, bg in ((bc.ROT, bc.ROT_B), (bc.SINGULAR, bc.SINGULAR_B)):
        x_ref, its_ref, status_ref, h_ref = bc.bicgstab(*mat, bg)
        assert status_ref == "breakdown"
        x, info = hp.bicgstab(_matrix(hp, gpu_backend_i32, *mat, 2), hp.HPCVector.from_global(bg, gpu_backend_i32))
        assert (info.converged, info.iterations, info.status) == (False, its_ref, "breakdown")
        assert len(info.residual_norms) == len(h_ref) == its_ref + 1
        xv = x.local_values()
        assert np.all(np.isfinite(xv)) and np.allclose(xv, x_ref, rtol=1e-14, atol=0)
        assert np.allclose(info.residual_norms, h_ref, rtol=1e-14, atol=0)
    bg = orc.fill_uniform(0, 5, pc.SEED_RHS)
    A = _matrix(hp, gpu_backend_i32, *pc.diag_matrix(-np.ones(5)), 5)
    x, info = hp.bicgstab(A, hp.HPCVector.from_global(bg, gpu_backend_i32))
    assert (info.converged, info.iterations, info.status, len(info.residual_norms)) == (True, 1, "converged", 2)
    assert np.allclose(x.local_values(), -bg, rtol=1e-14, atol=0)


# ---- 6. convergence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", bc.SIZES)
def test_convergence_on_the_convection_diffusion_cases(hp, cases, gpu_backend_i32, size):
    c = cases[size]
    n = len(c["b"])
    A = _matrix(hp, gpu_backend_i32, c["rowptr"], c["colidx"], c["vals"], n)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    bnorm = hp.norm(b)
    its = {}
    for name, M in (("jacobi", "jacobi"), ("none", None)):
        _, its_ref, status_ref, _ = c["ref"][name]
        x, info = hp.bicgstab(A, b, rtol=1e-8, M=M)
        true = hp.norm(b - A @ x) / bnorm
        print(f"{size} {name}: iterations {info.iterations} (restatement {its_ref}), true residual {true:.3e}")
        assert info.converged and info.status == "converged" and status_ref == "converged"
        assert len(info.residual_norms) == info.iterations + 1
        assert true <= pc.TRUE_RES_RTOL
        if name == "jacobi":
            assert abs(info.iterations - its_ref) <= 2
        its[name] = info.iterations
    assert 2 * its["jacobi"] <= its["none"], its
    x0 = hp.HPCVector.from_global(np.full(n, 1e-3), gpu_backend_i32)
    x, info = hp.bicgstab(A, b, x0=x0, rtol=1e-8, M="jacobi")
    assert info.converged and hp.norm(b - A @ x) / bnorm <= pc.TRUE_RES_RTOL
    hp.clear_plan_cache()


# ---- 7. argument errors -------------------------------------------------------------------------------------------------------
def test_bicgstab_argument_errors(hp, cases, gpu_backend_i32):
    c = cases[(16, 16)]
    n = len(c["b"])
    A = _matrix(hp, gpu_backend_i32, c["rowptr"], c["colidx"], c["vals"], n)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    with pytest.raises(ValueError):
        hp.bicgstab(A, b, M="ilu")
    with pytest.raises(ValueError):
        hp.bicgstab(A, b, check_every=0)
    rect = hp.HPCSparseMatrix_local(c["rowptr"], c["colidx"], c["vals"], n + 7, gpu_backend_i32)
    with pytest.raises(ValueError):
        hp.bicgstab(rect, b)
    d0 = np.ones(n)
    d0[n // 2] = 0.0
    with pytest.raises(ValueError):
        hp.bicgstab(_matrix(hp, gpu_backend_i32, *pc.diag_matrix(d0), n), b, M="jacobi")  # minimum(abs(diag)) > 0 is required
    # a negative diagonal is fine: positivity is CG's condition, not this solver's
    x, info = hp.bicgstab(_matrix(hp, gpu_backend_i32, *pc.diag_matrix(-np.ones(n)), n), b, M="jacobi")
    assert info.converged
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    A32 = hp.HPCSparseMatrix_local(c["rowptr"], c["colidx"], c["vals"].astype(np.float32), n, b32)
    with pytest.raises(TypeError):
        hp.bicgstab(A32, hp.HPCVector.from_global(c["b"], b32))


# ---- 8. ranks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_bicgstab_across_ranks(nranks):
    """The ranks share the one GPU (peer-window push transport, like tests/test_gpu_multirank.py); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
