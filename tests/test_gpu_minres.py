"""GPU tests of the MINRES solver: the gated step kernels on their own through the C ABI, ``hp.minres`` against the numpy
restatement, independence of the chunk, workspace reuse, a start vector, the exact and degenerate cases, CG's breakdown on the
same inputs, convergence on the saddle-point and shifted cases and the solve across ranks.  Cases and the restatement:
tests/_minres_cases.py.

Margins (none of them taken from the device's results; tests/test_minres_cases.py re-measures the CPU figures and prints them):
  * elements of rn, yn, w, x: bit-equal to numpy's separately rounded expressions (the library is built with
    -ffp-contract=off);
  * every scalar of the step and the history pair: bit-equal to the same expressions in Python floats (``_minres_cases.step``);
  * the sum bb: 1e-12 of math.fsum relative to the sum of |terms| (a two-stage tree of doubles in reduce_stage1's grid and
    order; the project's margin for its reductions);
  * history: HIST_RTOL = 1e-12 (the project's history margin) on the first HEAD = 13 entries: four summation orders on the CPU
    spread by <= 5.6e-15 there (180 times less), and by <= 1.1e-14 over the same head at 65 x 63 (90 times less);
  * iteration counts: within the fewest and the most of those four orders (``_minres_cases.EXPECTED``), 2 more either way;
  * x against numpy.linalg.solve: 10 times the restatement's own error on the same case (one more summation order); the true
    residual in the tested norm, sqrt(r . M r) <= 2 max(rtol sqrt(b . M b), atol) (the restatement: <= 0.97 of the limit).
"""
import math
import os

import numpy as np
import pytest

from tests import _grid_regimes as gr
from tests import _minres_cases as mc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_minres_worker.py")

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN = 0, 1, 2
# slots of the scalar buffer (include/hpcla_rocm.h)
SLOTS = dict(beta=0, oldb=1, yt=2, bb=3, alfa=4, cs=5, sn=6, dbar=7, epsln=8, oldeps=9, delta=10, gbar=11, gamma=12, phi=13,
             phibar=14)
NSCAL = 16


def _matrix(hp, backend, rowptr, colidx, vals):
    return hp.HPCSparseMatrix_local(rowptr, colidx, vals, len(rowptr) - 1, backend)


@pytest.fixture(scope="module")
def cases(orc):
    """Every case with its dense matrix, the dense solve and the restatement's result, computed once."""
    out = {}
    for key, case in mc.all_cases(orc).items():
        dense = mc.dense_of(*case[:3])
        out[key] = dict(case=case, dense=dense, x_ref=np.linalg.solve(dense, case[3]), ref=mc.minres(*case[:4], dinv=case[4]))
    return out


def _f64_bits(v):
    return np.float64(v).view(np.uint64)


def _solve(hp, backend, case, **kw):
    rowptr, colidx, vals, bg, dinv = case
    A = _matrix(hp, backend, rowptr, colidx, vals)
    b = hp.HPCVector.from_global(bg, backend)
    return hp.minres(A, b, M="jacobi" if dinv is not None else None, **kw)


# ---- 1. the kernels on their own ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("n", gr.MINRES_ALONE)
def test_gated_kernels_alone(hp, n, precond):
    """The grids are ceil(floor(n / 2) / 1024) capped at 2048 for minres_r, whose partials minres_r_stage2 walks 256 at a time,
    and ceil(floor(n / 2) / 256) capped at 4096 for minres_xw (tests/_grid_regimes.py restates both and
    tests/test_grid_regimes.py checks that these sizes reach every regime).
    n = 1: the scalar tail alone; 2: one double2 and no tail; 3: both; 1023: a body and a tail on one workgroup of minres_r and
    two of minres_xw; 2046: no tail, one workgroup of minres_r and four of minres_xw; 2049: the last odd size on one workgroup of
    minres_r; 2051: two partials, so the first size at which minres_r_stage2 adds anything; 614 403: 301 partials, a second and
    ragged trip (45 lanes) of minres_r_stage2, 1201 workgroups of minres_xw; 4 194 307: 2048 partials, eight full trips of
    minres_r_stage2, five grid-stride trips in minres_r, minres_xw capped at 4096 workgroups with a third trip; all four odd.
    Every phase of the body runs at every size: the whole body takes 0.9 s at the largest (measured on the MI355X)."""
    import torch
    lib = hp._capi.load()
    rng = np.random.default_rng(n)
    host = {k: rng.uniform(-1.0, 1.0, n) for k in ("t", "r2", "r1", "y", "w1", "w2", "x")}
    host["dinv"] = rng.uniform(0.5, 2.0, n)
    dinv_h = host["dinv"] if precond else None
    f64 = dict(dtype=torch.float64, device="cuda")
    work = torch.zeros(lib.hpcla_minres_work_bytes() // 8, **f64)
    up = lambda k: torch.from_numpy(host[k]).cuda()
    P = lambda t: t.data_ptr() if t is not None else None
    bits_eq = lambda t, want: np.array_equal(pc.bits(t.cpu().numpy()), pc.bits(want))
    read = lambda st: st.cpu().tolist()[:2]
    t, r2, dinv = up("t"), up("r2"), (up("dinv") if precond else None)
    old = dict(beta=0.7, oldb=1.3, cs=-0.6, sn=0.8, dbar=0.4, epsln=-0.3, phibar=-0.9)
    yt = 0.37

    def state(done=0, status=RUNNING, thr=0.0):
        return torch.tensor([done, status, np.float64(thr).view(np.int64), 0], dtype=torch.int64, device="cuda")

    def scalars(yt_=yt, **kw):
        v = [0.0] * NSCAL
        for k, val in dict(old, yt=yt_, **kw).items():
            v[SLOTS[k]] = val
        return torch.tensor(v, **f64)

    def k_r(sc, t_, r2_, r1_, yn_, j, st, pair, dinv_=dinv):
        assert lib.hpcla_minres_r_f64(None, P(sc), P(t_), P(r2_), P(dinv_), P(r1_), P(yn_), n, j, P(st), P(pair), P(work),
                                      None) == 0

    def k_xw(sc, y_, w2_, w1_, x_, j, st):
        assert lib.hpcla_minres_xw_f64(P(sc), P(y_), P(w2_), P(w1_), P(x_), n, j, P(st), None) == 0

    new = None
    for j in (1, 5):                                                 # j = 1: no r1 term, r1 is only written
        rn_h, yn_h = mc.residual_update(host["t"], host["r2"], host["r1"], dinv_h, old["beta"], old["oldb"], yt, j == 1)
        sc, st, pair = scalars(), state(), torch.tensor([3.0, 4.0], **f64)
        r1, yn = up("r1"), (torch.full((n,), 7.0, **f64) if precond else None)
        before = sc.clone()
        k_r(sc, t, r2, r1, yn, j, st, None)                          # the setup's form: rn, yn and bb, no step, no gate
        torch.cuda.synchronize()
        bb = sc[SLOTS["bb"]].item()
        assert bits_eq(r1, rn_h) and (not precond or bits_eq(yn, yn_h)) and read(st) == [0, RUNNING]
        before[SLOTS["bb"]] = bb
        assert torch.equal(sc.view(torch.int64), before.view(torch.int64)) and pair.cpu().tolist() == [3.0, 4.0]
        err = abs(bb - math.fsum((rn_h * yn_h).tolist())) / float(np.abs(rn_h * yn_h).sum())
        print(f"n = {n}, precond = {precond}, j = {j}: rn.yn off by {err:.2e} of the sum of |terms|")
        assert err <= 1e-12
        r1 = up("r1")
        k_r(sc, t, r2, r1, yn, j, st, pair)                          # the same pass with the step
        torch.cuda.synchronize()
        assert bits_eq(r1, rn_h) and (not precond or bits_eq(yn, yn_h)) and sc[SLOTS["bb"]].item() == bb
        gate, new = mc.step(old, yt, bb)
        assert gate is None
        got = sc.cpu().tolist()
        for k, v in new.items():
            assert _f64_bits(got[SLOTS[k]]) == _f64_bits(v), (k, got[SLOTS[k]], v)
        assert got[SLOTS["yt"]] == yt and got[15] == 0.0
        p = pair.cpu().tolist()
        assert _f64_bits(p[0]) == _f64_bits(new["phibar"] * new["phibar"]) and p[1] == bb
        assert read(st) == [0, RUNNING]                              # thr = 0 < phibar^2
        y, w1, x = up("y"), up("w1"), up("x")
        k_xw(sc, y, up("w2"), w1, x, j, st)
        torch.cuda.synchronize()
        w_h, x_h = mc.direction_update(host["y"], host["w1"], host["w2"], host["x"], new)
        assert bits_eq(w1, w_h) and bits_eq(x, x_h)
    j = 5

    # -- frozen: no kernel writes a byte (converged or broken down at j - 1; broken down at j; converged at another iteration)
    for frozen in ([j - 1, CONVERGED], [j - 1, BREAKDOWN], [j, BREAKDOWN], [j + 1, CONVERGED]):
        stf = state(*frozen)
        keep = stf.clone()
        scf, pairf = sc.clone(), torch.tensor([3.0, 4.0], **f64)
        vecs = [torch.full((n,), 7.0, **f64) for _ in range(4)]      # r1, yn, w1, x
        k_r(scf, t, r2, vecs[0], vecs[1] if precond else None, j, stf, pairf)
        k_r(scf, t, r2, vecs[0], vecs[1] if precond else None, j, stf, None)
        k_xw(scf, up("y"), up("w2"), vecs[2], vecs[3], j, stf)
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in vecs), frozen
        assert torch.equal(scf.view(torch.int64), sc.view(torch.int64)) and pairf.cpu().tolist() == [3.0, 4.0]
        assert torch.equal(stf, keep)

    # -- gate C from a hand-set threshold, and minres_xw still runs in the iteration that converged; minres_r then is frozen
    scc, stc, pairc = scalars(), state(thr=1e300), torch.tensor([3.0, 4.0], **f64)
    r1 = up("r1")
    k_r(scc, t, r2, r1, torch.full((n,), 7.0, **f64) if precond else None, j, stc, pairc)
    w1, x, u = up("w1"), up("x"), torch.full((n,), 7.0, **f64)
    k_xw(scc, up("y"), up("w2"), w1, x, j, stc)
    k_r(scc, t, r2, u, u.clone() if precond else None, j + 1, stc, pairc)
    torch.cuda.synchronize()
    assert read(stc) == [j, CONVERGED] and torch.equal(scc.view(torch.int64), sc.view(torch.int64))
    assert bits_eq(w1, w_h) and bits_eq(x, x_h) and bool((u == 7.0).all())

    # -- gate N: a NaN yt, an infinite yt, a negative bb (an indefinite M); gate G: everything 0 makes gbar = beta' = 0.
    #    Each reports a breakdown at j - 1, writes no scalar but bb, and minres_xw then leaves w and x alone
    zeros = torch.zeros(n, **f64)
    broken = [dict(yt_=math.nan), dict(yt_=math.inf)]
    if precond:
        broken.append(dict(dinv_=-up("dinv")))
    for kw in broken:
        scn, stn, pairn = scalars(kw.get("yt_", yt)), state(thr=1e300), torch.tensor([3.0, 4.0], **f64)
        before = scn.clone()
        k_r(scn, t, r2, up("r1"), torch.full((n,), 7.0, **f64) if precond else None, j, stn, pairn, kw.get("dinv_", dinv))
        w4, x4 = torch.full((n,), 7.0, **f64), torch.full((n,), 7.0, **f64)
        k_xw(scn, up("y"), up("w2"), w4, x4, j, stn)
        torch.cuda.synchronize()
        assert read(stn) == [j - 1, BREAKDOWN], kw
        before[SLOTS["bb"]] = scn[SLOTS["bb"]]
        assert torch.equal(scn.view(torch.int64), before.view(torch.int64)) and pairn.cpu().tolist() == [3.0, 4.0]
        assert bool((w4 == 7.0).all()) and bool((x4 == 7.0).all())
        if "dinv_" in kw:
            assert scn[SLOTS["bb"]].item() < 0
    scg, stg, pairg = scalars(0.0, dbar=0.0), state(thr=1e300), torch.tensor([3.0, 4.0], **f64)
    k_r(scg, zeros, zeros, zeros.clone(), zeros.clone() if precond else None, j, stg, pairg)
    torch.cuda.synchronize()
    assert read(stg) == [j - 1, BREAKDOWN] and scg[SLOTS["bb"]].item() == 0.0 and pairg.cpu().tolist() == [3.0, 4.0]
    assert mc.step(dict(old, dbar=0.0), 0.0, 0.0)[0] == "G"


# ---- 2. the head of the history against the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_history_heads_match_the_restatement(hp, cases, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    """First HEAD = 13 entries within HIST_RTOL = 1e-12: 180 times the spread of four summation orders on the CPU (5.6e-15,
    tests/test_minres_cases.py prints it)."""
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    for key in (("saddle", mc.RANK_SIZE, False), ("scaled_saddle", mc.RANK_SIZE, True), ("shifted", mc.SHIFT_SIZE, False)):
        case = cases[key]["case"]
        _, its_ref, status_ref, hist_ref = mc.minres(*case[:4], dinv=case[4], rtol=0.0, maxiter=mc.HEAD)
        assert (its_ref, status_ref, len(hist_ref)) == (mc.HEAD, "maxiter", mc.HEAD + 1)
        x, info = _solve(hp, backend, case, rtol=0.0, maxiter=mc.HEAD)
        assert (info.iterations, info.status, info.converged) == (mc.HEAD, "maxiter", False)
        assert len(info.residual_norms) == mc.HEAD + 1
        head = max(abs(g - w_) / w_ for g, w_ in zip(info.residual_norms[:mc.HEAD], hist_ref[:mc.HEAD]))
        print(f"{which} {key}: head deviation {head:.2e}")
        assert head <= mc.HIST_RTOL, (key, head)
    hp.clear_plan_cache()


def test_history_heads_at_the_large_size(hp, orc, gpu_backend_i32):
    """65 x 63: 8190 rows for the two saddle cases (minres_r on four stage-1 workgroups, minres_r_stage2 adding four partials)
    and 4095, odd, for the shifted one (two); the other solves of this file stay on one.  The first HEAD = 13 entries within
    HIST_RTOL = 1e-12: 90 times the spread of four summation orders on the CPU at this size (saddle 6.3e-15, scaled saddle
    1.1e-14, shifted 9.1e-15; tests/test_minres_cases.py re-measures them).  No convergence or count is asserted here."""
    for name, case, dinv in mc.large_cases(orc):
        _, its_ref, status_ref, hist_ref = mc.minres(*case, dinv=dinv, rtol=0.0, maxiter=mc.HEAD)
        assert (its_ref, status_ref, len(hist_ref)) == (mc.HEAD, "maxiter", mc.HEAD + 1)
        x, info = _solve(hp, gpu_backend_i32, (*case, dinv), rtol=0.0, maxiter=mc.HEAD)
        assert (info.iterations, info.status, info.converged) == (mc.HEAD, "maxiter", False)
        assert len(info.residual_norms) == mc.HEAD + 1
        head = max(abs(g - w_) / w_ for g, w_ in zip(info.residual_norms[:mc.HEAD], hist_ref[:mc.HEAD]))
        print(f"{name} {mc.LARGE_SIZE}: head deviation {head:.2e}")
        assert head <= mc.HIST_RTOL, (name, head)
    hp.clear_plan_cache()


# ---- 3. iteration counts, statuses and the answer -------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64wide"])
def test_convergence_counts_and_answers(hp, cases, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    for key, c in cases.items():
        rowptr, colidx, vals, bg, dinv = c["case"]
        x, info = _solve(hp, backend, c["case"])
        xv = x.local_values()
        want, lo, hi = mc.EXPECTED[key]
        x_res, its_ref, _, _ = c["ref"]
        err = np.linalg.norm(xv - c["x_ref"]) / np.linalg.norm(c["x_ref"])
        err_ref = np.linalg.norm(x_res - c["x_ref"]) / np.linalg.norm(c["x_ref"])
        limit = 1e-8 * mc.m_norm(bg, dinv)
        true = mc.m_norm(bg - c["dense"] @ xv, dinv) / limit
        print(f"{which} {key}: {info.status} at {info.iterations} (restatement {its_ref}, orders {lo} .. {hi}), against solve "
              f"{err:.2e} (restatement {err_ref:.2e}), true residual {true:.3f} of the limit")
        assert (info.status, info.converged) == ("converged", True)
        assert lo - 2 <= info.iterations <= hi + 2, (key, info.iterations)
        hist = info.residual_norms
        assert len(hist) == info.iterations + 1 and all(h1 <= h0 for h0, h1 in zip(hist, hist[1:]))
        assert hist[-1] <= limit < hist[-2]
        assert err <= 10 * err_ref, (key, err, err_ref)
        assert true <= pc.TRUE_RES_FACTOR, (key, true)
    hp.clear_plan_cache()


# ---- 4. the chunk, reuse, a start vector ------------------------------------------------------------------------------------
def test_answer_does_not_depend_on_the_chunk(hp, cases, gpu_backend_i32):
    for key in (("saddle", (24, 20), False), ("scaled_saddle", (24, 20), True)):
        runs = []
        for chunk in (1, 3, 8, 1000):
            x, info = _solve(hp, gpu_backend_i32, cases[key]["case"], check_every=chunk)
            assert info.converged
            runs.append((info.iterations, info.status, pc.bits(x.local_values()).copy(), pc.bits(info.residual_norms).copy()))
        for its, status, xb, hb in runs[1:]:
            assert (its, status) == runs[0][:2] and np.array_equal(xb, runs[0][2]) and np.array_equal(hb, runs[0][3])
    hp.clear_plan_cache()


def test_workspace_reuse_and_a_start_vector(hp, cases, gpu_backend_i32):
    c = cases["scaled_saddle", (16, 16), True]
    rowptr, colidx, vals, bg, dinv = c["case"]
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, vals)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    ws = hp.MinresWorkspace(b)
    assert ws.fits(b)
    x, info = hp.minres(A, b, M="jacobi", workspace=ws)
    assert x is ws.x and info.converged
    xv = x.local_values().copy()
    # a second solve on the now dirty workspace, one on a workspace dirtied by a different solve, and a fresh one: same bits
    x2, info2 = hp.minres(A, b, M="jacobi", workspace=ws)
    assert x2 is ws.x and info2 == info and np.array_equal(pc.bits(x2.local_values()), pc.bits(xv))
    hp.minres(A, b, rtol=0.0, maxiter=3, workspace=ws)
    x3, info3 = hp.minres(A, b, M="jacobi", workspace=ws)
    assert info3 == info and np.array_equal(pc.bits(x3.local_values()), pc.bits(xv))
    x4, info4 = hp.minres(A, b, M="jacobi")
    assert x4 is not ws.x and info4 == info and np.array_equal(pc.bits(x4.local_values()), pc.bits(xv))
    # the weights given as a vector are the same solve
    x5, info5 = hp.minres(A, b, M=hp.HPCVector.from_global(dinv, gpu_backend_i32))
    assert abs(info5.iterations - info.iterations) <= 2 and info5.converged
    # a start vector near the solution stops sooner; its threshold still refers to b
    for M, dv in (("jacobi", dinv), (None, None)):
        _, base = hp.minres(A, b, M=M)
        x0 = hp.HPCVector.from_global(c["x_ref"] * (1.0 + 1e-4), gpu_backend_i32)
        x6, info6 = hp.minres(A, b, x0=x0, M=M)
        limit = 1e-8 * mc.m_norm(bg, dv)
        assert info6.converged and 0 < info6.iterations < base.iterations
        assert info6.residual_norms[-1] <= limit < info6.residual_norms[-2] <= info6.residual_norms[0]
        start = mc.m_norm(bg - c["dense"] @ (c["x_ref"] * (1.0 + 1e-4)), dv)
        assert abs(info6.residual_norms[0] - start) <= 1e-8 * start      # r0 = b - A x0 cancels four digits on either side
        assert mc.m_norm(bg - c["dense"] @ x6.local_values(), dv) <= 2.0 * limit
    hp.clear_plan_cache()


# ---- 5. the exact and degenerate cases ----------------------------------------------------------------------------------------
def test_exact_and_degenerate_cases(hp, orc, cases, gpu_backend_i32):
    def system(d, bg):
        A = _matrix(hp, gpu_backend_i32, *pc.diag_matrix(d))
        return A, hp.HPCVector.from_global(np.asarray(bg, dtype=np.float64), gpu_backend_i32)

    def solve(d, bg, **kw):
        x, info = hp.minres(*system(d, bg), **kw)
        xv = x.local_values()
        assert np.all(np.isfinite(xv)) and len(info.residual_norms) == info.iterations + 1
        return xv, info

    bi = orc.fill_uniform(0, 5, pc.SEED_RHS)
    for sign in (1.0, -1.0):
        xv, info = solve(sign * np.ones(5), bi)
        assert (info.iterations, info.status, info.converged) == (1, "converged", True)
        assert np.all(np.abs(xv - sign * bi) <= 1e-15)
    _, cg_info = hp.cg(*system(-np.ones(5), bi))                                      # CG on the same -I
    assert (cg_info.status, cg_info.converged) == ("breakdown", False)
    xv, info = solve([1.0, -1.0, 2.0, 3.0], [1.0, 2.0, 1.0, 1.0])
    assert info.status == "converged" and info.iterations <= 4
    assert np.all(np.abs(xv - [1.0, -2.0, 0.5, 1.0 / 3.0]) <= 1e-8)
    xv, info = solve([1.0, 0.0], [1.0, 0.0])                                          # singular and consistent
    assert (xv.tolist(), info.iterations, info.status, info.residual_norms) == ([1.0, 0.0], 1, "converged", [1.0, 0.0])
    xv, info = solve([1.0, math.nan], [1.0, 1.0])
    assert (info.iterations, info.status, info.converged) == (0, "breakdown", False) and not xv.any()
    assert info.residual_norms == [math.sqrt(2.0)]
    xv, info = solve(np.ones(5), np.zeros(5))
    assert (info.iterations, info.status, info.residual_norms, info.converged) == (0, "converged", [0.0], True) and not xv.any()
    xv, info = solve(np.ones(5), bi, maxiter=0)
    assert (info.iterations, info.status, info.converged, len(info.residual_norms)) == (0, "maxiter", False, 1) and not xv.any()
    # CG breaks down on the saddle-point matrix MINRES solves
    case = cases["saddle", (16, 16), False]["case"]
    A = _matrix(hp, gpu_backend_i32, *case[:3])
    b = hp.HPCVector.from_global(case[3], gpu_backend_i32)
    assert hp.cg(A, b)[1].status == "breakdown" and hp.minres(A, b)[1].status == "converged"
    hp.clear_plan_cache()


# ---- 6. argument errors -------------------------------------------------------------------------------------------------------
def test_minres_argument_errors(hp, cases, gpu_backend_i32):
    case = cases["saddle", (16, 16), False]["case"]
    n = len(case[3])
    A = _matrix(hp, gpu_backend_i32, *case[:3])
    b = hp.HPCVector.from_global(case[3], gpu_backend_i32)
    weights = np.ones(n)
    weights[7] = 0.0
    with pytest.raises(ValueError):
        hp.minres(A, b, M=hp.HPCVector.from_global(weights, gpu_backend_i32))            # a non-positive weight
    weights[7] = -1.0
    with pytest.raises(ValueError):
        hp.minres(A, b, M=hp.HPCVector.from_global(weights, gpu_backend_i32))
    with pytest.raises(ValueError):
        hp.minres(A, b, M="ilu")
    with pytest.raises(ValueError):
        hp.minres(A, b, M=weights)
    Z = _matrix(hp, gpu_backend_i32, *pc.diag_matrix([1.0, 0.0, 2.0]))                   # a zero diagonal entry
    with pytest.raises(ValueError):
        hp.minres(Z, hp.HPCVector.from_global(np.ones(3), gpu_backend_i32), M="jacobi")
    with pytest.raises(ValueError):
        hp.minres(A, hp.HPCVector.from_global(np.ones(n + 1), gpu_backend_i32))          # b not on A's rows
    with pytest.raises(ValueError):
        hp.minres(A, b, check_every=0)
    for bad in (dict(rtol=-1.0), dict(atol=-1.0), dict(maxiter=-1)):
        with pytest.raises(ValueError):
            hp.minres(A, b, **bad)
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    A32 = hp.HPCSparseMatrix_local(case[0], case[1], case[2].astype(np.float32), n, b32)
    with pytest.raises(TypeError):
        hp.minres(A32, hp.HPCVector.from_global(case[3], b32))
    hp.clear_plan_cache()


# ---- 7. ranks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_minres_across_ranks(nranks):
    """The ranks share the one GPU (peer-window push transport, like tests/test_gpu_multirank.py); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
