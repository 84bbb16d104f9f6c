"""GPU tests of the least-squares solver: the gated step kernels on their own through the C ABI, ``hp.lsqr`` against the numpy
restatement, independence of the chunk, the freeze behind the deciding iteration, the exact and degenerate cases, convergence
on the tall and wide cases and the solve across ranks.  Cases and the restatement: tests/_lsqr_cases.py.

Margins (none of them taken from the device's results; tests/test_lsqr_cases.py re-measures the CPU figures and prints them):
  * elements of uh, vh, w, x: bit-equal to numpy's separately rounded expressions (the library is built with
    -ffp-contract=off);
  * every scalar of the step and the history pair: bit-equal to the same expressions in Python floats (``_lsqr_cases.step``);
  * the two sums: 1e-12 of math.fsum relative to the sum of |terms| (n <= 4.2e6 terms in a two-stage tree of doubles; the
    project's margin for its reductions);
  * histories: HIST_RTOL = 1e-12 on the first HEAD = 13 entries of both: four summation orders on the CPU spread by <= 7.1e-15
    there (140 times less), and by <= 1.2e-14 over the same head of the tall case at 65 x 63 (80 times less); the tail of
    normal_residual_norms is rounding-dominated near the stop and is not compared;
  * iteration counts: +-2 of the restatement's (identical across those orders except wide 16x16, 90-91);
  * x against numpy.linalg.lstsq on the dense augmented system: 1e-6 relative (restatement <= 1.8e-7); the true residual
    <= 2 rtol |b| where rule 1 stopped, the true normal residual <= 2 ntol |Abar|_F |rbar| where rule 2 stopped.
"""
import math
import os

import numpy as np
import pytest

from tests import _bicgstab_cases as bc
from tests import _grid_regimes as gr
from tests import _lsqr_cases as lc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_lsqr_worker.py")

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN, LEAST = 0, 1, 2, 3
# slots of the scalar buffer (include/hpcla_rocm.h)
SLOTS = dict(alpha=0, beta=1, uu=2, vv=3, phibar=4, rhobar=5, res2=6, anorm2=7, t1=8, t2=9, rho=10, c=11, s=12, theta=13, phi=14,
             rn2=15, arn=16, damp=17)
NSCAL = 24


def _matrix(hp, backend, rowptr, colidx, vals, ncols):
    return hp.HPCSparseMatrix_local(rowptr, colidx, vals, ncols, backend)


@pytest.fixture(scope="module")
def cases(orc):
    """The tall and wide cases with the restatement's results at both damps, computed once."""
    out = {}
    for kind, make in lc.CASES.items():
        for size in lc.SIZES:
            case = make(orc, *size)
            out[kind, size] = dict(case=case, dense=lc.dense_of(*case[:4]),
                                   ref={damp: lc.lsqr(*case, damp=damp) for damp in lc.DAMPS})
    return out


def _f64_bits(v):
    return np.float64(v).view(np.uint64)


# ---- 1. the kernels on their own ----------------------------------------------------------------------------------------
def _sum_err(got, terms):
    return abs(got - math.fsum(terms.tolist())) / float(np.abs(terms).sum())


@pytest.mark.parametrize("n", gr.LSQR_ALONE)
def test_gated_kernels_alone(hp, n):
    """The reductions (lsqr_u, lsqr_v) use the grid of the existing stage-1 reductions, ceil(floor(n / 2) / 1024) capped at
    2048: 2049 is the last size on one workgroup with a scalar tail, 2051 the first odd size on two, 4 194 307 =
    2 * 256 * 4 * 2048 + 3 caps the grid and is odd.  The elementwise kernel (lsqr_xw) uses ceil(floor(n / 2) / 256) capped at
    4096: 511 is the last odd size on one workgroup, 515 the first on two, and the largest size makes every thread stride
    twice.  614 403 is odd with 301 partials: the gated second stages walk them in two trips of 256 lanes, the last one ragged
    (45 lanes), and lsqr_xw has 1201 workgroups.  These are the sizes of test_gated_kernels_alone in
    tests/test_gpu_bicgstab.py: the grids are the same (tests/_grid_regimes.py holds the sizes, tests/test_grid_regimes.py
    checks that they reach every regime)."""
    import torch
    lib = hp._capi.load()
    rng = np.random.default_rng(n)
    host = {k: rng.uniform(-1.0, 1.0, n) for k in ("tu", "uh", "tv", "vh", "w", "x")}
    j = 5
    f64 = dict(dtype=torch.float64, device="cuda")
    work = torch.zeros(lib.hpcla_lsqr_work_bytes() // 8, **f64)
    up = lambda k: torch.from_numpy(host[k]).cuda()
    P = lambda t: t.data_ptr() if t is not None else None
    bits_eq = lambda t, want: np.array_equal(pc.bits(t.cpu().numpy()), pc.bits(want))
    read = lambda st: st.cpu().tolist()[:2]

    def state(done=0, status=RUNNING, thr=0.0, ntol2=0.0):
        return torch.tensor([done, status, np.float64(thr).view(np.int64), np.float64(ntol2).view(np.int64)], dtype=torch.int64,
                            device="cuda")

    def scalars(**kw):
        v = [0.0] * NSCAL
        for k, val in kw.items():
            v[SLOTS[k]] = val
        return torch.tensor(v, **f64)

    def k_u(sc, tu_, uh_, st):
        assert lib.hpcla_lsqr_u_f64(None, P(sc), P(tu_), P(uh_), n, j, P(st), P(work), None) == 0

    def k_v(sc, tv_, vh_, st, pair):
        assert lib.hpcla_lsqr_v_f64(None, P(sc), P(tv_), P(vh_), n, j, P(st), P(pair), P(work), None) == 0

    def k_xw(sc, vh_, x_, w_, st):
        assert lib.hpcla_lsqr_xw_f64(P(sc), P(vh_), P(x_), P(w_), n, j, P(st), None) == 0

    def check_step(sc, pair, old, uu, vv):
        """Every scalar slot and the pair against the Python-float step from the device's own two sums."""
        want = lc.step(old["alpha"], uu, vv, old["damp"], old["phibar"], old["rhobar"], old["res2"], old["anorm2"])
        got = sc.cpu().tolist()
        for k in ("alpha", "beta", "rho", "c", "s", "theta", "rhobar", "phi", "phibar", "t1", "t2", "rn2", "arn", "anorm2", "res2"):
            assert _f64_bits(got[SLOTS[k]]) == _f64_bits(want[k]), (k, got[SLOTS[k]], want[k])
        assert got[SLOTS["damp"]] == old["damp"] and got[SLOTS["uu"]] == uu and got[SLOTS["vv"]] == vv
        assert all(g == 0.0 for g in got[18:])
        p = pair.cpu().tolist()
        assert _f64_bits(p[0]) == _f64_bits(want["rn2"]) and _f64_bits(p[1]) == _f64_bits(want["arn2"])
        return want

    tu, tv = up("tu"), up("tv")
    # -- running, damp = 0 and 0.3: every step from hand-set scalars (phibar may be negative)
    for damp in lc.DAMPS:
        old = dict(alpha=1.3, beta=0.7, phibar=-0.9, rhobar=1.1, res2=0.2, anorm2=3.0, damp=damp)
        sc, st, pair = scalars(**old), state(), torch.tensor([3.0, 4.0], **f64)
        uh, vh, w, x = up("uh"), up("vh"), up("w"), up("x")
        k_u(sc, tu, uh, st)
        torch.cuda.synchronize()
        uh_h = host["tu"] / old["alpha"] - (old["alpha"] / old["beta"]) * host["uh"]
        uu = sc[SLOTS["uu"]].item()
        assert bits_eq(uh, uh_h)
        before = sc.clone()
        k_v(sc, tv, vh, st, None)                                    # the setup's form: vh and vv, no step, no gate
        torch.cuda.synchronize()
        beta1 = math.sqrt(uu)
        vh_h = host["tv"] / beta1 - (beta1 / old["alpha"]) * host["vh"]
        vv = sc[SLOTS["vv"]].item()
        assert bits_eq(vh, vh_h) and read(st) == [0, RUNNING]
        before[SLOTS["vv"]] = vv
        assert torch.equal(sc.view(torch.int64), before.view(torch.int64))
        vh = up("vh")
        k_v(sc, tv, vh, st, pair)                                    # the same pass with the step
        torch.cuda.synchronize()
        assert bits_eq(vh, vh_h) and sc[SLOTS["vv"]].item() == vv
        new = check_step(sc, pair, old, uu, vv)
        assert read(st) == [0, RUNNING]                              # thr = ntol2 = 0 < rn2, arn^2
        k_xw(sc, vh, x, w, st)
        torch.cuda.synchronize()
        assert bits_eq(x, host["x"] + new["t1"] * host["w"])
        assert bits_eq(w, vh_h / new["alpha"] - new["t2"] * host["w"])
        errs = {"uh.uh": _sum_err(uu, uh_h * uh_h), "vh.vh": _sum_err(vv, vh_h * vh_h)}
        print(f"n = {n}, damp = {damp}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert all(e <= 1e-12 for e in errs.values()), errs

    # -- frozen: no kernel writes a byte (converged, least squares or broken down at j - 1; stopped at another iteration)
    for frozen in ([j - 1, CONVERGED], [j - 1, LEAST], [j - 1, BREAKDOWN], [j, BREAKDOWN], [j + 1, CONVERGED], [j + 1, LEAST]):
        stf = state(*frozen)
        keep = stf.clone()
        scf, pairf = sc.clone(), torch.tensor([3.0, 4.0], **f64)
        vecs = [torch.full((n,), 7.0, **f64) for _ in range(4)]      # uh, vh, x, w
        k_u(scf, tu, vecs[0], stf)
        k_v(scf, tv, vecs[1], stf, pairf)
        k_v(scf, tv, vecs[1], stf, None)
        k_xw(scf, up("vh"), vecs[2], vecs[3], stf)
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in vecs), frozen
        assert torch.equal(scf.view(torch.int64), sc.view(torch.int64)) and pairf.cpu().tolist() == [3.0, 4.0]
        assert torch.equal(stf, keep)

    # -- the x-only form: stopped at this iteration, x = x + t1 w and nothing else; lsqr_u and lsqr_v write nothing
    for status in (CONVERGED, LEAST):
        stx = state(j, status)
        scx, x2, w2, u2 = sc.clone(), up("x"), up("w"), torch.full((n,), 7.0, **f64)
        k_u(scx, tu, u2, stx)
        k_v(scx, tv, u2, stx, pair)
        k_xw(scx, vh, x2, w2, stx)
        torch.cuda.synchronize()
        assert bits_eq(x2, host["x"] + new["t1"] * host["w"]) and bits_eq(w2, host["w"]) and bool((u2 == 7.0).all())
        assert torch.equal(scx.view(torch.int64), sc.view(torch.int64)) and read(stx) == [j, status]

    # -- gate U: tu = 0 and alpha / beta = 0 (beta = inf) make uh exactly 0: vh is left alone, vv = 0, and the step ends the
    #    solve -- by rule 1 when res2 = 0 (rn2 = 0 <= thr = 0), else by rule 2 (arn = 0)
    zeros = torch.zeros(n, **f64)
    for res2, want_status in ((0.0, CONVERGED), (0.2, LEAST)):
        old = dict(alpha=1.3, beta=math.inf, phibar=-0.9, rhobar=1.1, res2=res2, anorm2=3.0, damp=0.0)
        scu, stu, pairu = scalars(**old), state(), torch.tensor([3.0, 4.0], **f64)
        uh, vh3 = up("uh"), torch.full((n,), 7.0, **f64)
        k_u(scu, zeros, uh, stu)
        k_v(scu, tv, vh3, stu, pairu)
        torch.cuda.synchronize()
        assert not uh.cpu().numpy().any() and scu[SLOTS["uu"]].item() == 0.0
        assert bool((vh3 == 7.0).all()) and scu[SLOTS["vv"]].item() == 0.0
        got = check_step(scu, pairu, old, 0.0, 0.0)
        assert got["alpha"] == 0.0 and got["arn"] == 0.0 and got["rn2"] == res2
        assert read(stu) == [j, want_status]

    # -- the non-finite gate: a NaN scalar -> breakdown at j - 1, and lsqr_xw then leaves x and w alone
    old = dict(alpha=1.3, beta=0.7, phibar=math.nan, rhobar=1.1, res2=0.2, anorm2=3.0, damp=0.0)
    scn, stn, pairn = scalars(**old), state(thr=1e300, ntol2=1e300), torch.tensor([3.0, 4.0], **f64)
    uh, vh, x4, w4 = up("uh"), up("vh"), torch.full((n,), 7.0, **f64), torch.full((n,), 7.0, **f64)
    k_u(scn, tu, uh, stn)
    k_v(scn, tv, vh, stn, pairn)
    k_xw(scn, vh, x4, w4, stn)
    torch.cuda.synchronize()
    assert read(stn) == [j - 1, BREAKDOWN] and bool((x4 == 7.0).all()) and bool((w4 == 7.0).all())
    # -- rule 1 and rule 2 from hand-set thresholds (rn2 < 1 + 0.2, arn^2 > 0)
    for thr, ntol2, want_status in ((1e300, 0.0, CONVERGED), (0.0, 1e300, LEAST), (1e300, 1e300, CONVERGED)):
        old = dict(alpha=1.3, beta=0.7, phibar=-0.9, rhobar=1.1, res2=0.2, anorm2=3.0, damp=0.3)
        scr, str_, pairr = scalars(**old), state(thr=thr, ntol2=ntol2), torch.tensor([3.0, 4.0], **f64)
        uh, vh = up("uh"), up("vh")
        k_u(scr, tu, uh, str_)
        k_v(scr, tv, vh, str_, pairr)
        torch.cuda.synchronize()
        assert read(str_) == [j, want_status], (thr, ntol2)


# ---- 2. the heads of both histories against the restatement --------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_history_heads_match_the_restatement(hp, cases, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    """First HEAD = 13 entries of both histories within HIST_RTOL = 1e-12: 140 times the spread of four summation orders on the
    CPU (7.1e-15, tests/test_lsqr_cases.py prints it)."""
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    for kind in lc.CASES:
        case = cases[kind, lc.RANK_SIZE]["case"]
        A = _matrix(hp, backend, *case[:4])
        b = hp.HPCVector.from_global(case[4], backend)
        for damp in lc.DAMPS:
            _, its_ref, status_ref, hr, hn, _ = lc.lsqr(*case, damp=damp, rtol=0.0, ntol=0.0, maxiter=lc.HEAD)
            assert (its_ref, status_ref, len(hr), len(hn)) == (lc.HEAD, "maxiter", lc.HEAD + 1, lc.HEAD + 1)
            x, info = hp.lsqr(A, b, damp=damp, rtol=0.0, ntol=0.0, maxiter=lc.HEAD)
            assert (info.iterations, info.status, info.converged) == (lc.HEAD, "maxiter", False)
            assert len(info.residual_norms) == len(info.normal_residual_norms) == lc.HEAD + 1
            head = max(abs(g - w_) / w_ for got, want in ((info.residual_norms, hr), (info.normal_residual_norms, hn))
                       for g, w_ in zip(got[:lc.HEAD], want[:lc.HEAD]))
            print(f"{which} {kind} damp {damp}: head deviation {head:.2e}")
            assert head <= lc.HIST_RTOL, (kind, damp, head)
    hp.clear_plan_cache()


def test_history_heads_at_the_large_size(hp, orc, gpu_backend_i32):
    """The tall case at 65 x 63: 8190 x 4095, so lsqr_u runs on four stage-1 workgroups and lsqr_v, over an odd length, on two,
    and the gated second stages add four and two partials (the other solves of this file stay on one).  The first HEAD = 13
    entries of both histories within HIST_RTOL = 1e-12: 80 times the spread of four summation orders on the CPU at this size
    (1.2e-14 at damp 0, 1.0e-14 at damp 0.3; tests/test_lsqr_cases.py re-measures both).  No convergence or count is asserted."""
    case = lc.tall(orc, *lc.LARGE_SIZE)
    A = _matrix(hp, gpu_backend_i32, *case[:4])
    b = hp.HPCVector.from_global(case[4], gpu_backend_i32)
    for damp in lc.DAMPS:
        _, its_ref, status_ref, hr, hn, _ = lc.lsqr(*case, damp=damp, rtol=0.0, ntol=0.0, maxiter=lc.HEAD)
        assert (its_ref, status_ref, len(hr), len(hn)) == (lc.HEAD, "maxiter", lc.HEAD + 1, lc.HEAD + 1)
        x, info = hp.lsqr(A, b, damp=damp, rtol=0.0, ntol=0.0, maxiter=lc.HEAD)
        assert (info.iterations, info.status, info.converged) == (lc.HEAD, "maxiter", False)
        assert len(info.residual_norms) == len(info.normal_residual_norms) == lc.HEAD + 1
        head = max(abs(g - w_) / w_ for got, want in ((info.residual_norms, hr), (info.normal_residual_norms, hn))
                   for g, w_ in zip(got[:lc.HEAD], want[:lc.HEAD]))
        print(f"tall {lc.LARGE_SIZE} damp {damp}: head deviation {head:.2e}")
        assert head <= lc.HIST_RTOL, (damp, head)
    hp.clear_plan_cache()


# ---- 3. the chunk -----------------------------------------------------------------------------------------------------------
def test_answer_does_not_depend_on_the_chunk(hp, cases, gpu_backend_i32):
    case = cases["tall", (24, 20)]["case"]
    A = _matrix(hp, gpu_backend_i32, *case[:4])
    b = hp.HPCVector.from_global(case[4], gpu_backend_i32)
    runs = []
    for chunk in (1, 3, 8, 64):
        x, info = hp.lsqr(A, b, damp=0.3, check_every=chunk)
        assert info.converged
        runs.append((info.iterations, info.status, pc.bits(x.local_values()).copy(), pc.bits(info.residual_norms).copy(),
                     pc.bits(info.normal_residual_norms).copy(), info.anorm))
    for its, status, xb, hb, nb, an in runs[1:]:
        assert (its, status, an) == (runs[0][0], runs[0][1], runs[0][5])
        assert np.array_equal(xb, runs[0][2]) and np.array_equal(hb, runs[0][3]) and np.array_equal(nb, runs[0][4])


# ---- 4. freeze and reuse --------------------------------------------------------------------------------------------------------
def test_freeze_on_a_diagonal_system_and_a_dirty_workspace(hp, orc, gpu_backend_i32):
    rowptr, colidx, d, bg = pc.diagonal_case(orc)
    n = len(bg)
    x_ref, its_ref, status_ref, hr, hn, _ = lc.lsqr(rowptr, colidx, d, n, bg, maxiter=50)
    assert status_ref == "converged"
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, d, n)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    ws = hp.LSQRWorkspace(A, b)
    assert ws.fits(A, b)
    x, info = hp.lsqr(A, b, maxiter=50, workspace=ws)
    assert x is ws.x
    assert (info.converged, info.status) == (True, "converged") and abs(info.iterations - its_ref) <= 2
    assert len(info.residual_norms) == len(info.normal_residual_norms) == info.iterations + 1
    xv = x.local_values().copy()
    assert np.all(np.isfinite(xv)) and np.linalg.norm(bg - d * xv) <= 2e-8 * np.linalg.norm(bg)
    # a second solve on the now dirty workspace, and one on a workspace dirtied by a different solve: a fresh one's bits
    x2, info2 = hp.lsqr(A, b, maxiter=50, workspace=ws)
    assert x2 is ws.x and info2 == info and np.array_equal(pc.bits(x2.local_values()), pc.bits(xv))
    hp.lsqr(A, b, damp=0.7, rtol=0.0, ntol=0.0, maxiter=3, workspace=ws)
    x3, info3 = hp.lsqr(A, b, maxiter=50, workspace=ws)
    assert info3 == info and np.array_equal(pc.bits(x3.local_values()), pc.bits(xv))
    x4, info4 = hp.lsqr(A, b, maxiter=50)
    assert x4 is not ws.x and info4 == info and np.array_equal(pc.bits(x4.local_values()), pc.bits(xv))


# ---- 5. the exact and degenerate cases ----------------------------------------------------------------------------------------
def test_exact_and_degenerate_cases(hp, orc, gpu_backend_i32):
    def solve(mat, bg, **kw):
        A = _matrix(hp, gpu_backend_i32, *mat)
        x, info = hp.lsqr(A, hp.HPCVector.from_global(np.asarray(bg, dtype=np.float64), gpu_backend_i32), **kw)
        xv = x.local_values()
        assert np.all(np.isfinite(xv))
        assert len(info.residual_norms) == len(info.normal_residual_norms) == info.iterations + 1
        return xv, info

    xv, info = solve(lc.DIAG20, [1.0, 0.0], rtol=0.0, ntol=0.0)                      # gate U
    assert (xv.tolist(), info.iterations, info.status, info.converged) == ([0.5, 0.0], 1, "converged", True)
    assert (info.residual_norms, info.normal_residual_norms) == ([1.0, 0.0], [2.0, 0.0])
    xv, info = solve(lc.DIAG10, [0.0, 1.0])
    assert (xv.tolist(), info.iterations, info.status, info.converged) == ([0.0, 0.0], 0, "least_squares", True)
    assert (info.residual_norms, info.normal_residual_norms) == ([1.0], [0.0])
    xv, info = solve(lc.DIAG10, [1.0, 1.0])
    assert (info.iterations, info.status) == (1, "least_squares")
    assert xv[1] == 0.0 and abs(xv[0] - 1.0) <= 1e-15
    assert info.residual_norms == [math.sqrt(2.0), 1.0000000000000002] and info.normal_residual_norms[1] <= 1e-15
    xv, info = solve(lc.THREE_BY_TWO, [1.0, 2.0, 0.0])
    assert (info.iterations, info.status) == (2, "least_squares") and np.all(np.abs(xv - [0.0, 1.0]) <= 1e-15)
    bi = orc.fill_uniform(0, 5, pc.SEED_RHS)
    xv, info = solve(lc.identity(5), bi)
    assert (info.iterations, info.status) == (1, "converged") and np.all(np.abs(xv - bi) <= 4 * np.spacing(bi))
    xv, info = solve(lc.DIAG1NAN, [1.0, 1.0])
    assert (info.iterations, info.status, info.converged) == (0, "breakdown", False) and not xv.any()
    xv, info = solve(lc.identity(5), np.zeros(5))
    assert (info.iterations, info.status, info.residual_norms, info.converged) == (0, "converged", [0.0], True) and not xv.any()
    hp.clear_plan_cache()


# ---- 6. convergence ---------------------------------------------------------------------------------------------------------
def _check_answer(c, damp, xv, info, ref):
    case, dense = c["case"], c["dense"]
    b = case[4]
    _, its_ref, status_ref, _, _, _ = ref
    assert info.status == status_ref and info.converged
    assert abs(info.iterations - its_ref) <= 2, (info.iterations, its_ref)
    assert len(info.residual_norms) == len(info.normal_residual_norms) == info.iterations + 1
    Ab, bb = lc.augmented(dense, b, damp)
    x_ref = np.linalg.lstsq(Ab, bb, rcond=None)[0]
    err = np.linalg.norm(xv - x_ref) / np.linalg.norm(x_ref)
    rbar = bb - Ab @ xv
    rn = float(np.linalg.norm(rbar))
    line = f"{info.status} at {info.iterations} (restatement {its_ref}), against lstsq {err:.2e}"
    assert err <= 1e-6, err
    if info.status == "converged":
        true = np.linalg.norm(b - dense @ xv) / np.linalg.norm(b)
        line += f", true relative residual {true:.2e}"
        assert true <= pc.TRUE_RES_RTOL
    else:
        normal = np.linalg.norm(Ab.T @ rbar) / (np.linalg.norm(Ab) * rn)
        rel = abs(info.residual_norms[-1] - rn) / rn
        line += f", true normal residual {normal:.2e} of |Abar|_F |rbar|, last history entry off by {rel:.2e}"
        assert normal <= 2e-8 and rel <= 1e-11
    return line


@pytest.mark.parametrize("size", lc.SIZES)
def test_convergence_on_the_tall_and_wide_cases(hp, cases, gpu_backend_i32, size):
    """``hp.lsqr(hp.transpose(W), b)`` against ``hp.lsqr(T, b)`` is compared bit for bit: T's rows (the oracle's 5-point rows, then
    a diagonal) and W's rows (``transpose_csr``) both have ascending columns, which is the order ``transpose(.).materialize()``
    stores, so the materialised transpose(W) is T entry for entry and its cached transpose W is T's materialised transpose."""
    mats = {}
    for kind in lc.CASES:
        c = cases[kind, size]
        case = c["case"]
        A = mats[kind] = _matrix(hp, gpu_backend_i32, *case[:4])
        b = hp.HPCVector.from_global(case[4], gpu_backend_i32)
        for damp in lc.DAMPS:
            x, info = hp.lsqr(A, b, damp=damp)
            print(f"{kind} {size} damp {damp}: " + _check_answer(c, damp, x.local_values(), info, c["ref"][damp]))
    c = cases["wide", size]
    case = c["case"]
    b = hp.HPCVector.from_global(case[4], gpu_backend_i32)
    x0 = hp.HPCVector.from_global(np.full(case[3], 1e-3), gpu_backend_i32)
    x, info = hp.lsqr(mats["wide"], b, x0=x0)
    assert info.converged and info.status == "converged"
    assert np.linalg.norm(case[4] - c["dense"] @ x.local_values()) <= pc.TRUE_RES_RTOL * np.linalg.norm(case[4])
    # the lazy transpose of the wide matrix is the tall one
    tcase = cases["tall", size]["case"]
    for rp, ci in ((tcase[0], tcase[1]), (case[0], case[1])):
        assert all(np.all(np.diff(ci[rp[i]:rp[i + 1]]) > 0) for i in range(len(rp) - 1))
    bt = hp.HPCVector.from_global(tcase[4], gpu_backend_i32)
    x1, info1 = hp.lsqr(mats["tall"], bt, damp=0.3)
    x1 = x1.local_values().copy()
    W = _matrix(hp, gpu_backend_i32, *case[:4])                                      # a fresh W: nothing cached on it yet
    x2, info2 = hp.lsqr(hp.transpose(W), bt, damp=0.3)
    assert info2 == info1 and np.array_equal(pc.bits(x2.local_values()), pc.bits(x1))
    assert hp.transpose(W).materialize().cached_transpose is W
    hp.clear_plan_cache()


# ---- 7. argument errors -------------------------------------------------------------------------------------------------------
def test_lsqr_argument_errors(hp, orc, cases, gpu_backend_i32):
    case = cases["tall", (16, 16)]["case"]
    n = case[3]
    A = _matrix(hp, gpu_backend_i32, *case[:4])
    b = hp.HPCVector.from_global(case[4], gpu_backend_i32)
    on_cols = hp.HPCVector.from_global(np.ones(n), gpu_backend_i32)
    with pytest.raises(ValueError):
        hp.lsqr(A, on_cols)                                                          # b on the columns
    with pytest.raises(ValueError):
        hp.lsqr(A, b, x0=b)                                                          # x0 on the rows
    with pytest.raises(ValueError):
        hp.lsqr(A, b, x0=on_cols, damp=0.3)
    x, info = hp.lsqr(A, b, x0=on_cols, damp=0.0, maxiter=2)                         # x0 alone is fine
    assert info.status == "maxiter"
    with pytest.raises(ValueError):
        hp.lsqr(A, b, check_every=0)
    for bad in (dict(ntol=-1e-8), dict(rtol=-1.0), dict(atol=-1.0), dict(damp=-0.1), dict(maxiter=-1)):
        with pytest.raises(ValueError):
            hp.lsqr(A, b, **bad)
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    A32 = hp.HPCSparseMatrix_local(case[0], case[1], case[2].astype(np.float32), n, b32)
    with pytest.raises(TypeError):
        hp.lsqr(A32, hp.HPCVector.from_global(case[4], b32))
    # a square nonsymmetric matrix is accepted
    rowptr, colidx, vals, bg = bc.convection_diffusion(orc, 16, 16)
    S = _matrix(hp, gpu_backend_i32, rowptr, colidx, vals, len(bg))
    bs = hp.HPCVector.from_global(bg, gpu_backend_i32)
    x, info = hp.lsqr(S, bs, maxiter=20000)
    true = np.linalg.norm(bg - pc.matvec(rowptr, colidx, vals, x.local_values())) / np.linalg.norm(bg)
    print(f"square convection-diffusion 16x16: {info.status} at {info.iterations}, true relative residual {true:.2e}")
    assert info.converged
    hp.clear_plan_cache()


# ---- 8. ranks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_lsqr_across_ranks(nranks):
    """The ranks share the one GPU (peer-window push transport, like tests/test_gpu_multirank.py); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
