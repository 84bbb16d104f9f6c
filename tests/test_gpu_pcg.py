"""GPU tests of the converging CG solver: ``hp.diag``, the gated preconditioned update kernels on their own, ``hp.cg`` against
the fixed-iteration harness (same bits), the freeze behind the deciding iteration, convergence on the scaled Poisson cases
and the solve across ranks.  Cases and the numpy restatement: tests/_pcg_cases.py.

Margins (none of them taken from the device's results):
  * elements of r, x, p: bit-equal to numpy's separately rounded expressions (the library is built with -ffp-contract=off);
  * the two sums: 1e-12 relative to math.fsum -- n <= 4.2e6 terms of one sign summed in a two-stage tree of doubles, worst
    case n * 2^-53 = 4.7e-10, observed growth ~ sqrt(log n) ulps; 1e-12 is the project's margin for its reductions;
  * histories: CG_RTOL = 1e-12 on the first 13 entries (three summation orders on the CPU deviated by <= 1.5e-15 there,
    whole histories by 3e-10, which is why only the head is compared); at 65 x 63 four orders spread by <= 2.2e-14 over the
    same head (45 times less; tests/test_pcg_cases.py re-measures it);
  * iteration counts: +-2 of the restatement's (53 / 84 / 121 with Jacobi, identical across those orders; 209-211 / 296-297 /
    444-445 without);
  * true residual: <= 2 rtol (0.51-0.96 rtol across those orders).
"""
import math
import os

import numpy as np
import pytest

from tests import _grid_regimes as gr
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_pcg_worker.py")

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN = 0, 1, 2


def _matrix(hp, backend, rowptr, colidx, vals, n):
    return hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, backend)


@pytest.fixture(scope="module")
def scaled(orc):
    """The three scaled Poisson cases with the restatement's results, computed once."""
    out = {}
    for nx, ny in pc.SIZES:
        rowptr, colidx, vals, b = pc.scaled_poisson(orc, nx, ny)
        d = pc.host_diag(rowptr, colidx, vals)
        ref = {"jacobi": pc.pcg(rowptr, colidx, vals, b, dinv=1.0 / d, rtol=1e-8),
               "none": pc.pcg(rowptr, colidx, vals, b, rtol=1e-8)}
        out[(nx, ny)] = dict(rowptr=rowptr, colidx=colidx, vals=vals, b=b, d=d, ref=ref)
    return out


# ---- 1. diag ------------------------------------------------------------------------------------------------------------
def _random_with_gaps():
    """300 x 300, ~40 % of the diagonal missing, a stored -0.0 and a stored explicit 0.0 on it, empty rows."""
    rng = np.random.default_rng(0x51A6)
    n = 300
    rowptr, cols, vals = [0], [], []
    for i in range(n):
        if i in (5, 77, 299):                                   # empty rows (the last one included)
            rowptr.append(len(cols))
            continue
        c = set(int(v) for v in rng.choice(n, size=int(rng.integers(1, 12)), replace=False))
        c.discard(i)
        if rng.random() >= 0.4 or i in (10, 20):
            c.add(i)
        if not c:
            c.add((i + 1) % n)
        c = sorted(c)
        v = rng.uniform(-2.0, 2.0, size=len(c))
        if i == 10:
            v[c.index(i)] = -0.0
        if i == 20:
            v[c.index(i)] = 0.0
        cols += c
        vals += list(v)
        rowptr.append(len(cols))
    return np.array(rowptr, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals, dtype=np.float64), n


@pytest.mark.parametrize("which", ["i32", "i64"])
def test_diag_bits(hp, scaled, gpu_backend_i32, gpu_backend_i64, which):
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    for (nx, ny), c in scaled.items():
        A = _matrix(hp, backend, c["rowptr"], c["colidx"], c["vals"], nx * ny)
        d = hp.diag(A)
        assert np.array_equal(d.partition, A.row_partition)
        assert np.array_equal(pc.bits(d.local_values()), pc.bits(c["d"])), (nx, ny)
    rowptr, cols, vals, n = _random_with_gaps()
    want = pc.host_diag(rowptr, cols, vals)
    missing = sum(1 for i in range(n) if i not in cols[rowptr[i]:rowptr[i + 1]])
    assert 0.3 * n <= missing <= 0.5 * n and n % 64 != 0
    assert np.signbit(want[10]) and want[10] == 0.0 and not np.signbit(want[20])
    A = _matrix(hp, backend, rowptr, cols, vals, n)
    got = hp.diag(A).local_values()
    assert np.array_equal(pc.bits(got), pc.bits(want))
    assert not np.signbit(got[5]) and got[5] == 0.0                                   # empty row: +0.0
    inv = hp.diag(A, reciprocal=True).local_values()
    with np.errstate(divide="ignore"):
        assert np.array_equal(pc.bits(inv), pc.bits(1.0 / want))


def test_diag_rejects_rectangular_and_float32(hp, gpu_backend_i32):
    rowptr, cols, vals, n = _random_with_gaps()
    A = hp.HPCSparseMatrix_local(rowptr, cols, vals, n + 7, gpu_backend_i32)
    with pytest.raises(ValueError):
        hp.diag(A)
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    A32 = hp.HPCSparseMatrix_local(rowptr, cols, vals.astype(np.float32), n, b32)
    with pytest.raises(ValueError):
        hp.diag(A32)


@pytest.mark.parametrize("ti", [np.int32, np.int64])
@pytest.mark.parametrize("base", [0, 1])
def test_diag_through_the_c_abi(hp, ti, base):
    import torch
    lib = hp._capi.load()
    rowptr, cols, vals, n = _random_with_gaps()
    r0, r1 = 100, 251                                                                  # a slab: non-zero row_start, 151 rows
    a, b = int(rowptr[r0]), int(rowptr[r1])
    col_indices = np.unique(cols[a:b])
    colval = np.searchsorted(col_indices, cols[a:b])
    dev = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr, dtype=dt)).cuda()
    rp_d, cv_d = dev(rowptr[r0:r1 + 1] - a + base, ti), dev(colval + base, ti)
    nz_d, ci_d = dev(vals[a:b], np.float64), dev(col_indices, np.int64)
    out = torch.full((r1 - r0,), 7.0, dtype=torch.float64, device="cuda")
    sfx = "i32" if ti == np.int32 else "i64"
    fn = getattr(lib, f"hpcla_sparse_diag_f64_{sfx}")
    args = (rp_d.data_ptr(), cv_d.data_ptr(), nz_d.data_ptr(), r1 - r0, b - a, base, ci_d.data_ptr(), len(col_indices), r0, 0,
            out.data_ptr(), None)
    assert fn(*args) == 0
    torch.cuda.synchronize()
    assert np.array_equal(pc.bits(out.cpu().numpy()), pc.bits(pc.host_diag(rowptr[r0:r1 + 1] - a, cols[a:b], vals[a:b], r0)))
    # refused on the host, nothing launched: out keeps its bytes
    out.fill_(7.0)
    INVALID = -1
    bad = [(0, None), (10, None), (3, -1), (4, -1), (5, 2), (8, -1)]                   # (argument, value): nulls, negative sizes, base
    for pos, val in bad:
        a2 = list(args)
        a2[pos] = val
        assert fn(*a2) == INVALID, pos
    assert fn(None, None, None, 0, 0, base, None, 0, 0, 0, None, None) == 0            # zero sizes need no arrays
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- 2. the kernels on their own ----------------------------------------------------------------------------------------
def _fsum_rel(got, terms):
    want = math.fsum(terms.tolist())
    return abs(got - want) / abs(want)


@pytest.mark.parametrize("n", gr.PCG_ALONE)
def test_gated_kernels_alone(hp, n):
    """2049 is the last size on one stage-1 workgroup with a scalar tail (the grid is ceil(floor(n / 2) / 1024)), 2051 the first
    odd size on two; 614 403 is odd with 301 partials, which the second stage walks in two trips of 256 lanes, the last one
    ragged (45 lanes), and has 1201 workgroups in the direction kernel; 4 194 307 = 2 * 256 * 4 * 2048 + 3 caps the grid at 2048
    workgroups (eight full trips of the second stage) and is odd.  tests/_grid_regimes.py holds the sizes and
    tests/test_grid_regimes.py checks that they reach every regime of both grids."""
    import torch
    lib = hp._capi.load()
    rng = np.random.default_rng(n)
    host = {k: rng.uniform(-1.0, 1.0, n) for k in ("r", "Ap", "x", "p")}
    host["dinv"] = rng.uniform(0.5, 2.0, n)
    num, den, j = 0.7310585786300049, 1.9, 5
    scal = torch.tensor([num, den, -1.0], dtype=torch.float64, device="cuda")
    work = torch.zeros(lib.hpcla_pcg_work_bytes() // 8, dtype=torch.float64, device="cuda")
    rwork = torch.zeros(lib.hpcla_reduce_work_bytes() // 8, dtype=torch.float64, device="cuda")
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    up = lambda k: torch.from_numpy(host[k]).cuda()
    P = lambda t: t.data_ptr() if t is not None else None

    def residual(dinv, r, pair, st, den_idx=1):
        assert lib.hpcla_pcg_residual_f64(None, P(scal[0:1]), P(scal[den_idx:den_idx + 1]), P(Ap), P(dinv), P(r), n, j, P(st),
                                          P(pair), P(work), None) == 0

    def direction(dinv, r, x, p, pair, st):
        assert lib.hpcla_pcg_direction_f64(P(scal[0:1]), P(scal[1:2]), P(pair[1:2]), P(scal[0:1]), P(r), P(dinv), P(x), P(p), n, j,
                                           P(st), None) == 0

    Ap, dinv = up("Ap"), up("dinv")
    a = num / den
    # -- preconditioned, running
    r, x, p = up("r"), up("x"), up("p")
    pair = torch.zeros(2, dtype=torch.float64, device="cuda")
    residual(dinv, r, pair, state)
    direction(dinv, r, x, p, pair, state)
    torch.cuda.synchronize()
    r_new = host["r"] - a * host["Ap"]
    rr, rz = pair.cpu().tolist()
    beta = rz / num
    assert np.array_equal(pc.bits(r.cpu().numpy()), pc.bits(r_new))
    assert np.array_equal(pc.bits(x.cpu().numpy()), pc.bits(host["x"] + a * host["p"]))
    assert np.array_equal(pc.bits(p.cpu().numpy()), pc.bits(host["dinv"] * r_new + beta * host["p"]))
    e_rr, e_rz = _fsum_rel(rr, r_new * r_new), _fsum_rel(rz, r_new * (host["dinv"] * r_new))
    print(f"n = {n}: sum r^2 rel err {e_rr:.2e}, sum r (dinv r) rel err {e_rz:.2e}")
    assert e_rr <= 1e-12 and e_rz <= 1e-12
    assert state.cpu().tolist() == [0, RUNNING, 0, 0]                                   # thr = 0 < rr: still running
    # -- dinv = NULL and dinv = 1: the bits of the ungated pair
    r0, x0, p0 = up("r"), up("x"), up("p")
    rr0 = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert lib.hpcla_cg_residual_f64(None, 1.0, P(scal[0:1]), P(scal[1:2]), P(Ap), P(r0), n, P(rr0[0:1]), P(rwork), None) == 0
    assert lib.hpcla_cg_direction_f64(1.0, P(scal[0:1]), P(scal[1:2]), 1.0, P(rr0[0:1]), P(scal[0:1]), P(r0), P(x0), P(p0), n,
                                      None) == 0
    for d in (None, ones):
        r1, x1, p1 = up("r"), up("x"), up("p")
        pair1 = torch.zeros(2, dtype=torch.float64, device="cuda")
        residual(d, r1, pair1, state)
        direction(d, r1, x1, p1, pair1, state)
        torch.cuda.synchronize()
        for got, want in ((r1, r0), (x1, x0), (p1, p0), (pair1[0:1], rr0[0:1]), (pair1[1:2], rr0[0:1])):
            assert torch.equal(got.view(torch.int64), want.view(torch.int64)), ("identity" if d is None else "ones")
    # -- frozen: done_iter = j - 1 -> neither kernel writes a byte; done_iter = j -> only the direction kernel runs
    for done, dir_runs in ((j - 1, False), (j, True)):
        st = torch.tensor([done, CONVERGED, 0, 0], dtype=torch.int64, device="cuda")
        r2, x2, p2 = up("r"), up("x"), up("p")
        pair2 = torch.tensor([3.0, 4.0], dtype=torch.float64, device="cuda")
        residual(dinv, r2, pair2, st)
        direction(dinv, r2, x2, p2, pair2, st)
        torch.cuda.synchronize()
        assert np.array_equal(pc.bits(r2.cpu().numpy()), pc.bits(host["r"])) and pair2.cpu().tolist() == [3.0, 4.0]
        if dir_runs:
            b2 = 4.0 / num
            assert np.array_equal(pc.bits(x2.cpu().numpy()), pc.bits(host["x"] + a * host["p"]))
            assert np.array_equal(pc.bits(p2.cpu().numpy()), pc.bits(host["dinv"] * host["r"] + b2 * host["p"]))
        else:
            assert np.array_equal(pc.bits(x2.cpu().numpy()), pc.bits(host["x"]))
            assert np.array_equal(pc.bits(p2.cpu().numpy()), pc.bits(host["p"]))
        assert st.cpu().tolist() == [done, CONVERGED, 0, 0]
    # -- gate A: a non-positive pAp records the breakdown and leaves r alone; gate B: sum r^2 <= thr records convergence
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    r3 = up("r")
    pair3 = torch.tensor([3.0, 4.0], dtype=torch.float64, device="cuda")
    residual(dinv, r3, pair3, st, den_idx=2)
    torch.cuda.synchronize()
    assert st.cpu().tolist()[:2] == [j - 1, BREAKDOWN] and pair3.cpu().tolist() == [3.0, 4.0]
    assert np.array_equal(pc.bits(r3.cpu().numpy()), pc.bits(host["r"]))
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    st[2:3].view(torch.float64).fill_(4.0 * n)                                         # |r_new| < 2 elementwise: rr < 4 n = thr
    residual(dinv, up("r"), pair3, st)
    torch.cuda.synchronize()
    assert st.cpu().tolist()[:2] == [j, CONVERGED]


# ---- 3. same bits as the harness ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_cg_without_stop_has_the_bits_of_the_fixed_iteration_harness(hp, scaled, gpu_backend_i32, gpu_backend_i64, which,
                                                                     monkeypatch):
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    c = scaled[(24, 20)]
    n = len(c["b"])
    A = _matrix(hp, backend, c["rowptr"], c["colidx"], c["vals"], n)
    b = hp.HPCVector.from_global(c["b"], backend)
    x_ref, h_ref = hp.cg_fixed_iterations(A, b, 13)
    x_ref = x_ref.local_values()
    for M in (None, hp.HPCVector.from_global(np.ones(n), backend)):
        x, info = hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=13, M=M, check_every=8)      # 13 is no multiple of the chunk
        assert (info.iterations, info.status, info.converged) == (13, "maxiter", False)
        assert len(info.residual_norms) == 14 and info.residual_norms == h_ref
        assert np.array_equal(pc.bits(x.local_values()), pc.bits(x_ref))
    hp.clear_plan_cache()


# ---- 4. the freeze ----------------------------------------------------------------------------------------------------------
def test_freeze_on_a_diagonal_system_and_a_dirty_workspace(hp, orc, gpu_backend_i32):
    rowptr, colidx, d, bg = pc.diagonal_case(orc)
    n = len(bg)
    _, its_ref, status_ref, _ = pc.pcg(rowptr, colidx, d, bg, dinv=1.0 / d, rtol=1e-8, maxiter=50)
    assert (its_ref, status_ref) == (1, "converged")
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, d, n)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    ws = hp.PCGWorkspace(b)
    x, info = hp.cg(A, b, M="jacobi", rtol=1e-8, check_every=8, maxiter=50, workspace=ws)
    assert x is ws.x
    assert (info.converged, info.iterations, info.status, len(info.residual_norms)) == (True, 1, "converged", 2)
    xv = x.local_values()
    assert np.all(np.isfinite(xv)) and np.all(np.abs(xv - bg / d) <= 4 * np.spacing(np.abs(bg / d)))
    # (e) a second solve on the now dirty workspace, and one on a workspace dirtied by a different solve: a fresh one's bits
    x2, info2 = hp.cg(A, b, M="jacobi", rtol=1e-8, check_every=8, maxiter=50, workspace=ws)
    assert info2 == info and np.array_equal(pc.bits(x2.local_values()), pc.bits(xv))
    hp.cg(A, b, M=None, rtol=0.0, maxiter=3, workspace=ws)
    x3, info3 = hp.cg(A, b, M="jacobi", rtol=1e-8, check_every=8, maxiter=50, workspace=ws)
    assert info3 == info and np.array_equal(pc.bits(x3.local_values()), pc.bits(xv))


def test_freeze_on_the_identity(hp, orc, gpu_backend_i32):
    bg = orc.fill_uniform(0, 5, pc.SEED_RHS)
    A = _matrix(hp, gpu_backend_i32, *pc.diag_matrix(np.ones(5)), 5)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    x, info = hp.cg(A, b, M=None, rtol=0.0, atol=0.0)                                  # thr = 0, rr_1 = 0 exactly; iteration 2 would be 0/0
    assert (info.converged, info.iterations, info.status) == (True, 1, "converged")
    assert info.residual_norms[1] == 0.0 and np.array_equal(pc.bits(x.local_values()), pc.bits(bg))
    # b = 0: x = 0 without an iteration
    x, info = hp.cg(A, hp.HPCVector.from_global(np.zeros(5), gpu_backend_i32))
    assert (info.converged, info.iterations, info.status, info.residual_norms) == (True, 0, "converged", [0.0])
    assert not x.local_values().any()


def test_answer_does_not_depend_on_the_chunk(hp, scaled, gpu_backend_i32):
    c = scaled[(24, 20)]
    A = _matrix(hp, gpu_backend_i32, c["rowptr"], c["colidx"], c["vals"], len(c["b"]))
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    runs = []
    for chunk in (1, 3, 8, 64):
        x, info = hp.cg(A, b, M="jacobi", rtol=1e-8, check_every=chunk)
        assert info.converged
        runs.append((info.iterations, pc.bits(x.local_values()).copy(), pc.bits(info.residual_norms).copy()))
    for its, xb, hb in runs[1:]:
        assert its == runs[0][0] and np.array_equal(xb, runs[0][1]) and np.array_equal(hb, runs[0][2])


def test_breakdown(hp, orc, gpu_backend_i32):
    bg = orc.fill_uniform(0, 5, pc.SEED_RHS)
    A = _matrix(hp, gpu_backend_i32, *pc.diag_matrix(-np.ones(5)), 5)
    x, info = hp.cg(A, hp.HPCVector.from_global(bg, gpu_backend_i32))
    assert (info.converged, info.iterations, info.status, len(info.residual_norms)) == (False, 0, "breakdown", 1)
    assert not x.local_values().any()
    mat, bg = pc.diag_matrix([1.0, -1.0, 2.0, 3.0]), np.array([1.0, 2.0, 1.0, 1.0])
    x_ref, its_ref, status_ref, _ = pc.pcg(*mat, bg)
    assert (its_ref, status_ref) == (1, "breakdown")
    x, info = hp.cg(_matrix(hp, gpu_backend_i32, *mat, 4), hp.HPCVector.from_global(bg, gpu_backend_i32))
    assert (info.converged, info.iterations, info.status, len(info.residual_norms)) == (False, 1, "breakdown", 2)
    xv = x.local_values()
    assert np.all(np.isfinite(xv)) and np.allclose(xv, x_ref, rtol=1e-14, atol=0)


def test_cg_argument_errors(hp, scaled, gpu_backend_i32):
    c = scaled[(16, 16)]
    n = len(c["b"])
    A = _matrix(hp, gpu_backend_i32, c["rowptr"], c["colidx"], c["vals"], n)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    with pytest.raises(ValueError):
        hp.cg(A, b, M="ilu")
    with pytest.raises(ValueError):
        hp.cg(A, b, check_every=0)
    neg = _matrix(hp, gpu_backend_i32, *pc.diag_matrix(-np.ones(n)), n)
    with pytest.raises(ValueError):
        hp.cg(neg, b, M="jacobi")                                                      # minimum(diag) > 0 is required
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    A32 = hp.HPCSparseMatrix_local(c["rowptr"], c["colidx"], c["vals"].astype(np.float32), n, b32)
    with pytest.raises(TypeError):
        hp.cg(A32, hp.HPCVector.from_global(c["b"], b32))


# ---- 5. convergence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", pc.SIZES)
def test_convergence_on_the_scaled_cases(hp, scaled, gpu_backend_i32, size):
    c = scaled[size]
    n = len(c["b"])
    A = _matrix(hp, gpu_backend_i32, c["rowptr"], c["colidx"], c["vals"], n)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    bnorm = hp.norm(b)
    its = {}
    for name, M in (("jacobi", "jacobi"), ("none", None)):
        _, its_ref, status_ref, h_ref = c["ref"][name]
        x, info = hp.cg(A, b, rtol=1e-8, M=M)
        true = hp.norm(b - A @ x) / bnorm
        head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:pc.HEAD], h_ref[:pc.HEAD]))
        print(f"{size} {name}: iterations {info.iterations} (restatement {its_ref}), true residual {true:.3e}, head dev {head:.2e}")
        assert info.converged and info.status == "converged" and status_ref == "converged"
        assert len(info.residual_norms) == info.iterations + 1
        assert true <= pc.TRUE_RES_RTOL
        if name == "jacobi":
            assert head <= pc.CG_RTOL
            assert abs(info.iterations - its_ref) <= 2
        its[name] = info.iterations
    assert 2 * its["jacobi"] <= its["none"], its
    # x0: started from the Jacobi answer perturbed, the solve still meets the stop rule
    x0 = hp.HPCVector.from_global(np.full(n, 1e-3), gpu_backend_i32)
    x, info = hp.cg(A, b, x0=x0, rtol=1e-8, M="jacobi")
    assert info.converged and hp.norm(b - A @ x) / bnorm <= pc.TRUE_RES_RTOL
    hp.clear_plan_cache()


# ---- 6. one solve above one reduction workgroup ---------------------------------------------------------------------------
def test_history_head_at_the_large_size(hp, orc, gpu_backend_i32):
    """65 x 63: 4095 rows, odd, so both sums of every iteration and the p.Ap epilogue run on two stage-1 workgroups and the gated
    second stage adds two partials (the other solves of this file stay on one).  The first HEAD = 13 entries against the
    restatement within CG_RTOL = 1e-12: 45 times the spread of four summation orders on the CPU at this size (6.9e-15 with
    Jacobi, 2.2e-14 without; tests/test_pcg_cases.py re-measures both).  No convergence or count is asserted here."""
    rowptr, colidx, vals, bg = pc.scaled_poisson(orc, *pc.LARGE_SIZE)
    n = len(bg)
    d = pc.host_diag(rowptr, colidx, vals)
    A = _matrix(hp, gpu_backend_i32, rowptr, colidx, vals, n)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    for name, M, dinv in (("jacobi", "jacobi", 1.0 / d), ("none", None, None)):
        _, its_ref, status_ref, h_ref = pc.pcg(rowptr, colidx, vals, bg, dinv=dinv, rtol=0.0, atol=0.0, maxiter=pc.HEAD)
        assert (its_ref, status_ref, len(h_ref)) == (pc.HEAD, "maxiter", pc.HEAD + 1)
        x, info = hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=pc.HEAD, M=M)
        assert (info.iterations, info.status, info.converged) == (pc.HEAD, "maxiter", False)
        assert len(info.residual_norms) == pc.HEAD + 1
        head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:pc.HEAD], h_ref[:pc.HEAD]))
        print(f"{pc.LARGE_SIZE} {name}: head deviation {head:.2e}")
        assert head <= pc.CG_RTOL, (name, head)
    hp.clear_plan_cache()


# ---- 7. ranks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_cg_across_ranks(nranks):
    """The ranks share the one GPU (peer-window push transport, like tests/test_gpu_multirank.py); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
