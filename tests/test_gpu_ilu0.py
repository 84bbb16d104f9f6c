"""GPU tests of the fine-grained ILU(0) preconditioner: ``hp.ilu0`` against the restatements of tests/_ilu_cases.py (structure
exactly, values within ILU_RTOL), its application, its errors, ``hp.gmres`` and ``hp.bicgstab`` with ``M=hp.ilu0(A)`` against
``gmres_op`` / ``bicgstab_op`` run on the device's own factors, the untouched ``M=None`` / ``"jacobi"`` paths, and the build and
the solves across ranks.

Margins (none of them taken from the device's results):
  * factor values: ILU_RTOL, ten times the difference of the two sum orders on the CPU; 40 sweeps against the exact ILU(0):
    EXACT_RTOL, a hundred times the CPU restatement's own deviation (tests/_ilu_cases.py has both bases);
  * the application: rtol = 1e-12, atol = 1e-12 max|z|, the margin of tests/test_gpu_fsai.py;
  * histories: HIST_RTOL on the heads whose CPU spread stays below a tenth of it; iteration counts +-2; the true residual
    TRUE_RES_RTOL; the GMRES history rises by no more than RISE_RTOL; the counts are at most JACOBI_FACTOR of the device's own
    Jacobi solve.
"""
import os

import numpy as np
import pytest

from tests import _bicgstab_cases as bc
from tests import _gmres_cases as gc
from tests import _ilu_cases as ic
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_ilu_worker.py")
SIZE_NAMES = [f"convdiff{nx}x{ny}" for nx, ny in list(pc.SIZES) + [pc.LARGE_SIZE]]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(orc):
    """Every factor case (LARGE_SIZE included) as its one-rank block with the restatement's factors at 1 and 3 sweeps, once."""
    out = {}
    for name, (rowptr, colidx, vals, b) in ic.factor_cases(orc, large=True).items():
        bp, bcols, bv = ic.block_csr(rowptr, colidx, vals)
        out[name] = dict(rowptr=rowptr, colidx=colidx, vals=vals, b=b, n=len(b), bp=bp, bc=bcols, bv=bv,
                         f={s: ic.sweep_factors(bp, bcols, bv, s) for s in (1, 3)})
    return out


def _matrix(hp, backend, c):
    return hp.HPCSparseMatrix_local(c["rowptr"], c["colidx"], c["vals"], c["n"], backend)


def _operator(M, solve_sweeps=3):
    """The restatement's K on the device's own factors."""
    bp, bcols, f, lo = M.factors()
    return ic.operator([(bp, bcols, f, lo)], solve_sweeps)


# ---- 1. factors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_factors_match_the_restatement(hp, cases, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    """The three stencil sizes (1023 rows: a ragged last workgroup), every banded w (merges of up to 32 entries a side), the
    asymmetric pattern (empty triangles), the diagonal and the 1 x 1 case.  An Int64 backend's plans are narrowed to the Int32
    kernels by default; "i64wide" withholds that, so the _i64 entries run."""
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    for name, c in cases.items():
        if name == SIZE_NAMES[-1]:
            continue
        A = _matrix(hp, backend, c)
        assert hp.get_vector_plan(A, hp.HPCVector.zeros(A.col_partition, backend)).is_i64 == (which == "i64wide")
        for sweeps in (1, 3):
            M = hp.ilu0(A, sweeps=sweeps)
            bp, bcols, f, lo = M.factors()
            assert lo == 0 and np.array_equal(bp, c["bp"]) and np.array_equal(bcols, c["bc"]), name
            assert (M.sweeps, M.solve_sweeps, M.nnz) == (sweeps, 3, len(c["bc"]))
            want = c["f"][sweeps]
            dev = float(np.max(np.abs(f - want) / np.abs(want)))
            same = np.array_equal(pc.bits(f), pc.bits(want))
            print(f"{which} {name} sweeps={sweeps}: largest relative deviation {dev:.2e}, bit for bit: {same}")
            assert dev <= ic.ILU_RTOL, (name, sweeps, dev)
            M2 = hp.ilu0(A, sweeps=sweeps)
            assert np.array_equal(pc.bits(M2.factors()[2]), pc.bits(f)), name
        assert np.array_equal(pc.bits(M.update(A).factors()[2]), pc.bits(f)), name
    hp.clear_plan_cache()


def test_factors_match_the_restatement_at_4095_rows(hp, cases, gpu_backend_i32):
    """The 65 x 63 case, which the test above leaves out: four scan blocks of the count, the last one a row short.  Int32 only."""
    c = cases[SIZE_NAMES[-1]]
    assert c["n"] == 4095
    A = _matrix(hp, gpu_backend_i32, c)
    for sweeps in (1, 3):
        M = hp.ilu0(A, sweeps=sweeps)
        bp, bcols, f, lo = M.factors()
        assert lo == 0 and np.array_equal(bp, c["bp"]) and np.array_equal(bcols, c["bc"]) and M.nnz == len(c["bc"])
        want = c["f"][sweeps]
        dev = float(np.max(np.abs(f - want) / np.abs(want)))
        print(f"{SIZE_NAMES[-1]} sweeps={sweeps}: largest relative deviation {dev:.2e}, bit for bit: {np.array_equal(pc.bits(f), pc.bits(want))}")
        assert dev <= ic.ILU_RTOL, (sweeps, dev)
    assert np.array_equal(pc.bits(M.update(A).factors()[2]), pc.bits(f))
    hp.clear_plan_cache()


def test_forty_sweeps_reach_the_exact_factors(hp, cases, gpu_backend_i32):
    for name in ("convdiff16x16", "convdiff33x31"):
        c = cases[name]
        exact = ic.exact_ilu0(c["bp"], c["bc"], c["bv"])
        f = hp.ilu0(_matrix(hp, gpu_backend_i32, c), sweeps=ic.EXACT_SWEEPS).factors()[2]
        dev = float(np.max(np.abs(f - exact) / np.abs(exact)))
        print(f"{name}: {ic.EXACT_SWEEPS} sweeps deviate by {dev:.2e} from the exact ILU(0)")
        assert dev <= ic.EXACT_RTOL, (name, dev)
    hp.clear_plan_cache()


# ---- 2. apply -----------------------------------------------------------------------------------------------------------------------
def test_apply_matches_the_restatement_on_the_devices_factors(hp, cases, gpu_backend_i32):
    import torch
    for name in ("convdiff33x31", "banded16", "asymmetric", "diagonal", "one"):       # 1023, 37 and 1: odd local lengths
        c = cases[name]
        A = _matrix(hp, gpu_backend_i32, c)
        r = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
        for s in (1, 2, 3, 16):
            M = hp.ilu0(A, solve_sweeps=s)
            want = _operator(M, s)(c["b"])
            tol = dict(rtol=1e-12, atol=1e-12 * np.abs(want).max())
            z = M.apply(r)
            assert np.allclose(z.local_values(), want, **tol), (name, s)
            out = r.similar()
            assert M.apply(r, out=out) is out and np.array_equal(pc.bits(out.local_values()), pc.bits(z.local_values()))
            assert np.array_equal(pc.bits(r.local_values()), pc.bits(c["b"]))
            for lanes in (2, 4, 8):                                 # the lane-group kernels: another order of the row's sum
                M.lanes = lanes
                assert np.allclose(M.apply(r).local_values(), want, **tol), (name, s, lanes)
        # r as a view 8 bytes into a buffer: the same values
        buf = torch.zeros(c["n"] + 3, dtype=torch.float64, device=r.v.device)
        buf[1:c["n"] + 1].copy_(r.v)
        view = hp.HPCVector_local(buf[1:c["n"] + 1], gpu_backend_i32)
        assert view.v.data_ptr() % 16 == 8
        M.lanes = 1
        assert np.array_equal(pc.bits(M.apply(view).local_values()), pc.bits(M.apply(r).local_values())), name
    c = cases["diagonal"]
    z = hp.ilu0(_matrix(hp, gpu_backend_i32, c)).apply(hp.HPCVector.from_global(c["b"], gpu_backend_i32)).local_values()
    want = c["b"] / c["vals"]
    assert np.all(np.abs(z - want) <= 2 * np.spacing(np.abs(want)))      # r * (1 / d) against r / d
    c = cases["one"]
    z = hp.ilu0(_matrix(hp, gpu_backend_i32, c)).apply(hp.HPCVector.from_global(c["b"], gpu_backend_i32)).local_values()
    assert z.shape == (1,) and abs(z[0] - 1.2) <= 2 * np.spacing(1.2)
    hp.clear_plan_cache()


# ---- 3. errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64"])
def test_errors_and_a_good_call_afterwards(hp, cases, gpu_backend_i32, gpu_backend_i64, which):
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    mk = lambda m: hp.HPCSparseMatrix_local(*m, len(m[0]) - 1, backend)
    good = cases["banded8"]

    def good_call_passes():
        f = hp.ilu0(_matrix(hp, backend, good)).factors()[2]
        assert float(np.max(np.abs(f - good["f"][3]) / np.abs(good["f"][3]))) <= ic.ILU_RTOL

    messages = (rf"^ilu0: the diagonal of row {ic.FAULT_ROWS[0]} is zero or NaN$",
                rf"^ilu0: row {ic.FAULT_ROWS[1]} stores no diagonal$",
                rf"^ilu0: the diagonal of row {ic.FAULT_ROWS[2]} is zero or NaN$")
    for heal, message in enumerate(messages):
        with pytest.raises(ValueError, match=message):
            hp.ilu0(mk(ic.three_faults(heal)))
        good_call_passes()
    assert np.all(np.isfinite(hp.ilu0(mk(ic.three_faults(3))).factors()[2]))
    # a pivot that the sweeps drive to zero: [[1, 1], [1, 1]] has u_11 = 1 - 1 * 1
    singular = (np.array([0, 2, 4], dtype=np.int64), np.array([0, 1, 0, 1], dtype=np.int64), np.ones(4))
    with pytest.raises(ValueError, match=r"^ilu0: the pivot of row 1 is zero or not finite after 3 sweeps$"):
        hp.ilu0(mk(singular))
    good_call_passes()
    # the argument rules, on real objects
    A = _matrix(hp, backend, good)
    rect = hp.HPCSparseMatrix_local(good["rowptr"], good["colidx"], good["vals"], good["n"] + 3, backend)
    with pytest.raises(ValueError, match="square"):
        hp.ilu0(rect)
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    with pytest.raises(TypeError):
        hp.ilu0(hp.HPCSparseMatrix_local(good["rowptr"], good["colidx"], good["vals"].astype(np.float32), good["n"], b32))
    for kw in (dict(sweeps=0), dict(sweeps=65), dict(solve_sweeps=0), dict(solve_sweeps=17)):
        with pytest.raises(ValueError, match="^ilu0: "):
            hp.ilu0(A, **kw)
    # the solvers: cg refuses the object, gmres and bicgstab refuse one of another shape and anything that is no preconditioner
    M = hp.ilu0(A)
    b = hp.HPCVector.from_global(good["b"], backend)
    with pytest.raises(ValueError, match="M must be"):
        hp.cg(A, b, M=M)
    small =hp.ilu0(_matrix(hp, backend, cases["asymmetric"]))
    for solver in (hp.gmres, hp.bicgstab):
        with pytest.raises(ValueError, match="another shape or partition"):
            solver(A, b, M=small)
        with pytest.raises(ValueError, match="M must be"):
            solver(A, b, M=object())
    with pytest.raises(ValueError):
        M.apply(hp.HPCVector.from_global(cases["asymmetric"]["b"], backend))
    hp.clear_plan_cache()


# ---- 4. the solvers -----------------------------------------------------------------------------------------------------------------
def _bits_of(x, info):
    return info.iterations, info.status, pc.bits(x.local_values()).copy(), pc.bits(info.residual_norms).copy()


@pytest.mark.parametrize("name", SIZE_NAMES)
def test_gmres_with_ilu0(hp, cases, gpu_backend_i32, name):
    c = cases[name]
    A = _matrix(hp, gpu_backend_i32, c)
    M = hp.ilu0(A)
    K = _operator(M)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    csr = (c["rowptr"], c["colidx"], c["vals"], c["b"])
    _, its_ref, status_ref, _ = ic.gmres_op(*csr, K, rtol=1e-8)
    assert status_ref == "converged"
    runs = []
    for chunk in (1, 3, 8):
        x, info = hp.gmres(A, b, rtol=1e-8, M=M, check_every=chunk)
        runs.append(_bits_of(x, info))
    true = hp.norm(b - A @ x) / hp.norm(b)
    h = info.residual_norms
    rise = max(b_ / a_ - 1 for a_, b_ in zip(h, h[1:]))
    _, jacobi = hp.gmres(A, b, rtol=1e-8, M="jacobi")
    print(f"{name}: iterations {info.iterations} (restatement {its_ref}, Jacobi on the device {jacobi.iterations}), true residual "
          f"{true:.3e}, largest relative step of the history {rise:.2e}")
    assert info.converged and info.status == "converged" and len(h) == info.iterations + 1
    assert abs(info.iterations - its_ref) <= 2
    assert true <= pc.TRUE_RES_RTOL
    assert rise <= gc.RISE_RTOL
    assert jacobi.converged and info.iterations <= ic.JACOBI_FACTOR * jacobi.iterations
    for run in runs[1:]:
        assert run[:2] == runs[0][:2] and np.array_equal(run[2], runs[0][2]) and np.array_equal(run[3], runs[0][3])
    # the head, at a restart short enough for the head to cross it; restart = 8 crosses restarts over the whole solve
    _, _, _, h_ref = ic.gmres_op(*csr, K, rtol=1e-8, restart=ic.HEAD_RESTART, maxiter=ic.HEAD_GMRES + 3)
    _, info5 = hp.gmres(A, b, rtol=1e-8, M=M, restart=ic.HEAD_RESTART, maxiter=ic.HEAD_GMRES + 3)
    head = max(abs(g - w) / w for g, w in zip(info5.residual_norms[:ic.HEAD_GMRES], h_ref[:ic.HEAD_GMRES]))
    print(f"{name}: head deviation {head:.2e}")
    assert len(h_ref) >= ic.HEAD_GMRES and head <= ic.HIST_RTOL
    _, its8, status8, _ = ic.gmres_op(*csr, K, rtol=1e-8, restart=8)
    x8a, info8 = hp.gmres(A, b, rtol=1e-8, M=M, restart=8, check_every=8)
    first = _bits_of(x8a, info8)
    x8b, info8b = hp.gmres(A, b, rtol=1e-8, M=M, restart=8, check_every=3)
    second = _bits_of(x8b, info8b)
    assert status8 == "converged" and info8.converged and info8.iterations > 8 and abs(info8.iterations - its8) <= 2
    assert hp.norm(b - A @ x8b) / hp.norm(b) <= pc.TRUE_RES_RTOL
    assert first[:2] == second[:2] and np.array_equal(first[2], second[2]) and np.array_equal(first[3], second[3])
    hp.clear_plan_cache()


@pytest.mark.parametrize("name", SIZE_NAMES)
def test_bicgstab_with_ilu0(hp, cases, gpu_backend_i32, name):
    c = cases[name]
    A = _matrix(hp, gpu_backend_i32, c)
    M = hp.ilu0(A)
    K = _operator(M)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    _, its_ref, status_ref, h_ref = ic.bicgstab_op(c["rowptr"], c["colidx"], c["vals"], c["b"], K, rtol=1e-8)
    assert status_ref == "converged"
    runs = []
    for chunk in (1, 3, 8):
        x, info = hp.bicgstab(A, b, rtol=1e-8, M=M, check_every=chunk)
        runs.append(_bits_of(x, info))
    true = hp.norm(b - A @ x) / hp.norm(b)
    head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:ic.HEAD_BICGSTAB], h_ref[:ic.HEAD_BICGSTAB]))
    _, jacobi = hp.bicgstab(A, b, rtol=1e-8, M="jacobi")
    print(f"{name}: iterations {info.iterations} (restatement {its_ref}, Jacobi on the device {jacobi.iterations}), true residual "
          f"{true:.3e}, head deviation {head:.2e}")
    assert info.converged and len(info.residual_norms) == info.iterations + 1
    assert abs(info.iterations - its_ref) <= 2
    assert head <= ic.HIST_RTOL
    assert true <= pc.TRUE_RES_RTOL
    assert jacobi.converged and info.iterations <= ic.JACOBI_FACTOR * jacobi.iterations
    for run in runs[1:]:
        assert run[:2] == runs[0][:2] and np.array_equal(run[2], runs[0][2]) and np.array_equal(run[3], runs[0][3])
    hp.clear_plan_cache()


def test_x0_and_reused_workspaces(hp, cases, gpu_backend_i32):
    c = cases["convdiff24x20"]
    A = _matrix(hp, gpu_backend_i32, c)
    M = hp.ilu0(A)
    K = _operator(M)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    csr = (c["rowptr"], c["colidx"], c["vals"], c["b"])
    x0g = np.full(c["n"], 1e-3)
    x0 = hp.HPCVector.from_global(x0g, gpu_backend_i32)
    for solver, restated, Workspace in ((hp.gmres, ic.gmres_op, hp.GMRESWorkspace), (hp.bicgstab, ic.bicgstab_op, hp.BiCGStabWorkspace)):
        _, its0, status0, _ = restated(*csr, K, rtol=1e-8, x0=x0g)
        x, info = solver(A, b, x0=x0, rtol=1e-8, M=M)
        assert status0 == "converged" and info.converged and abs(info.iterations - its0) <= 2
        assert hp.norm(b - A @ x) / hp.norm(b) <= pc.TRUE_RES_RTOL
        # b = 0, maxiter
        x, info = solver(A, hp.HPCVector.from_global(np.zeros(c["n"]), gpu_backend_i32), M=M)
        assert (info.converged, info.iterations, info.residual_norms) == (True, 0, [0.0]) and not x.local_values().any()
        x, info = solver(A, b, rtol=1e-8, maxiter=5, M=M, check_every=3)
        assert (info.converged, info.iterations, info.status, len(info.residual_norms)) == (False, 5, "maxiter", 6)
        # a reused workspace gives a fresh one's bits, also after another preconditioner has used it
        fresh = _bits_of(*solver(A, b, rtol=1e-8, M=M))
        ws = Workspace(b)
        solver(A, b, rtol=1e-8, M="jacobi", workspace=ws)
        for _ in range(2):
            x, info = solver(A, b, rtol=1e-8, M=M, workspace=ws)
            used = _bits_of(x, info)
            assert x is ws.x and used[:2] == fresh[:2] and np.array_equal(used[2], fresh[2]) and np.array_equal(used[3], fresh[3])
    hp.clear_plan_cache()


# ---- 5. the other preconditioners are where they were ---------------------------------------------------------------------------
def test_none_and_jacobi_are_untouched(hp, cases, gpu_backend_i32):
    c = cases["convdiff24x20"]
    A = _matrix(hp, gpu_backend_i32, c)
    M = hp.ilu0(A)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    for solver, Workspace in ((hp.gmres, hp.GMRESWorkspace), (hp.bicgstab, hp.BiCGStabWorkspace)):
        ws = Workspace(b)
        solver(A, b, rtol=1e-8, M=M, workspace=ws)
        for pre in (None, "jacobi"):
            fresh = _bits_of(*solver(A, b, rtol=1e-8, M=pre, maxiter=400))
            used = _bits_of(*solver(A, b, rtol=1e-8, M=pre, maxiter=400, workspace=ws))
            assert used[:2] == fresh[:2] and np.array_equal(used[2], fresh[2]) and np.array_equal(used[3], fresh[3]), (solver, pre)
    hp.clear_plan_cache()


# ---- 6. ranks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_ilu0_across_ranks(nranks):
    """The ranks share the one GPU (as tests/test_gpu_fsai.py::test_fsai_across_ranks); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
