"""GPU tests of the factorised sparse approximate inverse preconditioner: ``hp.fsai`` against the Cholesky-order restatement of
tests/_fsai_cases.py (structure exactly, values within FSAI_RTOL), its product, its errors, ``hp.cg`` with ``M=hp.fsai(A)``
against ``pcg_op``, the untouched ``M=None`` / ``"jacobi"`` paths, and the build and the solve across ranks.

Margins (none of them taken from the device's results):
  * G's values: FSAI_RTOL, ten times the difference of the two CPU restatements (tests/_fsai_cases.py has the basis);
  * histories, iteration counts, true residual: those of tests/test_gpu_pcg.py (CG_RTOL on the first HEAD entries, +-2,
    TRUE_RES_RTOL), against ``pcg_op`` run with the restatement's G.
"""
import os

import numpy as np
import pytest

from tests import _fsai_cases as fc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_fsai_worker.py")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(orc):
    """Every SPD case and the scaled Poisson case at LARGE_SIZE with the restatement's G, computed once."""
    out = {}
    every = dict(fc.spd_cases(orc))
    every["large"] = (*pc.scaled_poisson(orc, *pc.LARGE_SIZE), None)
    for name, (rowptr, colidx, vals, b, pat) in every.items():
        out[name] = dict(rowptr=rowptr, colidx=colidx, vals=vals, b=b, pattern=pat, n=len(b),
                         G=fc.fsai_cholesky(rowptr, colidx, vals, pattern=pat))
    return out


@pytest.fixture(scope="module")
def solves(cases):
    """``pcg_op`` at rtol = 1e-8 on the cases the solver is run on, once."""
    names = [f"poisson{nx}x{ny}" for nx, ny in pc.SIZES] + ["large", "diagonal"]
    return {k: fc.pcg_op(*[cases[k][f] for f in ("rowptr", "colidx", "vals", "b", "G")], rtol=1e-8) for k in names}


def _matrix(hp, backend, c):
    return hp.HPCSparseMatrix_local(c["rowptr"], c["colidx"], c["vals"], c["n"], backend)


def _build(hp, backend, c):
    A = _matrix(hp, backend, c)
    return A, hp.fsai(A, pattern=hp.spgemm(A, A) if c["pattern"] is not None else None)


def _host_csr(M):
    """(rowptr, global columns, values) of a one-rank matrix."""
    return (M.rowptr_target.cpu().numpy().astype(np.int64), M.col_indices[M.colval.astype(np.int64)],
            M.nzval.cpu().numpy())


# ---- 1. G ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_G_matches_the_restatement(hp, cases, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    """Every banded w (m ramps from 1 across the lane-class edges 4|5, 8|9, 16|17 up to 32), the three Poisson sizes (1023 rows:
    a ragged last workgroup), the diagonal case and the A^2 pattern (hp.spgemm's structure against the host's).  An Int64
    backend's plans are narrowed to the Int32 kernels by default; "i64wide" withholds that, so the _i64 entries run."""
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    for name, c in cases.items():
        if name == "large":
            continue
        A, F = _build(hp, backend, c)
        assert hp.get_vector_plan(A, hp.HPCVector.zeros(A.col_partition, backend)).is_i64 == (which == "i64wide")
        gp, gc, gv = _host_csr(F.G)
        wp, wc, wv = c["G"]
        assert np.array_equal(gp, wp) and np.array_equal(gc, wc), name
        dev = float(np.max(np.abs(gv - wv) / np.abs(wv)))
        print(f"{which} {name}: largest row {F.max_row}, largest relative deviation of an entry {dev:.2e}")
        assert F.max_row == int(np.diff(wp).max()), name
        assert dev <= fc.FSAI_RTOL, (name, dev)
        assert np.array_equal(F.G.row_partition, F.Gt.row_partition) and F.G.shape == F.Gt.shape == (c["n"], c["n"])
    hp.clear_plan_cache()


def test_apply_is_the_two_products_and_two_builds_agree(hp, cases, gpu_backend_i32):
    for name in ("poisson33x31", "banded31", "pattern16x16"):
        c = cases[name]
        A, F = _build(hp, gpu_backend_i32, c)
        r = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
        z = F.apply(r)
        want = F.Gt @ (F.G @ r)
        assert np.array_equal(pc.bits(z.local_values()), pc.bits(want.local_values())), name
        out = r.similar()
        assert F.apply(r, out=out) is out and np.array_equal(pc.bits(out.local_values()), pc.bits(want.local_values()))
        # Gt holds G's values, moved: the host transpose of the device's G, bit for bit
        tp, tc, tv = fc.transpose_csr(*_host_csr(F.G), c["n"])
        hp_, hc, hv = _host_csr(F.Gt)
        assert np.array_equal(hp_, tp) and np.array_equal(hc, tc) and np.array_equal(pc.bits(hv), pc.bits(tv)), name
        # ... and close to what numpy gives for the restatement's product
        zr = pc.matvec(*fc.transpose_csr(*c["G"], c["n"]), pc.matvec(*c["G"], c["b"]))
        assert np.allclose(z.local_values(), zr, rtol=1e-12, atol=1e-12 * np.abs(zr).max()), name
        _, F2 = _build(hp, gpu_backend_i32, c)
        assert F2.G is not F.G and np.array_equal(pc.bits(_host_csr(F2.G)[2]), pc.bits(_host_csr(F.G)[2])), name
    hp.clear_plan_cache()


# ---- 2. errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64"])
def test_errors_and_a_good_call_afterwards(hp, cases, gpu_backend_i32, gpu_backend_i64, which):
    import torch
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    mk = lambda m: hp.HPCSparseMatrix_local(*m, len(m[0]) - 1, backend)
    good = cases["banded7"]

    def good_call_passes():
        _, F = _build(hp, backend, good)
        assert np.array_equal(_host_csr(F.G)[0], good["G"][0])
        assert float(np.max(np.abs(_host_csr(F.G)[2] - good["G"][2]) / np.abs(good["G"][2]))) <= fc.FSAI_RTOL

    for mat, row in (fc.not_spd_diag(), fc.not_spd_block()):
        with pytest.raises(ValueError, match=rf"fsai: A is not positive definite on the pattern of row {row}$"):
            hp.fsai(mk(mat))
        good_call_passes()
    with pytest.raises(ValueError, match=r"fsai: a pattern row has more than 32 owned entries"):
        hp.fsai(mk(fc.banded(fc.CAP_W)))
    good_call_passes()
    mat, row = fc.no_diagonal()
    with pytest.raises(ValueError, match=rf"fsai: row {row} stores no diagonal$"):
        hp.fsai(mk(mat))
    good_call_passes()
    # a NaN on the diagonal of row 123: the first system that holds it is row 123's own
    A = _matrix(hp, backend, good)
    row = 123
    pos = int(good["rowptr"][row] + np.flatnonzero(good["colidx"][good["rowptr"][row]:good["rowptr"][row + 1]] == row)[0])
    A.nzval[pos:pos + 1].fill_(float("nan"))
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match=rf"fsai: A is not positive definite on the pattern of row {row}$"):
        hp.fsai(A)
    good_call_passes()
    # the argument rules, on real objects
    rect = hp.HPCSparseMatrix_local(good["rowptr"], good["colidx"], good["vals"], good["n"] + 3, backend)
    with pytest.raises(ValueError, match="square"):
        hp.fsai(rect)
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    with pytest.raises(TypeError):
        hp.fsai(hp.HPCSparseMatrix_local(good["rowptr"], good["colidx"], good["vals"].astype(np.float32), good["n"], b32))
    with pytest.raises(ValueError, match="pattern"):
        hp.fsai(_matrix(hp, backend, good), pattern=_matrix(hp, backend, cases["diagonal"]))
    hp.clear_plan_cache()


# ---- 3. cg with M = fsai(A) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"poisson{nx}x{ny}" for nx, ny in pc.SIZES] + ["large"])
def test_cg_with_fsai(hp, cases, solves, gpu_backend_i32, name):
    c = cases[name]
    A, F = _build(hp, gpu_backend_i32, c)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    _, its_ref, status_ref, h_ref = solves[name]
    assert status_ref == "converged"
    runs = []
    for chunk in (1, 8, 50):
        x, info = hp.cg(A, b, rtol=1e-8, M=F, check_every=chunk)
        runs.append((info.iterations, info.status, pc.bits(x.local_values()).copy(), pc.bits(info.residual_norms).copy()))
    true = hp.norm(b - A @ x) / hp.norm(b)
    head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:pc.HEAD], h_ref[:pc.HEAD]))
    print(f"{name}: iterations {info.iterations} (restatement {its_ref}), true residual {true:.3e}, head deviation {head:.2e}")
    assert info.converged and info.status == "converged"
    assert len(info.residual_norms) == info.iterations + 1
    assert abs(info.iterations - its_ref) <= 2
    assert head <= pc.CG_RTOL
    assert true <= pc.TRUE_RES_RTOL
    for its, status, xb, hb in runs[1:]:
        assert (its, status) == runs[0][:2] and np.array_equal(xb, runs[0][2]) and np.array_equal(hb, runs[0][3])
    hp.clear_plan_cache()


def test_cg_with_fsai_x0_maxiter_zero_rhs_and_a_reused_workspace(hp, cases, solves, gpu_backend_i32):
    c = cases["poisson24x20"]
    n = c["n"]
    A, F = _build(hp, gpu_backend_i32, c)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    bnorm = hp.norm(b)
    x, info = hp.cg(A, b, rtol=1e-8, M=F)
    xb, fresh = pc.bits(x.local_values()).copy(), info
    # x0 given: the restatement from the same start, and the stop rule met
    x0g = np.full(n, 1e-3)
    _, its0, status0, _ = fc.pcg_op(c["rowptr"], c["colidx"], c["vals"], c["b"], c["G"], rtol=1e-8, x0=x0g)
    x, info = hp.cg(A, b, x0=hp.HPCVector.from_global(x0g, gpu_backend_i32), rtol=1e-8, M=F)
    assert info.converged and status0 == "converged" and abs(info.iterations - its0) <= 2
    assert hp.norm(b - A @ x) / bnorm <= pc.TRUE_RES_RTOL
    # maxiter hit: the restatement's head, no convergence
    _, _, status5, h5 = fc.pcg_op(c["rowptr"], c["colidx"], c["vals"], c["b"], c["G"], rtol=1e-8, maxiter=5)
    x, info = hp.cg(A, b, rtol=1e-8, maxiter=5, M=F, check_every=3)
    assert (info.converged, info.iterations, info.status, len(info.residual_norms)) == (False, 5, "maxiter", 6)
    assert status5 == "maxiter" and max(abs(g - w) / w for g, w in zip(info.residual_norms, h5)) <= pc.CG_RTOL
    # b = 0
    x, info = hp.cg(A, hp.HPCVector.from_global(np.zeros(n), gpu_backend_i32), M=F)
    assert (info.converged, info.iterations, info.status, info.residual_norms) == (True, 0, "converged", [0.0])
    assert not x.local_values().any()
    # a workspace reused across preconditioners gives a fresh one's bits
    ws = hp.PCGWorkspace(b)
    hp.cg(A, b, M="jacobi", rtol=1e-8, workspace=ws)
    x, info = hp.cg(A, b, rtol=1e-8, M=F, workspace=ws)
    assert x is ws.x and info == fresh and np.array_equal(pc.bits(x.local_values()), xb)
    x, info = hp.cg(A, b, rtol=1e-8, M=F, workspace=ws)
    assert info == fresh and np.array_equal(pc.bits(x.local_values()), xb)
    # an FSAI of another size is refused
    with pytest.raises(ValueError):
        hp.cg(A, b, M=_build(hp, gpu_backend_i32, cases["poisson16x16"])[1])
    hp.clear_plan_cache()


def test_cg_with_fsai_on_the_diagonal_case_ends_at_iteration_one(hp, cases, solves, gpu_backend_i32):
    c = cases["diagonal"]
    assert solves["diagonal"][1:3] == (1, "converged")
    A, F = _build(hp, gpu_backend_i32, c)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    x, info = hp.cg(A, b, rtol=1e-8, M=F, check_every=8, maxiter=50)
    assert (info.converged, info.iterations, info.status, len(info.residual_norms)) == (True, 1, "converged", 2)
    want = c["b"] / c["vals"]
    xv = x.local_values()
    assert np.all(np.isfinite(xv)) and np.all(np.abs(xv - want) <= 8 * np.spacing(np.abs(want)))


@pytest.mark.parametrize("which", ["i32", "i64", "i64wide"])
def test_cg_with_fsai_on_both_index_types(hp, cases, solves, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    c = cases["poisson16x16"]
    A, F = _build(hp, backend, c)
    b = hp.HPCVector.from_global(c["b"], backend)
    x, info = hp.cg(A, b, rtol=1e-8, M=F)
    assert hp.get_vector_plan(F.G, b).is_i64 == hp.get_vector_plan(F.Gt, b).is_i64 == (which == "i64wide")
    assert info.converged and abs(info.iterations - solves["poisson16x16"][1]) <= 2
    assert hp.norm(b - A @ x) / hp.norm(b) <= pc.TRUE_RES_RTOL
    hp.clear_plan_cache()


# ---- 4. the other preconditioners are where they were -----------------------------------------------------------------------
def test_none_and_jacobi_are_untouched(hp, cases, gpu_backend_i32):
    """M=None: the bits of the fixed-iteration harness, also on a workspace an FSAI solve has used.  M="jacobi": the
    restatement's head and count, as tests/test_gpu_pcg.py holds them."""
    c = cases["poisson24x20"]
    A, F = _build(hp, gpu_backend_i32, c)
    b = hp.HPCVector.from_global(c["b"], gpu_backend_i32)
    x_ref, h_ref = hp.cg_fixed_iterations(A, b, 13)
    x_ref = x_ref.local_values()
    ws = hp.PCGWorkspace(b)
    hp.cg(A, b, rtol=1e-8, M=F, workspace=ws)
    for workspace in (None, ws):
        x, info = hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=13, M=None, check_every=8, workspace=workspace)
        assert (info.iterations, info.status) == (13, "maxiter") and info.residual_norms == h_ref
        assert np.array_equal(pc.bits(x.local_values()), pc.bits(x_ref))
    d = pc.host_diag(c["rowptr"], c["colidx"], c["vals"])
    _, its_ref, _, hj = pc.pcg(c["rowptr"], c["colidx"], c["vals"], c["b"], dinv=1.0 / d, rtol=1e-8)
    fresh = hp.cg(A, b, rtol=1e-8, M="jacobi")
    used = hp.cg(A, b, rtol=1e-8, M="jacobi", workspace=ws)
    assert fresh[1] == used[1] and np.array_equal(pc.bits(fresh[0].local_values()), pc.bits(used[0].local_values()))
    assert abs(fresh[1].iterations - its_ref) <= 2
    assert max(abs(g - w) / w for g, w in zip(fresh[1].residual_norms[:pc.HEAD], hj[:pc.HEAD])) <= pc.CG_RTOL
    hp.clear_plan_cache()


# ---- 5. ranks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_fsai_across_ranks(nranks):
    """The ranks share the one GPU (as tests/test_gpu_qr.py::test_qr_across_ranks); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
