"""GPU tests of the smoothed-aggregation multigrid preconditioner: ``hp.amg`` level by level against the restatement of
tests/_amg_cases.py (aggregates, root counts and partitions exactly; ``P`` and ``Ac`` in pattern, and in values to 1e-13 of the
largest entry), ``M.apply`` against the restatement's cycle, ``hp.cg`` with ``M=hp.amg(A)`` against ``pcg_amg``, the errors, the
untouched ``M=None`` / ``"jacobi"`` paths, and across ranks the part of the setup that exchanges sizes only (the whole hierarchy
needs RCCL between ranks, which ranks sharing one GPU do not have: tests/_multirank_amg_worker.py).

Margins (none of them taken from the device's results): 1e-13 max|entry| on P and Ac (a few dozen separately rounded products and
sums per entry, summed in another order than scipy's); 1e-12 ||r|| on M r; histories, counts and the true residual as
tests/test_gpu_pcg.py holds them (CG_RTOL on the first HEAD entries, +-2, TRUE_RES_RTOL).
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import _amg_cases as ac
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_amg_worker.py")
SMALL = 8            # coarse_size at which every case but n = 1, 2 aggregates at least once
VALUE_TOL = 1e-13
APPLY_TOL = 1e-12

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matrices():
    return ac.cases()


@pytest.fixture(scope="module")
def refs(matrices):
    """name -> the restatement's hierarchy at coarse_size = SMALL, theta = 0 (0.25 on the anisotropic grid), once."""
    return {name: ac.setup(A, coarse_size=SMALL, theta=_theta(name)) for name, A in matrices.items()}


@pytest.fixture(scope="module")
def solves(matrices):
    """name -> (hierarchy at the default coarse_size, b, pcg_amg's result at rtol = 1e-8) on the grids and the one-level cases."""
    out = {}
    for name in ac.GRIDS + ["diagonal", "one", "two"]:
        A = matrices[name]
        levels = ac.setup(A)
        b = ac.rhs(A.shape[0])
        out[name] = (levels, b, ac.pcg_amg(A, b, levels, rtol=1e-8))
    return out


def _theta(name):
    return 0.25 if name.startswith("aniso") else 0.0


def _matrix(hp, backend, A):
    return hp.HPCSparseMatrix_local(A.indptr, A.indices, A.data, A.shape[1], backend)


def _host(M):
    """scipy CSR (sorted, stored zeros kept) of a one-rank matrix."""
    rowptr = M.rowptr_target.cpu().numpy().astype(np.int64)
    cols = M.col_indices[M.colval.astype(np.int64)] if M.nnz else np.zeros(0, dtype=np.int64)
    out = sp.csr_matrix((M.nzval.cpu().numpy(), cols, rowptr), shape=M.shape)
    out.sort_indices()
    return out


def _same_matrix(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), (what, "pattern")
    scale = float(np.abs(want.data).max()) if want.nnz else 1.0
    dev = float(np.abs(got.data - want.data).max()) / scale if want.nnz else 0.0
    assert dev <= VALUE_TOL, (what, dev)
    return dev


def _check_hierarchy(M, levels, name):
    assert [l.n for l in M.levels] == [l["n"] for l in levels], name
    worst = 0.0
    for k, (lvl, ref) in enumerate(zip(M.levels, levels)):
        what = f"{name} level {k}"
        # a row sum of m <= 301 terms in another order: m eps = 6.7e-14 at the star's hub bounds the difference
        assert abs(lvl.rho - ref["rho"]) <= 1e-13 * ref["rho"] and abs(lvl.w - ref["w"]) <= 1e-13 * ref["w"], what
        s = lvl.s.local_values()
        assert np.all(np.abs(s - ref["s"]) <= 1e-13 * np.abs(ref["s"]).max()), what
        if "agg" in ref:
            assert np.array_equal(lvl.aggregates.cpu().numpy(), ref["agg"]), what
            assert lvl.n_roots == int(ref["counts"].sum()) and lvl.rounds == ref["rounds"], what
            assert np.array_equal(lvl.coarse_partition, [0, int(ref["counts"].sum())]), what
        else:
            assert lvl.aggregates is None, what
        if "P" in ref:
            worst = max(worst, _same_matrix(_host(lvl.P), ref["P"], what + " P"))
            worst = max(worst, _same_matrix(_host(lvl.Pt), ref["Pt"], what + " Pt"))
            worst = max(worst, _same_matrix(_host(M.levels[k + 1].A), levels[k + 1]["A"], what + " Ac"))
        else:
            assert lvl.P is None and k == len(levels) - 1, what
            assert (lvl.inverse is not None) == ("inv" in ref) and (lvl.sweeps == ref.get("sweeps")), what
    assert abs(M.operator_complexity - ac.operator_complexity(levels)) <= 1e-12, name
    return worst


# ---- 1. the hierarchy -----------------------------------------------------------------------------------------------------------
WIDE = ["grid37x53", "aniso40x40", "star300", "random600", "path257"]      # the cases the un-narrowed Int64 kernels run on too


@pytest.mark.parametrize("name,which", [(n, w) for n in ac.cases() for w in ("i32", "i64")] + [(n, "i64wide") for n in WIDE])
def test_levels_match_the_restatement(hp, matrices, refs, gpu_backend_i32, gpu_backend_i64, name, which, monkeypatch):
    """Every case at coarse_size = 8: aggregates, root counts, rounds and partitions exactly, P, Pt and Ac in pattern and value.
    "i64wide" withholds the narrowing of an Int64 backend's plans, so the _i64 entries run."""
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    A = _matrix(hp, backend, matrices[name])
    M = hp.amg(A, theta=_theta(name), coarse_size=SMALL)
    worst = _check_hierarchy(M, refs[name], name)
    print(f"{which} {name}: levels {[l.n for l in M.levels]}, rounds {[l.rounds for l in M.levels]}, operator complexity "
          f"{M.operator_complexity:.3f}, largest deviation of an entry {worst:.2e}")
    hp.clear_plan_cache()


@pytest.mark.parametrize("name", ["grid37x53", "grid16x16x16", "star300", "random600", "path257", "diagonal", "two"])
def test_apply_matches_the_cycle_and_two_builds_agree(hp, matrices, refs, gpu_backend_i32, name):
    A = _matrix(hp, gpu_backend_i32, matrices[name])
    M = hp.amg(A, theta=_theta(name), coarse_size=SMALL)
    n = A.shape[0]
    rg = ac.rhs(n, seed=11)
    r = hp.HPCVector.from_global(rg, gpu_backend_i32)
    z = M.apply(r)
    want = ac.cycle(refs[name], rg)
    dev = float(np.linalg.norm(z.local_values() - want)) / float(np.linalg.norm(rg))
    print(f"{name}: ||M r - cycle(r)|| / ||r|| = {dev:.2e}")
    assert dev <= APPLY_TOL, (name, dev)
    out = r.similar()
    assert M.apply(r, out=out) is out and np.array_equal(pc.bits(out.local_values()), pc.bits(z.local_values()))
    assert np.array_equal(pc.bits(r.local_values()), pc.bits(rg))                        # r is read only
    M2 = hp.amg(_matrix(hp, gpu_backend_i32, matrices[name]), theta=_theta(name), coarse_size=SMALL)
    assert len(M2.levels) == len(M.levels)
    for a, b in zip(M.levels, M2.levels):
        assert a.A is not b.A and np.array_equal(pc.bits(a.A.nzval.cpu().numpy()), pc.bits(b.A.nzval.cpu().numpy())), name
        assert np.array_equal(pc.bits(a.s.local_values()), pc.bits(b.s.local_values())), name
        if a.P is not None:
            assert np.array_equal(pc.bits(a.P.nzval.cpu().numpy()), pc.bits(b.P.nzval.cpu().numpy())), name
            assert np.array_equal(a.aggregates.cpu().numpy(), b.aggregates.cpu().numpy()), name
        if a.inverse is not None:
            assert np.array_equal(pc.bits(a.inverse.local_values()), pc.bits(b.inverse.local_values())), name
    assert np.array_equal(pc.bits(M2.apply(r).local_values()), pc.bits(z.local_values())), name
    hp.clear_plan_cache()


@pytest.mark.parametrize("name,q", [("grid16x16x16", 2), ("grid37x53", 3), ("random600", 4), ("star300", 2)])
def test_the_split_galerkin_product(hp, matrices, gpu_backend_i32, name, q, monkeypatch):
    """The rows of Pt split into q runs, the form taken where ``Pt (A P)`` is over hp.spgemm's bound, forced on matrices that do
    not need it (q = 4 is more than some rows of Pt hold: empty runs): the coarse matrix has the restatement's pattern and its
    values within the same 1e-13 of the largest entry (the sums are associated run by run), two builds agree bit for bit, and
    the solve on the two-level hierarchy keeps the count."""
    import sys
    Ah = matrices[name]
    levels = ac.setup(Ah, max_levels=2, coarse_size=SMALL)
    A = _matrix(hp, gpu_backend_i32, Ah)
    usual = hp.amg(A, max_levels=2, coarse_size=SMALL)
    assert usual.levels[0].galerkin == 1
    monkeypatch.setattr(sys.modules[hp.amg.__module__], "FORCE_SPLIT", q)
    M = hp.amg(A, max_levels=2, coarse_size=SMALL)
    assert M.levels[0].galerkin == q and [l.n for l in M.levels] == [l["n"] for l in levels]
    dev = _same_matrix(_host(M.levels[1].A), levels[1]["A"], name + " Ac")
    M2 = hp.amg(A, max_levels=2, coarse_size=SMALL)
    assert np.array_equal(pc.bits(M2.levels[1].A.nzval.cpu().numpy()), pc.bits(M.levels[1].A.nzval.cpu().numpy()))
    bg = ac.rhs(Ah.shape[0])
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    _, its_ref, status_ref, _ = ac.pcg_amg(Ah, bg, levels, rtol=1e-8)
    x, info = hp.cg(A, b, rtol=1e-8, M=M)
    print(f"{name}: split in {q} deviates by {dev:.2e} of the largest entry; iterations {info.iterations} (restatement {its_ref})")
    assert status_ref == "converged" and info.converged and abs(info.iterations - its_ref) <= 2
    assert hp.norm(b - A @ x) / hp.norm(b) <= pc.TRUE_RES_RTOL
    hp.clear_plan_cache()


# ---- 2. cg with M = amg(A) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.GRIDS)
def test_cg_with_amg(hp, matrices, solves, gpu_backend_i32, name):
    A = _matrix(hp, gpu_backend_i32, matrices[name])
    levels, bg, (_, its_ref, status_ref, h_ref) = solves[name]
    M = hp.amg(A)
    assert [l.n for l in M.levels] == [l["n"] for l in levels]
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    assert status_ref == "converged"
    runs = []
    for chunk in (1, 8, 50):
        x, info = hp.cg(A, b, rtol=1e-8, M=M, check_every=chunk)
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


@pytest.mark.parametrize("which", ["i64", "i64wide"])
def test_cg_with_amg_on_int64(hp, matrices, solves, gpu_backend_i64, which, monkeypatch):
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    A = _matrix(hp, gpu_backend_i64, matrices["grid32x32"])
    _, bg, (_, its_ref, _, _) = solves["grid32x32"]
    b = hp.HPCVector.from_global(bg, gpu_backend_i64)
    x, info = hp.cg(A, b, rtol=1e-8, M=hp.amg(A))
    assert hp.get_vector_plan(A, b).is_i64 == (which == "i64wide")
    assert info.converged and abs(info.iterations - its_ref) <= 2
    assert hp.norm(b - A @ x) / hp.norm(b) <= pc.TRUE_RES_RTOL
    hp.clear_plan_cache()


@pytest.mark.parametrize("name", ["diagonal", "one", "two"])
def test_one_level_cases_solve(hp, matrices, solves, gpu_backend_i32, name):
    A = _matrix(hp, gpu_backend_i32, matrices[name])
    levels, bg, (x_ref, its_ref, status_ref, _) = solves[name]
    M = hp.amg(A)
    assert len(M.levels) == len(levels) == 1 and M.levels[0].inverse is not None and M.operator_complexity == 1.0
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    x, info = hp.cg(A, b, rtol=1e-8, M=M, maxiter=50)
    assert info.converged and status_ref == "converged" and abs(info.iterations - its_ref) <= 2
    assert np.allclose(x.local_values(), x_ref, rtol=1e-8, atol=0)
    if name == "diagonal":                                     # 37 singletons at coarse_size = 8: a stall, Jacobi sweeps
        Ms = hp.amg(A, coarse_size=SMALL, coarse_sweeps=2)
        assert len(Ms.levels) == 1 and Ms.levels[0].sweeps == 2 and Ms.levels[0].n_roots == 37
        x, info = hp.cg(A, b, rtol=1e-8, M=Ms, maxiter=50)
        assert info.converged and hp.norm(b - A @ x) / hp.norm(b) <= pc.TRUE_RES_RTOL
    hp.clear_plan_cache()


def test_cg_with_amg_x0_maxiter_zero_rhs_and_a_reused_workspace(hp, matrices, solves, gpu_backend_i32):
    name = "grid32x32"
    Ah = matrices[name]
    n = Ah.shape[0]
    A = _matrix(hp, gpu_backend_i32, Ah)
    levels, bg, _ = solves[name]
    M = hp.amg(A)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    bnorm = hp.norm(b)
    x, info = hp.cg(A, b, rtol=1e-8, M=M)
    xb, fresh = pc.bits(x.local_values()).copy(), info
    x0g = np.full(n, 1e-3)
    _, its0, status0, _ = ac.pcg_amg(Ah, bg, levels, rtol=1e-8, x0=x0g)
    x, info = hp.cg(A, b, x0=hp.HPCVector.from_global(x0g, gpu_backend_i32), rtol=1e-8, M=M)
    assert info.converged and status0 == "converged" and abs(info.iterations - its0) <= 2
    assert hp.norm(b - A @ x) / bnorm <= pc.TRUE_RES_RTOL
    _, _, status5, h5 = ac.pcg_amg(Ah, bg, levels, rtol=1e-8, maxiter=5)
    x, info = hp.cg(A, b, rtol=1e-8, maxiter=5, M=M, check_every=3)
    assert (info.converged, info.iterations, info.status, len(info.residual_norms)) == (False, 5, "maxiter", 6)
    assert status5 == "maxiter" and max(abs(g - w) / w for g, w in zip(info.residual_norms, h5)) <= pc.CG_RTOL
    x, info = hp.cg(A, b, rtol=1e-8, maxiter=0, M=M)
    assert (info.converged, info.iterations, info.status) == (False, 0, "maxiter") and not x.local_values().any()
    x, info = hp.cg(A, hp.HPCVector.from_global(np.zeros(n), gpu_backend_i32), M=M)
    assert (info.converged, info.iterations, info.status, info.residual_norms) == (True, 0, "converged", [0.0])
    assert not x.local_values().any()
    ws = hp.PCGWorkspace(b)
    hp.cg(A, b, M="jacobi", rtol=1e-8, workspace=ws)
    hp.cg(A, b, M=hp.fsai(A), rtol=1e-8, workspace=ws)
    x, info = hp.cg(A, b, rtol=1e-8, M=M, workspace=ws)
    assert x is ws.x and info == fresh and np.array_equal(pc.bits(x.local_values()), xb)
    x, info = hp.cg(A, b, rtol=1e-8, M=M, workspace=ws)
    assert info == fresh and np.array_equal(pc.bits(x.local_values()), xb)
    # every workspace owns its level vectors: a second one, and M.apply's, share none with the first
    held = ws.amg
    ws2 = hp.PCGWorkspace(b)
    hp.cg(A, b, rtol=1e-8, M=M, workspace=ws2)
    own = lambda w: {v.v.data_ptr() for vs in (w.x, w.b, w.t, w.r) for v in vs if v is not None}
    assert ws.amg is held and ws2.amg is not held and not (own(ws.amg) & own(ws2.amg)) and not (own(ws.amg) & own(M.workspace()))
    assert ws.amg.t[-1] is None and ws.amg.r[-1] is None            # the dense last level multiplies by nothing
    with pytest.raises(ValueError, match="another shape or partition"):
        hp.cg(A, b, M=hp.amg(_matrix(hp, gpu_backend_i32, matrices["grid16x16"])))
    hp.clear_plan_cache()


# ---- 3. errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["i32", "i64"])
def test_errors_and_a_good_call_afterwards(hp, matrices, refs, gpu_backend_i32, gpu_backend_i64, which):
    import torch
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    good = matrices["grid16x16"]

    def good_call_passes():
        _check_hierarchy(hp.amg(_matrix(hp, backend, good), coarse_size=SMALL), refs["grid16x16"], "good call")

    for value in (-4.0, 0.0, float("nan")):
        A = _matrix(hp, backend, good)
        row = 123
        pos = int(good.indptr[row] + np.flatnonzero(good.indices[good.indptr[row]:good.indptr[row + 1]] == row)[0])
        A.nzval[pos:pos + 1].fill_(value)
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match=rf"amg: the diagonal of row {row} is not positive"):
            hp.amg(A)
        good_call_passes()
    keep = sp.csr_matrix(good)                                   # row 77 does not store its diagonal
    lil = keep.tolil()
    lil[77, 77] = 0.0
    nodiag = lil.tocsr()
    nodiag.eliminate_zeros()
    with pytest.raises(ValueError, match=r"amg: the diagonal of row 77 is not positive"):
        hp.amg(_matrix(hp, backend, nodiag))
    good_call_passes()
    rect = hp.HPCSparseMatrix_local(good.indptr, good.indices, good.data, good.shape[1] + 3, backend)
    with pytest.raises(ValueError, match="square"):
        hp.amg(rect)
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    with pytest.raises(TypeError):
        hp.amg(hp.HPCSparseMatrix_local(good.indptr, good.indices, good.data.astype(np.float32), good.shape[1], b32))
    A = _matrix(hp, backend, good)
    for kw in (dict(theta=-0.1), dict(theta=1.0), dict(max_levels=0), dict(coarse_size=0), dict(coarse_size=1025),
               dict(coarse_sweeps=0)):
        with pytest.raises(ValueError, match="amg: "):
            hp.amg(A, **kw)
    with pytest.raises(ValueError, match="M must be"):
        hp.cg(A, hp.HPCVector.from_global(ac.rhs(256), backend), M=object())
    good_call_passes()
    hp.clear_plan_cache()


# ---- 4. the other preconditioners are where they were -----------------------------------------------------------------------
def test_none_and_jacobi_are_untouched(hp, matrices, gpu_backend_i32):
    """M=None: the bits of the fixed-iteration harness, also on a workspace an AMG solve has used.  M="jacobi": the bits of a
    fresh workspace on a used one, and the restatement's head and count."""
    Ah = matrices["grid32x32"]
    A = _matrix(hp, gpu_backend_i32, Ah)
    bg = ac.rhs(Ah.shape[0])
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    x_ref, h_ref = hp.cg_fixed_iterations(A, b, 13)
    x_ref = x_ref.local_values()
    before = hp.cg(A, b, rtol=1e-8, M="jacobi")
    before = (before[1], pc.bits(before[0].local_values()).copy())
    ws = hp.PCGWorkspace(b)
    hp.cg(A, b, rtol=1e-8, M=hp.amg(A), workspace=ws)
    for workspace in (None, ws):
        x, info = hp.cg(A, b, rtol=0.0, atol=0.0, maxiter=13, M=None, check_every=8, workspace=workspace)
        assert (info.iterations, info.status) == (13, "maxiter") and info.residual_norms == h_ref
        assert np.array_equal(pc.bits(x.local_values()), pc.bits(x_ref))
        x, info = hp.cg(A, b, rtol=1e-8, M="jacobi", workspace=workspace)
        assert info == before[0] and np.array_equal(pc.bits(x.local_values()), before[1])
    _, its_ref, _, hj = ac.pcg_jacobi(Ah, bg, rtol=1e-8)
    assert abs(before[0].iterations - its_ref) <= 2
    assert max(abs(g - w) / w for g, w in zip(before[0].residual_norms[:pc.HEAD], hj[:pc.HEAD])) <= pc.CG_RTOL
    hp.clear_plan_cache()


# ---- 5. ranks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_amg_across_ranks(nranks):
    """The ranks share the one GPU (as tests/test_gpu_fsai.py::test_fsai_across_ranks); checks in the worker."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
