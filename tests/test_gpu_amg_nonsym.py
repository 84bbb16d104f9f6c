"""GPU tests of the nonsymmetric mode of ``hp.amg`` (``symmetric=False``) and of ``hp.gmres`` / ``hp.bicgstab`` with an AMG
hierarchy as ``M``, against the restatement of tests/_amg_nonsym_cases.py.

1. The graph kernels through the C ABI, one block of a partition at a time (``ac.split_block``: ghost columns occur and stay out
   both ways), Int32 and Int64, on ``nc.graph_cases()``: the combined row pointer exactly, every row of E u E^T as the sorted
   list of its out-list followed by its in-list (an edge stored both ways twice) and as a set against the restatement's, the word
   behind the columns untouched; then the rounds, the join and the ids on that graph: states, owners and aggregates exactly.
2. The hierarchy of ``hp.amg(A, symmetric=False)``: aggregates, root counts, rounds and partitions exactly; P, R and Ac in pattern
   and in values to VALUE_TOL; ``M.apply`` against the restated cycle to APPLY_TOL; two builds bit for bit; the forced split.
3. GMRES (restart 30 and 8) and BiCGStab with the hierarchy: convergence, the true residual, the count within +-2 of the
   restatement's and within JACOBI_FACTOR of Jacobi's restated count, the heads of the histories, independence of ``check_every``,
   ``x0``, ``maxiter``, a zero right-hand side, a reused workspace, and a symmetric hierarchy on an SPD grid.
   ``aggregate_level(A, theta, symmetric=False)`` on 2 and 3 ranks sharing the GPU (tests/_multirank_amg_nonsym_worker.py).
4. The errors, each followed by a good call; the symmetric mode and ``M=hp.ilu0(A)`` as they were.

Margins, none taken from the device's results: VALUE_TOL and APPLY_TOL are those of tests/test_gpu_amg.py with its reasoning (a
few dozen separately rounded products and sums per entry, summed in another order than scipy's); the heads are held to
``_gmres_cases.HIST_RTOL`` = 1e-12: four summation orders of the dots spread them by 1.9e-15 (GMRES) and 5.7e-15 (BiCGStab) on the
CPU (tests/test_amg_nonsym_cases.py asserts ten times that stays below the margin); counts +-2 and TRUE_RES_RTOL as
tests/test_gpu_pcg.py holds them.
"""
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import _amg_cases as ac
from tests import _amg_nonsym_cases as nc
from tests import _gmres_cases as gc
from tests import _ilu_cases as ic
from tests import _pcg_cases as pc

pytestmark = pytest.mark.gpu

VALUE_TOL = 1e-13
APPLY_TOL = 1e-12
F64, I64, I32 = np.float64, np.int64, np.int32
FORMS = [("i32", I32, 0), ("i64", I64, 0), ("i32", I32, 1), ("i64", I64, 1)]


def _torch():
    import torch
    return torch


def _dev(a, dtype):
    a = np.array(a, dtype=dtype).reshape(-1)
    if a.size == 0:
        a = np.zeros(1, dtype=dtype)
    return _torch().from_numpy(a).cuda()


def _full(n, value, dtype):
    torch = _torch()
    t = {np.dtype(F64): torch.float64, np.dtype(I64): torch.int64, np.dtype(I32): torch.int32}[np.dtype(dtype)]
    return torch.full((max(int(n), 1),), value, dtype=t, device="cuda")


def _call(hp, name, *args):
    plain = [a.data_ptr() if hasattr(a, "data_ptr") else (int(a) if isinstance(a, (np.integer, np.bool_)) else a) for a in args]
    rc = getattr(hp._capi.load(), name)(*plain)
    assert rc == 0, (name, rc, hp._capi.last_error())


def _matrix(hp, backend, A):
    return hp.HPCSparseMatrix_local(A.indptr, A.indices, A.data, A.shape[1], backend)


def _host(M):
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


def _bits_of(x, info):
    return info.iterations, info.status, pc.bits(x.local_values()).copy(), pc.bits(info.residual_norms).copy()


def _same_runs(runs):
    for run in runs[1:]:
        assert run[:2] == runs[0][:2] and np.array_equal(run[2], runs[0][2]) and np.array_equal(run[3], runs[0][3])


# ---- 1. the graph kernels, one block at a time --------------------------------------------------------------------------------------
def _block_chain(hp, A, part, j, theta, form, want, tag):
    """weights, strength, symmetrise, rounds, join, ids on block j; returns the aggregates (global ids)."""
    sfx, Ti, base = form
    lib = hp._capi.load()
    lo, hi = int(part[j]), int(part[j + 1])
    n = hi - lo
    rowptr, split, vals, n_own, _ = ac.split_block(A, part, j, base, Ti)
    d_rowptr, d_split, d_vals = _dev(rowptr, Ti), _dev(split, Ti), _dev(vals, F64)
    diag, ratio, info = _full(n, 7.0, F64), _full(n, 7.0, F64), _full(2, 7, I64)
    _call(hp, f"hpcla_amg_weights_f64_{sfx}", d_rowptr, d_split, d_vals, n, n_own, base, diag, ratio, info, None)
    work = _full(lib.hpcla_amg_work_bytes(n) // 8, 0, I64)
    s_rowptr = _full(n + 1, -7, I64)
    structure = (d_rowptr, d_split, d_vals, diag, n, n_own, base, float(theta))
    _call(hp, f"hpcla_amg_strength_count_f64_{sfx}", *structure, s_rowptr, info, work, None)
    e_ptr = want["e_ptr"]
    assert np.array_equal(s_rowptr.cpu().numpy()[:n + 1], e_ptr), (tag, "s_rowptr")
    s_cols = _full(int(e_ptr[-1]) + 1, -7, I32)
    _call(hp, f"hpcla_amg_strength_fill_f64_{sfx}", *structure, s_rowptr, s_cols, None)

    indeg, u_rowptr, info = _full(n, -7, I64), _full(n + 2, -7, I64), _full(2, -7, I64)
    _call(hp, "hpcla_amg_symmetrise_count", s_rowptr, s_cols, n, indeg, u_rowptr, info, work, None)
    got_ptr = u_rowptr.cpu().numpy()
    assert np.array_equal(indeg.cpu().numpy()[:n], want["indeg"]), (tag, "in-degrees")
    assert np.array_equal(got_ptr[:n + 1], want["m_ptr"]) and got_ptr[n + 1] == -7, (tag, "u_rowptr and the word behind it")
    total = int(want["m_ptr"][-1])
    assert info.cpu().numpy().tolist() == [total, -7], (tag, "symmetrise info")
    u_cols = _full(total + 1, -7, I32)
    _call(hp, "hpcla_amg_symmetrise_fill", s_rowptr, s_cols, n, u_rowptr, indeg, u_cols, None)
    cols = u_cols.cpu().numpy()
    assert cols[total] == -7, (tag, "the word behind u_cols")
    for i in range(n):
        row = cols[got_ptr[i]:got_ptr[i + 1]]
        a, b = int(e_ptr[i]), int(e_ptr[i + 1])
        assert np.array_equal(row[:b - a], want["e_cols"][a:b]), (tag, i, "the out-list comes first, in its order")
        assert np.array_equal(np.sort(row), want["multi"][i]), (tag, i, "out-list and in-list")
        assert np.array_equal(np.unique(row), want["u_cols"][want["u_ptr"][i]:want["u_ptr"][i + 1]]), (tag, i, "as a set")

    key, state, state_next, m1, m2 = (_full(n, -7, I64) for _ in range(5))
    _call(hp, "hpcla_amg_mis_init", n, lo, key, state, None)
    counts = _full(lib.hpcla_amg_round_blocks(n), -7, I64)
    for r, want_state in enumerate(want["states"]):
        _call(hp, "hpcla_amg_mis_round", u_rowptr, u_cols, n, key, state, m1, m2, state_next, counts, None)
        assert np.array_equal(state_next.cpu().numpy()[:n], want_state), (tag, f"state after round {r + 1}")
        left = int(np.count_nonzero((want_state >= 0) & (want_state < ac.ROOT)))
        assert int(counts.cpu().numpy().sum()) == left and (left == 0) == (r == len(want["states"]) - 1), tag
        state, state_next = state_next, state
    owner_a, owner_b = _full(n, -7, I32), _full(n, -7, I32)
    rootid, info = _full(n, -7, I64), _full(2, -7, I64)
    _call(hp, "hpcla_amg_join", u_rowptr, u_cols, n, key, state, owner_a, owner_b, rootid, info, work, None)
    assert info.cpu().numpy().tolist() == [-1, want["n_roots"]], (tag, "join info")
    agg = _full(n, -7, I64)
    _call(hp, "hpcla_amg_aggregate_ids", owner_b, rootid, n, want["offset"], agg, None)
    got = agg.cpu().numpy()[:n]
    assert np.array_equal(got, want["agg"]), (tag, "aggregates")
    return got


def _block_want(A, part, j, theta, restated):
    agg, counts, roots, rounds, (u_ptr, u_cols) = restated
    lo, hi = int(part[j]), int(part[j + 1])
    e_ptr, e_cols = ac.strength(A, part, theta)
    a, b = int(e_ptr[lo]), int(e_ptr[hi])
    le_ptr, le_cols = e_ptr[lo:hi + 1] - a, e_cols[a:b] - lo
    n = hi - lo
    row = np.repeat(np.arange(n), np.diff(le_ptr))
    indeg = np.bincount(le_cols, minlength=n).astype(np.int64)
    m_ptr = np.concatenate([[0], np.cumsum(np.diff(le_ptr) + indeg)]).astype(np.int64)
    order = np.argsort(le_cols, kind="stable")
    in_ptr = np.concatenate([[0], np.cumsum(indeg)])
    multi = [np.sort(np.concatenate([le_cols[le_ptr[i]:le_ptr[i + 1]], row[order][in_ptr[i]:in_ptr[i + 1]]])) for i in range(n)]
    lu_ptr, lu_cols = u_ptr[lo:hi + 1] - u_ptr[lo], u_cols[u_ptr[lo]:u_ptr[hi]] - lo
    key, _ = ac.keys_of(part)
    return dict(e_ptr=le_ptr, e_cols=le_cols.astype(I32), indeg=indeg, m_ptr=m_ptr, multi=multi, u_ptr=lu_ptr, u_cols=lu_cols,
                states=list(ac.mis2_states(lu_ptr, lu_cols, key[lo:hi])), n_roots=int(counts[j]),
                offset=int(np.sum(counts[:j])), agg=agg[lo:hi])


@pytest.mark.parametrize("name", sorted(nc.graph_cases()))
def test_graph_kernels_on_every_block(hp, name):
    """Blocks of 1, 2, 3 and 8; the first block count runs all four index forms, the others Int32 and Int64 at base 0."""
    A, theta = nc.graph_cases()[name]
    n = A.shape[0]
    ran = 0
    for k in [k for k in nc.BLOCKS if k <= n]:
        part = ac.equal_blocks(n, k)
        restated = nc.aggregate(A, part, theta)
        rounds = 0
        for j in range(k):
            want = _block_want(A, part, j, theta, restated)
            rounds = max(rounds, len(want["states"]))
            for form in (FORMS if k == 1 else FORMS[:2]):
                _block_chain(hp, A, part, j, theta, form, want, (name, k, j, form[0], form[2]))
                ran += 1
        assert rounds == restated[3], (name, k)
    print(f"{name}: {ran} chains")


def test_graph_kernels_with_no_rows_and_no_edges(hp):
    work, info = _full(4, 0, I64), _full(2, -7, I64)
    u_rowptr = _full(3, -7, I64)
    _call(hp, "hpcla_amg_symmetrise_count", None, None, 0, None, u_rowptr, info, work, None)
    assert u_rowptr.cpu().numpy().tolist() == [0, -7, -7] and info.cpu().numpy().tolist() == [0, -7]
    _call(hp, "hpcla_amg_symmetrise_fill", None, None, 0, None, None, None, None)
    s_rowptr, indeg = _full(3, 0, I64), _full(2, -7, I64)                               # two rows, no edge
    _call(hp, "hpcla_amg_symmetrise_count", s_rowptr, None, 2, indeg, u_rowptr, info, work, None)
    assert u_rowptr.cpu().numpy().tolist() == [0, 0, 0] and indeg.cpu().numpy().tolist() == [0, 0]
    _call(hp, "hpcla_amg_symmetrise_fill", s_rowptr, None, 2, u_rowptr, indeg, None, None)
    lib = hp._capi.load()
    assert lib.hpcla_amg_symmetrise_count(None, None, -1, None, u_rowptr.data_ptr(), info.data_ptr(), work.data_ptr(), None) != 0
    assert lib.hpcla_amg_symmetrise_fill(None, None, 2, None, None, None, None) != 0


@pytest.mark.parametrize("sfx,Ti,base", FORMS)
def test_restrictor_kernel_alone(hp, sfx, Ti, base):
    """The values of R on the pattern of Tt A through a shuffled column space, rows in three workgroups' worth of groups, and a
    row offset: the bits of numpy's separately rounded expression."""
    A = nc.convection_diffusion(33, 31)
    n = A.shape[0]
    agg, counts, _, _, _ = nc.aggregate(A, [0, n], 0.0)
    ncoarse = int(counts.sum())
    s, _, _ = ac.weights(A)
    Tt = sp.csr_matrix((np.ones(n), agg, np.arange(n + 1)), shape=(n, ncoarse)).T.tocsr()
    Tt.sort_indices()
    TA = ac.structural_product(Tt, A)
    offset = 1000
    colval, col_indices = ac.compressed_columns(TA.indices, np.random.default_rng(3))
    row = np.repeat(np.arange(ncoarse), np.diff(TA.indptr))
    want = ((agg + offset)[TA.indices] == row + offset).astype(np.float64) - TA.data * s[TA.indices]
    r = _full(TA.nnz + 1, np.nan, F64)
    _call(hp, f"hpcla_amg_restrictor_f64_{sfx}", _dev(TA.indptr + base, Ti), _dev(colval + base, Ti), _dev(col_indices, I64),
          _dev(TA.data, F64), _dev(agg + offset, I64), _dev(s, F64), ncoarse, n, offset, base, r, None)
    got = r.cpu().numpy()
    assert np.array_equal(ac.bits(got[:TA.nnz]), ac.bits(want)) and np.isnan(got[TA.nnz])
    assert np.array_equal(ac.bits(want), ac.bits(nc.restrictor(A, agg, ncoarse, s).data))


# ---- 2. the hierarchy -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """(name, coarse_size) -> the restated hierarchy, once."""
    return {(name, cs): nc.setup(A, coarse_size=cs) for name, A in nc.solve_cases().items() for cs in nc.COARSE_SIZES}


def _check_hierarchy(M, levels, name):
    assert M.symmetric is False and [l.n for l in M.levels] == [l["n"] for l in levels], name
    worst = 0.0
    for k, (lvl, ref) in enumerate(zip(M.levels, levels)):
        what = f"{name} level {k}"
        assert abs(lvl.rho - ref["rho"]) <= 1e-13 * ref["rho"] and abs(lvl.w - ref["w"]) <= 1e-13 * ref["w"], what
        assert np.all(np.abs(lvl.s.local_values() - ref["s"]) <= 1e-13 * np.abs(ref["s"]).max()), what
        if "agg" in ref:
            assert np.array_equal(lvl.aggregates.cpu().numpy(), ref["agg"]), what
            assert lvl.n_roots == int(ref["counts"].sum()) and lvl.rounds == ref["rounds"], what
            assert np.array_equal(lvl.coarse_partition, [0, int(ref["counts"].sum())]), what
        if "P" in ref:
            assert lvl.Pt is None and lvl.galerkin == 1 and lvl.restriction_split == 1, what
            worst = max(worst, _same_matrix(_host(lvl.P), ref["P"], what + " P"))
            worst = max(worst, _same_matrix(_host(lvl.R), ref["R"], what + " R"))
            worst = max(worst, _same_matrix(_host(M.levels[k + 1].A), levels[k + 1]["A"], what + " Ac"))
        else:
            assert lvl.P is None and lvl.R is None and k == len(levels) - 1, what
            assert (lvl.inverse is not None) == ("inv" in ref), what
    # the last level inverts its matrix as it is: LAPACK's inverse leaves |inv A - I| <= n eps cond(A), with n <= 128 and the
    # condition of these coarse matrices below 1e3 that is under 1e-11; the inverse of (A + A') / 2 misses I by 1e-2 and more
    last = M.levels[-1]
    D = _host(last.A).toarray()
    assert np.abs(last.inverse.local_values() @ D - np.eye(last.n)).max() <= 1e-11, name
    assert np.linalg.cond(D) < 1e3 and np.abs(np.linalg.inv((D + D.T) / 2) @ D - np.eye(last.n)).max() > 1e-3 or last.n == 1, name
    assert abs(M.operator_complexity - ac.operator_complexity(levels)) <= 1e-12, name
    return worst


@pytest.mark.parametrize("cs", nc.COARSE_SIZES)
@pytest.mark.parametrize("name,which", [(n, "i32") for n in nc.hierarchy_cases()] + [("cd33x31", "i64"), ("upwind33x31", "i64wide")])
def test_levels_match_the_restatement(hp, refs, gpu_backend_i32, gpu_backend_i64, name, which, cs, monkeypatch):
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    A = _matrix(hp, backend, nc.hierarchy_cases()[name])
    M = hp.amg(A, coarse_size=cs, symmetric=False)
    worst = _check_hierarchy(M, refs[name, cs], name)
    print(f"{which} {name} coarse_size {cs}: levels {[l.n for l in M.levels]}, rounds {[l.rounds for l in M.levels[:-1]]}, "
          f"operator complexity {M.operator_complexity:.3f}, largest deviation of an entry {worst:.2e}")
    hp.clear_plan_cache()


def test_the_level_counts_the_cases_are_for(refs):
    assert len(refs["cd33x31", 128]) == 3 and len(refs["cd33x31", 8]) == 4 and len(refs["upwind33x31", 8]) == 4


@pytest.mark.parametrize("name", sorted(nc.hierarchy_cases()))
def test_apply_matches_the_cycle_and_two_builds_agree(hp, refs, gpu_backend_i32, name):
    Ah = nc.hierarchy_cases()[name]
    A = _matrix(hp, gpu_backend_i32, Ah)
    M = hp.amg(A, coarse_size=8, symmetric=False)
    rg = ac.rhs(Ah.shape[0], seed=11)
    r = hp.HPCVector.from_global(rg, gpu_backend_i32)
    z = M.apply(r)
    want = nc.cycle(refs[name, 8], rg)
    dev = float(np.linalg.norm(z.local_values() - want)) / float(np.linalg.norm(rg))
    print(f"{name}: ||M r - cycle(r)|| / ||r|| = {dev:.2e}")
    assert dev <= APPLY_TOL, (name, dev)
    assert np.array_equal(pc.bits(r.local_values()), pc.bits(rg))
    M2 = hp.amg(_matrix(hp, gpu_backend_i32, Ah), coarse_size=8, symmetric=False)
    assert len(M2.levels) == len(M.levels)
    for a, b in zip(M.levels, M2.levels):
        assert a.A is not b.A and np.array_equal(pc.bits(a.A.nzval.cpu().numpy()), pc.bits(b.A.nzval.cpu().numpy())), name
        if a.P is not None:
            assert np.array_equal(a.aggregates.cpu().numpy(), b.aggregates.cpu().numpy()), name
            assert np.array_equal(pc.bits(a.P.nzval.cpu().numpy()), pc.bits(b.P.nzval.cpu().numpy())), name
            assert np.array_equal(pc.bits(a.R.nzval.cpu().numpy()), pc.bits(b.R.nzval.cpu().numpy())), name
        if a.inverse is not None:
            assert np.array_equal(pc.bits(a.inverse.local_values()), pc.bits(b.inverse.local_values())), name
    assert np.array_equal(pc.bits(M2.apply(r).local_values()), pc.bits(z.local_values())), name
    hp.clear_plan_cache()


def test_a_symmetric_matrix_gets_the_bits_of_pt(hp, gpu_backend_i32):
    """On the 37 x 53 grid the first level's aggregates, P and R are those of the symmetric mode, R = Pt bit for bit."""
    A = _matrix(hp, gpu_backend_i32, ac.cases()["grid37x53"])
    S, N = hp.amg(A), hp.amg(A, symmetric=False)
    assert S.symmetric is True and S.levels[0].R is S.levels[0].Pt and N.levels[0].Pt is None
    assert [l.n for l in S.levels] == [l.n for l in N.levels]
    assert np.array_equal(S.levels[0].aggregates.cpu().numpy(), N.levels[0].aggregates.cpu().numpy())
    for a, b in ((S.levels[0].P, N.levels[0].P), (S.levels[0].Pt, N.levels[0].R)):
        a, b = _host(a), _host(b)
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        assert np.array_equal(pc.bits(a.data), pc.bits(b.data))
    hp.clear_plan_cache()


def test_the_forced_split(hp, refs, gpu_backend_i32, monkeypatch):
    """The rows of R in 3 runs on 33 x 31 (two levels): the restatement's coarse matrix to VALUE_TOL, two builds bit for bit."""
    Ah = nc.hierarchy_cases()["cd33x31"]
    levels = nc.setup(Ah, max_levels=2)
    A = _matrix(hp, gpu_backend_i32, Ah)
    monkeypatch.setattr(sys.modules[hp.amg.__module__], "FORCE_SPLIT", 3)
    M = hp.amg(A, max_levels=2, symmetric=False)
    assert M.levels[0].galerkin == 3 and M.levels[0].restriction_split == 1 and [l.n for l in M.levels] == [l["n"] for l in levels]
    dev = _same_matrix(_host(M.levels[1].A), levels[1]["A"], "split Ac")
    M2 = hp.amg(A, max_levels=2, symmetric=False)
    assert np.array_equal(pc.bits(M2.levels[1].A.nzval.cpu().numpy()), pc.bits(M.levels[1].A.nzval.cpu().numpy()))
    assert M.levels[1].sweeps == 4 and M.levels[1].inverse is None                     # 152 rows: the sweeps' last level
    bg = ac.rhs(Ah.shape[0])
    _, its_ref, status_ref, _ = nc.gmres_amg(Ah, bg, levels)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    x, info = hp.gmres(A, b, M=M)
    print(f"split in 3 deviates by {dev:.2e}; iterations {info.iterations} (restatement {its_ref})")
    assert status_ref == "converged" and info.converged and abs(info.iterations - its_ref) <= nc.COUNT_SLACK
    assert hp.norm(b - A @ x) / hp.norm(b) <= pc.TRUE_RES_RTOL
    hp.clear_plan_cache()


# ---- 3. the solves --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved(refs):
    """name -> (A, b, levels, Jacobi's restated GMRES(30) count), once."""
    out = {}
    for name, A in nc.solve_cases().items():
        b = ac.rhs(A.shape[0])
        jac = nc.gmres_jacobi(A, b)
        assert jac[2] == "converged"
        out[name] = (A, b, refs[name, 128], jac[1])
    return out


@pytest.mark.parametrize("name", sorted(nc.solve_cases()))
def test_gmres_with_amg(hp, solved, gpu_backend_i32, name):
    Ah, bg, levels, jacobi = solved[name]
    A = _matrix(hp, gpu_backend_i32, Ah)
    M = hp.amg(A, symmetric=False)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    for restart in gc.RESTARTS:
        _, its_ref, status_ref, _ = nc.gmres_amg(Ah, bg, levels, restart=restart)
        assert status_ref == "converged"
        runs = []
        for chunk in (1, 3, 8):
            x, info = hp.gmres(A, b, rtol=1e-8, restart=restart, M=M, check_every=chunk)
            runs.append(_bits_of(x, info))
        true = hp.norm(b - A @ x) / hp.norm(b)
        h = info.residual_norms
        rise = max(b_ / a_ - 1 for a_, b_ in zip(h, h[1:]))
        print(f"{name} restart {restart}: iterations {info.iterations} (restatement {its_ref}, Jacobi restated {jacobi}), true "
              f"residual {true:.3e}, largest relative step of the history {rise:.2e}")
        assert info.converged and info.status == "converged" and len(h) == info.iterations + 1
        assert abs(info.iterations - its_ref) <= nc.COUNT_SLACK
        assert true <= pc.TRUE_RES_RTOL and rise <= gc.RISE_RTOL
        if restart == 30:
            assert info.iterations <= nc.JACOBI_FACTOR * jacobi
        _same_runs(runs)
    _, _, _, h_ref = nc.gmres_amg(Ah, bg, levels, restart=gc.HEAD_RESTART, maxiter=nc.HEAD + 3)
    _, info5 = hp.gmres(A, b, rtol=1e-8, M=M, restart=gc.HEAD_RESTART, maxiter=nc.HEAD + 3)
    head = max(abs(g - w) / w for g, w in zip(info5.residual_norms[:nc.HEAD], h_ref[:nc.HEAD]))
    print(f"{name}: head deviation {head:.2e}")
    assert len(h_ref) >= nc.HEAD and head <= gc.HIST_RTOL
    hp.clear_plan_cache()


@pytest.mark.parametrize("name", sorted(nc.solve_cases()))
def test_bicgstab_with_amg(hp, solved, gpu_backend_i32, name):
    Ah, bg, levels, _ = solved[name]
    A = _matrix(hp, gpu_backend_i32, Ah)
    M = hp.amg(A, symmetric=False)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    _, its_ref, status_ref, h_ref = nc.bicgstab_amg(Ah, bg, levels)
    assert status_ref == "converged"
    runs = []
    for chunk in (1, 3, 8):
        x, info = hp.bicgstab(A, b, rtol=1e-8, M=M, check_every=chunk)
        runs.append(_bits_of(x, info))
    true = hp.norm(b - A @ x) / hp.norm(b)
    head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:nc.HEAD_BICGSTAB], h_ref[:nc.HEAD_BICGSTAB]))
    print(f"{name}: iterations {info.iterations} (restatement {its_ref}), true residual {true:.3e}, head deviation {head:.2e}")
    assert info.converged and abs(info.iterations - its_ref) <= nc.COUNT_SLACK
    assert true <= pc.TRUE_RES_RTOL and head <= gc.HIST_RTOL
    _same_runs(runs)
    hp.clear_plan_cache()


def test_x0_maxiter_zero_rhs_and_a_reused_workspace(hp, solved, gpu_backend_i32):
    Ah, bg, levels, _ = solved["cd24x20"]
    n = Ah.shape[0]
    A = _matrix(hp, gpu_backend_i32, Ah)
    M = hp.amg(A, symmetric=False)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    x0g = ac.rhs(n, seed=5)
    x0 = hp.HPCVector.from_global(x0g, gpu_backend_i32)
    for solver, restated, kw in ((hp.gmres, nc.gmres_amg, dict(restart=8)), (hp.bicgstab, nc.bicgstab_amg, {})):
        _, its_ref, status_ref, _ = restated(Ah, bg, levels, x0=x0g, **kw)
        x, info = solver(A, b, x0=x0, M=M, **kw)
        assert status_ref == "converged" and info.converged and abs(info.iterations - its_ref) <= nc.COUNT_SLACK, solver.__name__
        assert hp.norm(b - A @ x) / hp.norm(b) <= pc.TRUE_RES_RTOL
        _, its_ref, status_ref, h_ref = restated(Ah, bg, levels, maxiter=5, **kw)
        x, info = solver(A, b, M=M, maxiter=5, **kw)
        assert status_ref == "maxiter" and info.status == "maxiter" and info.iterations == 5 and not info.converged
        assert max(abs(g - w) / w for g, w in zip(info.residual_norms[:5], h_ref[:5])) <= gc.HIST_RTOL
        x, info = solver(A, hp.HPCVector.from_global(np.zeros(n), gpu_backend_i32), M=M, **kw)
        assert info.converged and info.iterations == 0 and np.all(x.local_values() == 0.0)
    ws = hp.gmres.__globals__["GMRESWorkspace"](b, 30)
    x1, i1 = hp.gmres(A, b, M=M, workspace=ws)
    first = _bits_of(x1, i1)
    mine = ws.amg
    x2, i2 = hp.gmres(A, hp.HPCVector.from_global(x0g, gpu_backend_i32), M=M, workspace=ws)      # another right-hand side between
    x3, i3 = hp.gmres(A, b, M=M, workspace=ws)
    assert x3 is ws.x and ws.amg is mine and M._work is None                              # the solve's own level vectors, kept
    _same_runs([first, _bits_of(x3, i3)])
    wb = hp.bicgstab.__globals__["BiCGStabWorkspace"](b)
    y1, j1 = hp.bicgstab(A, b, M=M, workspace=wb)
    first = _bits_of(y1, j1)
    y2, j2 = hp.bicgstab(A, b, M=M, workspace=wb)
    _same_runs([first, _bits_of(y2, j2)])
    hp.clear_plan_cache()


def test_a_symmetric_hierarchy_through_gmres_and_bicgstab(hp, gpu_backend_i32):
    Ah = ac.cases()["grid37x53"]
    levels = ac.setup(Ah)
    bg = ac.rhs(Ah.shape[0])
    A = _matrix(hp, gpu_backend_i32, Ah)
    M = hp.amg(A)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    csr = nc.csr_arrays(Ah)
    K = lambda r: ac.cycle(levels, r)
    for solver, restated in ((hp.gmres, ic.gmres_op), (hp.bicgstab, ic.bicgstab_op)):
        _, its_ref, status_ref, _ = restated(*csr, bg, K)
        x, info = solver(A, b, M=M)
        print(f"{solver.__name__}: iterations {info.iterations} (restatement {its_ref})")
        assert status_ref == "converged" and info.converged and abs(info.iterations - its_ref) <= nc.COUNT_SLACK
        assert hp.norm(b - A @ x) / hp.norm(b) <= pc.TRUE_RES_RTOL
    hp.clear_plan_cache()


@pytest.mark.parametrize("nranks", [2, 3])
def test_nonsymmetric_aggregation_across_ranks(nranks):
    """The ranks share the one GPU (as tests/test_gpu_amg.py::test_amg_across_ranks); checks in the worker."""
    import os
    from hpcla_amd.launch import spawn_ranks
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_multirank_amg_nonsym_worker.py")
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([worker], nranks, env_extra={"HPCLA_PUSH_TIMEOUT_S": "30"}, timeout=120, forward_rank0_stdout=False) == 0


# ---- 4. errors, and the paths that were there ------------------------------------------------------------------------------------
def test_errors_and_a_good_call_afterwards(hp, gpu_backend_i32):
    Ah = nc.convection_diffusion(16, 16)
    A = _matrix(hp, gpu_backend_i32, Ah)
    b = hp.HPCVector.from_global(ac.rhs(256), gpu_backend_i32)
    M = hp.amg(A, symmetric=False)
    with pytest.raises(ValueError, match="symmetric=False"):
        hp.cg(A, b, M=M)
    other = hp.amg(_matrix(hp, gpu_backend_i32, nc.convection_diffusion(24, 20)), symmetric=False)
    for solver in (hp.gmres, hp.bicgstab):
        with pytest.raises(ValueError, match="another shape or partition"):
            solver(A, b, M=other)
    for value in nc.BAD_SYMMETRIC:
        with pytest.raises(TypeError, match="symmetric"):
            hp.amg(A, symmetric=value)
        with pytest.raises(TypeError, match="symmetric"):
            hp.amg.__globals__["aggregate_level"](A, symmetric=value)
    bad = Ah.copy().tolil()
    bad[77, 77] = -4.0
    bad[200, 200] = 0.0
    with pytest.raises(ValueError, match="row 77 is not positive"):
        hp.amg(_matrix(hp, gpu_backend_i32, bad.tocsr()), symmetric=False)
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    with pytest.raises(TypeError):
        hp.amg(hp.HPCSparseMatrix_local(Ah.indptr, Ah.indices, Ah.data.astype(np.float32), 256, b32), symmetric=False)
    for solver in (hp.gmres, hp.bicgstab):
        x, info = solver(A, b, M=M)
        assert info.converged and hp.norm(b - A @ x) / hp.norm(b) <= pc.TRUE_RES_RTOL
    hp.clear_plan_cache()


def test_the_symmetric_mode_is_what_it_was(hp, gpu_backend_i32):
    """``hp.amg(A)`` and ``hp.cg(M=hp.amg(A))`` against the symmetric restatement, as tests/test_gpu_amg.py holds them."""
    Ah = ac.cases()["grid37x53"]
    levels = ac.setup(Ah)
    A = _matrix(hp, gpu_backend_i32, Ah)
    M = hp.amg(A)
    assert M.symmetric is True and [l.n for l in M.levels] == [l["n"] for l in levels]
    for k, (lvl, ref) in enumerate(zip(M.levels, levels)):
        if "P" in ref:
            assert lvl.R is lvl.Pt and np.array_equal(lvl.aggregates.cpu().numpy(), ref["agg"]) and lvl.rounds == ref["rounds"]
            _same_matrix(_host(lvl.P), ref["P"], f"level {k} P")
            _same_matrix(_host(lvl.Pt), ref["Pt"], f"level {k} Pt")
            _same_matrix(_host(M.levels[k + 1].A), levels[k + 1]["A"], f"level {k} Ac")
    bg = ac.rhs(Ah.shape[0])
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    _, its_ref, status_ref, h_ref = ac.pcg_amg(Ah, bg, levels, rtol=1e-8)
    x, info = hp.cg(A, b, rtol=1e-8, M=M)
    head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:pc.HEAD], h_ref[:pc.HEAD]))
    assert info.converged and abs(info.iterations - its_ref) <= 2 and head <= pc.CG_RTOL
    hp.clear_plan_cache()


def test_gmres_with_ilu0_is_what_it_was(hp, gpu_backend_i32):
    rowptr, colidx, vals = ic.asymmetric_pattern()
    n = len(rowptr) - 1
    bg = ac.rhs(n)
    A = hp.HPCSparseMatrix_local(rowptr, colidx, vals, n, gpu_backend_i32)
    M = hp.ilu0(A)
    bp, bcols, f, lo = M.factors()
    K = ic.operator([(bp, bcols, f, lo)], 3)
    b = hp.HPCVector.from_global(bg, gpu_backend_i32)
    _, its_ref, status_ref, h_ref = ic.gmres_op(rowptr, colidx, vals, bg, K, rtol=1e-8)
    x, info = hp.gmres(A, b, rtol=1e-8, M=M)
    k = min(ic.HEAD_GMRES, len(h_ref), len(info.residual_norms))
    head = max(abs(g - w) / w for g, w in zip(info.residual_norms[:k], h_ref[:k]))
    assert status_ref == "converged" and info.converged and abs(info.iterations - its_ref) <= 2 and head <= ic.HIST_RTOL
    hp.clear_plan_cache()
