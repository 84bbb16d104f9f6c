"""GPU tests of ``hp.amg(A, B=...)``, the near-nullspace candidates of the tentative prolongator, against the restatement of
tests/_amg_candidates_cases.py (``cc``).

1. ``hpcla_amg_fit_f64`` alone on hand-made member lists: ``Tv``, the coarse candidates and the error word bit for bit.
2. ``hpcla_amg_prolongator_b_f64_*`` and ``hpcla_amg_restrictor_b_f64_*`` alone, all four index forms, bit for bit.
3. Hierarchies at coarse_size = 8: aggregates, partitions and patterns exactly, ``Tv`` and the coarse candidates bit for bit, P, R
   and ``A_c`` to 1e-13 of the largest entry (the margin of tests/test_gpu_amg.py), two builds equal in bits, ``M.apply`` within
   1e-12 ||r|| of the restated cycle.
4. Solves: the count within 2 of the restatement's, the true residual within ``pc.TRUE_RES_RTOL``, and the default hierarchy
   on the same matrix at least twice as slow.
5. Errors, each followed by a good call; ``B=None`` after a ``B=`` build.

Expected values of 1 and 2 are exact: the fit's arithmetic is part of the method (sequential sums in ascending member order,
separately rounded products and sums, a correctly rounded sqrt and division), the value kernels are one multiply and one
subtraction per entry.  No margin is taken from the device's results.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import _amg_cases as ac
from tests import _amg_candidates_cases as cc
from tests import _amg_nonsym_cases as nc
from tests import _pcg_cases as pc

pytestmark = pytest.mark.gpu

F64, I64, I32 = np.float64, np.int64, np.int32
FORMS = [("i32", I32, 0), ("i32", I32, 1), ("i64", I64, 0), ("i64", I64, 1)]
FORM_IDS = [f"{sfx}-base{base}" for sfx, _, base in FORMS]
VALUE_TOL = 1e-13
APPLY_TOL = 1e-12
GROUPS_PER_WORKGROUP = 32                                        # 256 threads, 8 lanes per aggregate


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
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
    tdt = {np.dtype(F64): torch.float64, np.dtype(I64): torch.int64, np.dtype(I32): torch.int32}[np.dtype(dtype)]
    return torch.full((max(int(n), 1),), value, dtype=tdt, device="cuda")


def _call(hp, name, *args):
    plain = [a.data_ptr() if hasattr(a, "data_ptr") else (int(a) if isinstance(a, (np.integer, np.bool_)) else a) for a in args]
    rc = getattr(hp._capi.load(), name)(*plain)
    assert rc == 0, (name, rc, hp._capi.last_error())


def _same_bits(got, want, what):
    got, want = ac.bits(np.asarray(got)), ac.bits(np.asarray(want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} words differ, first at {bad[:5].tolist()}"


def _matrix(hp, backend, A):
    return hp.HPCSparseMatrix_local(A.indptr, A.indices, A.data, A.shape[1], backend)


def _block(hp, backend, B):
    """The candidates as the interface takes them: an HPCVector for one column, an HPCMatrix otherwise."""
    B = np.asarray(B, dtype=np.float64)
    if B.shape[1] == 1:
        return hp.HPCVector.from_global(B[:, 0].copy(), backend)
    return hp.HPCMatrix.from_global(B, backend)


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


# ---- 1. the fit alone -------------------------------------------------------------------------------------------------------------
def _run_fit(hp, B, ptr, members, n, k):
    n_agg = len(ptr) - 1
    tv, bc, info = _full(n * k, 7.0, F64), _full(n_agg * k * k + 1, np.nan, F64), _full(2, 7, I64)
    _call(hp, "hpcla_amg_fit_f64", _dev(B, F64), n, k, _dev(ptr, I64), _dev(members, I64), len(members), n_agg, tv, bc, info, None)
    word, behind = info.cpu().numpy().tolist()
    assert behind == 7
    bc = bc.cpu().numpy()
    assert np.isnan(bc[n_agg * k * k]), "the word behind the coarse candidates"
    return tv.cpu().numpy()[:n * k].reshape(n, k), bc[:n_agg * k * k].reshape(n_agg * k, k), word


@pytest.mark.parametrize("k", [1, 2, 3, 6, 8])
def test_the_fit_alone(hp, k):
    """Aggregates of 1, k - 1, k, k + 1, 7, 8, 9, 64, 65 and 301 members; 37 aggregates (not a multiple of a workgroup's 32) without
    a report, 257 with aggregates of fewer than k members, a zero column, a NaN and a repeated column: the bits of the
    restatement, the smallest reporting aggregate in the error word, the rows outside every aggregate untouched, twice."""
    cycle = len(cc.fit_sizes(k))
    bad = [(cycle, "zero"), (2 * cycle + 1, "nan")] + ([(3 * cycle + 2, "repeat")] if k > 1 else [])
    for n_agg, kw in ((37, dict(short=False)), (257, dict(bad=bad)), (3, dict(bad=[(1, "nan")], short=False))):
        assert n_agg % GROUPS_PER_WORKGROUP
        B, ptr, members, n = cc.fit_case(k, n_agg, seed=100 * k + n_agg, **kw)
        Tv, Bc, reports = cc.fit(B, ptr, members)
        outside = np.setdiff1d(np.arange(n), members)
        assert len(outside) == 5
        Tv[outside] = 7.0
        word = cc.fit_word(reports)
        sizes = np.diff(ptr)
        if "bad" in kw:
            for a, kind in kw["bad"]:
                assert sizes[a] >= k and (a, 0 if kind == "zero" else k - 1) in reports, (a, kind)
            assert ("short" in kw) or k == 1 or any(sizes[a] < k for a, _ in reports)
            assert word == min(8 * a + j for a, j in reports) >= 0
            for a, j in reports:                                 # a dropped column of Q and its row of R: +0.0
                rows = members[ptr[a]:ptr[a + 1]]
                assert not ac.bits(Tv[rows, j]).any() and not ac.bits(Bc[k * a + j]).any()
        else:
            assert word == -1 and sizes.min() >= k and set(cc.fit_sizes(k)) - set(sizes.tolist()) <= set(range(k))
        first = None
        for _ in range(2):
            got_tv, got_bc, got_word = _run_fit(hp, B, ptr, members, n, k)
            print(f"k = {k}, {n_agg} aggregates of {sizes.min()} to {sizes.max()} members: word {got_word} (restated {word})")
            assert got_word == word, (k, n_agg)
            _same_bits(got_tv, Tv, (k, n_agg, "Tv"))
            _same_bits(got_bc, Bc, (k, n_agg, "Bc"))
            first = first or (got_tv, got_bc)
            _same_bits(got_tv, first[0], "a second call")
            _same_bits(got_bc, first[1], "a second call")
    assert set(cc.fit_sizes(k)) >= {1, k, k + 1, 7, 8, 9, 64, 65, 301}


def test_the_fit_with_no_aggregates_and_with_an_empty_one(hp):
    info = _full(1, 7, I64)
    _call(hp, "hpcla_amg_fit_f64", None, 0, 3, None, None, 0, 0, None, None, info, None)
    assert info.cpu().numpy().tolist() == [-1]
    B = np.random.default_rng(4).standard_normal((4, 3))          # aggregates {0, 1, 2, 3} and {}: the empty one drops column 0
    Tv, Bc, word = _run_fit(hp, B, np.array([0, 4, 4]), np.arange(4), 4, 3)
    want_tv, want_bc, reports = cc.fit(B, np.array([0, 4, 4]), np.arange(4))
    assert word == cc.fit_word(reports) == 8 and reports == [(1, 0), (1, 1), (1, 2)]
    _same_bits(Tv, want_tv, "Tv")
    _same_bits(Bc, want_bc, "Bc")


# ---- 2. the two value entries alone -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_levels():
    """k -> the first level of a restated hierarchy with k candidates: elasticity (3) and the scaled grid (1)."""
    E, modes = cc.elasticity(16, 16)
    S, d = cc.scaled(33, 31)
    return {3: cc.setup(E, modes, coarse_size=cc.SMALL)[0], 1: cc.setup(S, 1.0 / d, coarse_size=cc.SMALL)[0]}


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("sfx,Ti,base", FORMS, ids=FORM_IDS)
def test_the_value_entries_alone(hp, first_levels, sfx, Ti, base, k):
    """P's values on the pattern of A T and R's on that of Tt A, through a shuffled column space, with aggregate ids that start
    at 1000: the bits of numpy's separately rounded expressions.  Most columns of a row belong to other aggregates."""
    lvl = first_levels[k]
    A, agg, Tv, s, n = lvl["A"], lvl["agg"], lvl["Tv"], lvl["s"], lvl["n"]
    n_agg = int(lvl["counts"].sum())
    shift = 1000
    AT = ac.structural_product(A, lvl["T"])
    own = AT.indices // k == agg[np.repeat(np.arange(n), np.diff(AT.indptr))]
    assert 0.05 < own.mean() < 0.9
    want = cc.prolongator_values(AT, agg, Tv, s)
    _same_bits(want, lvl["P"].data, "the restatement's own P")
    colval, col_indices = ac.compressed_columns(AT.indices + k * shift, np.random.default_rng(5))
    p = _full(AT.nnz + 1, np.nan, F64)
    _call(hp, f"hpcla_amg_prolongator_b_f64_{sfx}", _dev(AT.indptr + base, Ti), _dev(colval + base, Ti), _dev(col_indices, I64),
          _dev(AT.data, F64), _dev(agg + shift, I64), _dev(s, F64), _dev(Tv, F64), k, n, base, p, None)
    got = p.cpu().numpy()
    _same_bits(got[:AT.nnz], want, (sfx, base, k, "p"))
    assert np.isnan(got[AT.nnz])

    Tt = lvl["T"].T.tocsr()
    Tt.sort_indices()
    TA = ac.structural_product(Tt, A)
    assert TA.shape == (k * n_agg, n)
    want = cc.restrictor_values(TA, agg, Tv, s)
    colval, col_indices = ac.compressed_columns(TA.indices, np.random.default_rng(6))
    r = _full(TA.nnz + 1, np.nan, F64)
    _call(hp, f"hpcla_amg_restrictor_b_f64_{sfx}", _dev(TA.indptr + base, Ti), _dev(colval + base, Ti), _dev(col_indices, I64),
          _dev(TA.data, F64), _dev(agg + shift, I64), _dev(s, F64), _dev(Tv, F64), k, k * n_agg, n, k * shift, base, r, None)
    got = r.cpu().numpy()
    _same_bits(got[:TA.nnz], want, (sfx, base, k, "r"))
    assert np.isnan(got[TA.nnz])


# ---- 3. hierarchies ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return cc.hierarchy_cases()


@pytest.fixture(scope="module")
def refs(cases):
    return {name: cc.setup(A, B, coarse_size=cc.SMALL, symmetric=sym) for name, (A, B, sym) in cases.items()}


def _check_hierarchy(M, levels, k, sym, name):
    assert M.candidates_per_aggregate == k and M.symmetric is sym and [l.n for l in M.levels] == [l["n"] for l in levels], name
    worst = 0.0
    for depth, (lvl, ref) in enumerate(zip(M.levels, levels)):
        what = f"{name} level {depth}"
        assert abs(lvl.rho - ref["rho"]) <= 1e-13 * ref["rho"] and abs(lvl.w - ref["w"]) <= 1e-13 * ref["w"], what
        assert np.all(np.abs(lvl.s.local_values() - ref["s"]) <= 1e-13 * np.abs(ref["s"]).max()), what
        assert tuple(lvl.candidates.shape) == (ref["n"], k) and lvl.candidates.is_contiguous(), what
        _same_bits(lvl.candidates.cpu().numpy(), ref["B"], what + " candidates")
        if "agg" in ref:
            n_agg = int(ref["counts"].sum())
            assert np.array_equal(lvl.aggregates.cpu().numpy(), ref["agg"]), what
            assert lvl.n_roots == n_agg and lvl.rounds == ref["rounds"], what
            assert np.array_equal(lvl.coarse_partition, [0, k * n_agg]), what
        if "P" in ref:
            _same_bits(lvl.Tv.cpu().numpy(), ref["Tv"], what + " Tv")
            T = _host(lvl.T)
            assert np.array_equal(T.indptr, ref["T"].indptr) and np.array_equal(T.indices, ref["T"].indices), what
            _same_bits(T.data, ref["T"].data, what + " T")      # exact zeros stay stored
            worst = max(worst, _same_matrix(_host(lvl.P), ref["P"], what + " P"))
            worst = max(worst, _same_matrix(_host(lvl.R), ref["R"], what + " R"))
            assert (lvl.Pt is lvl.R) if sym else (lvl.Pt is None), what
            worst = max(worst, _same_matrix(_host(M.levels[depth + 1].A), levels[depth + 1]["A"], what + " Ac"))
        else:
            assert lvl.P is None and lvl.T is None and depth == len(levels) - 1, what
            assert (lvl.inverse is not None) == ("inv" in ref) and (lvl.sweeps == ref.get("sweeps")), what
    assert abs(M.operator_complexity - ac.operator_complexity(levels)) <= 1e-12, name
    return worst


HIERARCHIES = [(name, "i32") for name in cc.hierarchy_cases()] + [("elas16x16", "i64wide"), ("cdscaled33x31", "i64wide"),
                                                                  ("scaled16x16", "i64")]


@pytest.mark.parametrize("name,which", HIERARCHIES)
def test_levels_match_the_restatement(hp, cases, refs, gpu_backend_i32, gpu_backend_i64, name, which, monkeypatch):
    monkeypatch.setenv("HPCLA_NARROW_INDICES", "0" if which == "i64wide" else "1")
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    Ah, B, sym = cases[name]
    M = hp.amg(_matrix(hp, backend, Ah), coarse_size=cc.SMALL, symmetric=sym, B=_block(hp, backend, B))
    worst = _check_hierarchy(M, refs[name], B.shape[1], sym, name)
    print(f"{which} {name}: levels {[l.n for l in M.levels]}, k = {B.shape[1]}, operator complexity {M.operator_complexity:.3f}, "
          f"largest deviation of an entry {worst:.2e}")
    hp.clear_plan_cache()


@pytest.mark.parametrize("name", list(cc.hierarchy_cases()))
def test_apply_matches_the_cycle_and_two_builds_agree(hp, cases, refs, gpu_backend_i32, name):
    torch = _torch()
    Ah, B, sym = cases[name]
    backend = gpu_backend_i32
    M = hp.amg(_matrix(hp, backend, Ah), coarse_size=cc.SMALL, symmetric=sym, B=_block(hp, backend, B))
    rg = ac.rhs(Ah.shape[0], seed=11)
    r = hp.HPCVector.from_global(rg, backend)
    z = M.apply(r)
    want = ac.cycle(refs[name], rg)
    dev = float(np.linalg.norm(z.local_values() - want)) / float(np.linalg.norm(rg))
    print(f"{name}: ||M r - cycle(r)|| / ||r|| = {dev:.2e}")
    assert dev <= APPLY_TOL, (name, dev)
    if B.shape[1] > 1:                                           # a block that is not row-major is packed, to the same bits
        t = torch.from_numpy(np.asfortranarray(B)).to(backend.torch_device)
        assert not t.is_contiguous()
        second = hp.HPCMatrix(np.array([0, B.shape[0]]), np.array([0, B.shape[1]]), t, backend)
    else:
        second = _block(hp, backend, B)
    M2 = hp.amg(_matrix(hp, backend, Ah), coarse_size=cc.SMALL, symmetric=sym, B=second)
    assert len(M2.levels) == len(M.levels)
    for a, b in zip(M.levels, M2.levels):
        _same_bits(a.A.nzval.cpu().numpy(), b.A.nzval.cpu().numpy(), name)
        _same_bits(a.candidates.cpu().numpy(), b.candidates.cpu().numpy(), name)
        if a.P is not None:
            _same_bits(a.Tv.cpu().numpy(), b.Tv.cpu().numpy(), name)
            _same_bits(a.P.nzval.cpu().numpy(), b.P.nzval.cpu().numpy(), name)
            _same_bits(a.R.nzval.cpu().numpy(), b.R.nzval.cpu().numpy(), name)
        if a.inverse is not None:
            _same_bits(a.inverse.local_values(), b.inverse.local_values(), name)
    _same_bits(M2.apply(r).local_values(), z.local_values(), name)
    hp.clear_plan_cache()


# ---- 4. solves --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved():
    """name -> (A, B, symmetric, b, the restated count with B, the restated count of the default hierarchy)."""
    out = {}
    for name, (A, B, sym) in cc.solve_cases().items():
        b = ac.rhs(A.shape[0])
        _, its, ok = cc.solve(cc.SOLVES[name], A, b, cc.setup(A, B, symmetric=sym), rtol=1e-8)
        _, base, ok_base = cc.solve(cc.SOLVES[name], A, b, cc.default_setup(A, sym), rtol=1e-8)
        assert ok and ok_base
        out[name] = (A, B, sym, b, its, base)
    return out


@pytest.mark.parametrize("name", sorted(cc.SOLVES))
def test_solves_with_candidates(hp, solved, gpu_backend_i32, name):
    backend = gpu_backend_i32
    Ah, B, sym, bg, its_ref, base_ref = solved[name]
    A = _matrix(hp, backend, Ah)
    b = hp.HPCVector.from_global(bg, backend)
    solver = hp.cg if cc.SOLVES[name] == "cg" else hp.gmres
    M = hp.amg(A, symmetric=sym, B=_block(hp, backend, B))
    x, info = solver(A, b, rtol=1e-8, M=M)
    true = hp.norm(b - A @ x) / hp.norm(b)
    _, plain = solver(A, b, rtol=1e-8, M=hp.amg(A, symmetric=sym))
    print(f"{name}: iterations {info.iterations} (restatement {its_ref}), true residual {true:.3e}; the default hierarchy takes "
          f"{plain.iterations} (restatement {base_ref}); operator complexity {M.operator_complexity:.3f}")
    assert info.converged and abs(info.iterations - its_ref) <= 2, (name, info.iterations, its_ref)
    assert true <= pc.TRUE_RES_RTOL
    assert plain.converged and plain.iterations >= 2 * info.iterations, (name, plain.iterations, info.iterations)
    hp.clear_plan_cache()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_a_good_call_afterwards(hp, cases, refs, gpu_backend_i32):
    backend = gpu_backend_i32
    Ah, B, _ = cases["scaled16x16"]
    n = Ah.shape[0]
    A = _matrix(hp, backend, Ah)

    def good_call_passes():
        _check_hierarchy(hp.amg(_matrix(hp, backend, Ah), coarse_size=cc.SMALL, B=_block(hp, backend, B)), refs["scaled16x16"], 1,
                         True, "good call")

    rng = np.random.default_rng(9)
    with pytest.raises(ValueError, match="amg: B must have 1..8 columns, got 9"):
        hp.amg(A, B=hp.HPCMatrix.from_global(rng.standard_normal((n, 9)), backend))
    good_call_passes()
    b32 = hp.backend_rocm_serial(np.float32, np.int32)
    with pytest.raises(TypeError):
        hp.amg(hp.HPCSparseMatrix_local(Ah.indptr, Ah.indices, Ah.data.astype(np.float32), n, b32),
               B=hp.HPCVector.from_global(B[:, 0].astype(np.float32), b32))
    with pytest.raises(TypeError, match="amg: the candidates B must be Float64"):
        hp.amg(A, B=hp.HPCVector.from_global(B[:, 0].astype(np.float32), b32))
    with pytest.raises(TypeError, match="amg: B must be an HPCVector or an HPCMatrix"):
        hp.amg(A, B=B)
    good_call_passes()
    with pytest.raises(ValueError, match=f"amg: B has {n + 1} rows, A has {n}"):
        hp.amg(A, B=hp.HPCVector.from_global(np.ones(n + 1), backend))
    good_call_passes()
    two = np.stack([B[:, 0], B[:, 0]], axis=1)
    zero = np.stack([B[:, 0], np.zeros(n)], axis=1)
    nan = B.copy()
    nan[100, 0] = np.nan
    for block, column in ((two, 1), (zero, 1), (nan, 0)):
        with pytest.raises(ValueError) as first:
            cc.setup(Ah, block, coarse_size=cc.SMALL)
        row = int(str(first.value).split("row ")[1].split(" ")[0])
        assert f"candidate column {column}" in str(first.value)
        for _ in range(2):                                       # the same error, call after call
            with pytest.raises(ValueError, match=rf"amg: the aggregate of row {row} \(level of {n} rows\) has \d+ members and "
                                                 rf"cannot carry candidate column {column} of B's {block.shape[1]}"):
                hp.amg(A, coarse_size=cc.SMALL, B=_block(hp, backend, block))
        good_call_passes()
    P = ac.path(257)                                             # 72 aggregates: a stall at k = 3, and the last has 2 members
    with pytest.raises(ValueError, match=r"amg: the aggregate of row 255 \(level of 257 rows\) has 2 members and cannot carry "
                                         r"candidate column 2 of B's 3"):
        hp.amg(_matrix(hp, backend, P), coarse_size=cc.SMALL, B=hp.HPCMatrix.from_global(cc.path_candidates(257), backend))
    good_call_passes()
    hp.clear_plan_cache()


def test_no_candidates_after_a_build_with_candidates(hp, cases, gpu_backend_i32):
    """``B=None`` after a ``B=`` build: the bits of a ``B=None`` build made before it, level by level."""
    backend = gpu_backend_i32
    Ah, B, _ = cases["elas16x16"]
    A = _matrix(hp, backend, Ah)
    before = hp.amg(A, coarse_size=cc.SMALL)
    hp.amg(A, coarse_size=cc.SMALL, B=_block(hp, backend, B))
    after = hp.amg(A, coarse_size=cc.SMALL, B=None)
    assert after.candidates_per_aggregate is None and [l.n for l in after.levels] == [l.n for l in before.levels]
    for a, b in zip(before.levels, after.levels):
        assert b.candidates is None and b.Tv is None and b.T is None
        _same_bits(a.A.nzval.cpu().numpy(), b.A.nzval.cpu().numpy(), "A")
        _same_bits(a.s.local_values(), b.s.local_values(), "s")
        if a.P is not None:
            assert np.array_equal(a.aggregates.cpu().numpy(), b.aggregates.cpu().numpy())
            _same_bits(a.P.nzval.cpu().numpy(), b.P.nzval.cpu().numpy(), "P")
        if a.inverse is not None:
            _same_bits(a.inverse.local_values(), b.inverse.local_values(), "inverse")
    hp.clear_plan_cache()
