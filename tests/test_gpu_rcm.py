"""hp.rcm and hp.bandwidth on the device (csrc/rcm.hip, linearalgebrampi.jl_amd/rcm.py) against the numpy restatement of
tests/_rcm_cases.py -- which tests/test_rcm_cases.py holds against the sequential queue algorithm and scipy -- on one rank, and
through tests/_multirank_rcm_worker.py on 2 and 3 ranks sharing the GPU.

The result is a list of integers: every comparison is array_equal, no tolerance appears except in the end-to-end products,
where the permutation changes the order of a row's sum.  The cap-edge cases assert through ``narrow_launches`` /
``wide_levels`` that the one-workgroup kernel and the device-wide path each ran where the replay in the restatement says."""
import os

import numpy as np
import pytest

from tests import _rcm_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_rcm_worker.py")

pytestmark = pytest.mark.gpu

_cache = {}
FACTS = ("components", "levels", "bandwidth_before", "bandwidth_after", "narrow_launches", "wide_levels")


def _backend(hp, Ti, T=np.float64):
    key = (np.dtype(Ti).name, np.dtype(T).name)
    if key not in _cache:
        _cache[key] = hp.backend_rocm_serial(T, Ti)
    return _cache[key]


def _matrix(hp, name, Ti, T=np.float64):
    C = rc.matrix(name)
    return hp.HPCSparseMatrix_local(C.indptr, C.indices, C.data.astype(T), C.shape[1], _backend(hp, Ti, T))


def _snapshot(A):
    return A.nzval.clone(), A.rowptr_target.clone(), A.colval_target().clone()


def _assert_result(p, info, name, symmetric, paths=True):
    import torch
    want, facts, _ = rc.expected(name, symmetric)
    assert p.dtype == torch.int64 and p.is_cuda and p.dim() == 1
    got = p.cpu().numpy()
    assert rc.is_permutation(got, len(want)), name
    assert np.array_equal(got, want), (name, int(np.flatnonzero(got != want)[0]))
    for f in FACTS[:4] + (FACTS[4:] if paths else ()):
        assert getattr(info, f) == facts[f], (name, f, getattr(info, f), facts[f])


def test_the_library_has_the_caps_the_cases_assume(hp):
    lib = hp._capi.load()
    assert lib.hpcla_rcm_frontier_cap() == rc.FRONTIER_CAP and lib.hpcla_rcm_candidate_cap() == rc.CANDIDATE_CAP


@pytest.mark.parametrize("Ti", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("name", rc.SYMMETRIC_CASES)
def test_rcm_matches_the_restatement(hp, name, Ti):
    import torch
    A = _matrix(hp, name, Ti)
    snap = _snapshot(A)
    p, info = hp.rcm(A)
    assert isinstance(info, hp.RCMInfo)
    _assert_result(p, info, name, True)
    assert hp.bandwidth(A) == rc.bandwidth_of_matrix(rc.matrix(name))
    p2, info2 = hp.rcm(A)                                                 # the same tensors twice
    assert torch.equal(p, p2) and info2 == info
    assert A.structural_hash is None                                       # never hashed
    assert all(torch.equal(a, b) for a, b in zip(_snapshot(A), snap)), name + ": the input changed"


def test_path_choice_at_the_caps(hp):
    """Either side of each cap, the path that ran (the restatement's results were asserted above; here: which kernel)."""
    got = {}
    for name in ("star_cap", "star_cap_plus1", "tree_frontier_cap", "tree_frontier_cap_plus1", "degree_sum_cap",
                 "degree_sum_cap_plus1", "path300", "pairs500", "random20000", "star_chunk_wrap", "path1024_k6", "path1025_k6",
                 "path3000_k6", "tree_then_narrow"):
        p, info = hp.rcm(_matrix(hp, name, np.int32))
        assert np.array_equal(p.cpu().numpy(), rc.expected(name)[0]), name
        got[name] = (info.narrow_launches, info.wide_levels)
    assert got["star_cap"] == (2, 1) and got["star_cap_plus1"] == (2, 2)
    assert got["tree_frontier_cap"] == (1, 0) and got["tree_frontier_cap_plus1"] == (2, 1)
    assert got["degree_sum_cap"] == (1, 0) and got["degree_sum_cap_plus1"] == (2, 2)
    assert got["path300"] == (1, 0) and got["pairs500"] == (1, 0)
    assert got["random20000"][1] > 1
    assert got["star_chunk_wrap"] == (2, 2)                                 # the centre's row: one chunk more than the expand's grid.y
    assert got["path1024_k6"] == got["path1025_k6"] == got["path3000_k6"] == (1, 0)
    assert got["tree_then_narrow"] == (2, 1)                                # the second launch resumes on the wide level's 10 vertices


def test_float32_values_are_never_read(hp):
    import torch
    A = _matrix(hp, "delaunay2000", np.int32, np.float32)
    assert A.nzval.dtype == torch.float32
    A.nzval.fill_(float("nan"))                                             # only the structure counts
    p, info = hp.rcm(A)
    _assert_result(p, info, "delaunay2000", True)
    assert hp.bandwidth(A) == rc.bandwidth_of_matrix(rc.matrix("delaunay2000"))


@pytest.mark.parametrize("Ti", [np.int32, np.int64], ids=["i32", "i64"])
def test_nonsymmetric_pattern(hp, Ti):
    A = _matrix(hp, "nonsymmetric", Ti)
    p, info = hp.rcm(A, symmetric=False)                                    # E u E^T
    _assert_result(p, info, "nonsymmetric", False, paths=False)
    assert info.narrow_launches == 1 and info.wide_levels == 0
    p, info = hp.rcm(A, symmetric=True)                                     # the promise broken: the directed walk
    _assert_result(p, info, "nonsymmetric", True)
    # doubled lists longer than a lane group, device-wide levels that meet repeated neighbours: the numbering of the set
    # union, the paths of the walk on the lists as the device holds them
    W = _matrix(hp, "nonsymmetric_wide", Ti)
    p, info = hp.rcm(W, symmetric=False)
    _assert_result(p, info, "nonsymmetric_wide", False, paths=False)
    paths = rc.trace_facts(rc.traced("nonsymmetric_wide", doubled=True)[0], W.shape[0])
    assert (info.narrow_launches, info.wide_levels) == (paths["narrow_launches"], paths["wide_levels"]) and info.wide_levels > 1
    p, info = hp.rcm(W, symmetric=True)
    _assert_result(p, info, "nonsymmetric_wide", True)
    # on a symmetric pattern the two agree
    B = _matrix(hp, "delaunay2000", Ti)
    p, info = hp.rcm(B, symmetric=False)
    _assert_result(p, info, "delaunay2000", True)


def test_end_to_end_on_a_shuffled_grid(hp):
    """The reordering brings back the 16-bit columns, the permuted product is the product permuted, and CG on the permuted
    system solves the original one."""
    name = "grid256x256"
    C = rc.matrix(name)
    n = C.shape[0]
    b = _backend(hp, np.int32)
    A = _matrix(hp, name, np.int32)
    rng = np.random.default_rng(256)
    xg = rng.standard_normal(n)
    x = hp.HPCVector.from_global(xg, b)
    p, info = hp.rcm(A)
    _assert_result(p, info, name, True)
    assert hp.get_vector_plan(A, x).cols16 is None
    B = hp.select(A, p, p)
    xp = hp.take(x, p)
    assert hp.get_vector_plan(B, xp).cols16 is not None
    assert hp.bandwidth(B) == info.bandwidth_after == 256
    lhs, rhs = (B @ xp).local_values(), hp.take(A @ x, p).local_values()
    bound = 1e-13 * abs(C).sum(axis=1).max() * np.abs(xg).max()
    err = np.abs(lhs - rhs).max()
    print(f"permuted product: max abs difference {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    rtol = 1e-8
    fg = rng.standard_normal(n)
    f = hp.HPCVector.from_global(fg, b)
    up, cg_info = hp.cg(B, hp.take(f, p), rtol=rtol, maxiter=5000)
    assert cg_info.converged
    u = hp.HPCVector.from_global(np.full(n, np.nan), b)
    hp.put_(u, p, up)
    res = np.linalg.norm(C @ u.local_values() - fg) / np.linalg.norm(fg)
    print(f"cg on the permuted system: {cg_info.iterations} iterations, true relative residual of the original system {res:.3e}")
    assert res <= rtol


def test_argument_errors(hp):
    b = _backend(hp, np.int32)
    C = rc.matrix("grid33x31")
    R = C[:, :1000]
    A = hp.HPCSparseMatrix_local(R.indptr, R.indices, R.data, 1000, b)
    with pytest.raises(ValueError, match="rcm: the matrix must be square, got 1023 x 1000"):
        hp.rcm(A)
    S = hp.HPCSparseMatrix_local(C.indptr, C.indices, C.data, C.shape[1], b)
    with pytest.raises(TypeError, match="rcm: an HPCSparseMatrix is required"):
        hp.rcm(C)
    with pytest.raises(TypeError, match="bandwidth: an HPCSparseMatrix is required"):
        hp.bandwidth(C)
    # unequal partitions need two ranks to exist: tests/_multirank_rcm_worker.py raises them on every rank; here the rule
    # itself, on a matrix whose column partition is replaced by hand
    S.col_partition = np.array([0, 1, C.shape[1]], dtype=np.int64)
    with pytest.raises(ValueError, match="rcm: A's rows and columns must be partitioned alike"):
        hp.rcm(S)


def test_an_empty_and_a_diagonal_matrix(hp):
    b = _backend(hp, np.int32)
    n = 37
    D = hp.HPCSparseMatrix_local(np.arange(n + 1), np.arange(n), np.ones(n), n, b)
    p, info = hp.rcm(D)
    assert np.array_equal(p.cpu().numpy(), np.arange(n)[::-1])              # no neighbours: index order, reversed
    assert (info.components, info.levels, info.bandwidth_before, info.bandwidth_after) == (n, 0, 0, 0)
    assert hp.bandwidth(D) == 0


@pytest.mark.parametrize("nranks", [2, 3])
def test_rcm_across_ranks(nranks):
    """Ranks share the GPU; every rank's p against the restatement on its owned block, the permuted matrix gathered against
    scipy, the errors on every rank."""
    from hpcla_amd.launch import spawn_ranks
    assert spawn_ranks([WORKER], nranks, env_extra={"HPCLA_PUSH_TIMEOUT_S": "30"}, timeout=300, forward_rank0_stdout=False) == 0
