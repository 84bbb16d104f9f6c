"""The numpy restatement of hp.rcm (tests/_rcm_cases.py) against itself and against scipy, and the argument rules that need no
device: the level form the kernels run equals the sequential queue algorithm element for element on every case, both are
permutations, ``symmetric=False`` is the restatement on E u E^T, and the bandwidth stays within 5 % of scipy's
``reverse_cuthill_mckee`` (scipy leaves its tie order unspecified: the margin covers that and nothing else)."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import reverse_cuthill_mckee

from tests import _rcm_cases as rc


@pytest.mark.parametrize("name", rc.CASES)
def test_the_level_form_equals_the_queue_algorithm(name):
    A = rc.matrix(name)
    n = A.shape[0]
    for symmetric in (True, False):
        p, facts, g = rc.expected(name, symmetric)
        assert rc.is_permutation(p, n), (name, symmetric)
        q = rc.rcm_sequential(*g)
        assert rc.is_permutation(q, n) and np.array_equal(p, q), (name, symmetric)
        assert facts["bandwidth_after"] == rc.bandwidth_of_graph(*g, q)


def test_the_cases_are_what_their_names_say():
    assert rc.matrix("path1").shape == (1, 1) and rc.matrix("path1").nnz == 1
    assert rc.expected("components9")[1]["components"] == 9
    assert rc.expected("pairs500")[1]["components"] == 500 and rc.expected("pairs500")[1]["levels"] == 1000
    assert rc.expected("path300")[1]["levels"] == 300 and rc.expected("path300")[1]["bandwidth_after"] == 1
    for name, degree in (("star_cap", rc.CANDIDATE_CAP), ("star_cap_plus1", rc.CANDIDATE_CAP + 1)):
        assert int(np.diff(rc.expected(name)[2][0]).max()) == degree
    # which path walks what: the caps' edges, from the replay of the two paths in the level form
    paths = {name: (rc.expected(name)[1]["narrow_launches"], rc.expected(name)[1]["wide_levels"]) for name in rc.SYMMETRIC_CASES}
    assert paths["star_cap"] == (2, 1)                       # the centre's level is narrow; its 8191 new leaves are a wide frontier
    assert paths["star_cap_plus1"] == (2, 2)                 # the centre's level itself is wide
    assert paths["tree_frontier_cap"] == (1, 0) and paths["tree_frontier_cap_plus1"] == (2, 1)
    assert paths["degree_sum_cap"] == (1, 0) and paths["degree_sum_cap_plus1"] == (2, 2)      # 129 new vertices at a mean degree of 84: kept wide
    assert paths["path300"] == (1, 0) and paths["pairs500"] == (1, 0)
    assert paths["random20000"][1] > 1
    # the level that decides: its size and degree sum sit exactly on the caps
    for name, size, total in (("tree_frontier_cap", rc.FRONTIER_CAP, None), ("tree_frontier_cap_plus1", rc.FRONTIER_CAP + 1, None),
                              ("degree_sum_cap", 64, rc.CANDIDATE_CAP), ("degree_sum_cap_plus1", 64, rc.CANDIDATE_CAP + 2)):
        p, _, (indptr, indices) = rc.expected(name)
        order = p[::-1]
        level = order[2:2 + 64] if size == 64 else order[2 + 64:]
        assert len(level) == size, name
        if total is not None:
            assert int(np.diff(indptr)[level].sum()) == total, name


def test_the_nonsymmetric_case_is_not_symmetric_and_its_union_is():
    A = rc.matrix("nonsymmetric")
    P = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    assert (P != P.T).nnz > 0
    indptr, indices = rc.block_graph(A, symmetric=False)
    U = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=A.shape)
    assert (U != U.T).nnz == 0
    Q = sp.csr_matrix(P + P.T)
    Q.setdiag(0)
    Q.eliminate_zeros()
    assert U.nnz == Q.nnz
    directed, union = rc.expected("nonsymmetric", True)[0], rc.expected("nonsymmetric", False)[0]
    assert not np.array_equal(directed, union)


@pytest.mark.parametrize("name", rc.SCIPY_CASES)
def test_bandwidth_within_five_percent_of_scipy(name):
    A = rc.matrix(name)
    p = rc.expected(name)[0]
    ps = reverse_cuthill_mckee(sp.csr_matrix(A), symmetric_mode=True)
    ours, theirs = rc.bandwidth_of_matrix(A[p][:, p]), rc.bandwidth_of_matrix(A[ps][:, ps])
    print(f"{name}: bandwidth {ours} (restatement) / {theirs} (scipy)")
    assert ours == rc.expected(name)[1]["bandwidth_after"]
    assert ours <= 1.05 * theirs, (name, ours, theirs)


def test_blocks_of_a_partition_are_walked_alone():
    """What a rank sees: its own rows and columns, other ranks' columns dropped."""
    A = rc.matrix("grid33x31")
    n = A.shape[0]
    for lo, hi in ((0, 400), (400, 401), (401, n)):
        p, facts, g = rc.expected("grid33x31", True, lo, hi)
        assert rc.is_permutation(p, hi - lo) and np.array_equal(p, rc.rcm_sequential(*g))
        assert len(g[0]) == hi - lo + 1 and (len(g[1]) == 0 or g[1].max() < hi - lo)


def test_argument_rules():
    from hpcla_amd.rcm import RCMInfo, check_arguments
    check_arguments((10, 10), [0, 4, 10], [0, 4, 10])
    with pytest.raises(ValueError, match="rcm: the matrix must be square, got 10 x 12"):
        check_arguments((10, 12), [0, 4, 10], [0, 6, 12])
    with pytest.raises(ValueError, match="rcm: A's rows and columns must be partitioned alike"):
        check_arguments((10, 10), [0, 4, 10], [0, 5, 10])
    with pytest.raises(ValueError, match=r"rcm: rank 1 holds 2147483647 rows; at most 2\^31 - 2 per rank"):
        check_arguments((2 ** 31 + 2, 2 ** 31 + 2), [0, 3, 2 ** 31 + 2], [0, 3, 2 ** 31 + 2])
    check_arguments((2 ** 31, 2 ** 31), [0, 2, 2 ** 31], [0, 2, 2 ** 31])                 # 2^31 - 2 rows on a rank: accepted
    info = RCMInfo()
    assert (info.components, info.levels, info.bandwidth_before, info.bandwidth_after, info.narrow_launches, info.wide_levels) == (0,) * 6
