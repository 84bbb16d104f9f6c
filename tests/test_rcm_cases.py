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


# ---- the kernels one by one (the restatements tests/test_gpu_rcm_kernels.py holds the C entries against) ------------------------------
def _cuts(n, k):
    return [(n * j) // k for j in range(k + 1)]


@pytest.mark.parametrize("name", ["grid33x31", "delaunay2000", "nonsymmetric"])
def test_graph_of_block_equals_block_graph(name):
    """On sorted, duplicate-free blocks the two kernels' graph is ``block_graph``; a shuffled stored order permutes each row and
    nothing else; both bases and index types give the same graph."""
    A = rc.matrix(name)
    n = A.shape[0]
    for k in (1, 3, 8):
        cuts = _cuts(n, k)
        for j in range(k):
            lo, hi = cuts[j], cuts[j + 1]
            want = rc.block_graph(A, lo, hi)
            for base, Ti in ((0, np.int32), (1, np.int64)):
                rowptr, colval, ci = rc.split_block(A, lo, hi, base, Ti)
                assert rowptr.dtype == Ti and colval.dtype == Ti and ci.dtype == np.int64 and rowptr[0] == base
                assert np.array_equal(ci[colval - base] - base, A[lo:hi].indices) and np.all(np.diff(ci) > 0)
                g_rowptr, g_cols = rc.graph_of_block(rowptr, colval, ci, hi - lo, lo, base)
                assert np.array_equal(g_rowptr, want[0]) and np.array_equal(g_cols, want[1]), (name, k, j, base)
                if k > 1:
                    assert len(ci) > 0 and (ci[0] - base < lo or ci[-1] - base >= hi), "a block of a cut has ghost columns"
                s_rowptr, s_colval, s_ci = rc.split_block(A, lo, hi, base, Ti, shuffle_seed=j)
                assert np.array_equal(s_rowptr, rowptr) and np.array_equal(s_ci, ci)
                h_rowptr, h_cols = rc.graph_of_block(s_rowptr, s_colval, s_ci, hi - lo, lo, base)
                assert np.array_equal(h_rowptr, want[0])
                rows = np.repeat(np.arange(hi - lo), np.diff(h_rowptr))
                assert np.array_equal(h_cols[np.lexsort((h_cols, rows))], want[1])
                if len(h_cols) > 50:
                    assert not np.array_equal(h_cols, want[1]), "the shuffle changed nothing"
    # a repeated column stays as often as it is stored, in stored order; no rows: one word
    g_rowptr, g_cols = rc.graph_of_block([0, 4, 5], [2, 0, 2, 1, 1], [10, 11, 12], 2, 11, 0)
    assert g_rowptr.tolist() == [0, 2, 3] and g_cols.tolist() == [1, 1, 0]
    assert rc.graph_of_block([1], [], [], 0, 5, 1)[0].tolist() == [0]


def test_the_doubled_graph_and_its_degrees():
    for name in rc.NONSYMMETRIC_CASES:
        indptr, indices = rc.block_graph(rc.matrix(name))
        d_ptr, d_cols = rc.doubled_graph(indptr, indices)
        u_ptr, u_cols = rc.block_graph(rc.matrix(name), symmetric=False)
        n = len(indptr) - 1
        assert d_ptr[-1] == 2 * len(indices)
        for i in (0, 1, n // 2, n - 1):
            assert np.array_equal(d_cols[d_ptr[i]:d_ptr[i] + indptr[i + 1] - indptr[i]], indices[indptr[i]:indptr[i + 1]])
            assert np.array_equal(np.unique(d_cols[d_ptr[i]:d_ptr[i + 1]]), u_cols[u_ptr[i]:u_ptr[i + 1]])
        assert np.array_equal(rc.degrees_of(d_ptr, d_cols, True), np.diff(u_ptr))
        assert np.array_equal(rc.degrees_of(d_ptr, d_cols, False), np.diff(d_ptr))
        assert np.array_equal(rc.degrees_of(u_ptr, u_cols, True), np.diff(u_ptr))
    # the wide case reaches what it is there for: repeats in lists longer than a lane group
    assert int((np.diff(d_ptr) > 8).sum()) >= 1000 and int(d_ptr[-1] - u_ptr[-1]) >= 1000
    print(f"nonsymmetric_wide: {int((np.diff(d_ptr) > 8).sum())} doubled lists above 8 entries, {int(d_ptr[-1] - u_ptr[-1])} repeats")
    assert rc.degrees_of([0, 0, 3, 3, 4], [2, 2, 2, 0], True).tolist() == [0, 1, 0, 1]


def test_init_expand_keys_and_number_restated():
    deg = np.array([2, 0, 1, 0, 1])
    by = np.lexsort((np.arange(5), deg))
    rank, parent, head, z = rc.init_of(deg, by)
    assert by.tolist() == [1, 3, 2, 4, 0] and rank.tolist() == [4, 0, 2, 1, 3] and z == 2 and head.tolist() == [1, 3]
    assert parent.tolist() == [rc.UNVISITED, 0, rc.UNVISITED, 1, rc.UNVISITED]
    # vertices 2 (number 2) and 4 (number 3) both list 0, 2 lists it twice: the smaller number wins, 0 is claimed once
    g = (np.array([0, 2, 2, 4, 4, 5]), np.array([2, 4, 0, 0, 0]))
    order = np.array([1, 3, 2, 4, rc.FREE])
    parent[[2, 4]] = 1
    after, claimed = rc.expand_of(*g, parent, order, 2, 4)
    assert claimed.tolist() == [0] and after.tolist() == [2, 0, 1, 1, 1] and parent[0] == rc.UNVISITED
    keys = rc.keys_of(claimed, after, rank)
    assert keys.tolist() == [(2 << 32) | 4] and rc.number_of(keys, by).tolist() == [0]


@pytest.mark.parametrize("name", rc.CASES)
def test_the_trace_sums_to_the_level_form(name):
    """Launch by launch the walk gives what ``rcm_levels`` gives as a whole: the records sum to its facts, the last ``order``
    reversed is its ``p``, and every state follows from the one before."""
    p, facts, g = rc.expected(name)
    trace, _ = rc.traced(name)
    n = len(p)
    got = rc.trace_facts(trace, n)
    assert got == {k: facts[k] for k in got}, (name, got, facts)
    assert np.array_equal(trace[-1]["order_after"][::-1], p) and trace[-1]["record"][:2] == (n, n) and trace[-1]["record"][3] == rc.DONE
    assert trace[0]["first"] and not any(t["first"] for t in trace[1:] if t["kind"] == "narrow")
    for a, b in zip(trace, trace[1:]):
        assert np.array_equal(a["parent_after"], b["parent"]) and np.array_equal(a["order_after"], b["order"])
        if a["kind"] == "narrow":
            assert a["record"][3] == rc.WIDE and b["kind"] == "wide" and a["record"][:2] == (b["lo"], b["hi"])
    for t in trace:
        if t["kind"] == "narrow" and t["record"][5] == 0:
            assert t["record"][2] == t["cursor"]                            # no start found: the cursor it was given
        if t["kind"] == "wide":
            assert np.all(t["parent"][t["cand"]] == rc.UNVISITED) and len(np.unique(t["cand"])) == len(t["cand"])
            lo, hi = t["lo"], t["hi"]
            assert np.all((t["parent_after"][t["cand"]] >= lo) & (t["parent_after"][t["cand"]] < hi))
    if name in rc.NONSYMMETRIC_CASES:
        # E u E^T with its repeats, as the device walks it: the numbering of the set form, whatever the paths
        doubled, _ = rc.traced(name, doubled=True)
        assert np.array_equal(doubled[-1]["order_after"][::-1], rc.expected(name, False)[0])
        f2, want = rc.trace_facts(doubled, n), rc.expected(name, False)[1]
        assert (f2["components"], f2["levels"]) == (want["components"], want["levels"])


def test_the_new_cases_are_what_their_names_say():
    facts = {name: rc.expected(name)[1] for name in ("star_chunk_wrap", "path1024_k6", "path1025_k6", "path3000_k6")}
    assert int(np.diff(rc.expected("star_chunk_wrap")[2][0]).max()) == 1024 * 256 + 1       # 1025 chunks of 256
    assert (facts["star_chunk_wrap"]["narrow_launches"], facts["star_chunk_wrap"]["wide_levels"]) == (2, 2)
    assert facts["star_chunk_wrap"]["levels"] == 3
    for length in (1024, 1025, 3000):
        name = f"path{length}_k6"
        trace, (indptr, _) = rc.traced(name)
        assert (facts[name]["narrow_launches"], facts[name]["wide_levels"], facts[name]["components"]) == (1, 0, 2)
        assert facts[name]["levels"] == length + 2
        deg, by = trace[0]["deg"], trace[0]["by_degree"]
        assert np.all(deg[by[:length]] <= 2) and np.all(deg[by[length:]] == 5) and len(by) == length + 6
        order = trace[0]["order_after"]
        assert order[0] == by[0] and order[length] == by[length]            # the starts: position 0, then position ``length``
        assert trace[0]["record"] == (length + 6, length + 6, length + 1, rc.DONE, length + 2, 2)
        # the first start leaves the cursor at 1; sweep k of the scan looks at positions 1 + 1024 k .. 1024 (k + 1)
        sweep, lane = divmod(length - 1, 1024)
        assert (sweep, lane) == {1024: (0, 1023), 1025: (1, 0), 3000: (2, 951)}[length]
    # a wide level that hands 10 vertices back to the one-workgroup kernel, which walks one more level
    kinds = [(t["kind"], t["hi"] - t["lo"]) for t in rc.traced("tree_then_narrow")[0]]
    assert kinds == [("narrow", 0), ("wide", rc.FRONTIER_CAP + 1), ("narrow", 10)]
    assert rc.traced("tree_then_narrow")[0][2]["record"][3:] == (rc.DONE, 1, 0)
    doubled, _ = rc.traced("nonsymmetric_wide", doubled=True)
    f2 = rc.trace_facts(doubled, 20000)
    print(f"nonsymmetric_wide on E u E^T: {f2}; directed: {rc.expected('nonsymmetric_wide')[1]}")
    assert f2["wide_levels"] > 1
    assert "nonsymmetric_wide" not in rc.SYMMETRIC_CASES and "nonsymmetric" not in rc.SYMMETRIC_CASES


def test_a_state_taken_mid_walk_is_the_walk_so_far():
    """``state_at`` against a walk stopped by a frontier cap of its own: the same parent and order at the level it stops at."""
    g = rc.expected("grid33x31")[2]
    final = rc.traced("grid33x31")[0][-1]
    cut = next(t for t in rc.rcm_trace(*g, frontier_cap=20))
    lo, hi = cut["record"][:2]
    assert cut["record"][3] == rc.WIDE and hi - lo == 21 and (lo, hi) in [m[:2] for m in final["marks"]]
    parent, order = rc.state_at(final, lo, hi)
    assert np.array_equal(parent, cut["parent_after"]) and np.array_equal(order, cut["order_after"])
