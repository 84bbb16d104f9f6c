"""CPU tests of the smoothed-aggregation restatement (tests/_amg_cases.py) in 1, 2, 3 and 8 blocks, and of ``hp.amg``'s argument
rules on host values.

Margins, none of them taken from the device: the aggregation's properties are exact; ``Ac`` symmetric to 1e-13 max|Ac| and
``u . M v == v . M u`` to 1e-12 relative (the cycle is symmetric by construction, what is left is rounding of a few dozen
operations per entry); the iteration bounds 0.3 and 0.1 of Jacobi's count and the factor 0.5 on the anisotropic grid are the
method's, stated with the cases in tests/_amg_cases.py."""
import os
import re
import sys

import numpy as np
import pytest

from tests import _amg_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_amg_work_bytes", "hpcla_amg_round_blocks", "hpcla_amg_weights_f64_i32", "hpcla_amg_weights_f64_i64",
               "hpcla_amg_smoother_f64", "hpcla_amg_strength_count_f64_i32", "hpcla_amg_strength_count_f64_i64",
               "hpcla_amg_strength_fill_f64_i32", "hpcla_amg_strength_fill_f64_i64", "hpcla_amg_mis_init", "hpcla_amg_mis_round",
               "hpcla_amg_join", "hpcla_amg_aggregate_ids", "hpcla_amg_prolongator_f64_i32", "hpcla_amg_prolongator_f64_i64",
               "hpcla_amg_presmooth_f64", "hpcla_amg_postsmooth_f64"]
SMALL = 8            # coarse_size that makes every case but n = 1, 2 aggregate at least once


@pytest.fixture(scope="module")
def matrices():
    return ac.cases()


@pytest.fixture(scope="module")
def hierarchies(matrices):
    """(name, blocks) -> the restatement's levels at coarse_size = SMALL (so that the small cases aggregate too), once."""
    out = {}
    for name, A in matrices.items():
        for k in ac.BLOCKS:
            if A.shape[0] >= k:
                out[name, k] = ac.setup(A, ac.equal_blocks(A.shape[0], k), coarse_size=SMALL)
    return out


def _distance2(indptr, indices, n):
    import scipy.sparse as sp
    S = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    S = S + S.T + sp.identity(n)
    return (S @ S).tocsr()


# ---- the aggregation ------------------------------------------------------------------------------------------------------------
def test_every_row_is_in_one_aggregate_near_its_root_and_roots_keep_their_distance(hierarchies):
    seen = 0
    for (name, k), levels in hierarchies.items():
        for lvl in levels:
            if "agg" not in lvl:
                continue
            seen += 1
            n, part, agg, roots = lvl["n"], lvl["partition"], lvl["agg"], lvl["roots"]
            nc = int(lvl["counts"].sum())
            assert agg.shape == (n,) and agg.min() >= 0 and agg.max() == nc - 1, (name, k)
            assert len(np.unique(agg)) == nc == int(roots.sum()), (name, k)              # every aggregate is used, one root each
            D2 = _distance2(*lvl["graph"], n)
            r = np.flatnonzero(roots)
            close = D2[r][:, r].tocoo()
            assert np.all(close.row == close.col), (name, k, "two roots within distance 2")
            root_of = r[agg]                                                             # ids are ordered like the roots
            assert np.array_equal(agg[r], np.arange(nc)), (name, k)
            assert np.all(np.asarray(D2[np.arange(n), root_of]).ravel() > 0), (name, k, "a row further than 2 from its root")
            # contiguous per block: block j owns ids [sum counts[:j], sum counts[:j+1]) and only its own rows carry them
            offs = np.concatenate([[0], np.cumsum(lvl["counts"])])
            for j in range(len(part) - 1):
                mine = agg[part[j]:part[j + 1]]
                assert mine.size == 0 or (mine.min() >= offs[j] and mine.max() < offs[j + 1]), (name, k, j)
            assert 1 <= lvl["rounds"] <= ac.MAX_ROUNDS, (name, k, lvl["rounds"])
    assert seen >= 40


def test_one_level_cases(hierarchies):
    for k in ac.BLOCKS:
        levels = hierarchies["diagonal", k]
        assert len(levels) == 1 and np.array_equal(levels[0]["agg"], np.arange(37)) and "sweeps" in levels[0]   # a stall
    assert len(hierarchies["one", 1]) == 1 and len(hierarchies["two", 1]) == 1 and "inv" in hierarchies["two", 2][0]
    hub = hierarchies["star300", 1]
    assert [l["n"] for l in hub] == [301, 1] and hub[0]["rounds"] <= 3


def test_coarse_matrices_are_symmetric_and_the_cycle_is_too(matrices, hierarchies):
    rng = np.random.default_rng(5)
    for (name, k), levels in hierarchies.items():
        for lvl in levels[1:]:
            Ac = lvl["A"]
            assert abs(Ac - Ac.T).max() <= 1e-13 * abs(Ac).max(), (name, k)
        n = levels[0]["n"]
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        uMv, vMu = float(u @ ac.cycle(levels, v)), float(v @ ac.cycle(levels, u))
        assert abs(uMv - vMu) <= 1e-12 * max(abs(uMv), abs(vMu), np.linalg.norm(u) * np.linalg.norm(ac.cycle(levels, v))), (name, k)
        assert float(u @ ac.cycle(levels, u)) > 0, (name, k)


def test_levels_of_the_description(matrices):
    """The sizes the method's description lists for one block at coarse_size = 100."""
    want = {"grid32x32": [1024, 148, 11], "grid64x64": [4096, 587, 38], "grid16x16x16": [4096, 404, 11]}
    for name, sizes in want.items():
        levels = ac.setup(matrices[name], coarse_size=100)
        assert [l["n"] for l in levels] == sizes, name
        assert 1.25 <= ac.operator_complexity(levels) <= 1.6, name


# ---- iteration counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.BOUND_GRIDS)
def test_amg_needs_at_most_three_tenths_of_jacobis_iterations(matrices, name):
    A = matrices[name]
    n = A.shape[0]
    b = ac.rhs(n)
    jacobi = ac.pcg_jacobi(A, b)[1]
    for k in ac.BLOCKS:
        x, its, status, _ = ac.pcg_amg(A, b, ac.setup(A, ac.equal_blocks(n, k), coarse_size=100))
        print(f"{name} in {k} blocks: {its} against {jacobi} ({its / jacobi:.3f})")
        assert status == "converged" and its <= ac.JACOBI_FACTOR * jacobi, (name, k, its, jacobi)
        assert np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b)


def test_amg_needs_at_most_a_tenth_on_128_squared():
    A = ac.grid2d(128, 128)
    b = ac.rhs(A.shape[0])
    jacobi = ac.pcg_jacobi(A, b)[1]
    levels = ac.setup(A, coarse_size=100)
    its = ac.pcg_amg(A, b, levels)[1]
    print(f"128x128: {its} against {jacobi} ({its / jacobi:.3f}), levels {[l['n'] for l in levels]}")
    assert its <= ac.JACOBI_FACTOR_128 * jacobi


def test_theta_pays_on_the_anisotropic_grid(matrices):
    A = matrices["aniso40x40"]
    b = ac.rhs(A.shape[0])
    plain = ac.pcg_amg(A, b, ac.setup(A, theta=0.0, coarse_size=100))[1]
    tuned = ac.pcg_amg(A, b, ac.setup(A, theta=0.25, coarse_size=100))[1]
    print(f"anisotropic 40x40: theta 0.25 {tuned}, theta 0 {plain}")
    assert tuned <= ac.ANISO_FACTOR * plain


def test_every_case_solves(matrices, hierarchies):
    for (name, k), levels in hierarchies.items():
        A = matrices[name]
        b = ac.rhs(A.shape[0])
        x, its, status, _ = ac.pcg_amg(A, b, levels)
        assert status == "converged" and np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b), (name, k, its)


# ---- the package, without a device ----------------------------------------------------------------------------------------------
def test_public_names_exist(hp):
    assert callable(hp.amg) and hp.AMG and hp.AMGLevel and hp.AMGWorkspace and hp.amg.__module__.endswith("amg")
    assert not hasattr(hp, "amg_aggregate")
    assert "AMG" in hp.cg.__doc__ and "theta" in hp.amg.__doc__


def test_argument_rules_on_host_values(hp):
    mod = sys.modules[hp.amg.__module__]
    call = lambda **kw: mod.check_arguments(**{**ac.GOOD_ARGUMENTS, **kw})
    call()
    call(theta=0.999, coarse_size=1, max_levels=1, coarse_sweeps=1)
    call(coarse_size=1024)
    for kw, exc in ac.BAD_ARGUMENTS:
        with pytest.raises(exc, match="amg: "):
            call(**kw)
    call()


def test_header_declares_the_new_entries_and_ctypes_binds_them(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    lib = hp._capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in hp._capi.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_c_entries_refuse_bad_arguments_without_a_gpu(hp):
    lib = hp._capi.load()
    assert lib.hpcla_amg_work_bytes(-1) == -1 and lib.hpcla_amg_work_bytes(5000) == 8 * (1 + 5)
    assert lib.hpcla_amg_round_blocks(257) == 2 and lib.hpcla_amg_round_blocks(0) == 1
    assert lib.hpcla_amg_weights_f64_i32(None, None, None, 4, 3, 0, None, None, None, None) != 0            # n_own != nrows
    assert lib.hpcla_amg_weights_f64_i64(None, None, None, 4, 4, 0, None, None, None, None) != 0            # null info
    assert lib.hpcla_amg_strength_count_f64_i32(None, None, None, None, 4, 4, 0, 1.0, None, None, None, None) != 0   # theta
    assert lib.hpcla_amg_strength_fill_f64_i64(None, None, None, None, 4, 4, 2, 0.0, None, None, None) != 0          # index base
    assert lib.hpcla_amg_mis_init(1 << 31, 0, None, None, None) != 0
    assert lib.hpcla_amg_mis_round(None, None, 4, None, None, None, None, None, None, None) != 0
    assert lib.hpcla_amg_join(None, None, -1, None, None, None, None, None, None, None, None) != 0
    assert lib.hpcla_amg_aggregate_ids(None, None, 4, -1, None, None) != 0
    assert lib.hpcla_amg_prolongator_f64_i32(None, None, None, None, None, None, 4, 0, None, None) != 0
    assert lib.hpcla_amg_presmooth_f64(None, None, None, 4, None) != 0
    assert lib.hpcla_amg_postsmooth_f64(None, None, None, None, -1, None) != 0
    assert lib.hpcla_amg_presmooth_f64(None, None, None, 0, None) == 0 and lib.hpcla_amg_smoother_f64(1.0, None, None, 0, None) == 0
    assert lib.hpcla_amg_postsmooth_f64(None, None, None, None, -1, None) != 0
    assert hp._capi.last_error() == "amg_smooth: negative size"
    assert lib.hpcla_amg_strength_count_f64_i32(None, None, None, None, 4, 4, 0, 1.0, None, None, None, None) != 0
    assert hp._capi.last_error() == "amg_strength_count: theta must lie in [0, 1)"


# ---- the helpers that feed the kernels one block at a time -----------------------------------------------------------------------
def test_split_block_maps_back_to_the_rows_of_A(matrices):
    """Through (lo, ghosts) the split columns give the block's rows of A exactly, in every (case, blocks) pair, index type and
    base; ghosts below lo stand in front of the owned columns."""
    front = 0
    for name, A in matrices.items():
        n = A.shape[0]
        for k in ac.BLOCKS:
            part = ac.equal_blocks(n, k)
            for j in range(k):
                lo, hi = part[j], part[j + 1]
                for base, Ti in ((0, np.int32), (1, np.int64)):
                    rowptr, split, vals, n_own, ghosts = ac.split_block(A, part, j, base, Ti)
                    assert rowptr.dtype == split.dtype == Ti and n_own == hi - lo and len(rowptr) == n_own + 1, (name, k, j)
                    assert np.array_equal(rowptr - base, A.indptr[lo:hi + 1] - A.indptr[lo]), (name, k, j)
                    c = split.astype(np.int64) - base
                    assert np.all(np.diff(ghosts) > 0) and not np.any((ghosts >= lo) & (ghosts < hi)), (name, k, j)
                    assert c.size == 0 or (c.min() >= 0 and c.max() < n_own + len(ghosts)), (name, k, j)
                    back = np.where(c < n_own, c + lo, ghosts[np.maximum(c - n_own, 0)] if len(ghosts) else -1)
                    a, b = A.indptr[lo], A.indptr[hi]
                    assert np.array_equal(back, A.indices[a:b]) and np.array_equal(ac.bits(vals), ac.bits(A.data[a:b])), (name, k, j)
                    assert len(ghosts) == 0 or set(ghosts) == set(A.indices[a:b]) - set(range(lo, hi)), (name, k, j)
                    first = c[(rowptr[:-1] - base)[np.diff(rowptr) > 0]]
                    front += int(np.sum(first >= n_own))
    assert front > 1000                                            # rows that open with a ghost


def test_weights_in_stored_order_lie_within_the_pairwise_ones(matrices, hierarchies):
    worst, longest = 0.0, 0
    for (name, k), levels in hierarchies.items():
        for lvl in levels:
            A = lvl["A"]
            d, ratio = ac.weights_stored_order(A)
            assert np.array_equal(ac.bits(d), ac.bits(A.diagonal())), (name, k)
            rho = float(ratio.max())
            worst = max(worst, abs(rho - lvl["rho"]) / lvl["rho"])
            pairwise = np.asarray(abs(A).sum(axis=1)).ravel() / d
            worst = max(worst, float(np.max(np.abs(ratio - pairwise) / pairwise)))
            longest = max(longest, int(np.diff(A.indptr).max()))
    print(f"stored order against pairwise: {worst:.2e} over rows of up to {longest} entries")
    assert worst <= 1e-13
    hub = matrices["star300"]                                      # a plain loop over the longest row of the fine cases
    total = 0.0
    for v in hub.data[hub.indptr[0]:hub.indptr[1]]:
        total = total + abs(v)
    assert ac.weights_stored_order(hub)[1][0] == total / hub[0, 0]
    # what the bit comparison on the device can tell apart: the same rows summed by 8 lanes (lane l takes entries l, l + 8, ...)
    # and combined pairwise differ from the stored order in a bit on some row of the random case's levels
    differ = rows = 0
    for lvl in hierarchies["random600", 8]:
        A = lvl["A"]
        d, ratio = ac.weights_stored_order(A)
        for i in range(A.shape[0]):
            v = np.abs(A.data[A.indptr[i]:A.indptr[i + 1]])
            lanes = [float(np.cumsum(v[l::8])[-1]) if len(v) > l else 0.0 for l in range(8)]
            while len(lanes) > 1:
                lanes = [a + b for a, b in zip(lanes[::2], lanes[1::2])]
            differ += int(lanes[0] / d[i] != ratio[i])
            rows += 1
    print(f"a lane-parallel sum differs from the stored order on {differ} of {rows} rows")
    assert differ >= 10


def test_mis2_states_end_in_the_roots_of_the_block(hierarchies):
    seen = 0
    for (name, k), levels in hierarchies.items():
        for lvl in levels:
            if "agg" not in lvl:
                continue
            part = lvl["partition"]
            indptr, indices = lvl["graph"]
            key, _ = ac.keys_of(part)
            for j in range(len(part) - 1):
                lo, hi = part[j], part[j + 1]
                ptr = indptr[lo:hi + 1] - indptr[lo]
                cols = indices[indptr[lo]:indptr[hi]] - lo
                assert cols.size == 0 or (cols.min() >= 0 and cols.max() < hi - lo), (name, k, j)
                states = list(ac.mis2_states(ptr, cols, key[lo:hi]))
                assert (1 if hi > lo else 0) <= len(states) <= lvl["rounds"], (name, k, j, len(states))
                if states:
                    assert np.array_equal(states[-1] == ac.ROOT, lvl["roots"][lo:hi]), (name, k, j)
                    assert np.all((states[-1] == ac.ROOT) | (states[-1] == -1)), (name, k, j)
                    assert all(np.any((s >= 0) & (s < ac.ROOT)) for s in states[:-1]), (name, k, j)
                seen += 1
    assert seen >= 300


def test_compressed_columns_are_shuffled_and_map_back(hierarchies):
    rng = np.random.default_rng(3)
    lvl = hierarchies["grid37x53", 3][0]
    cols = lvl["P"].indices[lvl["P"].indptr[100]:lvl["P"].indptr[900]]
    local, col_indices = ac.compressed_columns(cols, rng)
    assert np.array_equal(col_indices[local], cols) and np.array_equal(np.sort(col_indices), np.unique(cols))
    assert np.any(np.diff(col_indices) < 0) and local.min() == 0 and local.max() == len(col_indices) - 1
    one, ids = ac.compressed_columns(np.array([5, 5, 5]), rng)
    assert np.array_equal(one, [0, 0, 0]) and np.array_equal(ids, [5])


def test_the_levels_the_kernel_tests_walk_have_the_edges_they_name(matrices):
    """tests/test_gpu_precond_kernels.py asserts the same on what it ran; here without a device, so that a changed generator
    fails in the CPU suite first."""
    stats = ac.chain_coverage(ac.chain_levels(matrices))
    print(stats)
    assert stats["levels"] >= 120 and stats["one_row_blocks"] >= 1 and stats["stored_zeros"] >= 1 and stats["isolated"] >= 1
    assert stats["chains"] >= 400 and stats["ghost_entries"] >= 75_000
    assert stats["longest_row"] >= 128                             # of A T: sixteen trips of the prolongator's 8-lane loop
