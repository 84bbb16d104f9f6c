"""CPU tests of the restatement of the nonsymmetric mode of ``hp.amg`` (tests/_amg_nonsym_cases.py) and of the argument rules:
the symmetrised graph is E u E^T, no row stays without an aggregate, a symmetric A gives what the symmetric restatement gives
bit for bit, the cycle in GMRES and BiCGStab converges within 0.3 of Jacobi's count, and four summation orders of the dots move
the compared heads of the histories far less than the margin the GPU tests hold them to."""
import numpy as np
import pytest

from tests import _amg_cases as ac
from tests import _amg_nonsym_cases as nc
from tests import _bicgstab_cases as bc
from tests import _gmres_cases as gc


@pytest.fixture(scope="module")
def solved():
    """name -> (A, b, levels at the default coarse_size, GMRES(30) with the cycle, GMRES(30) with Jacobi), once."""
    out = {}
    for name, A in nc.solve_cases().items():
        b = ac.rhs(A.shape[0])
        levels = nc.setup(A)
        out[name] = (A, b, levels, nc.gmres_amg(A, b, levels), nc.gmres_jacobi(A, b))
    return out


def _edge_set(indptr, indices):
    row = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return set(zip(row.tolist(), np.asarray(indices).tolist()))


@pytest.mark.parametrize("name", sorted(nc.graph_cases()))
def test_the_graph_is_the_union_with_its_transpose_and_every_row_is_aggregated(name):
    A, theta = nc.graph_cases()[name]
    n = A.shape[0]
    for k in [k for k in nc.BLOCKS if k <= n]:
        part = ac.equal_blocks(n, k)
        E = _edge_set(*ac.strength(A, part, theta))
        indptr, indices = nc.strength(A, part, theta)
        U = _edge_set(indptr, indices)
        assert U == E | {(j, i) for i, j in E}, (name, k)
        assert U == {(j, i) for i, j in U} and len(U) == len(indices), (name, k)          # symmetric as a set, no entry twice
        _, block = ac.keys_of(part)
        assert all(block[i] == block[j] and i != j for i, j in U), (name, k)              # no ghost column either way
        agg, counts, roots, rounds, _ = nc.aggregate(A, part, theta)                      # asserts that no row is left
        assert agg.min() >= 0 and agg.max() == counts.sum() - 1 and rounds <= ac.MAX_ROUNDS
        assert np.array_equal(np.unique(agg), np.arange(counts.sum()))
        assert np.all(block[np.flatnonzero(roots)[agg]] == block), (name, k)              # aggregates do not cross blocks


def _roots_within_two(indptr, indices, roots):
    """Pairs of distinct roots joined by a path of at most two edges of the undirected graph."""
    import scipy.sparse as sp
    n = len(indptr) - 1
    G = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    G = ((G + G.T + sp.identity(n)) > 0).astype(np.float64)
    r = np.flatnonzero(roots)
    near = (G @ G)[r][:, r].toarray() > 0
    return int(near.sum()) - len(r)


@pytest.mark.parametrize("name", sorted(nc.graph_cases()))
def test_the_roots_are_a_maximal_distance_two_independent_set(name):
    import scipy.sparse as sp
    A, theta = nc.graph_cases()[name]
    n = A.shape[0]
    _, _, roots, _, (indptr, indices) = nc.aggregate(A, [0, n], theta)
    assert _roots_within_two(indptr, indices, roots) == 0, name
    G = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n)) + sp.identity(n)
    assert np.all((G @ (G @ roots.astype(np.float64))) > 0), name                        # every row within two edges of a root


def test_the_directed_graph_alone_does_not_give_an_independent_set():
    """What the symmetrised graph is for: on the out-star the leaves have no outgoing edge, each sees only itself and every one
    becomes a root, two edges from every other through the hub."""
    A, theta = nc.graph_cases()["outstar300"]
    _, _, roots, _, graph = ac.aggregate(A, [0, A.shape[0]], theta)
    assert int(roots.sum()) >= 300 and _roots_within_two(*graph, roots) > 0
    _, counts, roots, _, graph = nc.aggregate(A, [0, A.shape[0]], theta)
    assert _roots_within_two(*graph, roots) == 0


def test_one_way_strength_and_stored_zeros():
    A, theta = nc.graph_cases()["oneway64"]
    E = _edge_set(*ac.strength(A, [0, 64], theta))
    assert E == {(i, i + 1) for i in range(63)}                                           # -0.01 is below 0.25
    assert _edge_set(*nc.strength(A, [0, 64], theta)) == E | {(i + 1, i) for i in range(63)}
    Z, _ = nc.graph_cases()["zeros97"]
    assert int(np.sum(Z.data == 0)) > 97
    assert _edge_set(*nc.strength(Z, [0, 97], 0.0)) == {(i, (i + 1) % 97) for i in range(97)} | {((i + 1) % 97, i) for i in range(97)}


@pytest.mark.parametrize("name", ac.GRIDS)
def test_a_symmetric_matrix_gives_the_symmetric_method(name):
    """Aggregates, P and the first level's R = Pt bit for bit; the coarse matrix is symmetric to rounding only, so deeper levels
    are compared in their sizes."""
    A = ac.cases()[name]
    sym, non = ac.setup(A), nc.setup(A)
    assert [l["n"] for l in sym] == [l["n"] for l in non]
    assert np.array_equal(sym[0]["agg"], non[0]["agg"]) and sym[0]["rounds"] == non[0]["rounds"]
    for what, a, b in (("P", sym[0]["P"], non[0]["P"]), ("R", sym[0]["Pt"], non[0]["R"])):
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), (name, what)
        assert np.array_equal(ac.bits(a.data), ac.bits(b.data)), (name, what)


def test_the_restriction_is_the_petrov_galerkin_one():
    """R = Tt (I - A S) as dense matrices, and A_c = R A P."""
    A = nc.convection_diffusion(16, 16)
    levels = nc.setup(A, coarse_size=8)
    for lvl, nxt in zip(levels[:-1], levels[1:]):
        n, ncoarse = lvl["n"], nxt["n"]
        T = np.zeros((n, ncoarse))
        T[np.arange(n), lvl["agg"]] = 1.0
        D = lvl["A"].toarray()
        want = T.T @ (np.eye(n) - D @ np.diag(lvl["s"]))
        assert np.abs(lvl["R"].toarray() - want).max() <= 1e-14
        assert np.abs(nxt["A"].toarray() - lvl["R"].toarray() @ D @ lvl["P"].toarray()).max() <= 1e-13
    assert np.abs(levels[-1]["inv"] @ levels[-1]["A"].toarray() - np.eye(levels[-1]["n"])).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(nc.solve_cases()))
def test_the_count_is_within_the_bound_of_jacobis(solved, name):
    A, b, levels, amg, jac = solved[name]
    assert amg[2] == "converged" and jac[2] == "converged"
    print(f"{name}: GMRES(30) with the cycle {amg[1]}, with Jacobi {jac[1]}, ratio {amg[1] / jac[1]:.3f}")
    assert amg[1] <= nc.JACOBI_FACTOR * jac[1]
    true = np.linalg.norm(b - A @ amg[0]) / np.linalg.norm(b)
    assert true <= 2e-8
    bi = nc.bicgstab_amg(A, b, levels)
    assert bi[2] == "converged" and np.linalg.norm(b - A @ bi[0]) / np.linalg.norm(b) <= 2e-8
    if name != "cd65x63":                                                                 # four levels as well
        small = nc.setup(A, coarse_size=8)
        assert len(small) == len(levels) + 1
        g8 = nc.gmres_amg(A, b, small)
        print(f"{name}: coarse_size 8: {g8[1]}, ratio {g8[1] / jac[1]:.3f}")
        assert g8[2] == "converged" and g8[1] <= nc.JACOBI_FACTOR * jac[1]


@pytest.mark.parametrize("name", sorted(nc.solve_cases()))
def test_the_summation_order_moves_the_heads_less_than_a_tenth_of_the_margin(solved, name):
    """The GPU tests hold the first HEAD entries to ``gc.HIST_RTOL`` = 1e-12.  Measured here: the four orders of
    ``_bicgstab_cases.DOTS`` spread the GMRES heads by at most 1.9e-15 and the BiCGStab heads by at most 5.7e-15 (relative), and
    every order gives the same count, so the margin is not widened."""
    A, b, levels, amg, _ = solved[name]
    for restart in gc.RESTARTS:
        runs = [nc.gmres_amg(A, b, levels, restart=restart, dot=d) for d in bc.DOTS.values()]
        H = np.array([r[3][:nc.HEAD] for r in runs])
        spread = float(((H.max(0) - H.min(0)) / H.min(0)).max())
        assert len({r[1] for r in runs}) == 1 and 10 * spread <= gc.HIST_RTOL, (name, restart, spread)
    runs = [nc.bicgstab_amg(A, b, levels, dot=d) for d in bc.DOTS.values()]
    H = np.array([r[3][:nc.HEAD_BICGSTAB] for r in runs])
    spread = float(((H.max(0) - H.min(0)) / H.min(0)).max())
    assert max(r[1] for r in runs) - min(r[1] for r in runs) <= 1 and 10 * spread <= bc.HIST_RTOL, (name, spread)


def test_the_argument_rules(hp):
    import sys
    amg = sys.modules[hp.amg.__module__]
    amg.check_arguments(**ac.GOOD_ARGUMENTS)
    assert "symmetric=False" in hp.amg.__doc__ and "AMG" in hp.gmres.__doc__ and "AMG" in hp.bicgstab.__doc__
    assert "symmetric=False" in hp.cg.__doc__
    for value in (True, False, np.bool_(False)):
        amg.check_arguments(**dict(ac.GOOD_ARGUMENTS, symmetric=value))
    for value in nc.BAD_SYMMETRIC:
        with pytest.raises(TypeError, match="symmetric"):
            amg.check_arguments(**dict(ac.GOOD_ARGUMENTS, symmetric=value))
    for overrides, exc in ac.BAD_ARGUMENTS:                                               # what was refused stays refused
        with pytest.raises(exc):
            amg.check_arguments(**dict(ac.GOOD_ARGUMENTS, symmetric=False, **overrides))

