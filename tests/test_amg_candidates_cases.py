"""CPU tests of the restatement of ``hp.amg(A, B=...)`` (tests/_amg_candidates_cases.py), of the argument rules of ``B`` on host
values and of the new C entries' refusals without a device.

Margins, none taken from a device: ``Q'Q = I`` and ``Q R = B[members]`` to 16 k eps (classical Gram-Schmidt run twice leaves a
few eps per column; the second relative to the block's largest entry); ``P B_c = (I - S A) B`` to 1e-12 of the largest entry of
``B`` (T B_c = B to the fit's rounding, and a row of A adds at most a few dozen separately rounded products); the counts: at
most 0.5 of the default hierarchy's, the condition the GPU solves lean on."""
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import _amg_cases as ac
from tests import _amg_candidates_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NEW_SYMBOLS = ["hpcla_amg_fit_f64", "hpcla_amg_prolongator_b_f64_i32", "hpcla_amg_prolongator_b_f64_i64",
               "hpcla_amg_restrictor_b_f64_i32", "hpcla_amg_restrictor_b_f64_i64"]


@pytest.fixture(scope="module")
def hierarchies():
    """name -> (A, B, symmetric, levels at coarse_size = SMALL), once."""
    return {name: (A, B, sym, cc.setup(A, B, coarse_size=cc.SMALL, symmetric=sym))
            for name, (A, B, sym) in cc.hierarchy_cases().items()}


def test_generators():
    A, d = cc.scaled(33, 31)
    assert A.shape == (1023, 1023) and abs(A - A.T).max() == 0 and d.min() >= 0.1 and d.max() <= 10.0
    G = ac.grid2d(33, 31)
    assert np.allclose(A @ (1.0 / d), d * (G @ np.ones(1023)), rtol=0, atol=1e-12 * d.max() * 4)
    E, modes = cc.elasticity(16, 16)
    assert E.shape == (544, 544) and modes.shape == (544, 3) and abs(E - E.T).max() <= 1e-15
    assert np.linalg.eigvalsh(E.toarray()).min() > 0
    r = E @ modes                                               # rigid-body modes: no force away from the clamped edge
    interior = np.flatnonzero(np.repeat((np.arange(17 * 17) % 17 > 1), 2)[np.repeat(np.arange(17 * 17) % 17 != 0, 2)])
    assert np.abs(r[interior]).max() <= 1e-12 * np.abs(modes).max()
    assert [cc.elasticity(nx, ny)[0].shape[0] for nx, ny in ((32, 32), (48, 16))] == [2112, 1632]
    C, _ = cc.scaled_nonsym(33, 31)
    assert abs(C - C.T).max() > 0 and np.all(C.diagonal() > 0)


def test_the_fit_is_orthonormal_and_reproduces_the_block(hierarchies):
    seen = 0
    for name, (_, _, _, levels) in hierarchies.items():
        for lvl in levels:
            if "Tv" not in lvl:
                continue
            B, Tv, Bc, ptr, members = lvl["B"], lvl["Tv"], lvl["Bc"], lvl["ptr"], lvl["members"]
            k = B.shape[1]
            assert np.array_equal(np.sort(members), np.arange(lvl["n"])), name
            for a in range(len(ptr) - 1):
                rows = members[ptr[a]:ptr[a + 1]]
                assert np.all(np.diff(rows) > 0) and np.all(lvl["agg"][rows] == a), name
                Q, R = Tv[rows], Bc[k * a:k * a + k]
                assert np.abs(Q.T @ Q - np.eye(k)).max() <= 16 * k * EPS, (name, a)
                assert np.abs(Q @ R - B[rows]).max() <= 16 * k * EPS * np.abs(B[rows]).max(), (name, a)
                assert np.array_equal(ac.bits(np.tril(R, -1)), ac.bits(np.zeros((k, k)))) and np.all(np.diag(R) > 0), (name, a)
                seen += 1
    assert seen >= 900                                          # aggregates looked at: the loop is not empty


def test_sequential_sums_are_what_the_restatement_takes():
    x = np.random.default_rng(1).standard_normal(301) * 10.0 ** np.random.default_rng(2).uniform(-8, 8, 301)
    total = 0.0
    for v in x:
        total = total + v
    assert cc.seqsum(x) == total and cc.seqsum([]) == 0.0 and np.signbit(cc.seqsum([-0.0, -0.0])) == False
    differ = sum(cc.seqsum(np.random.default_rng(s).standard_normal(65)) != float(np.sum(np.random.default_rng(s).standard_normal(65)))
                 for s in range(50))
    assert differ >= 10                                         # what a bit comparison can tell from a pairwise sum


def test_dropped_columns():
    rng = np.random.default_rng(3)
    Bm = rng.standard_normal((9, 3))
    for kind, col in (("repeat", 2), ("zero", 0), ("nan", 2), ("few", 2)):
        M = Bm.copy()
        if kind == "repeat":
            M[:, 2] = M[:, 0]
        elif kind == "zero":
            M[:, 0] = 0.0
        elif kind == "nan":
            M[4, 2] = np.nan
        else:
            M = M[:2]
        Q, R, dropped = cc.fit_block(M)
        assert dropped == [col], kind
        assert not Q[:, col].any() and not np.signbit(Q[:, col]).any() and not R[col].any() and not np.signbit(R[col]).any(), kind
        live = [c for c in range(3) if c != col]
        assert np.abs(Q[:, live].T @ Q[:, live] - np.eye(2)).max() <= 48 * EPS, kind
    Q, R, dropped = cc.fit_block(np.zeros((0, 2)))
    assert dropped == [0, 1] and Q.shape == (0, 2)
    assert cc.fit_word([(5, 1), (3, 2), (3, 1)]) == 8 * 3 + 1 and cc.fit_word([]) == -1
    A, d = cc.scaled(16, 16)
    with pytest.raises(ValueError, match="cannot carry candidate column 1"):
        cc.setup(A, np.stack([1.0 / d, 1.0 / d], axis=1), coarse_size=cc.SMALL)
    # the path's 72 aggregates stall at k = 3 (216 >= 0.8 * 257): the fit comes before that rule, and the last one has 2 members
    with pytest.raises(ValueError, match=r"the aggregate of row 255 \(level of 257 rows\) has 2 members and cannot carry "
                                         r"candidate column 2"):
        cc.setup(ac.path(257), cc.path_candidates(257), coarse_size=cc.SMALL)


def test_the_prolongator_carries_the_smoothed_candidates(hierarchies):
    """P B_c = (I - S A) B and T B_c = B on every level; k unknowns per aggregate; no column is dropped in any case."""
    for name, (_, B0, sym, levels) in hierarchies.items():
        k = B0.shape[1]
        assert len(levels) >= 2 and np.array_equal(ac.bits(levels[0]["B"]), ac.bits(B0)), name
        for lvl, nxt in zip(levels, levels[1:]):
            A, B, s, P, Bc = lvl["A"], lvl["B"], lvl["s"], lvl["P"], lvl["Bc"]
            n_agg = int(lvl["counts"].sum())
            assert P.shape == (lvl["n"], k * n_agg) and nxt["n"] == k * n_agg and nxt["B"] is Bc, name
            scale = np.abs(B).max()
            assert np.abs(lvl["T"] @ Bc - B).max() <= 16 * k * EPS * scale, name
            want = B - s[:, None] * (A @ B)
            assert np.abs(P @ Bc - want).max() <= 1e-12 * scale, name
            assert np.array_equal(lvl["T"].indptr, k * np.arange(lvl["n"] + 1)), name
            if sym:
                assert abs(nxt["A"] - nxt["A"].T).max() <= 1e-13 * abs(nxt["A"]).max(), name
            else:
                assert lvl["R"].shape == P.T.shape and np.array_equal(lvl["R"].indices, P.T.tocsr().sorted_indices().indices), name


def test_k_one_with_the_constant_keeps_the_aggregation_and_the_pattern():
    """B = ones: the aggregates, the sizes and every pattern are the default hierarchy's (T's entries become 1 / sqrt(m))."""
    A = ac.grid2d(33, 31)
    mine = cc.setup(A, np.ones((1023, 1)), coarse_size=cc.SMALL)
    theirs = ac.setup(A, coarse_size=cc.SMALL)
    assert [l["n"] for l in mine][:2] == [l["n"] for l in theirs][:2]
    assert np.array_equal(mine[0]["agg"], theirs[0]["agg"]) and np.array_equal(mine[0]["P"].indices, theirs[0]["P"].indices)
    m = np.bincount(mine[0]["agg"])[mine[0]["agg"]]
    assert np.array_equal(ac.bits(mine[0]["Tv"][:, 0]), ac.bits(1.0 / np.sqrt(m.astype(np.float64))))


@pytest.mark.parametrize("name", sorted(cc.SOLVES))
def test_the_right_candidates_halve_the_count(name):
    """The conditions the GPU solves lean on: both hierarchies converge, and the one with candidates takes at most 0.5 of the
    default one's iterations (CG; GMRES(30) on the nonsymmetric case)."""
    A, B, sym = cc.solve_cases()[name]
    b = ac.rhs(A.shape[0])
    kind = cc.SOLVES[name]
    x, its, ok = cc.solve(kind, A, b, cc.setup(A, B, symmetric=sym), rtol=1e-8)
    _, base, ok_base = cc.solve(kind, A, b, cc.default_setup(A, sym), rtol=1e-8)
    print(f"{name}: {its} against {base} ({its / base:.3f})")
    assert ok and ok_base and its <= cc.COUNT_FACTOR * base, (name, its, base)
    assert np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b)


# ---- the package, without a device ----------------------------------------------------------------------------------------------
def test_argument_rules_of_B_on_host_values(hp):
    mod = sys.modules[hp.amg.__module__]
    call = lambda **kw: mod.check_arguments(**{**ac.GOOD_ARGUMENTS, **kw})
    call(B=None)
    call(B=cc.GOOD_B)
    call(B=(np.float64, (10, 1), [0, 5, 10]), symmetric=False)
    call(B=(np.float64, (10, 8), [0, 5, 10]))
    for bad, exc in cc.BAD_B:
        with pytest.raises(exc, match="amg: "):
            call(B=bad)
    assert mod.MAX_CANDIDATES == cc.MAX_K == 8
    assert "B" in hp.amg.__doc__ and "candidates_per_aggregate" in hp.AMG.__doc__
    assert "only near-nullspace candidate" not in mod.__doc__


def test_header_declares_the_new_entries_and_ctypes_binds_them(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    lib = hp._capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in hp._capi.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_c_entries_refuse_bad_arguments_without_a_gpu(hp):
    lib = hp._capi.load()
    assert lib.hpcla_amg_fit_f64(None, 4, 0, None, None, 4, 1, None, None, None, None) != 0
    assert hp._capi.last_error() == "amg_fit: k must lie in 1..8"
    assert lib.hpcla_amg_fit_f64(None, 4, 9, None, None, 4, 1, None, None, None, None) != 0
    assert lib.hpcla_amg_fit_f64(None, -1, 3, None, None, 4, 1, None, None, None, None) != 0
    assert lib.hpcla_amg_fit_f64(None, 4, 3, None, None, 4, 1, None, None, None, None) != 0
    assert hp._capi.last_error() == "amg_fit: null info"
    assert lib.hpcla_amg_prolongator_b_f64_i32(None, None, None, None, None, None, None, 9, 4, 0, None, None) != 0
    assert lib.hpcla_amg_prolongator_b_f64_i64(None, None, None, None, None, None, None, 3, 4, 0, None, None) != 0
    assert hp._capi.last_error() == "amg_prolongator_b: null array"
    assert lib.hpcla_amg_prolongator_b_f64_i32(None, None, None, None, None, None, None, 3, 0, 0, None, None) == 0
    assert lib.hpcla_amg_restrictor_b_f64_i32(None, None, None, None, None, None, None, 0, 4, 4, 0, 0, None, None) != 0
    assert lib.hpcla_amg_restrictor_b_f64_i64(None, None, None, None, None, None, None, 3, 4, 4, -1, 0, None, None) != 0
    assert lib.hpcla_amg_restrictor_b_f64_i64(None, None, None, None, None, None, None, 3, 4, 4, 0, 2, None, None) != 0
    assert lib.hpcla_amg_restrictor_b_f64_i32(None, None, None, None, None, None, None, 3, 0, 4, 0, 0, None, None) == 0
