"""GPU tests of the setup kernels of ``hp.amg`` and ``hp.fsai`` and of the two fused smoother kernels ON THEIR OWN, through the C
ABI (``hp._capi``), on inputs the host layer never builds: one block of a row partition at a time with its ghost columns, both
index widths, ``index_base`` 0 and 1, the capped grid of the smoother kernels, and hand-built rows at the rules' edges.

1. The AMG chain (weights, smoother, strength count / fill, keys, the rounds of the independent set, join, ids, prolongator) on
   every block of every level that aggregates of ``ac.chain_levels``: the restatement of tests/_amg_cases.py in 1, 2, 3 and 8
   blocks at coarse_size = 8.  A block arrives in rank-local split form (``ac.split_block``): owned columns first in id, ghosts
   behind them in id but, where their global column is below the block, in FRONT of the owned entries of a row.  Every block runs
   with Int32 indices and base 0; six cases at 3 and 8 blocks run the other three forms too (Int32 base 1, Int64 base 0 and 1).
   The prolongator reads its columns through a shuffled ``col_indices`` (``ac.compressed_columns``).
2. Hand-built rows: the strength rule at equality, signed zeros, NaN and ghosts; the weights' error word with four failing rows
   in three workgroups; keys of rows beyond 2^40; a graph without edges; calls with no rows.
3. ``hpcla_amg_presmooth_f64`` / ``hpcla_amg_postsmooth_f64`` at the sizes of ``gr.AMG_SMOOTH_ALONE`` (tests/_grid_regimes.py:
   one workgroup, several, the grid capped at 4096 with a third trip and the odd element).
4. The FSAI kernels block by block in all four index forms, the independence of a row's bits from the lane class, a caller's
   ``max_m`` below the truth, the order of the error word, and a pattern that is not A's.

Expected values: every AMG figure and the smoothers' are exact -- integers, or the bits of numpy's separately rounded
expression (the library is built with -ffp-contract=off; the weights' row sum is ``ac.weights_stored_order``: one entry at a
time in stored order, as the kernel's comment defines it).  G's structure is exact; its values lie within ``fc.FSAI_RTOL`` of
``fc.fsai_cholesky`` (the margin of tests/test_gpu_fsai.py; tests/_fsai_cases.py has its basis), and bit-equal between index
forms, lane classes and equivalent patterns.  No margin is introduced here.
"""
import time

import numpy as np
import pytest

from tests import _amg_cases as ac
from tests import _fsai_cases as fc
from tests import _grid_regimes as gr
from tests import _pcg_cases as pc

pytestmark = pytest.mark.gpu

F64, I64, I32 = np.float64, np.int64, np.int32
INVALID = -1                                                     # HPCLA_ERR_INVALID of include/hpcla_rocm.h
FORMS = [("i32", I32, 0), ("i32", I32, 1), ("i64", I64, 0), ("i64", I64, 1)]
FORM_IDS = [f"{sfx}-base{base}" for sfx, _, base in FORMS]
ALL_FORMS_ON = ("grid37x53", "grid16x16x16", "aniso40x40", "star300", "random600", "path257")
ALL_FORMS_BLOCKS = (3, 8)
FSAI_CAP, FSAI_NO_DIAG, FSAI_NOT_SPD = 1, 2, 3                   # the codes of csrc/fsai.hip's error word
RAN = {}                                                         # case name -> what its chains covered


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _tdtype(dtype):
    torch = _torch()
    return {np.dtype(F64): torch.float64, np.dtype(I64): torch.int64, np.dtype(I32): torch.int32}[np.dtype(dtype)]


def _dev(a, dtype):
    """A host array on the device, with at least one element: an empty array still has an address."""
    a = np.array(a, dtype=dtype).reshape(-1)
    if a.size == 0:
        a = np.zeros(1, dtype=dtype)
    return _torch().from_numpy(a).cuda()


def _full(n, value, dtype):
    return _torch().full((max(int(n), 1),), value, dtype=_tdtype(dtype), device="cuda")


def _host(t, n=None):
    a = t.cpu().numpy()
    return a if n is None else a[:int(n)]


def _status(hp, name, *args):
    """The entry's status; a tensor stands for its address, numpy integers become Python's."""
    plain = []
    for a in args:
        if hasattr(a, "data_ptr"):
            plain.append(a.data_ptr())
        elif isinstance(a, (np.integer, np.bool_)):
            plain.append(int(a))
        else:
            plain.append(a)
    return getattr(hp._capi.load(), name)(*plain)


def _call(hp, name, *args):
    rc = _status(hp, name, *args)
    assert rc == 0, (name, rc, hp._capi.last_error())


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.float64 or want.dtype == np.float64:
        got, want = ac.bits(got), ac.bits(want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5].tolist()}: {got[bad[:5]].tolist()} != {want[bad[:5]].tolist()}"


@pytest.fixture(scope="module")
def matrices():
    return ac.cases()


# ---- 1. the AMG chain, one block at a time ------------------------------------------------------------------------------------------
def _level_reference(lvl):
    """What the restatement says of a whole level, once: the weights in stored order, the keys, every row's owner (the root of
    its aggregate: ids are numbered like the roots), A T and P."""
    A = lvl["A"]
    d, ratio = ac.weights_stored_order(A)
    assert np.array_equal(ac.bits(lvl["w"] / d), ac.bits(lvl["s"]))
    key, _ = ac.keys_of(lvl["partition"])
    owner = np.flatnonzero(lvl["roots"])[lvl["agg"]]
    AT = ac.aggregate_product(lvl)
    P = lvl["P"] if "P" in lvl else ac.prolongator(A, lvl["agg"], int(lvl["counts"].sum()), lvl["s"])   # a stalled level keeps none
    assert np.array_equal(P.indptr, AT.indptr) and np.array_equal(P.indices, AT.indices)
    return dict(d=d, ratio=ratio, key=key, owner=owner, AT=AT, P=P, offsets=np.concatenate([[0], np.cumsum(lvl["counts"])]))


def _block_reference(lvl, ref, j, seed):
    part = lvl["partition"]
    lo, hi = int(part[j]), int(part[j + 1])
    indptr, indices = lvl["graph"]
    AT, P = ref["AT"], ref["P"]
    a, b = int(AT.indptr[lo]), int(AT.indptr[hi])
    flags = lvl["roots"][lo:hi].astype(np.int64)
    want = dict(lo=lo, n=hi - lo, diag=ref["d"][lo:hi], ratio=ref["ratio"][lo:hi], s=lvl["s"][lo:hi],
                s_rowptr=indptr[lo:hi + 1] - indptr[lo], s_cols=indices[indptr[lo]:indptr[hi]] - lo, key=ref["key"][lo:hi],
                owner=ref["owner"][lo:hi] - lo, rootid=np.cumsum(flags) - flags, n_roots=int(lvl["counts"][j]),
                offset=int(ref["offsets"][j]), agg=lvl["agg"][lo:hi], at_rowptr=AT.indptr[lo:hi + 1].astype(np.int64) - a,
                at=AT.data[a:b], p=P.data[a:b])
    assert int(flags.sum()) == want["n_roots"] and want["owner"].min() >= 0 and want["owner"].max() < hi - lo
    want["states"] = list(ac.mis2_states(want["s_rowptr"], want["s_cols"], want["key"]))
    want["at_colval"], want["col_indices"] = ac.compressed_columns(AT.indices[a:b], np.random.default_rng(seed))
    return want


def _run_chain(hp, lvl, j, want, theta, form, tag):
    """The chain of C entries on block j in one index form; every output is compared with ``want`` and returned."""
    sfx, Ti, base = form
    lib = hp._capi.load()
    n, lo = want["n"], want["lo"]
    rowptr, split, vals, n_own, ghosts = ac.split_block(lvl["A"], lvl["partition"], j, base, Ti)
    assert n_own == n and n > 0
    d_rowptr, d_split, d_vals = _dev(rowptr, Ti), _dev(split, Ti), _dev(vals, F64)
    out = {}

    diag, ratio, info = _full(n, 7.0, F64), _full(n, 7.0, F64), _full(2, 7, I64)
    _call(hp, f"hpcla_amg_weights_f64_{sfx}", d_rowptr, d_split, d_vals, n, n_own, base, diag, ratio, info, None)
    out["diag"], out["ratio"] = _host(diag, n), _host(ratio, n)
    _same(out["diag"], want["diag"], (tag, "diag"))
    _same(out["ratio"], want["ratio"], (tag, "ratio"))
    assert _host(info).tolist() == [-1, 7], (tag, "weights info")

    s = _full(n, 7.0, F64)
    _call(hp, "hpcla_amg_smoother_f64", float(lvl["w"]), diag, s, n, None)
    out["s"] = _host(s, n)
    _same(out["s"], want["s"], (tag, "s"))

    work = _full(lib.hpcla_amg_work_bytes(n) // 8, 0, I64)
    s_rowptr, info = _full(n + 1, -7, I64), _full(2, -7, I64)
    structure = (d_rowptr, d_split, d_vals, diag, n, n_own, base, float(theta))
    _call(hp, f"hpcla_amg_strength_count_f64_{sfx}", *structure, s_rowptr, info, work, None)
    out["s_rowptr"] = _host(s_rowptr, n + 1)
    _same(out["s_rowptr"], want["s_rowptr"], (tag, "s_rowptr"))
    total = int(want["s_rowptr"][-1])
    assert _host(info).tolist() == [total, -7], (tag, "strength info")
    s_cols = _full(total + 1, -7, I32)
    _call(hp, f"hpcla_amg_strength_fill_f64_{sfx}", *structure, s_rowptr, s_cols, None)
    out["s_cols"] = _host(s_cols)
    _same(out["s_cols"], np.concatenate([want["s_cols"], [-7]]).astype(I32), (tag, "s_cols and the word behind them"))

    key, state, state_next, m1, m2 = (_full(n, -7, I64) for _ in range(5))
    _call(hp, "hpcla_amg_mis_init", n, lo, key, state, None)
    out["key"] = _host(key, n)
    _same(out["key"], want["key"], (tag, "key"))
    _same(_host(state, n), want["key"], (tag, "first state"))
    counts = _full(lib.hpcla_amg_round_blocks(n), -7, I64)
    assert counts.numel() == -(-n // 256)
    assert len(want["states"]) >= 1
    for r, want_state in enumerate(want["states"]):
        _call(hp, "hpcla_amg_mis_round", s_rowptr, s_cols, n, key, state, m1, m2, state_next, counts, None)
        _same(_host(state_next, n), want_state, (tag, f"state after round {r + 1}"))
        left = int(np.count_nonzero((want_state >= 0) & (want_state < ac.ROOT)))
        assert int(_host(counts).sum()) == left, (tag, f"undecided after round {r + 1}")
        assert (left == 0) == (r == len(want["states"]) - 1), tag
        state, state_next = state_next, state
    out["state"], out["rounds"] = _host(state, n), len(want["states"])

    owner_a, owner_b = _full(n, -7, I32), _full(n, -7, I32)
    rootid, info = _full(n, -7, I64), _full(2, -7, I64)
    _call(hp, "hpcla_amg_join", s_rowptr, s_cols, n, key, state, owner_a, owner_b, rootid, info, work, None)
    out["owner"], out["rootid"] = _host(owner_b, n), _host(rootid, n)
    _same(out["owner"], want["owner"].astype(I32), (tag, "owner"))
    _same(out["rootid"], want["rootid"], (tag, "rootid"))
    assert _host(info).tolist() == [-1, want["n_roots"]], (tag, "join info")

    agg = _full(n, -7, I64)
    _call(hp, "hpcla_amg_aggregate_ids", owner_b, rootid, n, want["offset"], agg, None)
    out["agg"] = _host(agg, n)
    _same(out["agg"], want["agg"], (tag, "agg"))

    nnz = len(want["at"])
    p = _full(nnz + 1, np.nan, F64)
    _call(hp, f"hpcla_amg_prolongator_f64_{sfx}", _dev(want["at_rowptr"] + base, Ti), _dev(want["at_colval"] + base, Ti),
          _dev(want["col_indices"], I64), _dev(want["at"], F64), _dev(want["agg"], I64), _dev(want["s"], F64), n, base, p, None)
    out["p"] = _host(p)
    _same(out["p"][:nnz], want["p"], (tag, "p"))
    assert np.isnan(out["p"][nnz]), (tag, "the word behind p")
    return out


@pytest.mark.parametrize("name", sorted(ac.cases()))
def test_amg_chain_on_every_block_of_every_level(hp, matrices, name):
    t0 = time.perf_counter()
    theta = ac.theta_of(name)
    stats = dict(levels=0, chains=0, runs=0, one_row_blocks=0, stored_zeros=0, isolated=0, longest_row=0, rounds=[])
    for (_, k), levels in ac.chain_levels(matrices, [name]).items():
        for depth, lvl in enumerate(levels):
            ref = _level_reference(lvl)
            part = lvl["partition"]
            stats["levels"] += 1
            stats["stored_zeros"] += int(np.sum(lvl["A"].data == 0))
            stats["isolated"] += int(np.any(np.diff(lvl["graph"][0]) == 0))
            forms = FORMS if name in ALL_FORMS_ON and k in ALL_FORMS_BLOCKS else FORMS[:1]
            for j in range(len(part) - 1):
                assert part[j + 1] > part[j], (name, k, depth, j)                 # no block of these levels is empty
                want = _block_reference(lvl, ref, j, seed=1000 * k + 10 * depth + j)
                first = None
                for form in forms:
                    tag = (name, k, depth, j, form[0], form[2])
                    got = _run_chain(hp, lvl, j, want, theta, form, tag)
                    stats["runs"] += 1
                    if first is None:
                        first = got
                    for what in first:                                            # the forms agree bit for bit, outputs 0-based
                        _same(got[what], first[what], (tag, what, "against the first form"))
                stats["chains"] += 1
                stats["one_row_blocks"] += int(want["n"] == 1)
                stats["longest_row"] = max(stats["longest_row"], int(np.diff(want["at_rowptr"]).max()))
                stats["rounds"].append(first["rounds"])
                assert first["rounds"] <= lvl["rounds"], (name, k, depth, j)
    RAN[name] = stats
    rounds = stats["rounds"]
    print(f"{name}: {stats['levels']} levels, {stats['chains']} blocks, {stats['runs']} chains run, rounds "
          f"{min(rounds) if rounds else 0}..{max(rounds) if rounds else 0}, longest row of A T {stats['longest_row']}, "
          f"{time.perf_counter() - t0:.2f} s")


def test_the_chains_covered_the_edges_they_are_for(matrices):
    """What the parametrised test above walks (it takes every block of ``ac.chain_levels``, none left out): enough levels, a
    block of one row, a stored zero, a level with an isolated row.  Where that test ran in this session its own counts agree."""
    cover = ac.chain_coverage(ac.chain_levels(matrices))
    print(cover)
    assert cover["levels"] >= 120 and cover["one_row_blocks"] >= 1 and cover["stored_zeros"] >= 1 and cover["isolated"] >= 1
    assert cover["longest_row"] >= 128 and cover["ghost_entries"] >= 75_000
    if set(RAN) == set(matrices):
        for what in ("levels", "chains", "one_row_blocks", "stored_zeros", "isolated"):
            assert sum(s[what] for s in RAN.values()) == cover[what], what
        assert max(s["longest_row"] for s in RAN.values()) == cover["longest_row"]
        rounds = [r for s in RAN.values() for r in s["rounds"]]
        print(f"{cover['chains']} (case, blocks, level, block) chains, {sum(s['runs'] for s in RAN.values())} runs over the index "
              f"forms, rounds {min(rounds)}..{max(rounds)}, longest row fed to the prolongator {cover['longest_row']}")


# ---- 2. hand-built rows ---------------------------------------------------------------------------------------------------------------
NEAR_ONE = -(1.0 - 2.0 ** -53)                                   # the largest magnitude below 1


def _strength_rows():
    """Six owned rows (diagonal 4: with theta = 0.25 the rule's right side is exactly 1) and two ghosts, ids 6 and 7, in split
    form: (rowptr, colval, vals, kept at theta 0.25, kept at theta 0)."""
    rows = [
        [(6, -100.0), (0, 4.0), (1, -1.0), (2, NEAR_ONE), (3, 0.0), (4, -0.0), (5, float("nan")), (7, -3.0)],
        [(0, -1.0), (1, 4.0), (3, 1e-300)],
        [(7, 1.0), (0, NEAR_ONE), (2, 4.0)],
        [(1, 1e-300), (3, 4.0), (6, float("nan"))],
        [(4, 4.0), (5, 2.0)],
        [(6, 5.0), (0, float("nan")), (4, 2.0), (5, 4.0)],
    ]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    colval = np.array([c for r in rows for c, _ in r])
    vals = np.array([v for r in rows for _, v in r])
    quarter = [[1], [0], [], [], [5], [4]]
    zero = [[1, 2], [0, 3], [0], [1], [5], [4]]
    return rowptr, colval, vals, quarter, zero


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_strength_rule_at_its_boundary(hp, form):
    """|a| == theta sqrt(d_i d_c) is kept, one ulp below is dropped; +0.0, -0.0, NaN and ghosts of any size never enter; theta = 0
    keeps every stored nonzero owned coupling, however small."""
    sfx, Ti, base = form
    rowptr, colval, vals, quarter, zero = _strength_rows()
    n = 6
    assert 0.25 * np.sqrt(4.0 * 4.0) == 1.0 and abs(NEAR_ONE) < 1.0 and np.nextafter(abs(NEAR_ONE), 2.0) == 1.0
    args = (_dev(rowptr + base, Ti), _dev(colval + base, Ti), _dev(vals, F64), _dev(np.full(n, 4.0), F64), n, n, base)
    work = _full(hp._capi.load().hpcla_amg_work_bytes(n) // 8, 0, I64)
    for theta, kept in ((0.25, quarter), (0.0, zero)):
        want_ptr = np.concatenate([[0], np.cumsum([len(r) for r in kept])])
        want_cols = np.array([c for r in kept for c in r] + [-7], dtype=I32)
        s_rowptr, info, s_cols = _full(n + 1, -7, I64), _full(1, -7, I64), _full(len(want_cols), -7, I32)
        _call(hp, f"hpcla_amg_strength_count_f64_{sfx}", *args, theta, s_rowptr, info, work, None)
        _same(_host(s_rowptr), want_ptr, (form, theta, "s_rowptr"))
        assert int(_host(info)[0]) == want_ptr[-1], (form, theta)
        _call(hp, f"hpcla_amg_strength_fill_f64_{sfx}", *args, theta, s_rowptr, s_cols, None)
        _same(_host(s_cols), want_cols, (form, theta, "s_cols"))


def _weights_faults(heal):
    """700 rows (three workgroups) of path(700) with four failing rows, the first ``heal`` of them (in row order) put right:
    row 100 is empty, row 257 has a NaN diagonal, row 300 stores no diagonal, row 600 a negative one."""
    import scipy.sparse as sp
    A = ac.path(700).tolil()
    if heal < 1:
        A[100, 99] = A[100, 100] = A[100, 101] = 0.0
    if heal < 3:
        A[300, 300] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    if heal < 2:
        A[257, 257] = np.nan
    if heal < 4:
        A[600, 600] = -2.0
    return sp.csr_matrix(A)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_weights_error_word_is_the_smallest_failing_row(hp, form):
    sfx, Ti, base = form
    failing = [100, 257, 300, 600]
    for heal in range(5):
        A = _weights_faults(heal)
        n = A.shape[0]
        assert len(A.indptr) == 701 and (A.indptr[101] - A.indptr[100] == 0) == (heal < 1)
        assert (300 in A.indices[A.indptr[300]:A.indptr[301]]) == (heal >= 3)
        rowptr, split, vals, n_own, _ = ac.split_block(A, [0, n], 0, base, Ti)
        diag, ratio, info = _full(n, 7.0, F64), _full(n, 7.0, F64), _full(1, 7, I64)
        _call(hp, f"hpcla_amg_weights_f64_{sfx}", _dev(rowptr, Ti), _dev(split, Ti), _dev(vals, F64), n, n, base, diag, ratio, info, None)
        assert int(_host(info)[0]) == (failing[heal] if heal < 4 else -1), (form, heal)
        d, r = ac.weights_stored_order(A)
        good = np.ones(n, dtype=bool)
        good[failing[heal:]] = False
        got_d, got_r = _host(diag), _host(ratio)
        _same(got_d[good], d[good], (form, heal, "diag of the other rows"))
        _same(got_r[good], r[good], (form, heal, "ratio of the other rows"))
        bad = np.array(failing[heal:], dtype=np.int64)
        assert np.array_equal(np.isnan(got_d[bad]), np.isnan(d[bad])), (form, heal)
        assert np.array_equal(got_d[bad][~np.isnan(d[bad])], d[bad][~np.isnan(d[bad])]), (form, heal)      # 0 where none is stored


def test_keys_of_rows_far_out(hp):
    n, row_start = 257, 2 ** 40 + 12345
    key, state = _full(n, -7, I64), _full(n, -7, I64)
    _call(hp, "hpcla_amg_mis_init", n, row_start, key, state, None)
    want = (ac.hash31(row_start + np.arange(n, dtype=np.int64)) << 31) | np.arange(n, dtype=np.int64)
    _same(_host(key), want, "key")
    _same(_host(state), want, "state")
    assert len(np.unique(want)) == n and want.min() >= 0 and want.max() < 2 ** 62
    assert not np.array_equal(want, ac.keys_of([0, n])[0])          # the global row enters the hash


def test_a_graph_without_edges_makes_every_row_a_root(hp):
    n = 300
    lib = hp._capi.load()
    s_rowptr = _full(n + 1, 0, I64)
    key, state, state_next, m1, m2 = (_full(n, -7, I64) for _ in range(5))
    counts = _full(lib.hpcla_amg_round_blocks(n), -7, I64)
    _call(hp, "hpcla_amg_mis_init", n, 0, key, state, None)
    _call(hp, "hpcla_amg_mis_round", s_rowptr, None, n, key, state, m1, m2, state_next, counts, None)
    _same(_host(state_next), np.full(n, ac.ROOT, dtype=I64), "state")
    assert _host(counts).tolist() == [0, 0]
    owner_a, owner_b, rootid, info = _full(n, -7, I32), _full(n, -7, I32), _full(n, -7, I64), _full(2, -7, I64)
    work = _full(lib.hpcla_amg_work_bytes(n) // 8, 0, I64)
    _call(hp, "hpcla_amg_join", s_rowptr, None, n, key, state_next, owner_a, owner_b, rootid, info, work, None)
    _same(_host(owner_b), np.arange(n, dtype=I32), "owner")
    _same(_host(rootid), np.arange(n, dtype=I64), "rootid")
    assert _host(info).tolist() == [-1, n]
    agg = _full(n, -7, I64)
    _call(hp, "hpcla_amg_aggregate_ids", owner_b, rootid, n, 1000, agg, None)
    _same(_host(agg), 1000 + np.arange(n, dtype=I64), "agg")
    # the join's own error word, which no real aggregation sets: a state without a root leaves every row free, in all ten
    # workgroups of the join (8 lanes a row), and the word is the smallest of them
    lost = _full(n, -1, I64)
    _call(hp, "hpcla_amg_join", s_rowptr, None, n, key, lost, owner_a, owner_b, rootid, info, work, None)
    _same(_host(owner_b), np.full(n, -1, dtype=I32), "owner of a row without a root in reach")
    assert _host(info).tolist() == [0, 0]
    _call(hp, "hpcla_amg_join", s_rowptr, None, n, key, state_next, owner_a, owner_b, rootid, info, work, None)
    assert _host(info).tolist() == [-1, n]                          # and a good call afterwards


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_calls_with_no_rows(hp, form):
    """nrows = 0: every entry returns 0 without an array and sets the words the sources say it sets, nothing else."""
    sfx, _, base = form
    word = lambda k: _full(k, 7, I64)
    info = word(2)
    _call(hp, f"hpcla_amg_weights_f64_{sfx}", None, None, None, 0, 0, base, None, None, info, None)
    assert _host(info).tolist() == [-1, 7]
    _call(hp, "hpcla_amg_smoother_f64", 1.0, None, None, 0, None)
    s_rowptr, info, work = word(2), word(2), word(2)
    _call(hp, f"hpcla_amg_strength_count_f64_{sfx}", None, None, None, None, 0, 0, base, 0.25, s_rowptr, info, work, None)
    assert _host(s_rowptr).tolist() == [0, 7] and _host(info).tolist() == [0, 7]
    _call(hp, f"hpcla_amg_strength_fill_f64_{sfx}", None, None, None, None, 0, 0, base, 0.25, None, None, None)
    _call(hp, "hpcla_amg_mis_init", 0, 0, None, None, None)
    counts = word(2)
    _call(hp, "hpcla_amg_mis_round", None, None, 0, None, None, None, None, None, counts, None)
    assert _host(counts).tolist() == [0, 7]
    info = word(3)
    _call(hp, "hpcla_amg_join", None, None, 0, None, None, None, None, None, info, work, None)
    assert _host(info).tolist() == [-1, 0, 7]
    _call(hp, "hpcla_amg_aggregate_ids", None, None, 0, 0, None, None)
    _call(hp, f"hpcla_amg_prolongator_f64_{sfx}", None, None, None, None, None, None, 0, base, None, None)
    _call(hp, "hpcla_amg_presmooth_f64", None, None, None, 0, None)
    _call(hp, "hpcla_amg_postsmooth_f64", None, None, None, None, 0, None)
    g_rowptr, info = word(2), word(4)
    _call(hp, f"hpcla_fsai_count_f64_{sfx}", None, None, None, None, 0, 0, base, g_rowptr, info, work, None)
    assert _host(g_rowptr).tolist() == [0, 7] and _host(info).tolist() == [0, 0, -1, 7]
    _call(hp, f"hpcla_fsai_factor_f64_{sfx}", None, None, None, None, None, 0, 0, base, 0, 8, None, None, None, info, None)
    assert _host(info).tolist() == [0, 0, -1, 7] and _host(work).tolist() == [7, 7]


# ---- 3. the two smoother kernels ---------------------------------------------------------------------------------------------------------
PAD = 2                                                          # doubles of poison on each side: the operand stays on 16 bytes


def _poisoned(values):
    """(whole device buffer, the operand inside it), NaN on both sides."""
    torch = _torch()
    n = len(values)
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float64, device="cuda")
    buf[PAD:PAD + n].copy_(torch.from_numpy(np.array(values)))
    return buf, buf[PAD:PAD + n]


def _bits_equal(a, b):
    torch = _torch()
    return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


@pytest.mark.parametrize("n", gr.AMG_SMOOTH_ALONE)
def test_smoother_kernels_alone(hp, n):
    """x = s .* b and x = x + s .* (b - t) bit for bit against numpy's separately rounded expressions, in the callers' poisoned
    buffers; at R4_N on the capped grid: 2 097 153 double2 over 4096 x 256 lanes, a third trip of lane 0, and the odd element."""
    torch = _torch()
    assert gr.amg_smooth_regime(n) is not None
    rng = np.random.default_rng(77 + n % 1000)
    sv, bv, tv, xv = (rng.uniform(-2.0, 2.0, n) for _ in range(4))
    (sb, s), (bb, b), (tb, t), (xb, x) = (_poisoned(v) for v in (sv, bv, tv, xv))
    assert all(v.data_ptr() % 16 == 0 for v in (s, b, t, x))
    snaps = [buf.clone() for buf in (sb, bb, tb)]

    def image(values):
        img = torch.full_like(xb, float("nan"))
        img[PAD:PAD + n].copy_(torch.from_numpy(np.array(values)))
        return img

    def inputs_unchanged(what):
        for buf, snap in zip((sb, bb, tb), snaps):
            assert _bits_equal(buf, snap), (n, what, "s, b or t changed")

    for again in range(2):                                       # a second call gives the same bits
        _call(hp, "hpcla_amg_presmooth_f64", s, b, x, n, None)
        assert _bits_equal(xb, image(sv * bv)), (n, "presmooth", again)
        inputs_unchanged("presmooth")
    for again in range(2):
        x.copy_(torch.from_numpy(xv.copy()))
        _call(hp, "hpcla_amg_postsmooth_f64", s, b, t, x, n, None)
        assert _bits_equal(xb, image(xv + sv * (bv - tv))), (n, "postsmooth", again)
        inputs_unchanged("postsmooth")

    # a pointer 8 bytes off in any position: refused, nothing written
    before = xb.clone()
    ptr = [v.data_ptr() for v in (s, b, t, x)]
    for pos in (0, 1, 3):
        a = list(ptr)
        a[pos] += 8
        assert _status(hp, "hpcla_amg_presmooth_f64", a[0], a[1], a[3], n, None) == INVALID, (n, pos)
        assert "16-byte" in hp._capi.last_error()
    for pos in range(4):
        a = list(ptr)
        a[pos] += 8
        assert _status(hp, "hpcla_amg_postsmooth_f64", *a, n, None) == INVALID, (n, pos)
        assert "16-byte" in hp._capi.last_error()
    torch.cuda.synchronize()
    assert _bits_equal(xb, before), (n, "a refused call wrote")
    inputs_unchanged("refused calls")


# ---- 4. the FSAI kernels ----------------------------------------------------------------------------------------------------------------
def _fsai_run(hp, a_block, p_block, lo, form, max_m=None):
    """hpcla_fsai_count then hpcla_fsai_factor on one block in split form (``a_block``: rowptr, colval, vals, n_own of
    ``ac.split_block``; ``p_block`` the pattern's, None: A's own).  G's arrays start poisoned (-7, NaN)."""
    sfx, Ti, base = form
    rowptr, split, vals, n = a_block[:4]
    a_rowptr, a_split, a_vals = _dev(rowptr, Ti), _dev(split, Ti), _dev(vals, F64)
    p_rowptr, p_split = (a_rowptr, a_split) if p_block is None else (_dev(p_block[0], Ti), _dev(p_block[1], Ti))
    g_rowptr, info = _full(n + 1, -7, I64), _full(4, -7, I64)
    work = _full(hp._capi.load().hpcla_fsai_work_bytes(n) // 8, 0, I64)
    _call(hp, f"hpcla_fsai_count_f64_{sfx}", p_rowptr, p_split, a_rowptr, a_split, n, n, base, g_rowptr, info, work, None)
    nnz, m, count_word, behind = (int(v) for v in _host(info))
    assert behind == -7
    g_cols, g_vals = _full(nnz + 1, -7, I64), _full(nnz + 1, np.nan, F64)
    _call(hp, f"hpcla_fsai_factor_f64_{sfx}", p_rowptr, p_split, a_rowptr, a_split, a_vals, n, n, base, lo, m if max_m is None else max_m,
          g_rowptr, g_cols, g_vals, info, None)
    tail = _host(info)
    assert tail[:2].tolist() == [nnz, m] and tail[3] == -7
    cols, gv = _host(g_cols), _host(g_vals)
    assert cols[nnz] == -7 and np.isnan(gv[nnz])                   # the words behind G
    return dict(rowptr=_host(g_rowptr), nnz=nnz, m=m, cols=cols[:nnz], vals=gv[:nnz], count_word=count_word, word=int(tail[2]))


def _rel(got, want):
    """The largest relative deviation of an entry; an entry the restatement has as zero (a pattern column A does not couple to
    the rest of J) must be zero, and nothing may be NaN."""
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    zero = want == 0.0
    assert np.all(got[zero] == 0.0), "an entry that is zero in the restatement is not"
    return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]))) if np.any(~zero) else 0.0


@pytest.fixture(scope="module")
def fsai_cases(orc):
    cases = fc.spd_cases(orc)
    return {name: cases[name] for name in ("banded3", "banded7", "banded15", "banded31", "pattern16x16", "poisson33x31")}


@pytest.mark.parametrize("name", ["banded7", "banded31", "pattern16x16", "poisson33x31"])
def test_fsai_block_by_block_in_every_index_form(hp, fsai_cases, name):
    rowptr, colidx, vals, _, pattern = fsai_cases[name]
    n = len(rowptr) - 1
    A = fc.to_scipy(rowptr, colidx, vals)
    P = None if pattern is None else fc.to_scipy(*pattern)
    worst = 0.0
    for k in (1, 3, 8):
        part = fc.equal_blocks(n, k)
        gp, gc, gv = fc.fsai_blocks(rowptr, colidx, vals, part, pattern)
        for j in range(k):
            lo, hi = part[j], part[j + 1]
            a, b = int(gp[lo]), int(gp[hi])
            first = None
            for form in FORMS:
                tag = (name, k, j, form[0], form[2])
                a_block = ac.split_block(A, part, j, form[2], form[1])
                p_block = None if P is None else ac.split_block(P, part, j, form[2], form[1])
                got = _fsai_run(hp, a_block, p_block, lo, form)
                _same(got["rowptr"], gp[lo:hi + 1] - a, (tag, "g_rowptr"))
                assert (got["nnz"], got["m"]) == (b - a, int(np.diff(gp[lo:hi + 1]).max())), tag
                _same(got["cols"], gc[a:b], (tag, "g_cols"))
                assert got["count_word"] == -1 and got["word"] == -1, tag
                worst = max(worst, _rel(got["vals"], gv[a:b]))
                if first is None:
                    first = got
                _same(got["vals"], first["vals"], (tag, "values against the first form"))
            if k > 1:
                assert len(a_block[4]) > 0, (name, k, j)            # the block has ghosts
    print(f"{name}: largest relative deviation of an entry {worst:.2e} (FSAI_RTOL {fc.FSAI_RTOL:.1e})")
    assert worst <= fc.FSAI_RTOL, (name, worst)


@pytest.mark.parametrize("name,classes", [("banded3", (4, 8, 16, 32)), ("banded15", (16, 32))])
def test_fsai_rows_do_not_depend_on_the_lane_class(hp, fsai_cases, name, classes):
    """csrc/fsai.hip: "the bits of a row do not depend on MT" -- the group is padded with rows of the identity."""
    rowptr, colidx, vals, _, _ = fsai_cases[name]
    n = len(rowptr) - 1
    A = fc.to_scipy(rowptr, colidx, vals)
    block = ac.split_block(A, [0, n], 0)
    runs = [_fsai_run(hp, block, None, 0, FORMS[0], max_m=mt) for mt in classes]
    assert runs[0]["m"] <= classes[0] and (classes[0] == 4 or runs[0]["m"] > classes[0] // 2)
    gp, gc, gv = fc.fsai_cholesky(rowptr, colidx, vals)
    assert _rel(runs[0]["vals"], gv) <= fc.FSAI_RTOL
    for mt, run in zip(classes, runs):
        assert run["word"] == -1, (name, mt)
        _same(run["cols"], gc, (name, mt, "g_cols"))
        _same(run["vals"], runs[0]["vals"], (name, mt, "values against the narrowest class"))


def test_fsai_max_m_below_the_truth_writes_no_capped_row(hp, fsai_cases):
    rowptr, colidx, vals, _, _ = fsai_cases["banded7"]
    n = len(rowptr) - 1
    block = ac.split_block(fc.to_scipy(rowptr, colidx, vals), [0, n], 0)
    full = _fsai_run(hp, block, None, 0, FORMS[0])
    capped = _fsai_run(hp, block, None, 0, FORMS[0], max_m=4)
    assert full["m"] == 8 and full["word"] == -1
    m = np.diff(full["rowptr"])
    over = np.repeat(m > 4, m)
    first = int(np.flatnonzero(m > 4)[0])
    assert first == 4 and capped["word"] == (first << 2) | FSAI_CAP
    assert np.all(capped["cols"][over] == -7) and np.all(np.isnan(capped["vals"][over]))     # the poison they were given
    _same(capped["vals"][~over], full["vals"][~over], "rows with m <= 4")
    _same(capped["cols"][~over], full["cols"][~over], "columns of rows with m <= 4")


def test_fsai_count_names_the_first_row_over_the_cap(hp):
    """banded(32): rows 32 .. 299 have m = 33, in both workgroups of the scan; the word is row 32's."""
    rowptr, colidx, vals = fc.banded(fc.CAP_W)
    n = len(rowptr) - 1
    for form in (FORMS[0], FORMS[3]):
        sfx, Ti, base = form
        r, c, _, _, _ = ac.split_block(fc.to_scipy(rowptr, colidx, vals), [0, n], 0, base, Ti)
        d_r, d_c = _dev(r, Ti), _dev(c, Ti)
        g_rowptr, info = _full(n + 1, -7, I64), _full(4, -7, I64)
        work = _full(hp._capi.load().hpcla_fsai_work_bytes(n) // 8, 0, I64)
        _call(hp, f"hpcla_fsai_count_f64_{sfx}", d_r, d_c, d_r, d_c, n, n, base, g_rowptr, info, work, None)
        m = np.minimum(np.arange(n), fc.CAP_W) + 1
        _same(_host(g_rowptr), np.concatenate([[0], np.cumsum(m)]), (form, "g_rowptr"))
        assert _host(info).tolist() == [int(m.sum()), fc.CAP_W + 1, (fc.CAP_W << 2) | FSAI_CAP, -7], form


def test_fsai_error_word_names_the_smallest_row(hp):
    """Three faults, healed one at a time from the smallest row up: each time the word names the smallest one left."""
    words = [(40 << 2) | FSAI_NOT_SPD, (300 << 2) | FSAI_NO_DIAG, (520 << 2) | FSAI_NOT_SPD, -1]
    w = 3
    rowptr, colidx, vals = fc.three_faults(3)
    clean = _fsai_run(hp, ac.split_block(fc.to_scipy(rowptr, colidx, vals), [0, 600], 0), None, 0, FORMS[0])
    assert clean["word"] == -1 and clean["m"] == w + 1
    row_of = np.repeat(np.arange(600), np.diff(clean["rowptr"]))
    for heal, word in enumerate(words):
        rowptr, colidx, vals = fc.three_faults(heal)
        for form in (FORMS[0], FORMS[3]):
            got = _fsai_run(hp, ac.split_block(fc.to_scipy(rowptr, colidx, vals), [0, 600], 0, form[2], form[1]), None, 0, form)
            assert got["word"] == word, (heal, form, got["word"], word)
            assert got["count_word"] == ((300 << 2) | FSAI_NO_DIAG if heal < 2 else -1), (heal, form)
            _same(got["rowptr"], clean["rowptr"], (heal, "g_rowptr"))
            _same(got["cols"], clean["cols"], (heal, "g_cols"))
            reads = np.zeros(600, dtype=bool)                       # rows whose J holds a faulty row: f .. f + w
            for f in fc.FAULT_ROWS[heal:]:
                reads[f:f + w + 1] = True
            keep = ~reads[row_of]
            _same(got["vals"][keep], clean["vals"][keep], (heal, form, "rows that read no faulty entry"))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_fsai_pattern_that_is_not_A(hp, form):
    """Pattern rows with columns above the diagonal, ghosts in front of the owned columns and entries A does not store, while A
    stores entries outside the pattern: the restatement's G, and the bits of the call without the ignorable entries."""
    A, P, Pthin, part, j = fc.pattern_is_not_a()
    lo, hi = part[j], part[j + 1]
    cut = lambda M: (M.indptr[lo:hi + 1] - M.indptr[lo], M.indices[M.indptr[lo]:M.indptr[hi]].astype(np.int64))
    gp, gc, gv = fc.fsai_cholesky(*cut(A), A.data[A.indptr[lo]:A.indptr[hi]], row_start=lo, pattern=cut(P))
    a_block = ac.split_block(A, part, j, form[2], form[1])
    full = _fsai_run(hp, a_block, ac.split_block(P, part, j, form[2], form[1]), lo, form)
    thin = _fsai_run(hp, a_block, ac.split_block(Pthin, part, j, form[2], form[1]), lo, form)
    for got in (full, thin):
        _same(got["rowptr"], gp, (form, "g_rowptr"))
        _same(got["cols"], gc, (form, "g_cols"))
        assert got["word"] == -1 and (got["nnz"], got["m"]) == (len(gc), int(np.diff(gp).max()))
        assert _rel(got["vals"], gv) <= fc.FSAI_RTOL, (form, _rel(got["vals"], gv))
    _same(full["vals"], thin["vals"], (form, "full against thinned pattern"))
